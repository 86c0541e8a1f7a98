"""Timing of a key per frame (wm_embed_select, wm_detect_select) at 4K.  On the GPU box.
usage: python tools/select_bench.py [--rows 2160 --cols 3840 --frames 16 --iters 10 --rounds 5] [--configs f32:ME,f32:NVF,u8:ME,u8:NVF]
                                    [--json out.json]
       python tools/select_bench.py --trace [--trace-legs a0,c] [--iters 5]   (under rocprofv3 --kernel-trace --stats: two legs, untimed)
       python tools/select_bench.py --from-trace kernel_stats.csv [--json out.json]   (the per-sweep table of such a run; no GPU)

One process, the legs alternating in --rounds rounds (tools/convert16_bench.py's scheme).  Device span by events on ONE stream that every
engine's slot 0 is set to, around one embed call and around one detect call of a batch of --frames frames (the batch's base is the
input; the detector reads the embed's output), median over --iters spans per round, then the median of the rounds.
 (a) wm_embed / wm_detect of the batch with ONE key on a context whose W is that key (fused kernels off): the floor.  The library's
     defaults: f32 ME batches take the checked hand-over (the embed's hand-over instance, then k_gram_ho and the checking detector).
 (a0) the same with wm_set_checked_handover(0): the sweeps (c) .. (e) share their bodies with, kernel for kernel.
 (b) what a caller does without the calls: --frames queued one-frame wm_embed / wm_detect calls on --frames per-key contexts on the
     sweeps, one span around all of them.
 (c) wm_embed_select / wm_detect_select with --frames distinct keys.
 (d) the same with an all-equal table.
 (e) the same with runs of 4 equal keys.
Reported: microseconds per batch and leg, the rounds, (d) / (a) and (d) / (a0), (c) / (b), (c) - (a) and (c) - (a0), and beside those the time of a pure read
(wm_membench kind 2, the sweeps' grid shape, and kind 5, the shape that streams fastest) of the extra W bytes -- (frames - 1) planes per
sweep that reads W: two sweeps in an embed (stats, embed), one in a detect -- taken in the same rounds.  Checks that (c) writes what the
per-key contexts of (b) write.  The per-sweep split of (c) - (a) comes from a kernel trace (--trace, --from-trace): the new kernels are
not in the wm_prof_* list."""
import argparse
import csv
import json
import re

import numpy as np

import benchlib as bl

SWEEPS = (("stats", ("k_me_stats", "k_nvf_stats")), ("embed", ("k_embed",)), ("detect", ("k_detect",)), ("gram", ("k_gram",)))


def from_trace(path):
    """{config: {sweep: {"single_us", "select_us", "delta_us"}}} from rocprofv3's kernel_stats.csv of a --trace run: mean duration per
    launch of every sweep kernel, the single-key kernel beside its *_sel twin with the same element type and mask"""
    rows = list(csv.DictReader(open(path)))
    name_col = next(c for c in rows[0] if c.lower() in ("name", "kernelname", "kernel_name"))
    avg_col = next(c for c in rows[0] if c.lower().startswith("average"))
    table = {}
    for r in rows:
        m = re.search(r"(?:wmk::)?(k_\w+)<([^>]*)>", r[name_col])
        if not m:
            continue
        base, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
        sel = base.endswith("_sel")
        stem = base[:-4] if sel else base
        sweep = next((s for s, names in SWEEPS if stem in names), None)
        if sweep is None or sweep == "gram":
            continue
        if not sel and stem == "k_embed" and args[-1] not in ("false", "0"):
            continue  # (the hand-over instance: another kernel)
        dt = "u8" if args[0].startswith("unsigned char") or args[0] == "uint8_t" else "f32"
        mask = "NVF" if stem == "k_nvf_stats" else "ME" if stem == "k_me_stats" else ("NVF" if args[3 if stem == "k_embed" else 1] == "1" else "ME")
        vec = args[5 if stem == "k_embed" else (1 if stem == "k_me_stats" else 2 if stem == "k_nvf_stats" else 4)]
        if vec not in ("true", "1"):
            continue  # (the generic remainder of a sweep, if any: microseconds)
        e = table.setdefault(dt + ":" + mask, {}).setdefault(sweep, {})
        e["select_us" if sel else "single_us"] = round(float(r[avg_col]) * 1e-3, 2)
    for cfg in table.values():
        for e in cfg.values():
            if "single_us" in e and "select_us" in e:
                e["delta_us"] = round(e["select_us"] - e["single_us"], 2)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="f32:ME,f32:NVF,u8:ME,u8:NVF")
    ap.add_argument("--trace", action="store_true", help="the legs of --trace-legs only, untimed, for a kernel trace")
    ap.add_argument("--trace-legs", default="a0,c", help="one single-key leg and one select leg (the trace tells kernels apart, not legs)")
    ap.add_argument("--from-trace", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    def write(res):
        if a.json:
            bl.write_json(a.json, res)

    if a.from_trace:
        res = {"per_sweep_from_kernel_trace": from_trace(a.from_trace)}
        print("SELECT_TRACE " + json.dumps(res), flush=True)
        return write(res)

    import torch
    wm, synth = bl.load()
    R, Cc, F = a.rows, a.cols, a.frames
    plane_bytes = R * Cc * 4
    seeds = [3000 + 7 * k for k in range(F)]
    keys = wm.KeySet.from_seeds(R, Cc, seeds)
    stream = torch.cuda.Stream()
    tables = {"c": list(range(F)), "d": [0] * F, "e": [(f // 4) % F for f in range(F)]}
    configs = []
    mb = {2: [], 5: []}

    for cfg in a.configs.split(","):
        dt, mname = cfg.split(":")
        mk = wm.MASK_TYPE[mname]
        xs = synth.synth_frames_torch(R, Cc, F, "cuda", dtype=dt, first_frame=1)
        ys = {leg: torch.empty_like(xs) for leg in ("a", "a0", "b", "c", "d", "e")}
        corr = np.zeros(F, np.float32)
        torch.cuda.synchronize()
        batch = wm.Watermark.generated(R, Cc, seeds[0], 3, 40.0, nslots=1, max_frames=F)  # (a); (c) .. (e) do not use its W
        batch.set_fused(False)
        plain = wm.Watermark.generated(R, Cc, seeds[0], 3, 40.0, nslots=1, max_frames=F)  # (a0)
        plain.set_fused(False)
        plain.set_checked_handover(False)
        singles = []
        for k in range(F):
            e = wm.Watermark.generated(R, Cc, seeds[k], 3, 40.0, nslots=1, max_frames=1)
            e.set_fused(False)
            singles.append(e)
        with torch.cuda.stream(stream):
            for e in [batch, plain] + singles:
                e.set_stream_current(0)
        px = wm.plane_of(xs, 1)
        py = {leg: wm.plane_of(t, 1) for leg, t in ys.items()}
        p1x = [wm.plane_of(xs[f], 1) for f in range(F)]
        p1y = [wm.plane_of(ys["b"][f], 1) for f in range(F)]

        def sync_all(leg):
            for e in (singles if leg == "b" else [plain] if leg == "a0" else [batch]):
                e.sync(0)

        def embed(leg):
            if leg in ("a", "a0"):
                (batch if leg == "a" else plain).embed_async(px, px, py[leg], mk, 0)
            elif leg == "b":
                for f in range(F):
                    singles[f].embed_async(p1x[f], p1x[f], p1y[f], mk, 0)
            else:
                batch.embed_select_async(px, px, py[leg], keys, tables[leg], mk, 0)

        def detect(leg):
            if leg in ("a", "a0"):
                (batch if leg == "a" else plain).detect_async(py[leg], mk, 0)
            elif leg == "b":
                for f in range(F):
                    singles[f].detect_async(p1y[f], mk, 0)
            else:
                batch.detect_select_async(py[leg], keys, tables[leg], mk, 0, corr)

        def span_us(fn, leg, n):
            ts = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(leg)
                e1.record(stream)
                sync_all(leg)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            return float(np.median(ts))

        legs = tuple(a.trace_legs.split(",")) if a.trace else ("a", "a0", "b", "c", "d", "e")
        for leg in legs:  # warm-up: arenas, staging, code objects
            for _ in range(2):
                embed(leg)
                detect(leg)
            sync_all(leg)
        if a.trace:
            for _ in range(a.iters):
                for leg in legs:
                    embed(leg)
                    detect(leg)
                    sync_all(leg)
            for e in [batch, plain] + singles:
                e.close()
            continue
        same = bool(torch.equal(ys["b"], ys["c"]))
        t = {op: {leg: [] for leg in legs} for op in ("embed", "detect")}
        for _ in range(a.rounds):
            for kind in mb:
                mb[kind].append(bl.membench_us(kind, (F - 1) * plane_bytes, 0.1)[0])
            for leg in legs:
                t["embed"][leg].append(span_us(embed, leg, a.iters))
                t["detect"][leg].append(span_us(detect, leg, a.iters))
        r = {"dtype": dt, "mask": mname, "select_output_equals_per_key_contexts": same}
        for op in ("embed", "detect"):
            med = {leg: float(np.median(v)) for leg, v in t[op].items()}
            spread_a = (max(t[op]["a"]) - min(t[op]["a"])) / med["a"]
            r[op] = {"us": {leg: round(v, 1) for leg, v in med.items()}, "us_rounds": {leg: [round(x, 1) for x in v] for leg, v in t[op].items()},
                     "a_spread_rel": round(spread_a, 4), "d_over_a": round(med["d"] / med["a"], 4), "d_within_a_spread": bool(abs(med["d"] - med["a"]) <= max(t[op]["a"]) - min(t[op]["a"])),
                     "a0_spread_rel": round((max(t[op]["a0"]) - min(t[op]["a0"])) / med["a0"], 4), "d_over_a0": round(med["d"] / med["a0"], 4),
                     "d_within_a0_spread": bool(abs(med["d"] - med["a0"]) <= max(t[op]["a0"]) - min(t[op]["a0"])), "c_minus_a0_us": round(med["c"] - med["a0"], 1),
                     "c_over_b": round(med["c"] / med["b"], 4), "c_below_b": bool(med["c"] < med["b"]), "e_over_a": round(med["e"] / med["a"], 4),
                     "c_minus_a_us": round(med["c"] - med["a"], 1), "w_reading_sweeps": 2 if op == "embed" else 1}
        r["pair_c_over_a"] = round((r["embed"]["us"]["c"] + r["detect"]["us"]["c"]) / (r["embed"]["us"]["a"] + r["detect"]["us"]["a"]), 4)
        configs.append(r)
        print(json.dumps(r), flush=True)
        for e in [batch, plain] + singles:
            e.close()
    if a.trace:
        return
    read2, read5 = float(np.median(mb[2])), float(np.median(mb[5]))
    for r in configs:
        for op in ("embed", "detect"):
            n = r[op]["w_reading_sweeps"]
            for ref in ("a", "a0"):
                r[op]["c_minus_%s_over_pure_read_kind2" % ref] = round(r[op]["c_minus_%s_us" % ref] / (n * read2), 3)
                r[op]["c_minus_%s_over_pure_read_kind5" % ref] = round(r[op]["c_minus_%s_us" % ref] / (n * read5), 3)
    res = {"rows": R, "cols": Cc, "frames": F, "iters": a.iters, "rounds": a.rounds,
           "extra_w_bytes_per_sweep": (F - 1) * plane_bytes,
           "membench_read_us_of_extra_w_bytes": {"kind2": round(read2, 1), "kind5": round(read5, 1), "kind2_rounds": [round(x, 1) for x in mb[2]],
                                                 "kind5_rounds": [round(x, 1) for x in mb[5]]},
           "configs": configs}
    print("SELECT_BENCH " + json.dumps(res), flush=True)
    write(res)
    keys.close()


if __name__ == "__main__":
    main()
