"""Timing of wm_detect_keys_tiles (the detector's sums kept per tile and per key of a bank) against the two ways the PARENT
build answers the same question or shares the same reads: its wm_detect_keys at the same K and F (the call whose march this one
reuses, with another end), and K queued wm_detect_tiles calls on K engines (what the per-key tile map costs without this call).
On the GPU box.
usage: python tools/keys_tiles_bench.py --parent-lib watermarking-gpu_amd/libwm_ab_parent.so [--rows 2160 --cols 3840
           --tile 128x128 --keys 1,4,16 --frames 1,8 --mask 0 --iters 10 --rounds 5 --reps 3] [--json out.json]

Child processes alternate between the two builds --reps times (tools/ab.py's scheme).  A child of the parent build times
wm_detect_keys and the K queued wm_detect_tiles calls (K engines, one slot each, all enqueued, then every slot synced); a child of
this build times wm_detect_keys_tiles and, as a check that the two builds run alike, its own wm_detect_keys.  Per call: the median
over --rounds rounds of the median of --iters synchronous calls, in microseconds; the ratios are formed from the medians over the
children.  f32 frames.  wm_membench kind 2 (pure read) is printed first as the box's read-rate yardstick.  Without --parent-lib one
process times what this build has."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

import benchlib as bl

ROOT = bl.ROOT
TAG = "KEYS_TILES_BENCH "


def timed(fn, a):
    rounds = bl.alternate({"fn": fn}, a.rounds, a.iters, bl.wall_median_us, warm=3)["fn"]
    return round(bl.median_of_rounds(rounds), 1), [round(v, 1) for v in rounds]


def child(a):
    import torch
    wm, synth = bl.load()
    has_kt = hasattr(wm.lib(), "wm_detect_keys_tiles")  # (an older build, named by WM_AB_LIB, lacks it)
    R, Cc, mk = a.rows, a.cols, wm.MASK_TYPE(a.mask)
    th, tw = (int(v) for v in a.tile.split("x"))
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    res = {"lib": os.path.basename(wm.LIB_PATH), "has_keys_tiles": has_kt, "cases": []}
    if a.membench:
        nb = 1 << 30
        mean_us, _ = bl.membench_us(2, nb, 0.5)
        res["membench_read_us"] = round(mean_us, 1)
        res["membench_read_gbs"] = round(nb / mean_us / 1e3)
    Kmax = max(a.keys)
    seeds = [7100 + k for k in range(Kmax)]
    for F in a.frames:
        xs = synth.synth_frames_torch(R, Cc, F, "cuda", dtype="f32")
        pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
        for K in a.keys:
            kb = wm.KeySet.from_seeds(R, Cc, seeds[:K])
            eng = wm.Watermark.generated(R, Cc, seeds[0], 3, 40.0, nslots=1, max_frames=F)
            corr = np.zeros((F, K), np.float32)
            r = {"K": K, "F": F}
            r["detect_keys_us"], r["detect_keys_us_rounds"] = timed(lambda: eng.detect_keys_async(pimg, kb, mk, wm.WM_SLOT_SYNC, corr), a)
            if has_kt:
                mp = torch.empty((F, K, ny, nx), dtype=torch.float32, device="cuda")
                sm = torch.empty((F, K, ny, nx, 3), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                r["keys_tiles_us"], r["keys_tiles_us_rounds"] = timed(
                    lambda: eng.detect_keys_tiles_async(pimg, kb, th, tw, mk, wm.WM_SLOT_SYNC, mp, sm), a)
            else:
                engs = [wm.Watermark.generated(R, Cc, sd, 3, 40.0, nslots=1, max_frames=F) for sd in seeds[:K]]
                mps = [torch.empty((F, ny, nx), dtype=torch.float32, device="cuda") for _ in engs]
                sms = [torch.empty((F, ny, nx, 3), dtype=torch.float64, device="cuda") for _ in engs]
                torch.cuda.synchronize()

                def queued():
                    for e, m, s in zip(engs, mps, sms):
                        e.detect_tiles_async(pimg, th, tw, mk, 0, m, s)
                    for e in engs:
                        e.sync(0)
                r["queued_tiles_us"], r["queued_tiles_us_rounds"] = timed(queued, a)
                for e in engs:
                    e.close()
            res["cases"].append(r)
            eng.close()
            kb.close()
    print(TAG + json.dumps(res), flush=True)
    return res


def ints(s):
    return [int(v) for v in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--tile", default="128x128")
    ap.add_argument("--keys", type=ints, default=[1, 4, 16])
    ap.add_argument("--frames", type=ints, default=[1, 8])
    ap.add_argument("--mask", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--membench", type=int, default=1)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    meta = {"rows": a.rows, "cols": a.cols, "tile": a.tile, "mask": a.mask, "dtype": "f32", "iters": a.iters, "rounds": a.rounds}
    if a.child or not a.parent_lib:
        res = child(a)
        if a.json and not a.child:
            bl.write_json(a.json, dict(meta, run=res))
        return
    libs = [("parent", os.path.join(ROOT, a.parent_lib) if not os.path.isabs(a.parent_lib) else a.parent_lib), ("this", None)]
    runs = {"parent": [], "this": []}
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--cols", str(a.cols), "--tile", a.tile,
            "--keys", ",".join(map(str, a.keys)), "--frames", ",".join(map(str, a.frames)), "--mask", str(a.mask), "--iters", str(a.iters),
            "--rounds", str(a.rounds)]
    for rep in range(a.reps):
        for name, lib in libs:
            env = dict(os.environ)
            env.pop("WM_AB_LIB", None)
            if lib:
                env["WM_AB_LIB"] = lib
            p = subprocess.run(argv + ["--membench", "1" if rep == 0 and name == "parent" else "0"], cwd=ROOT, env=env, capture_output=True, text=True,
                               timeout=600)
            line = next((l for l in p.stdout.splitlines() if l.startswith(TAG)), None)
            if p.returncode != 0 or line is None:
                sys.exit(f"child ({name}, rep {rep}) failed with {p.returncode}:\n{p.stdout}\n{p.stderr}")
            runs[name].append(json.loads(line[len(TAG):]))
            if rep == 0 and name == "parent":
                print("membench read:", {k: v for k, v in runs[name][-1].items() if k.startswith("membench")}, flush=True)
            key = "queued_tiles_us" if name == "parent" else "keys_tiles_us"
            print(f"== {name} rep {rep}: " + "; ".join(f"K={c['K']} F={c['F']} detect_keys {c['detect_keys_us']} {key[:-3]} {c[key]}"
                                                         for c in runs[name][-1]["cases"]), flush=True)
    summary = []
    med = lambda name, i, key: float(np.median([r["cases"][i][key] for r in runs[name]]))
    for i, c in enumerate(runs["this"][0]["cases"]):
        pk, pq, tk, kt = med("parent", i, "detect_keys_us"), med("parent", i, "queued_tiles_us"), med("this", i, "detect_keys_us"), med("this", i, "keys_tiles_us")
        s = {"K": c["K"], "F": c["F"], "parent_detect_keys_us": round(pk, 1), "parent_queued_tiles_us": round(pq, 1), "this_detect_keys_us": round(tk, 1),
             "keys_tiles_us": round(kt, 1), "keys_tiles_us_reps": [r["cases"][i]["keys_tiles_us"] for r in runs["this"]],
             "ratio_keys_tiles_over_parent_detect_keys": round(kt / pk, 3), "ratio_keys_tiles_over_parent_queued_tiles": round(kt / pq, 3),
             "ratio_this_detect_keys_over_parent_detect_keys": round(tk / pk, 3)}
        summary.append(s)
        print(json.dumps(s), flush=True)
    if a.json:
        bl.write_json(a.json, dict(meta, reps=a.reps, membench={k: v for k, v in runs["parent"][0].items() if k.startswith("membench")}, summary=summary,
                                   runs=runs))


if __name__ == "__main__":
    main()
