"""Timing of the 9- to 16-bit front (wm_unpack16, wm_pack16, wm_embed16) at 4K.  On the GPU box.
usage: python tools/convert16_bench.py [--rows 2160 --cols 3840 --bits 10 --iters 20 --rounds 5 --batch 8] [--json out.json]

One process, the routes alternating in --rounds rounds (tools/convert_bench.py's scheme).  Device span by events on the slot's stream
around --batch calls queued back to back, per call.
 (a) wm_unpack16 (u16 -> f32) and wm_pack16 (f32 -> u16) on device planes: each moves 6 N bytes (2 N on the u16 side, 4 N on the f32
     side).  Beside them, in the same rounds, wm_membench's pure copy of the same byte count (3 N read + 3 N written), kind 1 (the
     sweeps' grid shape) and kind 4 (the shape that streams fastest).  Reported: each call's time divided by the copy's time.
     The timed calls are queued behind a plug of eight NVF embeds (about 280 us of device work), so that they wait in the queue
     when the device reaches them; the unplugged span is reported beside it (the two agreeing says the host kept up).
 (b) wm_embed16 on a device u16 plane (out of place and in place), the three explicit calls (wm_unpack16, wm_embed, wm_pack16 on
     caller-owned f32 planes), and wm_embed alone on the f32 planes of the same frame, all queued on the slot (the batched sweeps,
     never the fused kernels), ME and NVF.  wm_embed16 minus wm_embed is what the two conversions cost; the two routes must give the
     same bytes."""
import argparse
import json

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    wm, synth = bl.load()
    R, Cc, bits = a.rows, a.cols, a.bits
    N = R * Cc
    eng = wm.Watermark(R, Cc, synth.synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=1)
    k_in, k_out = wm.depth_scale(bits)
    frame = synth.synth_frame(R, Cc, frame=1)
    v_host = np.rint(np.clip(frame * np.float32(k_out), 0, (1 << bits) - 1)).astype(np.uint16)
    v = torch.from_numpy(v_host.view(np.int16)).cuda()
    out16, inplace16 = torch.empty_like(v), torch.empty_like(v)
    X, Y = torch.empty((R, Cc), dtype=torch.float32, device="cuda"), torch.empty((R, Cc), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pv, pout, pin, pX, pY = (wm.plane_any(t) for t in (v, out16, inplace16, X, Y))
    eng.unpack16_async(pv, bits, pX, wm.WM_SLOT_SYNC)

    # (a) the two conversions beside a copy of the same bytes
    conv = {"unpack16": lambda: eng.unpack16_async(pv, bits, pX, 0), "pack16": lambda: eng.pack16_async(pX, pout, bits, 0)}
    moved = 6 * N

    def plug():
        for _ in range(8):
            eng.embed_async(pX, pX, pY, wm.MASK_TYPE.NVF, 0)
    for fn in conv.values():
        for _ in range(3):
            fn()
    eng.sync(0)
    # every entry takes its own measurement of a round: the two copies (`moved // 2` read and as much written), then per conversion
    # the plugged span and the unplugged one
    takes = {kind: (lambda n, kind=kind: bl.membench_us(kind, moved // 2, 0.2)[0]) for kind in (1, 4)}
    for k, fn in conv.items():
        takes[k] = lambda n, fn=fn: bl.device_span_us(eng, fn, n, a.batch, plug)
        takes[k, "unplugged"] = lambda n, fn=fn: bl.device_span_us(eng, fn, n, a.batch)
    rounds = bl.alternate(takes, a.rounds, a.iters, lambda take, n: take(n))
    copy1, copy4 = bl.median_of_rounds(rounds[1]), bl.median_of_rounds(rounds[4])
    rates = {}
    for k in conv:
        us = bl.median_of_rounds(rounds[k])
        rates[k] = {"us": round(us, 2), "us_rounds": [round(t, 2) for t in rounds[k]], "us_unplugged": round(bl.median_of_rounds(rounds[k, "unplugged"]), 2), "bytes": moved, "GBps": round(moved / us * 1e-3, 1),
                    "time_over_copy_kind1": round(us / copy1, 3), "time_over_copy_kind4": round(us / copy4, 3)}
        print(json.dumps({k: rates[k]}), flush=True)

    # (b) the video call against its parts and against the embed alone
    embeds = []
    for mk in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        def three_calls():
            eng.unpack16_async(pv, bits, pX, 0)
            eng.embed_async(pX, pX, pY, mk, 0)
            eng.pack16_async(pY, pout, bits, 0)

        def reset_inplace():
            inplace16.copy_(v)
            torch.cuda.synchronize()

        routes = {
            "embed16": lambda: eng.embed16_async(pv, pout, bits, mk, 0),
            "embed16_inplace": lambda: eng.embed16_async(pin, pin, bits, mk, 0),
            "three_calls": three_calls,
            "embed_f32": lambda: eng.embed_async(pX, pX, pY, mk, 0),
        }
        eng.unpack16_async(pv, bits, pX, wm.WM_SLOT_SYNC)
        three_calls()
        eng.sync(0)
        want = out16.clone()
        out16.zero_()
        routes["embed16"]()
        eng.sync(0)
        same = bool(torch.equal(out16, want))
        reset_inplace()
        for fn in routes.values():
            for _ in range(3):
                fn()
        eng.sync(0)

        def span(fn, n):
            if fn is routes["embed16_inplace"]:
                reset_inplace()  # (the frame is marked again and again within a span: the time does not depend on it)
            return bl.device_span_us(eng, fn, n, a.batch)

        t = bl.alternate(routes, a.rounds, a.iters, span)
        med = {k: bl.median_of_rounds(ts) for k, ts in t.items()}
        r = {"mask": mk.name, "same_bytes_as_three_calls": same}
        for k in routes:
            r[k + "_us"] = round(med[k], 2)
            r[k + "_us_rounds"] = [round(x, 2) for x in t[k]]
        r["embed16_minus_embed_f32_us"] = round(med["embed16"] - med["embed_f32"], 2)
        r["embed16_over_embed_f32"] = round(med["embed16"] / med["embed_f32"], 3)
        embeds.append(r)
        print(json.dumps(r), flush=True)
    res = {"rows": R, "cols": Cc, "bits": bits, "iters": a.iters, "rounds": a.rounds, "batch": a.batch,
           "membench_copy_us": {"kind1": round(copy1, 2), "kind4": round(copy4, 2), "kind1_rounds": [round(x, 2) for x in rounds[1]],
                                "kind4_rounds": [round(x, 2) for x in rounds[4]], "bytes_read_plus_written": moved},
           "conversions": rates, "embed": embeds}
    print("CONVERT16_BENCH " + json.dumps(res), flush=True)
    if a.json:
        bl.write_json(a.json, res)
    eng.close()


if __name__ == "__main__":
    main()
