"""Timing of the payload calls beside the calls they share their sweeps with.  On the GPU box.
usage: python tools/bits_bench.py [--rows 2160 --cols 3840 --tile 128x128 --nbits 64 --frames 1,16 --masks 0,1 --iters 20 --rounds 5]
                                   [--json out.json]

One process.  For every (mask, F) on f32 planes the two routes of a pair alternate for --rounds rounds of --iters synchronous
calls (tools/offsets_bench.py's scheme); per call the median of the rounds' medians in microseconds, the rounds themselves (their
spread is the yardstick's noise) and the ratio:
  embed   wm_embed on the batched sweeps (wm_set_fused(0))      against  wm_embed_signs with a random {-1, +1} table per frame
  detect  wm_detect_tiles + a device-to-host copy of its sums   against  wm_detect_bits (--nbits bits, wm_bits_layout's table)
The Gram and stats sweeps of the two embeds are the same launches, so only the last sweep can differ: wm_embed's per-kernel device
times (wm_prof_*) are printed beside the pair to show what share of the call that sweep is (k_embed_signs and k_bits_fold are not
profiling names), and the two embeds are also timed by events on the slot's stream (device span: no host share)."""
import argparse
import ctypes as C
import json

import numpy as np

import benchlib as bl


def pair(a, fa, fb, warm=5):
    """the two routes alternate: (median of a, rounds of a, median of b, rounds of b)"""
    t = bl.alternate({"a": fa, "b": fb}, a.rounds, a.iters, bl.wall_median_us, warm)
    ta, tb = t["a"], t["b"]
    return bl.median_of_rounds(ta), [round(v, 1) for v in ta], bl.median_of_rounds(tb), [round(v, 1) for v in tb]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--tile", default="128x128")
    ap.add_argument("--nbits", type=int, default=64)
    ap.add_argument("--frames", default="1,16")
    ap.add_argument("--masks", default="0,1")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    wm, synth = bl.load()
    kernels_us = lambda eng, fn, n: {k: round(v, 2) for k, v in bl.prof_us_per_launch(eng, fn, n).items()}
    span = lambda eng, enqueue: round(bl.device_span_us(eng, enqueue, a.iters), 1)
    R, Cc = a.rows, a.cols
    th, tw = (int(v) for v in a.tile.split("x"))
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    tile_bit = wm.Watermark.bits_layout(ny, nx, a.nbits, 12345)
    W = synth.synth_watermark(R, Cc)
    cases = []
    for mask in (int(v) for v in a.masks.split(",")):
        mk = wm.MASK_TYPE(mask)
        for F in (int(v) for v in a.frames.split(",")):
            xs = synth.synth_frames_torch(R, Cc, F, "cuda")
            eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
            eng.set_fused(False)
            eng.set_checked_handover(False)  # (the plain k_embed instance: the one k_embed_signs is the twin of)
            pin = wm.plane_of(xs if F > 1 else xs[0], 1)
            ys = torch.empty_like(xs)
            pout = wm.plane_of(ys if F > 1 else ys[0], 1)
            signs = (2 * np.random.default_rng(F).integers(0, 2, (F, ny, nx)) - 1).astype(np.int8)
            av = (C.c_float * F)()
            emb = lambda: eng.embed_async(pin, pin, pout, mk, wm.WM_SLOT_SYNC, av)
            sgn = lambda: eng.embed_signs_async(pin, pin, pout, th, tw, signs, mk, wm.WM_SLOT_SYNC, av)
            torch.cuda.synchronize()
            e_us, e_rounds, s_us, s_rounds = pair(a, emb, sgn)
            r = {"mask": mk.name, "F": F, "embed_us": round(e_us, 1), "embed_us_rounds": e_rounds, "embed_signs_us": round(s_us, 1),
                 "embed_signs_us_rounds": s_rounds, "ratio_signs_over_embed": round(s_us / e_us, 3),
                 "embed_spread": round((max(e_rounds) - min(e_rounds)) / e_us, 3), "embed_kernels_us": kernels_us(eng, emb, 10),
                 "embed_device_span_us": span(eng, lambda: eng.embed_async(pin, pin, pout, mk, 0, av)),
                 "embed_signs_device_span_us": span(eng, lambda: eng.embed_signs_async(pin, pin, pout, th, tw, signs, mk, 0, av))}
            # the detectors read the marked planes
            mp = torch.empty((F, ny, nx), dtype=torch.float32, device="cuda")
            sm = torch.empty((F, ny, nx, 3), dtype=torch.float64, device="cuda")
            host = torch.empty((F, ny, nx, 3), dtype=torch.float64).pin_memory()
            soft = np.zeros((F, a.nbits), np.float32)

            def til():
                eng.detect_tiles_async(pout, th, tw, mk, wm.WM_SLOT_SYNC, mp, sm)
                host.copy_(sm)

            bit = lambda: eng.detect_bits_async(pout, th, tw, tile_bit, a.nbits, mk, wm.WM_SLOT_SYNC, soft)
            payload = np.random.default_rng(100 + F).integers(0, 256, (F, (a.nbits + 7) // 8)).astype(np.uint8)
            eng.embed_bits_async(pin, pin, pout, th, tw, tile_bit, a.nbits, payload, mk, wm.WM_SLOT_SYNC)
            t_us, t_rounds, b_us, b_rounds = pair(a, til, bit)
            r.update(tiles_d2h_us=round(t_us, 1), tiles_d2h_us_rounds=t_rounds, detect_bits_us=round(b_us, 1), detect_bits_us_rounds=b_rounds,
                     ratio_bits_over_tiles_d2h=round(b_us / t_us, 3), min_abs_soft=round(float(np.abs(soft).min()), 4),
                     payload_read_back=bool(np.array_equal(np.packbits(soft > 0, axis=1, bitorder="little"), payload)),
                     detect_bits_kernels_us=kernels_us(eng, bit, 10))
            cases.append(r)
            print(json.dumps(r), flush=True)
            eng.close()
    res = {"rows": R, "cols": Cc, "tile": a.tile, "nbits": a.nbits, "iters": a.iters, "rounds": a.rounds, "dtype": "f32", "cases": cases}
    print("BITS_BENCH " + json.dumps(res), flush=True)
    if a.json:
        bl.write_json(a.json, res)


if __name__ == "__main__":
    main()
