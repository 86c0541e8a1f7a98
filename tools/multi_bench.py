"""Timing of one frame marked for K recipients: K queued wm_embed_signs calls against one wm_embed_signs_multi call.  On the GPU box.
usage: python tools/multi_bench.py [--rows 2160 --cols 3840 --tile 128x128 --copies 1,4,16,64 --masks 0,1 --iters 10 --rounds 5]
                                    [--json out.json]

One process (WM_AB_LIB: another build of the library).  3840 x 2160, fused off, checked hand-over off, p = 3, F = 1; two plane
setups: f32 with a grey base that is another picture, and u8 with the base = the input.  For every (mask, setup, K) the two routes
alternate for --rounds rounds of --iters repeats, each repeat timed by two events on slot 0's stream around everything the route
enqueues (device span: the tables' uploads, the launches and the gaps between them, no host share) and by the host clock around
the route including its wm_sync:
  A  K wm_embed_signs calls queued on the slot, copy k into plane k of the output, then one wm_sync
  B  one wm_embed_signs_multi call with the same K tables into the same planes, then wm_sync
Per route the median of the rounds' medians and the rounds themselves; per copy = that / K; ratio = B / A.  Per (mask, setup) the
slope of B between K = 16 and K = 64 in microseconds per extra copy, beside the time of a pure store of one plane on the same box
(wm_membench kind 0 over rows * cols * 4 bytes, and over the copy's own size for u8): the claim to test is that the slope lies
closer to that store than to A's time per copy."""
import argparse
import json
import os

import numpy as np

import benchlib as bl


def rounds_of(eng, fa, fb, rounds, iters, warm=2):
    """{"A" / "B": (device medians of the rounds, wall medians of the rounds)}, device and wall taken from the same repeats"""
    for _ in range(warm):
        bl.span_and_wall_us(eng, fa)
        bl.span_and_wall_us(eng, fb)

    def medians(fn, n):
        ts = [bl.span_and_wall_us(eng, fn) for _ in range(n)]
        return round(float(np.median([t[0] for t in ts])), 1), round(float(np.median([t[1] for t in ts])), 1)

    return {name: tuple(zip(*r)) for name, r in bl.alternate({"A": fa, "B": fb}, rounds, iters, medians).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--tile", default="128x128")
    ap.add_argument("--copies", default="1,4,16,64")
    ap.add_argument("--masks", default="0,1")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    wm, synth = bl.load()
    R, Cc = a.rows, a.cols
    th, tw = (int(v) for v in a.tile.split("x"))
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    Ks = [int(v) for v in a.copies.split(",")]
    W = synth.synth_watermark(R, Cc)
    xf = synth.synth_frames_torch(R, Cc, 2, "cuda")  # frame 0: the input; frame 1: the grey base of the f32 setup
    store = {"store_plane_f32_us": round(bl.membench_us(0, R * Cc * 4, 0.3)[0], 1), "store_plane_u8_us": round(bl.membench_us(0, R * Cc, 0.3)[0], 1)}
    print(json.dumps(store), flush=True)
    cases, slopes = [], []
    for mask in (int(v) for v in a.masks.split(",")):
        mk = wm.MASK_TYPE(mask)
        for setup in ("f32 grey base", "u8 base = input"):
            u8 = setup.startswith("u8")
            x = xf[0].to(torch.uint8) if u8 else xf[0]
            base = x if u8 else xf[1]
            pin, pbase = wm.plane_of(x, 1), wm.plane_of(base, 1)
            eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=1)
            eng.set_fused(False)
            eng.set_checked_handover(False)
            by_k = {}
            for K in Ks:
                signs = (2 * np.random.default_rng(K).integers(0, 2, (1, K, ny, nx)) - 1).astype(np.int8)
                tables = [np.ascontiguousarray(signs[:, k]) for k in range(K)]
                out = torch.empty((K, R, Cc), dtype=x.dtype, device="cuda")
                pk = [wm.plane_of(out[k], 1) for k in range(K)]
                pall = wm.plane_of(out, 1)

                def route_a():
                    for k in range(K):
                        eng.embed_signs_async(pin, pbase, pk[k], th, tw, tables[k], mk, 0)

                def route_b():
                    eng.embed_signs_multi_async(pin, pbase, pall, th, tw, K, signs, mk, 0)

                torch.cuda.synchronize()
                route_a()
                eng.sync(0)
                ya = out.clone()
                out.zero_()
                torch.cuda.synchronize()  # (clone and zero_ run on torch's stream, the routes on the slot's)
                route_b()
                eng.sync(0)
                same = bool(torch.equal(ya, out))
                del ya
                r = rounds_of(eng, route_a, route_b, a.rounds, a.iters)
                ua, ub = float(np.median(r["A"][0])), float(np.median(r["B"][0]))
                c = {"mask": mk.name, "setup": setup, "K": K, "same_bits": same,
                     "A_device_us": round(ua, 1), "A_device_us_rounds": r["A"][0], "A_wall_us": round(float(np.median(r["A"][1])), 1),
                     "B_device_us": round(ub, 1), "B_device_us_rounds": r["B"][0], "B_wall_us": round(float(np.median(r["B"][1])), 1),
                     "A_us_per_copy": round(ua / K, 2), "B_us_per_copy": round(ub / K, 2), "ratio_B_over_A": round(ub / ua, 3)}
                by_k[K] = c
                cases.append(c)
                print(json.dumps(c), flush=True)
                del out
            if 16 in by_k and 64 in by_k:
                s = {"mask": mk.name, "setup": setup,
                     "B_slope_us_per_copy_16_to_64": round((by_k[64]["B_device_us"] - by_k[16]["B_device_us"]) / 48, 2),
                     "A_us_per_copy_at_64": by_k[64]["A_us_per_copy"],
                     "store_plane_us": store["store_plane_u8_us" if u8 else "store_plane_f32_us"]}
                s["slope_closer_to_store_than_to_A"] = bool(abs(s["B_slope_us_per_copy_16_to_64"] - s["store_plane_us"]) <
                                                            abs(s["B_slope_us_per_copy_16_to_64"] - s["A_us_per_copy_at_64"]))
                slopes.append(s)
                print(json.dumps(s), flush=True)
            eng.close()
    res = {"rows": R, "cols": Cc, "tile": a.tile, "iters": a.iters, "rounds": a.rounds, "group": wm.lib().wm_embed_signs_group(),
           "lib": os.environ.get("WM_AB_LIB") and "WM_AB_LIB" or "tree", **store, "cases": cases, "slopes": slopes}
    print("MULTI_BENCH " + json.dumps(res), flush=True)
    if a.json:
        bl.write_json(a.json, res)


if __name__ == "__main__":
    main()
