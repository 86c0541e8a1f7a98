"""Timing of wm_locate (the offset of a crop anywhere in its key, by FFT) beside the brute-force route the engine had before it:
wm_detect_offsets over the same admissible offsets in calls of at most 4096 scores.  On the GPU box.
usage: python tools/locate_bench.py [--key 2160x3840 --crop 1600x3000 --frames 1,4 --iters 5 --rounds 3 --sample 6 --full]
                                     [--json profiles/r23_locate_bench.json]

For every (mask, F): microseconds per synchronous wm_locate call (median of --rounds medians of --iters calls) and the device span
of the call; the brute-force route as a SAMPLE of --sample wm_detect_offsets calls (rectangles of 4096 / F offsets spread over the
admissible region) whose median is scaled to the number of calls the whole region
takes -- labelled "sampled"; --full runs every call instead.  Then the seven transform passes of one frame (wm_fft_bench) against
wm_membench kind 4 (pure copy) on the plane's bytes in the same run: the fraction of the copy rate each pass reaches."""
import argparse
import json

import numpy as np
import torch

import benchlib as bl

wm, synth = bl.load()


def shape(s):
    return tuple(int(v) for v in s.split("x"))


def brute_calls(ny, nx, per_call):
    """the rectangles (oy0, ox0, h, w) of at most per_call offsets that tile the ny x nx admissible region"""
    h = max(1, min(ny, int(np.sqrt(per_call))))
    w = max(1, min(nx, per_call // h))
    return [(oy, ox, min(h, ny - oy), min(w, nx - ox)) for oy in range(0, ny, h) for ox in range(0, nx, w)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key", default="2160x3840")
    ap.add_argument("--crop", default="1600x3000")
    ap.add_argument("--frames", default="1,4")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    (KR, KC), (R, Cc) = shape(a.key), shape(a.crop)
    ny, nx, pr, pc = wm.locate_shape(R, Cc, KR, KC)
    oy, ox = ny // 3, (nx // 3) | 1
    print(f"key {KR}x{KC}, crop {R}x{Cc} at ({oy}, {ox}): {ny} x {nx} = {ny * nx} admissible offsets, transform {pr} x {pc}")
    # the yardstick and the passes, in the same run
    plane = pr * pc * 8
    copy_us, n = bl.membench_us(4, plane, 0.5)
    print(f"wm_membench kind 4 (copy, {plane >> 20} MiB read + {plane >> 20} MiB written): {copy_us:.1f} us/launch = {2 * plane / copy_us / 1e3:.0f} GB/s ({n} launches)")
    passes = {}
    for name, us in wm.fft_bench(pr, pc, 20).items():
        moved = 3 * plane if name == "product" else 2 * plane
        passes[name] = {"us": round(us, 1), "GBps": round(moved / us / 1e3), "of_copy_rate": round((moved / us) / (2 * plane / copy_us), 3)}
        print(f"  {name:16s} {us:8.1f} us  {passes[name]['GBps']:5d} GB/s  {passes[name]['of_copy_rate']:.2f} of the copy rate")
    # a marked 4K frame, cropped
    keys = wm.KeySet.from_seeds(KR, KC, [2300])
    results = []
    for F in [int(v) for v in a.frames.split(",")]:
        eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=F)
        calls = brute_calls(ny, nx, 4096 // F)
        for mask in (0, 1):
            mk = wm.MASK_TYPE(mask)
            emb = wm.Watermark.generated(KR, KC, 2300, 3, 40.0)
            crops = []
            for f in range(F):
                xt = torch.from_numpy(synth.synth_frame(KR, KC, frame=f)).cuda()
                crops.append(emb.makeWatermark(xt, xt, mk)[0][oy:oy + R, ox:ox + Cc].contiguous())
            emb.close()
            xs = torch.stack(crops)
            pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
            torch.cuda.synchronize()
            loc = np.zeros((F, 4), np.float32)
            fn = lambda: eng.locate_async(pimg, keys, 0, mk, wm.WM_SLOT_SYNC, loc)
            t = bl.alternate({"locate": fn}, a.rounds, a.iters, bl.wall_median_us, warm=2)["locate"]
            span = bl.device_span_us(eng, lambda: eng.locate_async(pimg, keys, 0, mk, 0, loc), 3)
            found = [(int(l[0]), int(l[1])) for l in loc]
            # the brute-force route: every call, or a sample of the full-sized ones spread over the region
            full = [c for c in calls if c[2] * c[3] == calls[0][2] * calls[0][3]]
            picked = calls if a.full else [full[(i * len(full)) // a.sample] for i in range(a.sample)]
            ts = []
            for (oy0, ox0, h, w) in picked:
                out = np.zeros(F * h * w, np.float32)
                ts.append(bl.wall_median_us(lambda: eng.detect_offsets_async(pimg, keys, 0, oy0, ox0, h, w, mk, wm.WM_SLOT_SYNC, out), 1,
                                            warmup=0 if a.full else 1))
            brute = float(np.sum(ts)) if a.full else float(np.median(ts)) * len(full) + float(np.median(ts)) * sum(
                c[2] * c[3] for c in calls if c not in full) / (full[0][2] * full[0][3])
            r = {"mask": mk.name, "F": F, "locate_us": round(bl.median_of_rounds(t), 1), "locate_us_rounds": [round(v, 1) for v in t],
                 "locate_device_span_us": round(span, 1), "found": found, "true": (oy, ox), "z": [round(float(l[3]), 1) for l in loc],
                 "brute_force_us": round(brute, 1), "brute_force": "every call" if a.full else f"sampled: median of {len(picked)} of {len(calls)} calls, scaled",
                 "brute_force_calls": len(calls), "brute_force_call_us": [round(v, 1) for v in ts] if not a.full else None,
                 "ratio_brute_over_locate": round(brute / bl.median_of_rounds(t), 1)}
            assert all(fd == (oy, ox) for fd in found), found
            results.append(r)
            print(json.dumps(r), flush=True)
        eng.close()
    if a.json:
        bl.write_json(a.json, {"key": [KR, KC], "crop": [R, Cc], "offsets": ny * nx, "transform": [pr, pc], "plane_bytes": plane,
                               "membench_copy_us": round(copy_us, 1), "membench_copy_GBps": round(2 * plane / copy_us / 1e3),
                               "passes": passes, "iters": a.iters, "rounds": a.rounds, "results": results})


if __name__ == "__main__":
    main()
