"""Timing of wm_detect_offsets (one image / batch against a rectangle of window offsets into one key) beside what the engine
could do before it: wm_detect_keys on a bank ALREADY FILLED with the same windows copied out (the fill, its copies and the
bank's memory are not charged to that route).  On the GPU box.
usage: python tools/offsets_bench.py [--rows 2160 --cols 3840 --mask 0 --rects 1x4,4x4,8x8,17x17 --frames 1,8 --iters 10
                                      --rounds 5 --max-bank 289] [--json out.json]

For every (ny x nx, F): microseconds per synchronous call (the two routes alternate for --rounds rounds of --iters calls; the
median of the rounds' medians, and their spread), the marginal microseconds per offset (slope against the 1 x 1 call), the
same for the parent route where its bank is at most --max-bank planes, and the bank memory the new call avoids.  wm_membench
kind 2 (pure read) is printed first as the box's read-rate yardstick."""
import argparse
import json

import numpy as np
import torch

import benchlib as bl

wm, synth = bl.load()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--mask", type=int, default=0)
    ap.add_argument("--rects", default="1x4,4x4,8x8,17x17")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-bank", type=int, default=289)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = wm.lib()
    R, Cc, mk = a.rows, a.cols, wm.MASK_TYPE(a.mask)
    nb = 1 << 30
    mean_us, n = bl.membench_us(2, nb, 0.5)
    print(f"wm_membench kind 2 (read, {nb >> 20} MiB): {mean_us:.1f} us/launch = {nb / mean_us / 1e3:.0f} GB/s ({n} launches)")
    print(f"offsets per group (shared key row): {L.wm_detect_offsets_group()}")
    rects = [(1, 1)] + [tuple(int(v) for v in r.split("x")) for r in a.rects.split(",")]
    Fs = [int(v) for v in a.frames.split(",")]
    oy0, ox0 = 5, 9  # (an odd column offset: window bases are 4-byte aligned only)
    KR, KC = R + oy0 + max(r[0] for r in rects), Cc + ox0 + max(r[1] for r in rects) + 3
    keys = wm.KeySet.from_seeds(KR, KC, [1000])
    key_t = torch.from_numpy(keys.plane(0)).cuda()
    plane = R * Cc * 4
    # the parent route's banks: the windows copied out, filled before anything is timed
    banks = {}
    for (ny, nx) in rects:
        if ny * nx <= a.max_bank:
            b = wm.KeySet(R, Cc, ny * nx)
            for i in range(ny):
                for j in range(nx):
                    b.set(i * nx + j, key_t[oy0 + i:oy0 + i + R, ox0 + j:ox0 + j + Cc].contiguous())
            banks[(ny, nx)] = b
    results = []
    for F in Fs:
        xs = torch.stack([torch.from_numpy(synth.synth_frame(R, Cc, frame=f)) for f in range(F)]).cuda()
        eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=F)
        pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
        torch.cuda.synchronize()
        base = {}
        for (ny, nx) in rects:
            K = ny * nx
            out_o = np.zeros(F * K, np.float32)
            out_k = np.zeros(F * K, np.float32)
            new = lambda: eng.detect_offsets_async(pimg, keys, 0, oy0, ox0, ny, nx, mk, wm.WM_SLOT_SYNC, out_o)
            bank = banks.get((ny, nx))
            old = (lambda: eng.detect_keys_async(pimg, bank, mk, wm.WM_SLOT_SYNC, out_k)) if bank is not None else None
            t = bl.alternate({"new": new, "old": old}, a.rounds, a.iters, bl.wall_median_us, warm=3)  # the routes alternate
            tn, to = t["new"], t.get("old", [])
            if old:
                assert np.array_equal(out_o.view(np.uint32), out_k.view(np.uint32)), "the two routes must give the same bits"
            t_new, t_old = bl.median_of_rounds(tn), (bl.median_of_rounds(to) if old else None)
            if K == 1:
                base[F] = (t_new, t_old)
            r = {"ny": ny, "nx": nx, "F": F, "offsets_us": round(t_new, 1), "offsets_us_rounds": [round(v, 1) for v in tn],
                 "offsets_marginal_us": round((t_new - base[F][0]) / (K - 1), 2) if K > 1 else None,
                 "keys_route_us": round(t_old, 1) if old else None, "keys_route_us_rounds": [round(v, 1) for v in to],
                 "keys_route_marginal_us": round((t_old - base[F][1]) / (K - 1), 2) if old and K > 1 else None,
                 "ratio_new_over_keys_route": round(t_new / t_old, 3) if old else None,
                 "bank_bytes_avoided": K * plane}
            results.append(r)
            print(json.dumps(r), flush=True)
        eng.close()
    if a.json:
        bl.write_json(a.json, {"rows": R, "cols": Cc, "mask": a.mask, "key_rows": KR, "key_cols": KC, "group": L.wm_detect_offsets_group(),
                               "membench_read_us": mean_us, "iters": a.iters, "rounds": a.rounds, "results": results})


if __name__ == "__main__":
    main()
