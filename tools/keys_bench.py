"""Timing of wm_detect_keys (one image / batch against a bank of K keys) beside its baselines, on the GPU box.
usage: python tools/keys_bench.py [--rows 2160 --cols 3840 --mask 0 --keys 1,4,16,64 --frames 1,8 --iters 20] [--json out.json]

For every (K, F): microseconds per synchronous wm_detect_keys call (median), the marginal microseconds per key (slope against
K = 1), the fraction of the 8 TB/s HBM peak the algorithmic bytes imply (x read twice -- Gram sweep and key sweep -- and every
key plane once per call), and two baselines over the same keys as K contexts from wm_create_generated: K synchronous
wm_detect calls (one image: the fused single-launch kernels) and K wm_detect calls queued on one stream followed by one wait.
wm_membench kind 2 (pure read) is printed first as the box's read-rate yardstick."""
import argparse
import ctypes as C
import json

import numpy as np
import torch

import benchlib as bl

wm, synth = bl.load()
PEAK = 8.0e12


def timed(fn, iters):
    return bl.wall_median_us(fn, iters, warmup=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--mask", type=int, default=0)
    ap.add_argument("--keys", default="1,4,16,64")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = wm.lib()
    R, Cc, mk = a.rows, a.cols, wm.MASK_TYPE(a.mask)
    nb = 1 << 30
    mean_us, n = bl.membench_us(2, nb, 0.5)
    print(f"wm_membench kind 2 (read, {nb >> 20} MiB): {mean_us:.1f} us/launch = {nb / mean_us / 1e3:.0f} GB/s ({n} launches)")
    Ks = [int(v) for v in a.keys.split(",")]
    Fs = [int(v) for v in a.frames.split(",")]
    seeds = [1000 + 17 * k for k in range(max(Ks))]
    bank = {K: wm.KeySet.from_seeds(R, Cc, seeds[:K]) for K in Ks}
    plane = R * Cc * 4
    rows = []
    for F in Fs:
        xs = torch.stack([torch.from_numpy(synth.synth_frame(R, Cc, frame=f)) for f in range(F)]).cuda()
        x = xs if F > 1 else xs[0]
        eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=F)
        ctxs = [wm.Watermark.generated(R, Cc, seeds[k], 3, 40.0, nslots=1, max_frames=F) for k in range(max(Ks))]
        stream = torch.cuda.Stream()
        for e in ctxs:
            L.wm_set_stream(e._ctx, 0, C.c_void_p(stream.cuda_stream))
        pimg = wm.plane_of(x, 1)
        corr = (C.c_float * F)()
        torch.cuda.synchronize()
        t1 = None
        for K in Ks:
            out = np.zeros(F * K, np.float32)
            t = timed(lambda: eng.detect_keys_async(pimg, bank[K], mk, wm.WM_SLOT_SYNC, out), a.iters)
            if K == 1:
                t1 = t
            marg = (t - t1) / (K - 1) if K > 1 and t1 is not None else float("nan")
            alg = 2 * F * plane + K * plane
            frac = alg / (t * 1e-6) / PEAK

            def sync_calls():
                for e in ctxs[:K]:
                    L.wm_detect(e._ctx, int(mk), C.byref(pimg), corr, None, wm.WM_SLOT_SYNC)

            def queued():
                for e in ctxs[:K]:
                    L.wm_detect(e._ctx, int(mk), C.byref(pimg), corr, None, 0)
                for e in ctxs[:K]:
                    L.wm_sync(e._ctx, 0)

            ts = timed(sync_calls, max(3, a.iters // 4))
            tq = timed(queued, max(3, a.iters // 4))
            r = {"K": K, "F": F, "detect_keys_us": round(t, 1), "marginal_us_per_key": round(marg, 2), "alg_bytes": alg,
                 "frac_of_8TBs": round(frac, 3), "K_sync_detect_us": round(ts, 1), "K_queued_detect_us": round(tq, 1),
                 "ratio_vs_queued": round(t / tq, 3)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        for e in ctxs:
            e.close()
        eng.close()
    if a.json:
        bl.write_json(a.json, {"rows": R, "cols": Cc, "mask": a.mask, "membench_read_us": mean_us, "results": rows})


if __name__ == "__main__":
    main()
