"""Timing of wm_embed_keys (one image marked with every key of a bank in one call) beside its baselines, on the GPU box.
usage: python tools/embed_keys_bench.py [--rows 2160 --cols 3840 --mask 0 --base in --keys 1,2,4,8,16 --iters 20] [--json out.json]

For every K (one f32 frame; --base: in = the input itself, grey = another grey plane, rgb = a planar-RGB plane): microseconds per
synchronous wm_embed_keys call (median), the marginal microseconds per key (slope against K = 1), the per-key plane estimate
(W read by the stats sweep and by every write sweep, y written: 3 planes, 7 for an RGB base whose write sweep runs per channel)
at the box's wm_membench copy rate, the fraction of the 8 TB/s HBM peak the bytes the sweeps move imply, and two baselines over the same keys as K contexts
from wm_create_generated: K synchronous wm_embed calls (one image: the fused single-launch kernels) and K wm_embed calls queued
on one stream followed by one wait.  Last, the round trip: wm_embed_keys, then wm_detect_keys on all K copies; every copy must
score highest at its own key.  wm_membench kinds 1 (copy) and 2 (read) are printed first as the box's yardsticks."""
import argparse
import ctypes as C
import json
import sys

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
    ap.add_argument("--base", choices=("in", "grey", "rgb"), default="in")
    ap.add_argument("--keys", default="1,2,4,8,16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = wm.lib()
    R, Cc, mk = a.rows, a.cols, wm.MASK_TYPE(a.mask)
    nb = 1 << 30
    bench = {}
    for kind, name in ((1, "copy"), (2, "read")):
        mean_us, n = bl.membench_us(kind, nb, 0.5)
        moved = nb * (2 if kind == 1 else 1)
        bench[name] = moved / (mean_us * 1e-6)
        print(f"wm_membench kind {kind} ({name}, {nb >> 20} MiB): {mean_us:.1f} us/launch = {bench[name] / 1e9:.0f} GB/s moved "
              f"({n} launches)", flush=True)
    Ks = [int(v) for v in a.keys.split(",")]
    Kmax = max(Ks)
    seeds = [3000 + 13 * k for k in range(Kmax)]
    bank = {K: wm.KeySet.from_seeds(R, Cc, seeds[:K]) for K in Ks}
    plane = R * Cc * 4
    x = torch.from_numpy(synth.synth_frame(R, Cc, frame=0)).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=Kmax)
    ctxs = [wm.Watermark.generated(R, Cc, seeds[k], 3, 40.0, nslots=1) for k in range(Kmax)]
    stream = torch.cuda.Stream()
    for e in ctxs:
        L.wm_set_stream(e._ctx, 0, C.c_void_p(stream.cuda_stream))
    nch = 3 if a.base == "rgb" else 1
    b = x if a.base == "in" else (x.flip(-1).contiguous() if a.base == "grey" else torch.stack([x, x.flip(-2), x.flip(-1)]).contiguous())
    copies = torch.empty((Kmax,) + tuple(b.shape), device="cuda")
    y = torch.empty_like(b)
    pin, pb, py = wm.plane_of(x), wm.plane_of(b, nch), wm.plane_of(y, nch)
    av = (C.c_float * 1)()
    torch.cuda.synchronize()
    rows = []
    t1 = None
    for K in Ks:
        pout = wm.plane_of(copies[:K], nch)
        aout = np.zeros(K, np.float32)
        t = timed(lambda: eng.embed_keys_async(pin, pb, pout, bank[K], mk, wm.WM_SLOT_SYNC, aout), a.iters)
        if K == 1:
            t1 = t
        marg = (t - t1) / (K - 1) if K > 1 and t1 is not None else None
        # planes the sweeps move: Gram and stats read x (stats: + K W); every write sweep reads x and the base (none when the
        # base is the input) and K W, and writes K y
        key_planes = 1 + 2 * nch
        alg = (2 + nch * (1 if a.base == "in" else 2)) * plane + key_planes * K * plane
        est_key_us = key_planes * plane / bench["copy"] * 1e6

        def sync_calls():
            for e in ctxs[:K]:
                L.wm_embed(e._ctx, int(mk), C.byref(pin), C.byref(pb), C.byref(py), av, None, wm.WM_SLOT_SYNC)

        def queued():
            for e in ctxs[:K]:
                L.wm_embed(e._ctx, int(mk), C.byref(pin), C.byref(pb), C.byref(py), av, None, 0)
            for e in ctxs[:K]:
                L.wm_sync(e._ctx, 0)

        ts = timed(sync_calls, max(3, a.iters // 4))
        tq = timed(queued, max(3, a.iters // 4))
        r = {"K": K, "embed_keys_us": round(t, 1), "marginal_us_per_key": round(marg, 2) if marg is not None else None,
             "key_planes": key_planes, "key_planes_estimate_us": round(est_key_us, 2), "marginal_over_estimate": round(marg / est_key_us, 3) if marg is not None else None,
             "alg_bytes": alg, "frac_of_8TBs": round(alg / (t * 1e-6) / PEAK, 3), "K_sync_embed_us": round(ts, 1),
             "K_queued_embed_us": round(tq, 1), "ratio_vs_queued": round(t / tq, 3)}
        rows.append(r)
        print(json.dumps(r, allow_nan=False), flush=True)
    # round trip: K copies, then every copy against the bank
    K = Kmax
    cp, _ = eng.makeWatermarkKeys(x, b, bank[K], mk)
    s = np.asarray(eng.detectKeys(cp if nch == 1 else cp[:, 0].contiguous(), bank[K], mk)).reshape(K, K)
    hits = int(sum(int(np.argmax(s[k])) == k for k in range(K)))
    margin = min(float(s[k, k]) / max(float(np.abs(np.delete(s[k], k)).max()), 1e-30) for k in range(K)) if K > 1 else None
    rt = {"round_trip_K": K, "identified": hits, "min_own_over_best_other": round(margin, 2) if margin is not None else None}
    print(json.dumps(rt, allow_nan=False), flush=True)
    for e in ctxs:
        e.close()
    eng.close()
    if a.json:
        bl.write_json(a.json, {"rows": R, "cols": Cc, "mask": a.mask, "base": a.base, "membench_bytes_per_s": bench, "results": rows, "round_trip": rt},
                      allow_nan=False)
    if hits != K:
        sys.exit(1)


if __name__ == "__main__":
    main()
