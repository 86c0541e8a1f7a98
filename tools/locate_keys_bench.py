"""Timing of wm_locate_keys (a crop against a bank of keys in one call: whose key, and where) beside the route the engine had before
it: nk queued wm_locate calls on the same bank and a sync.  On the GPU box.
usage: python tools/locate_keys_bench.py [--key 2160x3840 --crop 1600x3000 --at 187,281 --nk 16,64 --frames 1,4 --iters 3 --rounds 3]
                                         [--json profiles/r25_locate_keys_bench.json]

For every (mask, F, nk) the two routes alternate in the same run: microseconds per synchronous wm_locate_keys call and per nk queued
wm_locate calls + sync (median of --rounds medians of --iters repeats), their ratio, and the device span of each.  Frame f is marked
with key (3 f + 1) mod nk of the bank; both routes must name that key at the true offset.  Then the seven transform passes
(wm_fft_bench), the three-operand product (wm_locate_bits_bench) and the two passes the new call adds (wm_locate_keys_bench) against
wm_membench kind 4 (pure copy) on the plane's bytes in the same run."""
import argparse
import json

import numpy as np
import torch

import benchlib as bl

wm, synth = bl.load()


def pair(s, sep="x"):
    return tuple(int(v) for v in s.split(sep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key", default="2160x3840")
    ap.add_argument("--crop", default="1600x3000")
    ap.add_argument("--at", default="187,281")
    ap.add_argument("--nk", default="16,64")
    ap.add_argument("--frames", default="1,4")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    (KR, KC), (R, Cc), (oy, ox) = pair(a.key), pair(a.crop), pair(a.at, ",")
    nks, Fs = [int(v) for v in a.nk.split(",")], [int(v) for v in a.frames.split(",")]
    ny, nx, pr, pc = wm.locate_shape(R, Cc, KR, KC)
    print(f"key {KR}x{KC}, crop {R}x{Cc} at ({oy}, {ox}): {ny * nx} offsets, transform {pr} x {pc}")
    # the yardstick and the passes, in the same run
    plane = pr * pc * 8
    copy_us, n = bl.membench_us(4, plane, 0.5)
    print(f"wm_membench kind 4 (copy, {plane >> 20} MiB read + {plane >> 20} MiB written): {copy_us:.1f} us/launch = {2 * plane / copy_us / 1e3:.0f} GB/s ({n} launches)")
    moved = {"product": 3 * plane, "product3": 3 * plane, "keys_pair": 2 * plane, "keys_peak": ny * nx * 16}
    timed = list(wm.fft_bench(pr, pc, 20).items()) + [("product3", wm.locate_bits_bench(pr, pc, ny, nx, 20)["product3"])]
    timed += list(wm.locate_keys_bench(pr, pc, ny, nx, 20).items())
    passes = {}
    for name, us in timed:
        by = moved.get(name, 2 * plane)
        passes[name] = {"us": round(us, 1), "GBps": round(by / us / 1e3), "of_copy_rate": round((by / us) / (2 * plane / copy_us), 3),
                        "of_copy_time": round(us / copy_us, 3)}
        print(f"  {name:16s} {us:8.1f} us  {passes[name]['GBps']:5d} GB/s  {passes[name]['of_copy_rate']:.2f} of the copy rate")
    # the bank, and per mask the frames: frame f marked with key (3 f + 1) mod min(nk) -- an owner inside every key range timed
    NK = max(nks)
    bank = wm.KeySet.from_seeds(KR, KC, [4100 + k for k in range(NK)])
    owners = [(3 * f + 1) % min(nks) for f in range(max(Fs))]
    results = []
    for mask in (0, 1):
        mk = wm.MASK_TYPE(mask)
        crops = []
        for f in range(max(Fs)):
            emb = wm.Watermark(KR, KC, bank.plane(owners[f]), 3, 40.0)
            xt = torch.from_numpy(synth.synth_frame(KR, KC, frame=f)).cuda()
            crops.append(emb.makeWatermark(xt, xt, mk)[0][oy:oy + R, ox:ox + Cc].contiguous())
            emb.close()
        for F in Fs:
            eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=F)
            xs = torch.stack(crops[:F])
            pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
            for nk in nks:
                loc, locs = np.zeros((F, nk, 4), np.float32), np.zeros((nk, F, 4), np.float32)
                torch.cuda.synchronize()

                def new(slot=wm.WM_SLOT_SYNC):
                    eng.locate_keys_async(pimg, bank, 0, nk, mk, slot, loc)

                def old_enqueue():
                    for k in range(nk):
                        eng.locate_async(pimg, bank, k, mk, 0, locs[k])

                def old():
                    old_enqueue()
                    eng.sync(0)

                t = bl.alternate({"locate_keys": new, "locate_per_key": old}, a.rounds, a.iters, bl.wall_median_us, warm=1)
                spans = {"locate_keys": bl.device_span_us(eng, lambda: new(0), 3), "locate_per_key": bl.device_span_us(eng, old_enqueue, 3)}
                ranks = [wm.locate_keys_rank(loc[f]) for f in range(F)]
                found = [(int(loc[f][owners[f]][0]), int(loc[f][owners[f]][1])) for f in range(F)]
                found_old = [(int(locs[owners[f]][f][0]), int(locs[owners[f]][f][1])) for f in range(F)]
                t_new, t_old = bl.median_of_rounds(t["locate_keys"]), bl.median_of_rounds(t["locate_per_key"])
                r = {"mask": mk.name, "F": F, "nk": nk, "locate_keys_us": round(t_new, 1), "locate_keys_us_rounds": [round(v, 1) for v in t["locate_keys"]],
                     "locate_per_key_us": round(t_old, 1), "locate_per_key_us_rounds": [round(v, 1) for v in t["locate_per_key"]],
                     "ratio_per_key_over_locate_keys": round(t_old / t_new, 2),
                     "device_span_us": {k: round(v, 1) for k, v in spans.items()}, "ratio_device_spans": round(spans["locate_per_key"] / spans["locate_keys"], 2),
                     "owners": owners[:F], "ranked_best": [rk[0] for rk in ranks], "z_best": [round(rk[1], 1) for rk in ranks],
                     "z_next": [round(rk[2], 1) for rk in ranks], "found": found, "true": (oy, ox),
                     "largest_z_difference_to_wm_locate": round(float(np.abs(loc[:, :, 3] - locs[:, :, 3].T).max()), 4)}
                assert [rk[0] for rk in ranks] == owners[:F] and all(fd == (oy, ox) for fd in found + found_old), (ranks, found, found_old)
                results.append(r)
                print(json.dumps(r), flush=True)
            eng.close()
    bank.close()
    if a.json:
        bl.write_json(a.json, {"key": [KR, KC], "crop": [R, Cc], "at": [oy, ox], "offsets": ny * nx, "transform": [pr, pc], "plane_bytes": plane,
                               "membench_copy_us": round(copy_us, 1), "membench_copy_GBps": round(2 * plane / copy_us / 1e3), "passes": passes,
                               "iters": a.iters, "rounds": a.rounds,
                               "old_route": "nk queued wm_locate calls on the same bank (records only, no maps), then wm_sync",
                               "results": results})


if __name__ == "__main__":
    main()
