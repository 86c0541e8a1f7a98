"""Timing of the pooled crop search of a clip (wm_clip_pool + wm_locate_pooled: F image-sized passes and ONE transform tail) beside the
route the engine had before it: one batched wm_locate of the F frames with map_dev kept, and the maps summed on the device.  On the
GPU box.
usage: python tools/locate_clip_bench.py [--key 2160x3840 --crop 1600x3000 --at 187,281 --frames 4,16 --iters 3 --rounds 3]
                                         [--nbits 16 --nk 8] [--json profiles/r26_locate_clip_bench.json]

For every (mask, F) the two routes alternate in the same run: microseconds per route including its sync (median of --rounds medians
of --iters repeats), their ratio, and the device span of each.  Both routes must name the true offset.  Then wm_clip_pool alone: the
device span of the call and the Gram sweep's share of it (wm_prof_*); then the pool kernel by itself (wm_clip_pool_bench), by its
LDS tiles and by a direct gather from cache, against wm_membench kind 4 (pure copy) moving the same bytes (F crop planes read, one
written).  Last, wm_locate_bits_pooled and wm_locate_keys_pooled behind one wm_clip_pool against wm_locate_bits and wm_locate_keys
of the F frames."""
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
    ap.add_argument("--frames", default="4,16")
    ap.add_argument("--nbits", type=int, default=16)
    ap.add_argument("--nk", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    (KR, KC), (R, Cc), (oy, ox) = pair(a.key), pair(a.crop), pair(a.at, ",")
    Fs = [int(v) for v in a.frames.split(",")]
    ny, nx, pr, pc = wm.locate_shape(R, Cc, KR, KC)
    print(f"key {KR}x{KC}, crop {R}x{Cc} at ({oy}, {ox}): {ny * nx} offsets, transform {pr} x {pc}")
    bank = wm.KeySet.from_seeds(KR, KC, [4100 + k for k in range(a.nk)])
    tile = 128 if min(KR, KC) >= 256 else 32
    tny, tnx = wm.Watermark.tiles_shape(KR, KC, tile, tile)
    tb = (np.arange(tny * tnx) % a.nbits).astype(np.int32)
    results, pool_alone, tails = [], [], []
    for mask in (0, 1):
        mk = wm.MASK_TYPE(mask)
        emb = wm.Watermark(KR, KC, bank.plane(1), 3, 40.0)
        crops = []
        for f in range(max(Fs)):
            xt = torch.from_numpy(synth.synth_frame(KR, KC, frame=f)).cuda()
            crops.append(emb.makeWatermark(xt, xt, mk)[0][oy:oy + R, ox:ox + Cc].contiguous())
        emb.close()
        for F in Fs:
            eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=F)
            xs = torch.stack(crops[:F])
            pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
            pool = torch.zeros((R, Cc), dtype=torch.float32, device="cuda")
            maps = torch.zeros((F, ny, nx), dtype=torch.float32, device="cuda")
            loc_new, loc_old = np.zeros(4, np.float32), np.zeros((F, 4), np.float32)
            summed = [None]
            torch.cuda.synchronize()

            def new_enqueue():
                eng.pool_clip_async(pimg, mk, 0, pool)
                eng.locate_pooled_async(pool, bank, 1, 0, loc_new)

            def new():
                new_enqueue()
                eng.sync(0)

            def old():
                eng.locate_async(pimg, bank, 1, mk, 0, loc_old, maps)
                eng.sync(0)
                summed[0] = maps.sum(0)
                torch.cuda.synchronize()

            t = bl.alternate({"pooled": new, "per_frame": old}, a.rounds, a.iters, bl.wall_median_us, warm=1)
            spans = {"pooled": bl.device_span_us(eng, new_enqueue, 3),
                     "per_frame": bl.device_span_us(eng, lambda: eng.locate_async(pimg, bank, 1, mk, 0, loc_old, maps), 3)}
            at_old = divmod(int(torch.argmax(summed[0])), nx)
            t_new, t_old = bl.median_of_rounds(t["pooled"]), bl.median_of_rounds(t["per_frame"])
            r = {"mask": mk.name, "F": F, "pooled_us": round(t_new, 1), "pooled_us_rounds": [round(v, 1) for v in t["pooled"]],
                 "per_frame_us": round(t_old, 1), "per_frame_us_rounds": [round(v, 1) for v in t["per_frame"]],
                 "ratio_per_frame_over_pooled": round(t_old / t_new, 2), "device_span_us": {k: round(v, 1) for k, v in spans.items()},
                 "ratio_device_spans": round(spans["per_frame"] / spans["pooled"], 2), "found_pooled": [int(loc_new[0]), int(loc_new[1])],
                 "z_pooled": round(float(loc_new[3]), 1), "found_summed_maps": list(at_old), "z_per_frame": [round(float(z), 1) for z in loc_old[:, 3]],
                 "true": [oy, ox]}
            assert r["found_pooled"] == [oy, ox] and r["found_summed_maps"] == [oy, ox], r
            results.append(r)
            print(json.dumps(r), flush=True)
            # wm_clip_pool alone: the call's device span, the Gram sweep's share, and the rest against a copy of the same bytes
            span = bl.device_span_us(eng, lambda: eng.pool_clip_async(pimg, mk, 0, pool), 5)
            gram = sum(bl.prof_us_per_launch(eng, lambda: (eng.pool_clip_async(pimg, mk, 0, pool), eng.sync(0)), 3).values())
            moved = (F + 1) * R * Cc * 4
            copy_us, _ = bl.membench_us(4, moved // 2, 0.3)
            kern, equal = wm.clip_pool_bench(R, Cc, F, mask, 3, 10)
            assert equal, "the LDS-tile and the direct-gather pool kernels differ"
            pa = {"mask": mk.name, "F": F, "call_span_us": round(span, 1), "gram_sweep_us": round(gram, 1), "span_less_gram_us": round(span - gram, 1),
                  "kernel_lds_tile_us": round(kern["lds_tile"], 1), "kernel_gather_us": round(kern["gather"], 1),
                  "gather_over_lds_tile": round(kern["gather"] / kern["lds_tile"], 2), "bytes_moved": moved,
                  "kernel_lds_tile_GBps": round(moved / kern["lds_tile"] / 1e3), "membench_copy_us": round(copy_us, 1),
                  "membench_copy_GBps": round(moved / copy_us / 1e3), "kernel_lds_tile_over_copy_time": round(kern["lds_tile"] / copy_us, 2)}
            pool_alone.append(pa)
            print(json.dumps(pa), flush=True)
            # the other two tails behind one pooled plane, against the per-frame calls of the F frames
            lb, sb = np.zeros((F, 4), np.float32), np.zeros((F, a.nbits), np.float32)
            lbp, sbp = np.zeros(4, np.float32), np.zeros(a.nbits, np.float32)
            lk, lkp = np.zeros((F, a.nk, 4), np.float32), np.zeros((a.nk, 4), np.float32)

            def bits_new():
                eng.pool_clip_async(pimg, mk, 0, pool)
                eng.locate_bits_pooled_async(pool, bank, 1, tile, tile, tb, a.nbits, 0, lbp, sbp)
                eng.sync(0)

            def bits_old():
                eng.locate_bits_async(pimg, bank, 1, tile, tile, tb, a.nbits, mk, 0, lb, sb)
                eng.sync(0)

            def keys_new():
                eng.pool_clip_async(pimg, mk, 0, pool)
                eng.locate_keys_pooled_async(pool, bank, 0, a.nk, 0, lkp)
                eng.sync(0)

            def keys_old():
                eng.locate_keys_async(pimg, bank, 0, a.nk, mk, 0, lk)
                eng.sync(0)

            t = bl.alternate({"bits_pooled": bits_new, "bits_per_frame": bits_old, "keys_pooled": keys_new, "keys_per_frame": keys_old}, a.rounds, a.iters,
                             bl.wall_median_us, warm=1)
            m = {k: bl.median_of_rounds(v) for k, v in t.items()}
            best = wm.locate_keys_rank(lkp)
            tl = {"mask": mk.name, "F": F, "nbits": a.nbits, "nk": a.nk, **{k + "_us": round(v, 1) for k, v in m.items()},
                  "ratio_bits": round(m["bits_per_frame"] / m["bits_pooled"], 2), "ratio_keys": round(m["keys_per_frame"] / m["keys_pooled"], 2),
                  "keys_pooled_best": int(best[0]), "keys_pooled_z_best": round(float(best[1]), 1), "keys_pooled_z_next": round(float(best[2]), 1)}
            assert tl["keys_pooled_best"] == 1 and (int(lkp[1][0]), int(lkp[1][1])) == (oy, ox), tl
            tails.append(tl)
            print(json.dumps(tl), flush=True)
            eng.close()
    bank.close()
    if a.json:
        bl.write_json(a.json, {"key": [KR, KC], "crop": [R, Cc], "at": [oy, ox], "offsets": ny * nx, "transform": [pr, pc], "iters": a.iters,
                               "rounds": a.rounds, "new_route": "wm_clip_pool + wm_locate_pooled queued on one slot, then wm_sync",
                               "old_route": "one batched wm_locate of the F frames with map_dev kept, wm_sync, the maps summed on the device (torch)",
                               "results": results, "clip_pool_alone": pool_alone, "other_tails": tails})


if __name__ == "__main__":
    main()
