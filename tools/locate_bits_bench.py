"""Timing of wm_locate_bits (a payload-marked crop found and read in one call) beside the route the engine had before it: a bank
pre-filled with the nbits masked keys, one queued wm_locate call per bit with its map kept, and a sync (the host's combination of the
maps is NOT counted: the old route is timed at its best).  On the GPU box.
usage: python tools/locate_bits_bench.py [--key 2160x3840 --crop 1600x3000 --at 187,281 --tile 128x128 --bits 64 --frames 1,4
                                          --iters 3 --rounds 3] [--json profiles/r24_locate_bits_bench.json]

For every (mask, F) the two routes alternate in the same run: microseconds per synchronous wm_locate_bits call and per nbits queued
wm_locate calls + sync (median of --rounds medians of --iters repeats), their ratio, and the device span of each.  Then the seven
transform passes (wm_fft_bench) and the three passes the new call adds (wm_locate_bits_bench) against wm_membench kind 4 (pure copy)
on the plane's bytes in the same run."""
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
    ap.add_argument("--tile", default="128x128")
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--frames", default="1,4")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    (KR, KC), (R, Cc), (oy, ox), (th, tw), nbits = pair(a.key), pair(a.crop), pair(a.at, ","), pair(a.tile), a.bits
    ny, nx, pr, pc = wm.locate_shape(R, Cc, KR, KC)
    tny, tnx = wm.Watermark.tiles_shape(KR, KC, th, tw)
    tb = wm.Watermark.bits_layout(tny, tnx, nbits, 5)
    cover = wm.locate_bits_cover(R, Cc, KR, KC, th, tw, tb, nbits, oy, ox)
    print(f"key {KR}x{KC}, crop {R}x{Cc} at ({oy}, {ox}): {ny * nx} offsets, transform {pr} x {pc}, {tny} x {tnx} tiles, {nbits} bits, "
          f"least cover {int(cover.min())} px")
    # the yardstick and the passes, in the same run
    plane = pr * pc * 8
    copy_us, n = bl.membench_us(4, plane, 0.5)
    print(f"wm_membench kind 4 (copy, {plane >> 20} MiB read + {plane >> 20} MiB written): {copy_us:.1f} us/launch = {2 * plane / copy_us / 1e3:.0f} GB/s ({n} launches)")
    moved = {"product": 3 * plane, "key_pair": plane + pr * pc * 4, "product3": 3 * plane, "accumulate": ny * nx * 24}
    passes = {}
    for name, us in list(wm.fft_bench(pr, pc, 20).items()) + list(wm.locate_bits_bench(pr, pc, ny, nx, 20).items()):
        by = moved.get(name, 2 * plane)
        passes[name] = {"us": round(us, 1), "GBps": round(by / us / 1e3), "of_copy_rate": round((by / us) / (2 * plane / copy_us), 3),
                        "of_copy_time": round(us / copy_us, 3)}
        print(f"  {name:16s} {us:8.1f} us  {passes[name]['GBps']:5d} GB/s  {passes[name]['of_copy_rate']:.2f} of the copy rate")
    # the bank: the nbits masked keys, then the key itself
    key = synth.synth_watermark(KR, KC, seed=2300)
    tile = np.minimum(np.arange(KR) // th, tny - 1)[:, None] * tnx + np.minimum(np.arange(KC) // tw, tnx - 1)[None, :]
    bank = wm.KeySet(KR, KC, nbits + 1)
    for b in range(nbits):
        bank.set(b, np.where(tb[tile] == b, key, np.float32(0)).astype(np.float32))
    bank.set(nbits, key)
    results = []
    for F in [int(v) for v in a.frames.split(",")]:
        eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=1, max_frames=F)
        for mask in (0, 1):
            mk = wm.MASK_TYPE(mask)
            emb = wm.Watermark(KR, KC, key, 3, 40.0)
            crops, payloads = [], []
            for f in range(F):
                xt = torch.from_numpy(synth.synth_frame(KR, KC, frame=f)).cuda()
                bits = np.random.default_rng(f).permutation(np.arange(nbits) % 2 == 1)
                y = emb.makeWatermarkBits(xt, xt, th, tw, tb, nbits, np.packbits(bits, bitorder="little").tobytes(), mk)[0]
                crops.append(y[oy:oy + R, ox:ox + Cc].contiguous())
                payloads.append(bits)
            emb.close()
            xs = torch.stack(crops)
            pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
            loc, soft = np.zeros((F, 4), np.float32), np.zeros((F, nbits), np.float32)
            locs = np.zeros((nbits, F, 4), np.float32)
            maps = torch.empty((nbits, F, ny, nx), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def new(slot=wm.WM_SLOT_SYNC):
                eng.locate_bits_async(pimg, bank, nbits, th, tw, tb, nbits, mk, slot, loc, soft)

            def old_enqueue():
                for b in range(nbits):
                    eng.locate_async(pimg, bank, b, mk, 0, locs[b], maps[b])

            def old():
                old_enqueue()
                eng.sync(0)

            t = bl.alternate({"locate_bits": new, "locate_per_bit": old}, a.rounds, a.iters, bl.wall_median_us, warm=1)
            spans = {"locate_bits": bl.device_span_us(eng, lambda: new(0), 3), "locate_per_bit": bl.device_span_us(eng, old_enqueue, 3)}
            found = [(int(l[0]), int(l[1])) for l in loc]
            wrong = [int(((soft[f] > 0) != payloads[f])[cover >= 512].sum()) for f in range(F)]
            t_new, t_old = bl.median_of_rounds(t["locate_bits"]), bl.median_of_rounds(t["locate_per_bit"])
            r = {"mask": mk.name, "F": F, "locate_bits_us": round(t_new, 1), "locate_bits_us_rounds": [round(v, 1) for v in t["locate_bits"]],
                 "locate_per_bit_us": round(t_old, 1), "locate_per_bit_us_rounds": [round(v, 1) for v in t["locate_per_bit"]],
                 "ratio_per_bit_over_locate_bits": round(t_old / t_new, 2),
                 "device_span_us": {k: round(v, 1) for k, v in spans.items()}, "ratio_device_spans": round(spans["locate_per_bit"] / spans["locate_bits"], 2),
                 "found": found, "true": (oy, ox), "z": [round(float(l[3]), 1) for l in loc], "bit_errors_on_covered_bits": wrong,
                 "weakest_covered_soft": round(float(np.abs(soft[:, cover >= 512]).min()), 2)}
            assert all(fd == (oy, ox) for fd in found) and not any(wrong), (found, wrong)
            results.append(r)
            print(json.dumps(r), flush=True)
        eng.close()
    bank.close()
    if a.json:
        bl.write_json(a.json, {"key": [KR, KC], "crop": [R, Cc], "at": [oy, ox], "tile": [th, tw], "bits": nbits, "offsets": ny * nx,
                               "transform": [pr, pc], "plane_bytes": plane, "membench_copy_us": round(copy_us, 1),
                               "membench_copy_GBps": round(2 * plane / copy_us / 1e3), "passes": passes, "iters": a.iters, "rounds": a.rounds,
                               "old_route": "nbits queued wm_locate calls with their maps kept on a bank of masked keys, then wm_sync; the host's combination not counted",
                               "results": results})


if __name__ == "__main__":
    main()
