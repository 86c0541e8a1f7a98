"""Timing of the pixel-format front (wm_rgb2gray, wm_unpack_rgb8, wm_pack_rgb8) and of the image protocol built on it.  On the GPU box.
usage: python tools/convert_bench.py [--rows 2160 --cols 3840 --iters 20 --rounds 5 --batch 8] [--json out.json]

One process, the routes alternating in --rounds rounds (tools/bits_bench.py's scheme).
 (a) memory rate of each conversion on device planes: wm_rgb2gray f32 and u8, wm_unpack_rgb8 to f32 planes + grey, wm_pack_rgb8 from
     f32.  Device span by events on the slot's stream around --batch calls queued back to back, per call; bytes moved / time beside
     the pure-copy rate wm_membench reaches on the same box in the same run (kind 1: the sweeps' grid shape, kind 4: the shape that
     streams fastest), and the ratios.
 (b) the image protocol per image under ME and NVF: wm_embed onto the planar f32 RGB base, the grey of the result, wm_detect --
     the device route (wm_rgb2gray, everything queued on one slot, one wm_sync) against the route the sample program took before the
     front existed (wait for the embed, download the planar result, grey in a host loop -- numpy's float32 expression here --,
     upload it, wm_detect); wall-clock microseconds per image, and their ratio.  Both routes must score the same bits."""
import argparse
import ctypes as C
import json

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    wm, synth = bl.load()
    R, Cc = a.rows, a.cols
    N = R * Cc
    eng = wm.Watermark(R, Cc, synth.synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=1)
    rng = np.random.default_rng(15)
    px = torch.from_numpy(rng.integers(0, 256, (R, Cc, 3), dtype=np.uint8)).cuda()
    rgb_f, gray = torch.empty((3, R, Cc), dtype=torch.float32, device="cuda"), torch.empty((R, Cc), dtype=torch.float32, device="cuda")
    rgb_u = torch.empty((3, R, Cc), dtype=torch.uint8, device="cuda")
    px_out = torch.empty_like(px)
    torch.cuda.synchronize()
    eng.unpack_rgb8_async(px, rgb_f, gray, wm.WM_SLOT_SYNC)
    eng.unpack_rgb8_async(px, rgb_u, None, wm.WM_SLOT_SYNC)
    planes = {k: wm.plane_of(t, ch) for k, t, ch in (("rgb_f", rgb_f, 3), ("rgb_u", rgb_u, 3), ("gray", gray, 1))}
    pk_in, pk_out = wm.packed_of(px), wm.packed_of(px_out)
    # (a) bytes moved per call and the call
    conv = {
        "rgb2gray_f32": (16 * N, lambda: eng.rgb2gray_async(planes["rgb_f"], planes["gray"], 0)),
        "rgb2gray_u8": (7 * N, lambda: eng.rgb2gray_async(planes["rgb_u"], planes["gray"], 0)),
        "unpack_rgb8_f32_gray": (19 * N, lambda: eng.unpack_rgb8_async(pk_in, planes["rgb_f"], planes["gray"], 0)),
        "pack_rgb8_f32": (15 * N, lambda: eng.pack_rgb8_async(planes["rgb_f"], pk_out, 0)),
    }
    copy_bytes = 12 * N  # one planar f32 RGB image
    for fn in conv.values():
        for _ in range(3):
            fn[1]()
    eng.sync(0)
    # every entry takes its own measurement of a round: the two copies' GB/s (a copy reads and writes `copy_bytes`), then the spans
    takes = {kind: (lambda n, kind=kind: 2 * copy_bytes / bl.membench_us(kind, copy_bytes, 0.2)[0] * 1e-3) for kind in (1, 4)}
    takes.update({k: (lambda n, fn=fn: bl.device_span_us(eng, fn, n, a.batch)) for k, (_, fn) in conv.items()})
    rounds = bl.alternate(takes, a.rounds, a.iters, lambda take, n: take(n))
    copy1, copy4 = bl.median_of_rounds(rounds[1]), bl.median_of_rounds(rounds[4])
    rates = {}
    for k, (nbytes, _) in conv.items():
        us = bl.median_of_rounds(rounds[k])
        gbs = nbytes / us * 1e-3
        rates[k] = {"us": round(us, 2), "us_rounds": [round(v, 2) for v in rounds[k]], "bytes": nbytes, "GBps": round(gbs, 1),
                    "of_copy_kind1": round(gbs / copy1, 3), "of_copy_kind4": round(gbs / copy4, 3)}
        print(json.dumps({k: rates[k]}), flush=True)
    # (b) the protocol per image
    out = torch.empty_like(rgb_f)
    gray_y = torch.empty_like(gray)
    host_y = torch.empty((3, R, Cc), dtype=torch.float32).pin_memory()
    host_g = torch.empty((R, Cc), dtype=torch.float32).pin_memory()
    w = np.array([0.299, 0.587, 0.114], np.float32)
    pout, pgy = wm.plane_of(out, 3), wm.plane_of(gray_y, 1)
    proto = []
    for mk in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        av, cd, ch = (C.c_float * 1)(), (C.c_float * 1)(), (C.c_float * 1)()

        def device_route():
            eng.embed_async(planes["gray"], planes["rgb_f"], pout, mk, 0, av)
            eng.rgb2gray_async(pout, pgy, 0)
            eng.detect_async(pgy, mk, 0, cd)
            eng.sync(0)

        def host_route():
            eng.embed_async(planes["gray"], planes["rgb_f"], pout, mk, 0, av)
            eng.sync(0)
            host_y.copy_(out)
            y = host_y.numpy()
            np.add(w[0] * y[0] + w[1] * y[1], w[2] * y[2], out=host_g.numpy())
            gray_y.copy_(host_g)
            torch.cuda.current_stream().synchronize()
            eng.detect_async(pgy, mk, 0, ch)
            eng.sync(0)

        t = bl.alternate({"device": device_route, "host": host_route}, a.rounds, a.iters,
                         lambda fn, n: bl.wall_median_us(fn, n if fn is device_route else max(3, n // 4)), warm=3)
        td, th = t["device"], t["host"]
        d_us, h_us = bl.median_of_rounds(td), bl.median_of_rounds(th)
        r = {"mask": mk.name, "device_route_us": round(d_us, 1), "device_route_us_rounds": [round(v, 1) for v in td], "host_route_us": round(h_us, 1),
             "host_route_us_rounds": [round(v, 1) for v in th], "host_over_device": round(h_us / d_us, 1), "corr_device": cd[0], "corr_host": ch[0],
             "same_bits": bool(np.float32(cd[0]).view(np.uint32) == np.float32(ch[0]).view(np.uint32))}
        proto.append(r)
        print(json.dumps(r), flush=True)
    res = {"rows": R, "cols": Cc, "iters": a.iters, "rounds": a.rounds, "batch": a.batch, "membench_copy_GBps": {"kind1": round(copy1, 1), "kind4": round(copy4, 1),
           "kind1_rounds": [round(v, 1) for v in rounds[1]], "kind4_rounds": [round(v, 1) for v in rounds[4]], "bytes_each_way": copy_bytes},
           "conversions": rates, "protocol": proto}
    print("CONVERT_BENCH " + json.dumps(res), flush=True)
    if a.json:
        bl.write_json(a.json, res)
    eng.close()


if __name__ == "__main__":
    main()
