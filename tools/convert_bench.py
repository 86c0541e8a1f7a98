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
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_span_us(torch, wm, eng, enqueue, batch, n):
    """median microseconds per call between two events on slot 0's stream around `batch` calls queued back to back"""
    st = torch.cuda.ExternalStream(wm.lib().wm_get_stream(eng._ctx, 0))
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(batch):
            enqueue()
        e1.record(st)
        eng.sync(0)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / batch)
    return float(np.median(ts))


def wall_us(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def membench_gbs(wm, kind, nbytes, seconds=0.2):
    us, n = C.c_double(), C.c_int()
    rc = wm.lib().wm_membench(0, kind, nbytes, seconds, C.byref(us), C.byref(n))
    assert rc == 0, rc
    return 2 * nbytes / us.value * 1e-3  # (a copy reads and writes `nbytes`)


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
    sys.path.insert(0, ROOT)
    wm = importlib.import_module("watermarking-gpu_amd")
    synth = importlib.import_module("watermarking-gpu_amd.synth")
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
    rounds = {k: [] for k in conv}
    mb = {1: [], 4: []}
    for fn in conv.values():
        for _ in range(3):
            fn[1]()
    eng.sync(0)
    for _ in range(a.rounds):
        for kind in mb:
            mb[kind].append(membench_gbs(wm, kind, copy_bytes))
        for k, (_, fn) in conv.items():
            rounds[k].append(device_span_us(torch, wm, eng, fn, a.batch, a.iters))
    copy1, copy4 = float(np.median(mb[1])), float(np.median(mb[4]))
    rates = {}
    for k, (nbytes, _) in conv.items():
        us = float(np.median(rounds[k]))
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

        for _ in range(3):
            device_route()
            host_route()
        td, th = [], []
        for _ in range(a.rounds):
            td.append(wall_us(device_route, a.iters))
            th.append(wall_us(host_route, max(3, a.iters // 4)))
        d_us, h_us = float(np.median(td)), float(np.median(th))
        r = {"mask": mk.name, "device_route_us": round(d_us, 1), "device_route_us_rounds": [round(v, 1) for v in td], "host_route_us": round(h_us, 1),
             "host_route_us_rounds": [round(v, 1) for v in th], "host_over_device": round(h_us / d_us, 1), "corr_device": cd[0], "corr_host": ch[0],
             "same_bits": bool(np.float32(cd[0]).view(np.uint32) == np.float32(ch[0]).view(np.uint32))}
        proto.append(r)
        print(json.dumps(r), flush=True)
    res = {"rows": R, "cols": Cc, "iters": a.iters, "rounds": a.rounds, "batch": a.batch, "membench_copy_GBps": {"kind1": round(copy1, 1), "kind4": round(copy4, 1),
           "kind1_rounds": [round(v, 1) for v in mb[1]], "kind4_rounds": [round(v, 1) for v in mb[4]], "bytes_each_way": copy_bytes},
           "conversions": rates, "protocol": proto}
    print("CONVERT_BENCH " + json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
