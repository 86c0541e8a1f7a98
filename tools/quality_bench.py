"""Timing of wm_quality (PSNR and SSIM of a marked copy against its base) at 4K.  On the GPU box.
usage: python tools/quality_bench.py [--rows 2160 --cols 3840 --iters 10 --rounds 3 --batch 4] [--json out.json]

One process, the routes alternating in --rounds rounds (tools/convert16_bench.py's scheme).  Device span by events on the slot's stream
around --batch calls queued back to back, per call; the median over --iters spans, then over the rounds.
Configurations: F = 1 and 16 frames, f32 and u8 planes (both planes of one type), 1 and 3 channels, one tile per plane and 128 x 128
tiles.  Beside every wm_quality time, from the same rounds:
  - wm_membench's pure read of the bytes the call reads once (both planes), kind 2 (the sweeps' grid shape) and kind 5 (the shape that
    streams fastest): the read yardstick.  wm_quality is arithmetic-bound by design (f64 throughout), so the ratio says how far;
  - one wm_embed (ME, batched sweeps) of the same frames: in_gray = the first channel of the base, base and out with the call's
    channels -- what checking a copy costs beside making it."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

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


def membench_us(wm, kind, nbytes, seconds=0.15):
    us, n = C.c_double(), C.c_int()
    rc = wm.lib().wm_membench(0, kind, nbytes, seconds, C.byref(us), C.byref(n))
    assert rc == 0, rc
    return us.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    wm = importlib.import_module("watermarking-gpu_amd")
    synth = importlib.import_module("watermarking-gpu_amd.synth")
    R, Cc = a.rows, a.cols
    Fmax = max(a.frames)
    eng = wm.Watermark(R, Cc, synth.synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=Fmax)
    # content does not steer the kernels (no data-dependent branch): one synthetic frame, shifted per plane, and a noisy copy
    frame = torch.from_numpy(synth.synth_frame(R, Cc, frame=1)).cuda()
    g = torch.Generator(device="cuda").manual_seed(7)
    base = torch.stack([torch.stack([torch.roll(frame, (3 * f + c) * 5, 1) for c in range(3)]) for f in range(Fmax)])
    copy = torch.clamp(base + 2.55 * torch.randn(base.shape, generator=g, device="cuda"), 0, 255)
    planes = {"f32": (base, copy), "u8": (base.to(torch.uint8), copy.to(torch.uint8))}
    out = {k: torch.empty_like(v[0]) for k, v in planes.items()}
    torch.cuda.synchronize()
    results = []
    for F in a.frames:
        for kind, es in (("f32", 4), ("u8", 1)):
            for ch in (1, 3):
                x, y, o = (t[:F] if ch == 3 else t[:F, 0] for t in (planes[kind][0], planes[kind][1], out[kind]))
                px, py, po = wm.plane_of(x, ch), wm.plane_of(y, ch), wm.plane_of(o, ch)
                pgray = wm.plane_of(planes[kind][0][:F, 0], 1)
                nbytes = 2 * F * ch * R * Cc * es
                for tile in ((0, 0), (128, 128)):
                    ny, nx = (1, 1) if tile == (0, 0) else wm.Watermark.tiles_shape(R, Cc, *tile)
                    q = np.zeros((F, ch, 3), np.float32)
                    sums = torch.empty((F, ch, ny, nx, 5), dtype=torch.float64, device="cuda")
                    torch.cuda.synchronize()
                    routes = {"quality": lambda: eng.quality_async(px, py, 0, q, tile[0], tile[1], sums),
                              "embed": lambda: eng.embed_async(pgray, px, po, wm.MASK_TYPE.ME, 0)}
                    for fn in routes.values():
                        for _ in range(2):
                            fn()
                    eng.sync(0)
                    t = {k: [] for k in routes}
                    mb = {2: [], 5: []}
                    for _ in range(a.rounds):
                        for k in mb:
                            mb[k].append(membench_us(wm, k, nbytes))
                        for k, fn in routes.items():
                            t[k].append(device_span_us(torch, wm, eng, fn, a.batch, a.iters))
                    us = float(np.median(t["quality"]))
                    emb = float(np.median(t["embed"]))
                    r2, r5 = float(np.median(mb[2])), float(np.median(mb[5]))
                    r = {"frames": F, "dtype": kind, "channels": ch, "tile": list(tile), "quality_us": round(us, 2), "quality_us_rounds": [round(v, 2) for v in t["quality"]],
                         "us_per_plane_pair": round(us / (F * ch), 2), "bytes_read": nbytes, "GBps": round(nbytes / us * 1e-3, 1),
                         "read_kind2_us": round(r2, 2), "read_kind5_us": round(r5, 2), "time_over_read_kind2": round(us / r2, 2), "time_over_read_kind5": round(us / r5, 2),
                         "embed_us": round(emb, 2), "embed_us_rounds": [round(v, 2) for v in t["embed"]], "time_over_embed": round(us / emb, 2),
                         "psnr_first_plane": round(wm.psnr_from_mse(float(q[0, 0, 0])), 3), "ssim_first_plane": round(float(q[0, 0, 1]), 5)}
                    results.append(r)
                    print(json.dumps(r), flush=True)
    res = {"rows": R, "cols": Cc, "iters": a.iters, "rounds": a.rounds, "batch": a.batch, "results": results}
    print("QUALITY_BENCH " + json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
