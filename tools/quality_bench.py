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
import json

import numpy as np

import benchlib as bl


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
    wm, synth = bl.load()
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
                    # every entry takes its own measurement of a round: the two reads of `nbytes`, then the two spans
                    takes = {k: (lambda n, k=k: bl.membench_us(k, nbytes, 0.15)[0]) for k in (2, 5)}
                    takes.update({k: (lambda n, fn=fn: bl.device_span_us(eng, fn, n, a.batch)) for k, fn in routes.items()})
                    t = bl.alternate(takes, a.rounds, a.iters, lambda take, n: take(n))
                    us, emb, r2, r5 = (bl.median_of_rounds(t[k]) for k in ("quality", "embed", 2, 5))
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
        bl.write_json(a.json, res)
    eng.close()


if __name__ == "__main__":
    main()
