"""Timing of wm_detect_tiles (the detector's sums kept per tile) beside wm_detect on the batched sweeps (wm_set_fused(0)), the
call it shares every read with.  On the GPU box.
usage: python tools/tiles_bench.py [--rows 2160 --cols 3840 --tile 128x128 --cases f32:16,f32:1,u8:16 --mask 0 --iters 20
                                    --rounds 5] [--parent-lib watermarking-gpu_amd/libwm_ab_parent.so --reps 3] [--json out.json]

One process (the default): for every case (dtype:F) wm_detect and wm_detect_tiles alternate for --rounds rounds of --iters
synchronous calls; per call the median of the rounds' medians in microseconds, their spread, the ratio, and the per-kernel
device times (wm_prof_*: k_gram, k_detect, k_detect_tiles, k_tiles_fold) of a profiled pass behind the timed ones.
--parent-lib: the yardstick is ANOTHER build's wm_detect (the parent commit's library): child processes alternate between
the two builds --reps times (tools/ab.py's scheme), each child timing what its build has; the ratios are formed from the
medians over the children.  wm_membench kind 2 (pure read) is printed first as the box's read-rate yardstick."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import benchlib as bl

ROOT = bl.ROOT


def kernels_us(eng, fn, n):
    return {k: round(v, 2) for k, v in bl.prof_us_per_launch(eng, fn, n).items()}


def child(a):
    import torch
    wm, synth = bl.load()
    has_tiles = hasattr(wm.lib(), "wm_detect_tiles")  # (an older build, named by WM_AB_LIB, lacks it)
    R, Cc, mk = a.rows, a.cols, wm.MASK_TYPE(a.mask)
    th, tw = (int(v) for v in a.tile.split("x"))
    res = {"lib": os.path.basename(wm.LIB_PATH), "has_tiles": has_tiles, "cases": []}
    if a.membench:
        nb = 1 << 30
        mean_us, _ = bl.membench_us(2, nb, 0.5)
        res["membench_read_us"] = round(mean_us, 1)
        res["membench_read_gbs"] = round(nb / mean_us / 1e3)
    W = synth.synth_watermark(R, Cc)
    for case in a.cases.split(","):
        dt, F = case.split(":")
        F = int(F)
        xs = synth.synth_frames_torch(R, Cc, F, "cuda", dtype=dt)
        eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
        eng.set_fused(False)
        pimg = wm.plane_of(xs if F > 1 else xs[0], 1)
        corr = (C.c_float * F)()
        det = lambda: eng.detect_async(pimg, mk, wm.WM_SLOT_SYNC, corr)
        til = None
        if has_tiles:
            ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
            mp = torch.empty((F, ny, nx), dtype=torch.float32, device="cuda")
            sm = torch.empty((F, ny, nx, 3), dtype=torch.float64, device="cuda")
            til = lambda: eng.detect_tiles_async(pimg, th, tw, mk, wm.WM_SLOT_SYNC, mp, sm)
        torch.cuda.synchronize()
        t = bl.alternate({"det": det, "til": til}, a.rounds, a.iters, bl.wall_median_us, warm=5)  # the two calls alternate
        td, tt = t["det"], t.get("til")
        r = {"dtype": dt, "F": F, "detect_us": round(float(np.median(td)), 1), "detect_us_rounds": [round(v, 1) for v in td],
             "detect_kernels_us": kernels_us(eng, det, 10)}
        if til:
            r.update(tiles_us=round(float(np.median(tt)), 1), tiles_us_rounds=[round(v, 1) for v in tt],
                     ratio_tiles_over_detect=round(float(np.median(tt)) / float(np.median(td)), 3), tiles_kernels_us=kernels_us(eng, til, 10))
        res["cases"].append(r)
        eng.close()
    print("TILES_BENCH " + json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--tile", default="128x128")
    ap.add_argument("--cases", default="f32:16,f32:1,u8:16")
    ap.add_argument("--mask", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--membench", type=int, default=1)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child or not a.parent_lib:
        res = child(a)
        if a.json and not a.child:
            bl.write_json(a.json, {"rows": a.rows, "cols": a.cols, "tile": a.tile, "mask": a.mask, "iters": a.iters, "rounds": a.rounds, "run": res})
        return
    # alternating child processes: the parent build (its wm_detect is the yardstick), then this build
    libs = [("parent", os.path.join(ROOT, a.parent_lib) if not os.path.isabs(a.parent_lib) else a.parent_lib), ("this", None)]
    runs = {"parent": [], "this": []}
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--cols", str(a.cols), "--tile", a.tile, "--cases", a.cases,
            "--mask", str(a.mask), "--iters", str(a.iters), "--rounds", str(a.rounds)]
    for rep in range(a.reps):
        for name, lib in libs:
            env = dict(os.environ)
            env.pop("WM_AB_LIB", None)
            if lib:
                env["WM_AB_LIB"] = lib
            p = subprocess.run(argv + ["--membench", "1" if rep == 0 and name == "parent" else "0"], cwd=ROOT, env=env, capture_output=True, text=True,
                               timeout=600)
            line = next((l for l in p.stdout.splitlines() if l.startswith("TILES_BENCH ")), None)
            if p.returncode != 0 or line is None:
                sys.exit(f"child ({name}, rep {rep}) failed with {p.returncode}:\n{p.stdout}\n{p.stderr}")
            runs[name].append(json.loads(line[len("TILES_BENCH "):]))
            print(f"== {name} rep {rep}: " + "; ".join(f"{c['dtype']} F={c['F']} detect {c['detect_us']}" + (f" tiles {c['tiles_us']}" if "tiles_us" in c else "")
                                                         for c in runs[name][-1]["cases"]), flush=True)
    summary = []
    for i, case in enumerate(a.cases.split(",")):
        pd = [r["cases"][i]["detect_us"] for r in runs["parent"]]
        td = [r["cases"][i]["detect_us"] for r in runs["this"]]
        tt = [r["cases"][i]["tiles_us"] for r in runs["this"]]
        s = {"case": case, "parent_detect_us": round(float(np.median(pd)), 1), "parent_detect_us_reps": pd,
             "this_detect_us": round(float(np.median(td)), 1), "this_detect_us_reps": td,
             "tiles_us": round(float(np.median(tt)), 1), "tiles_us_reps": tt,
             "ratio_tiles_over_parent_detect": round(float(np.median(tt)) / float(np.median(pd)), 3),
             "ratio_this_detect_over_parent_detect": round(float(np.median(td)) / float(np.median(pd)), 3),
             "detect_kernels_us": runs["this"][-1]["cases"][i]["detect_kernels_us"], "tiles_kernels_us": runs["this"][-1]["cases"][i]["tiles_kernels_us"]}
        summary.append(s)
        print(json.dumps(s), flush=True)
    if a.json:
        bl.write_json(a.json, {"rows": a.rows, "cols": a.cols, "tile": a.tile, "mask": a.mask, "iters": a.iters, "rounds": a.rounds, "reps": a.reps,
                               "membench": {k: v for k, v in runs["parent"][0].items() if k.startswith("membench")}, "summary": summary, "runs": runs})


if __name__ == "__main__":
    main()
