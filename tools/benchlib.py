"""What the timing tools (tools/*_bench.py, quick_bench.py, ab.py) share: the library loader, the two clocks, the alternation of
routes, the wm_membench and wm_prof_* yardsticks and the JSON tail.  Nothing here knows which entry point a tool measures, and
nothing here rounds: rounding is part of each tool's output.  time.perf_counter is the only host clock."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "watermarking-gpu_amd"


def load():
    """(wm, synth): the package and its synthetic frames, from this repository.  WM_AB_LIB names another build of libwm_hip.so (the
    parent commit's, in an A/B run): wm.LIB_PATH points at it, and wm.ABI is trimmed to the symbols it exports, so that an older build
    binds; a tool that needs an entry added since asks hasattr(wm.lib(), name)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    wm = importlib.import_module(PKG)
    if os.environ.get("WM_AB_LIB"):
        try:
            import torch  # noqa: F401  (torch's HIP runtime first, as in wm.lib(): one runtime per process)
        except ImportError:
            pass
        wm.LIB_PATH = os.environ["WM_AB_LIB"]
        exported = C.CDLL(wm.LIB_PATH)
        wm.ABI = [e for e in wm.ABI if hasattr(exported, e[0])]
    return wm, importlib.import_module(PKG + ".synth")


def wall_median_us(fn, iters, warmup=0):
    """median host microseconds of `iters` calls of fn, each from just before the call to just after its return (a synchronous call:
    the whole call; an enqueue: the host's share), behind `warmup` calls that are made and not counted"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def slot_stream(eng, slot=0):
    import torch
    return torch.cuda.ExternalStream(importlib.import_module(PKG).lib().wm_get_stream(eng._ctx, slot))


def device_span_us(eng, enqueue, n, batch=1, plug=None, slot=0):
    """median microseconds per call, over n spans, between two events on the slot's stream around `batch` calls queued back to back:
    what the device spends on a call (uploads, launches and the gaps between them), without the host's share.  plug: queued in front
    of the first event -- work that keeps the device busy while the host enqueues the timed calls, so that they wait in the queue when
    the device reaches them (a guard for calls of under 10 us)"""
    import torch
    st = slot_stream(eng, slot)
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if plug:
            plug()
        e0.record(st)
        for _ in range(batch):
            enqueue()
        e1.record(st)
        eng.sync(slot)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / batch)
    return float(np.median(ts))


def span_and_wall_us(eng, enqueue, slot=0):
    """(device span, host wall) of ONE repeat in microseconds: the span between two events on the slot's stream around what `enqueue`
    queues; the wall clock starts in front of the first event's record and stops behind the wait for the second event"""
    import torch
    st = slot_stream(eng, slot)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(st)
    enqueue()
    e1.record(st)
    eng.sync(slot)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6


def alternate(routes, rounds, iters, measure, warm=0):
    """{name: [measure(fn, iters) of every round]}: `warm` untimed passes over all routes, then `rounds` rounds in which every route
    is measured once, in the mapping's order, so that drift of the box falls on all routes alike.  A route that is None (a build or a
    setup that lacks it) is skipped and has no list."""
    live = {name: fn for name, fn in routes.items() if fn is not None}
    for _ in range(warm):
        for fn in live.values():
            fn()
    out = {name: [] for name in live}
    for _ in range(rounds):
        for name, fn in live.items():
            out[name].append(measure(fn, iters))
    return out


def median_of_rounds(values):
    return float(np.median(values))


def membench_us(kind, nbytes, seconds, device=0):
    """(mean microseconds per launch, launches) of wm_membench's pure store / copy / read of `nbytes` for about `seconds`"""
    wm = importlib.import_module(PKG)
    us, n = C.c_double(), C.c_int()
    rc = wm.lib().wm_membench(device, kind, nbytes, seconds, C.byref(us), C.byref(n))
    assert rc == wm.WM_OK, rc
    return us.value, n.value


def prof_us_per_launch(eng, fn, n):
    """{kernel name: mean device microseconds per launch} over n calls of fn with the engine's profiling (wm_prof_*) on"""
    eng.prof_reset()
    eng.prof_enable(True)
    for _ in range(n):
        fn()
    rep = eng.prof_report()
    eng.prof_enable(False)
    return {name: ms * 1e3 / cnt for name, (cnt, ms) in rep.items()}


def write_json(path, obj, **kw):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, **kw)
