"""Checked Gram hand-over (wm.h wm_detect, wm_set_checked_handover): a plain wm_embed followed by wm_detect of its output plane on the
same slot takes the embed's Gram sums (k_gram_ho) without any promise from the caller -- the detector's sweep sums a digest of the
plane it reads and holds it against the one the embed left; a frame whose digest differs is redone on the device by the
ordinary sweeps (k_gram_redo / k_detect_redo).  Checked here: plain calls hand over over the tile geometries (every frame
trusted, no Gram sweep over y, scores as the ordinary path's); pixels changed behind the embed from another stream -- one
pixel, one bit, a zero-sum (+d, -2d, +d) triple, two swapped pixels -- are caught frame by frame and give the ordinary path's
scores bit for bit; whatever the hand-over does not cover takes the ordinary path; results are bit-stable.
test_gpu_checked_handover_coverage.py goes on from here: every pixel of small planes, both block mappings of the detector, every redo
pattern, and the calls that follow a redo on the slot."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

TOL_SWITCH = 1.2e-7
TOL_ORACLE = 1e-5


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames(R, Cc, F, first=0, dtype=np.float32):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=dtype) for f in range(F)])


def engine(wm, R, Cc, F, rps=0, checked=True, W=None):
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc) if W is None else W, 3, 40.0, nslots=2, max_frames=F)
    if rps:
        eng.set_rows_per_segment(rps)
    eng.set_checked_handover(checked)
    return eng


def embed_detect(wm, torch, eng, x, base=None, out=None, mask=None, slot=0, between=None):
    """embed x (base: x) into out (a new plane), then detect out on the same slot; returns (y, a, status, corr, detect status)"""
    mk = wm.MASK_TYPE.ME if mask is None else mask
    F = x.shape[0]
    y = torch.empty_like(x) if out is None else out
    a, st, corr, std = (C.c_float * F)(), (C.c_int * F)(), (C.c_float * F)(), (C.c_int * F)()
    eng.embed_async(x, x if base is None else base, y, mk, slot, a_out=a, status_out=st)
    if between is not None:
        eng.sync(slot)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            between(y)
        side.synchronize()
    eng.detect_async(y, mk, slot, corr_out=corr, status_out=std)
    eng.sync(slot)
    return y, list(a), list(st), list(corr), list(std)


def ordinary_scores(wm, eng_off, y, mask=None):
    F = y.shape[0]
    corr, st = (C.c_float * F)(), (C.c_int * F)()
    eng_off.detect_async(y, wm.MASK_TYPE.ME if mask is None else mask, 0, corr_out=corr, status_out=st)
    eng_off.sync(0)
    return list(corr), list(st)


# (rows, cols, frames, rows per segment): one strip; shifted last strip with short segments; one segment; segments of 3 and 5
# rows; frame quads (4 frames per block in the detector) with a short last quad
CASES = [(64, 256, 2, 0), (97, 516, 4, 8), (57, 772, 6, 5), (40, 260, 3, 40), (130, 1028, 5, 3), (270, 1024, 8, 0)]


@pytest.mark.parametrize("case", CASES)
def test_plain_calls_hand_over(wm, tc, case):
    R, Cc, F, rps = case
    eng, off = engine(wm, R, Cc, F, rps), engine(wm, R, Cc, F, rps, checked=False)
    x = tc.from_numpy(frames(R, Cc, F)).cuda()
    t0, r0 = eng.checked_handover_counts()
    eng.prof_enable(True)
    y, a, st, corr, std = embed_detect(wm, tc, eng, x)
    rep = eng.prof_report()
    t1, r1 = eng.checked_handover_counts()
    assert (t1 - t0, r1 - r0) == (F, 0)
    # the embed's Gram sweep over x is the only k_gram; the detector's came from the hand-over, the redo launches were empty
    assert rep["k_gram"][0] == 1 and rep["k_gram_ho_checked"][0] == 1 and rep["k_detect"][0] == 1, rep
    assert rep["k_gram_redo"][0] == 1 and rep["k_detect_redo"][0] == 1 and "k_gram_ho" not in rep, rep
    # the switch off: the same plane and strength, scores to the Gram sums' grouping
    y2, a2, st2, corr2, std2 = embed_detect(wm, tc, off, x)
    assert tc.equal(y, y2) and a == a2 and std == std2
    assert max(abs(p - q) for p, q in zip(corr, corr2)) <= TOL_SWITCH
    if R * Cc <= 130 * 1028:
        W = synth_watermark(R, Cc)
        for f in range(F):
            assert corr[f] == pytest.approx(O.detect(y[f].cpu().numpy(), W, mask=O.MASK_ME)[1], abs=TOL_ORACLE)
    eng.close(); off.close()


def _one_pixel(y):
    y[1, 33, 300] += 3.0


def _one_bit(y):
    import torch
    y.view(torch.int32)[2, 60, 17] ^= 1


def _triple(y):
    d = 0.5
    y[0, 20, 99] += d
    y[0, 20, 100] -= 2 * d
    y[0, 20, 101] += d
    y[3, 96, 511] += d
    y[3, 96, 512] -= 2 * d
    y[3, 96, 513] += d


def _swap(y):
    a, b = y[4, 10, 200].clone(), y[4, 11, 201].clone()
    y[4, 10, 200] = b
    y[4, 11, 201] = a


@pytest.mark.parametrize("change,changed", [(_one_pixel, {1}), (_one_bit, {2}), (_triple, {0, 3}), (_swap, {4})])
def test_changed_pixels_are_caught(wm, tc, change, changed):
    R, Cc, F = 97, 516, 5
    eng = engine(wm, R, Cc, F, 8)
    x = tc.from_numpy(frames(R, Cc, F)).cuda()
    if change is _swap:
        assert float(x[4, 10, 200]) != float(x[4, 11, 201])
    t0, r0 = eng.checked_handover_counts()
    y, a, st, corr, std = embed_detect(wm, tc, eng, x, between=change)
    t1, r1 = eng.checked_handover_counts()
    assert (t1 - t0, r1 - r0) == (F - len(changed), len(changed))
    fresh = engine(wm, R, Cc, F, 8, checked=False)
    ref, ref_st = ordinary_scores(wm, fresh, y)
    assert std == ref_st
    for f in range(F):
        if f in changed:
            assert corr[f] == ref[f], (f, corr[f], ref[f])  # the redo IS the ordinary path
        else:
            assert abs(corr[f] - ref[f]) <= TOL_SWITCH
    eng.close(); fresh.close()


def test_edge_cases_hand_over_or_take_the_ordinary_path(wm, tc):
    torch = tc
    R, Cc, F = 64, 512, 4
    W = synth_watermark(R, Cc)
    eng, off = engine(wm, R, Cc, F, W=W), engine(wm, R, Cc, F, checked=False, W=W)
    counts = eng.checked_handover_counts

    def delta(fn):
        t0, r0 = counts()
        out = fn()
        t1, r1 = counts()
        return out, (t1 - t0, r1 - r0)

    # an unsolvable (constant) frame in the batch: its passthrough plane is handed over and checked like the others
    xs = frames(R, Cc, F)
    xs[2] = 77.0
    x = torch.from_numpy(xs).cuda()
    (y, a, st, corr, std), d = delta(lambda: embed_detect(wm, torch, eng, x))
    assert d == (F, 0) and st[2] != 0 and std[2] != 0 and st[0] == 0
    ref, ref_st = ordinary_scores(wm, off, y)
    assert std == ref_st and max(abs(p - q) for p, q in zip(corr, ref)) <= TOL_SWITCH
    # a separate base
    x = torch.from_numpy(frames(R, Cc, F)).cuda()
    base = torch.from_numpy(frames(R, Cc, F, first=100)).cuda()
    (y, a, st, corr, std), d = delta(lambda: embed_detect(wm, torch, eng, x, base=base))
    assert d == (F, 0)
    ref, _ = ordinary_scores(wm, off, y)
    assert max(abs(p - q) for p, q in zip(corr, ref)) <= TOL_SWITCH
    # a second detect of the same plane: the sums are used up, the ordinary path (same score to the grouping)
    eng.prof_enable(True)
    eng.prof_reset()
    c2, d = delta(lambda: ordinary_scores(wm, eng, y)[0])
    assert d == (0, 0) and "k_gram_ho_checked" not in eng.prof_report() and eng.prof_report()["k_gram"][0] == 1
    assert max(abs(p - q) for p, q in zip(c2, ref)) <= TOL_SWITCH
    # a detect of the plane on ANOTHER slot: ordinary
    x2 = torch.from_numpy(frames(R, Cc, F, first=10)).cuda()
    y2 = torch.empty_like(x2)
    eng.embed_async(x2, x2, y2, wm.MASK_TYPE.ME, 0)
    cs = (C.c_float * F)()
    (_, d) = delta(lambda: (eng.detect_async(y2, wm.MASK_TYPE.ME, 1, corr_out=cs), eng.sync(1), eng.sync(0)))
    assert d == (0, 0)
    # ... while the slot's own detect still hands over
    (_, d) = delta(lambda: ordinary_scores(wm, eng, y2))
    assert d == (F, 0)
    # in place: input, base and output one plane
    fr = torch.from_numpy(frames(R, Cc, F, first=20)).cuda()
    fr2 = fr.clone()
    (res, d) = delta(lambda: embed_detect(wm, torch, eng, fr, base=fr, out=fr))
    assert d == (F, 0)
    off.embed_async(fr2, fr2, fr2, wm.MASK_TYPE.ME, 0)
    off.sync(0)
    assert torch.equal(fr, fr2)
    ref, _ = ordinary_scores(wm, off, fr2)
    assert max(abs(p - q) for p, q in zip(res[3], ref)) <= TOL_SWITCH
    # u8 planes, the NVF mask, one frame, an RGB base: untouched (no checked hand-over)
    xu = torch.from_numpy(frames(R, Cc, F, dtype=np.uint8)).cuda()
    (_, d) = delta(lambda: embed_detect(wm, torch, eng, xu))
    assert d == (0, 0)
    eng.prof_reset()
    (_, d) = delta(lambda: embed_detect(wm, torch, eng, x, mask=wm.MASK_TYPE.NVF))
    assert d == (0, 0) and eng.prof_report()["k_gram"][0] == 1 and "k_gram_ho_checked" not in eng.prof_report()
    (_, d) = delta(lambda: embed_detect(wm, torch, eng, x[:1].contiguous()))
    assert d == (0, 0)
    y3 = torch.empty_like(x)
    eng.embed_async(x, x, y3, wm.MASK_TYPE.ME, 0)
    rgb = torch.stack([x, x, x], dim=1).contiguous()
    out = torch.empty_like(rgb)
    eng.embed_async(x, rgb, out, wm.MASK_TYPE.ME, 0)  # replaces the slot's output: y3 is no longer what the slot last wrote
    (_, d) = delta(lambda: ordinary_scores(wm, eng, y3))
    assert d == (0, 0)
    # the switch off: nothing is handed over; on again: it is
    eng.set_checked_handover(False)
    (_, d) = delta(lambda: embed_detect(wm, torch, eng, x))
    assert d == (0, 0)
    eng.set_checked_handover(True)
    (_, d) = delta(lambda: embed_detect(wm, torch, eng, x))
    assert d == (F, 0)
    eng.close(); off.close()


def test_checked_handover_is_bit_stable(wm, tc):
    torch = tc
    R, Cc, F = 270, 1028, 8
    eng = engine(wm, R, Cc, F)
    xa = torch.from_numpy(frames(R, Cc, F)).cuda()
    first = {}
    for rnd in range(6):
        on = rnd % 2 == 0
        eng.set_checked_handover(on)
        y, a, st, corr, std = embed_detect(wm, torch, eng, xa, slot=rnd % 2)
        got = (corr, a, y.clone())
        if on not in first:
            first[on] = got
        assert got[0] == first[on][0] and got[1] == first[on][1] and torch.equal(got[2], first[on][2]), f"round {rnd} differs"
    assert max(abs(p - q) for p, q in zip(first[True][0], first[False][0])) <= TOL_SWITCH
    eng.set_checked_handover(True)
    # many calls on 2 slots in flight
    ys = [torch.empty_like(xa) for _ in range(2)]
    outs = [(C.c_float * F)() for _ in range(2)]
    t0, r0 = eng.checked_handover_counts()
    for rnd in range(10):
        for sl in range(2):
            eng.embed_async(xa, xa, ys[sl], wm.MASK_TYPE.ME, sl)
            eng.detect_async(ys[sl], wm.MASK_TYPE.ME, sl, corr_out=outs[sl])
        for sl in range(2):
            eng.sync(sl)
            assert list(outs[sl]) == first[True][0], (rnd, sl)
    t1, r1 = eng.checked_handover_counts()
    assert (t1 - t0, r1 - r0) == (20 * F, 0)
    eng.close()
