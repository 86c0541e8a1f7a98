"""The calls added after the hard-content battery (tests/test_gpu_hard_content.py) on its mixed batch: one frame of every hard family
-- clipped, letterboxed, binary, near-singular, impulse, exactly singular, flat -- in one call, f32 and u8, ME p = 3 and NVF p = 3, 5,
130 rows by 516 columns (two strips and a shifted last strip) and, f32, 514 (not a multiple of 4).  Each call is held to what wm.h
already promises for it: wm_detect_tiles to the oracle restated per tile (1e-5) and its sums to wm_detect (2e-7); every other call
bit for bit to the call it is defined by -- wm_detect_keys_tiles to wm_detect_tiles, wm_embed_signs / wm_embed_bits /
wm_embed_signs_multi to wm_embed with W, -W and a zero W, wm_detect_bits to wm_detect_tiles' sums added in order, wm_embed_select /
wm_detect_select and wm_detect_offsets to wm_embed / wm_detect on a context whose W is that key or window.  Unsolvable frames come
back WM_UNSOLVABLE with 0.0f, zero sums and out == base; zero-energy tiles, frames and keys score NaN with status OK."""
import numpy as np
import pytest

import bits_model as BM
import hard_frames as H
import test_gpu_hard_content as HC
import tiles_model as TM
from layouts import raw
from synth import synth_watermark

pytestmark = pytest.mark.gpu

R = HC.R
TOL, TOL_SUM = 1e-5, 2e-7
TH, TW = 32, 32
BIG = (256, 1024)  # one tile larger than the plane
CASES = [(dtype, cols, mask, p) for dtype in ("f32", "u8") for cols in ((516, 514) if dtype == "f32" else (516,))
         for (mask, p) in ((0, 3), (1, 3), (1, 5))]
DEAD = ("ramp", "rows", "flat77", "flat77.3", "flat0", "flat255")  # the exactly singular frames of the mixed batch
_batch = {}


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def batch(dtype, cols):
    if (dtype, cols) not in _batch:
        _batch[dtype, cols] = HC.mixed_batch(R, cols, dtype)
    return _batch[dtype, cols]


def key_of(cols, k, rows=R):
    return synth_watermark(rows, cols, 7300 + 17 * k + cols)


def seam_batch(cols, dtype):
    """a frame whose upper and lower 40 rows are bars at 0 (the 32 x 32 tiles of its first and last tile row lie inside them with
    their windows), and impulses on both sides of the tile seams: rows 31 / 32, columns 31 / 32, 247 / 248 (the last 4-column group
    of a strip's first 256 columns) and 255 / 256"""
    bar = H.letterbox(R, cols, 40, 0)
    spots = {"r31": (31, 100), "r32": (32, 101), "c31": (70, 31), "c32": (71, 32), "c247": (72, 247), "c248": (73, 248),
             "c255": (74, 255), "c256": (75, 256)}
    imp, items = H.impulse(R, cols, spots)
    xs = np.concatenate([bar[None], imp])
    return ["bar40"] + [n for n, _, _ in items], (HC.to_u8(xs) if dtype == "u8" else xs)


def engine(wm, cols, W, p, F, rows=R):
    e = wm.Watermark(rows, cols, W, p, 40.0, nslots=1, max_frames=F)
    e.set_fused(False)
    return e


def strengths(a):
    return np.array([np.nan if v is None else v for v in a], np.float32)


@pytest.mark.parametrize("dtype,cols,mask,p", CASES)
def test_detect_tiles(wm, tc, dtype, cols, mask, p):
    mt = wm.MASK_TYPE(mask)
    W = H.watermark(R, cols)
    for names, xs in (batch(dtype, cols), seam_batch(cols, dtype)):
        F = len(xs)
        eng = engine(wm, cols, W, p, F)
        xt = HC.dev(tc, xs)
        whole = np.asarray(eng.detectWatermark(xt, mt), np.float32)
        for th, tw in ((TH, TW), BIG):
            got, sums = eng.detectTiles(xt, th, tw, mt, sums=True)
            worst = 0.0
            for f, name in enumerate(names):
                st, ref, _ = TM.tile_map(xs[f], W, th, tw, p, mask)
                if name in DEAD:
                    assert st == 1 and not raw(got[f]).any() and not raw(sums[f]).any(), name
                    continue
                assert st == 0 and np.array_equal(np.isnan(got[f]), np.isnan(ref)), (name, got[f], ref)
                ok = ~np.isnan(ref)
                if ok.any():
                    worst = max(worst, float(np.abs(got[f][ok] - ref[ok]).max()))
                assert not np.isnan(ref).any() or name in ("bar40", "letterbox0", "pillar16"), name
                if name == "bar40" and (th, tw) == (TH, TW):  # the tile rows inside the two bars: NaN, status OK, zero sums
                    inside = [0, got.shape[1] - 1]   # (rows 0-31 of the upper bar, rows 96-129 of the lower one)
                    assert np.isnan(got[f][inside]).all() and not raw(sums[f][inside]).any() and np.isfinite(got[f][1:-1]).all()
                total = TM.score_of(sums[f].sum(axis=(0, 1)))
                assert abs(float(total) - float(whole[f])) <= TOL_SUM, (name, total, whole[f])
            print(f"{dtype} {cols} mask {mask} p {p} tiles {th}x{tw} F {F}: worst |diff| {worst:.2e}")
            assert worst <= TOL
        eng.close()


@pytest.mark.parametrize("dtype,cols,mask,p", CASES)
def test_detect_keys_tiles(wm, tc, dtype, cols, mask, p):
    """key k's map and sums are wm_detect_tiles' with key k as W, bit for bit; key 1 is never filled"""
    mt = wm.MASK_TYPE(mask)
    names, xs = batch(dtype, cols)
    F = len(xs)
    xt = HC.dev(tc, xs)
    planes = [key_of(cols, 0), H.zero_w(R, cols), key_of(cols, 2)]
    bank = wm.KeySet(R, cols, 3)
    bank.set(0, planes[0])
    bank.set(2, planes[2])
    eng = engine(wm, cols, H.watermark(R, cols), p, F)
    for th, tw in ((TH, TW), BIG):
        got, sums = eng.detectKeysTiles(xt, bank, th, tw, mt, sums=True)
        for k, pl in enumerate(planes):
            one = engine(wm, cols, pl, p, F)
            m1, s1 = one.detectTiles(xt, th, tw, mt, sums=True)
            one.close()
            assert np.array_equal(raw(got[:, k]), raw(m1)) and np.array_equal(raw(sums[:, k]), raw(s1)), (th, tw, k)
        solvable = [f for f, n in enumerate(names) if n not in DEAD]
        assert np.isnan(got[solvable, 1]).all() and not raw(got[[f for f in range(F) if f not in solvable]]).any()
    eng.close()
    bank.close()


@pytest.mark.parametrize("dtype,cols,mask,p", CASES)
def test_embed_signs_bits_and_multi(wm, tc, dtype, cols, mask, p):
    """wm_embed_signs: pixels and strengths are wm_embed's with W, -W and a zero W selected per tile; wm_embed_bits is wm_embed_signs
    with the payload's table; wm_embed_signs_multi (K = 3) is wm_embed_signs per table; out == base on the unsolvable and the
    zero-energy frames"""
    mt = wm.MASK_TYPE(mask)
    names, xs = batch(dtype, cols)
    F = len(xs)
    xt = HC.dev(tc, xs)
    W = H.watermark(R, cols)
    ny, nx = wm.Watermark.tiles_shape(R, cols, TH, TW)
    outs = []
    for w in (W, -W, H.zero_w(R, cols)):
        e = engine(wm, cols, w, p, F)
        y, a = e.makeWatermark(xt, xt, mt)
        outs.append((y.cpu().numpy(), strengths(a)))
        e.close()
    (yp, ap), (yn, an), (yz, az) = outs
    assert np.array_equal(raw(yz), raw(xs)) and np.array_equal(raw(ap), raw(an))
    eng = engine(wm, cols, W, p, F)
    K = 3
    signs = np.random.default_rng(cols + 7 * mask + p).integers(-1, 2, (F, K, ny, nx)).astype(np.int8)
    per_table = []
    for k in range(K):
        y, a = eng.makeWatermarkSigns(xt, xt, TH, TW, signs[:, k], mt)
        y = y.cpu().numpy()
        want = np.stack([BM.select(signs[f, k], TH, TW, yp[f], yn[f], yz[f]) for f in range(F)])
        assert np.array_equal(raw(y), raw(want)) and np.array_equal(raw(strengths(a)), raw(ap)), k
        per_table.append(y)
    for f, name in enumerate(names):
        dead = name in DEAD and mask == 0   # (an NVF embed needs no solve: a flat frame is then a zero-energy frame, a = +inf)
        assert np.isnan(ap[f]) == dead, name
        if dead or np.isinf(ap[f]):
            assert np.array_equal(raw(per_table[0][f]), raw(xs[f])), name
        if name.startswith("flat") and name != "flat77.3":
            assert dead or np.isinf(ap[f]), name
    copies, am = eng.makeWatermarkSignsMulti(xt, xt, TH, TW, signs, mt)
    copies = copies.cpu().numpy()
    for k in range(K):
        assert np.array_equal(raw(copies[:, k]), raw(per_table[k])), k
    assert np.array_equal(raw(am), raw(ap))
    nbits = 8
    tb = BM.layout(ny, nx, nbits, 4711)
    tb[tb == nbits - 1] = -1  # (the last bit has no tile: its tiles stay unmarked)
    payload = BM.pack_bits(np.arange(nbits) % 3 == 0)
    yb, ab = eng.makeWatermarkBits(xt, xt, TH, TW, tb, nbits, payload * F, mt)
    ys, as_ = eng.makeWatermarkSigns(xt, xt, TH, TW, np.stack([BM.signs_of(tb, payload, nbits).reshape(ny, nx)] * F), mt)
    assert np.array_equal(raw(yb), raw(ys)) and np.array_equal(raw(strengths(ab)), raw(strengths(as_)))
    eng.close()


@pytest.mark.parametrize("dtype,cols,mask,p", CASES)
def test_detect_bits(wm, tc, dtype, cols, mask, p):
    """the soft values are wm_detect_tiles' sums added per bit in ascending tile order, bit for bit; NaN where the sums are zero"""
    mt = wm.MASK_TYPE(mask)
    names, xs = batch(dtype, cols)
    F = len(xs)
    xt = HC.dev(tc, xs)
    ny, nx = wm.Watermark.tiles_shape(R, cols, TH, TW)
    nbits = 8
    tb = BM.layout(ny, nx, nbits, 99)
    tb[tb == nbits - 1] = -1
    eng = engine(wm, cols, H.watermark(R, cols), p, F)
    _, s = eng.detectTiles(xt, TH, TW, mt, sums=True)
    _, soft = eng.detectBits(xt, TH, TW, tb, nbits, mt)
    for f, name in enumerate(names):
        if name in DEAD:
            assert not raw(soft[f]).any(), name
            continue
        want = BM.soft_of_sums(s[f], tb, nbits)
        assert np.isnan(soft[f][nbits - 1]) and np.array_equal(np.isnan(soft[f]), np.isnan(want)), name
        ok = ~np.isnan(want)
        assert np.array_equal(raw(soft[f][ok]), raw(want[ok])), (name, soft[f], want)
    eng.close()


@pytest.mark.parametrize("dtype,cols,mask,p", CASES)
def test_select(wm, tc, dtype, cols, mask, p):
    """a schedule that gives adjacent frames different keys and includes the never-filled key: frame f of wm_embed_select /
    wm_detect_select is frame f of wm_embed / wm_detect on a context whose W is that key, bit for bit"""
    mt = wm.MASK_TYPE(mask)
    names, xs = batch(dtype, cols)
    F = len(xs)
    xt = HC.dev(tc, xs)
    planes = [key_of(cols, 0), H.zero_w(R, cols), key_of(cols, 2)]
    bank = wm.KeySet(R, cols, 3)
    bank.set(0, planes[0])
    bank.set(2, planes[2])
    kt = (np.arange(F) % 3).astype(np.int32)
    eng = engine(wm, cols, H.watermark(R, cols), p, F)
    yt, a = eng.makeWatermarkSelect(xt, xt, bank, kt, mt)
    corr = np.asarray(eng.detectSelect(yt, bank, kt, mt), np.float32)
    y, a = yt.cpu().numpy(), strengths(a)
    for k, pl in enumerate(planes):
        one = engine(wm, cols, pl, p, F)
        yk, ak = one.makeWatermark(xt, xt, mt)
        ck = np.asarray(one.detectWatermark(yt, mt), np.float32)
        one.close()
        sel = kt == k
        assert np.array_equal(raw(y[sel]), raw(yk.cpu().numpy()[sel])) and np.array_equal(raw(a[sel]), raw(strengths(ak)[sel])), k
        assert np.array_equal(raw(corr[sel]), raw(ck[sel])), (k, corr[sel], ck[sel])
    for f, name in enumerate(names):
        if name in DEAD and mask == 0:
            assert corr[f] == 0.0 and np.isnan(a[f]) and np.array_equal(raw(y[f]), raw(xs[f])), name
        elif kt[f] == 1:
            assert np.isinf(a[f]) and np.array_equal(raw(y[f]), raw(xs[f])), name
            assert corr[f] == 0.0 if name in DEAD else np.isnan(corr[f]), name
    eng.close()
    bank.close()


@pytest.mark.parametrize("dtype,cols,mask,p", CASES)
def test_detect_offsets(wm, tc, dtype, cols, mask, p):
    """3 x 3 offsets into a key 8 larger per axis: every score is wm_detect's on a context whose W is the window copied out, bit
    for bit; NaN for the never-filled key; 0.0f and WM_UNSOLVABLE for the singular frames"""
    mt = wm.MASK_TYPE(mask)
    names, xs = batch(dtype, cols)
    F = len(xs)
    xt = HC.dev(tc, xs)
    big = key_of(cols + 8, 5, rows=R + 8)
    bank = wm.KeySet(R + 8, cols + 8, 2)
    bank.set(0, big)
    eng = engine(wm, cols, H.watermark(R, cols), p, F)
    oy0, ox0 = 2, 3
    got = eng.detectOffsets(xt, bank, 0, oy0, ox0, 3, 3, mt)
    zero = eng.detectOffsets(xt, bank, 1, oy0, ox0, 3, 3, mt)
    dead = np.array([n in DEAD for n in names])
    for i in range(3):
        for j in range(3):
            one = engine(wm, cols, np.ascontiguousarray(big[oy0 + i:oy0 + i + R, ox0 + j:ox0 + j + cols]), p, F)
            want = np.asarray(one.detectWatermark(xt, mt), np.float32)
            one.close()
            assert np.array_equal(raw(got[:, i, j]), raw(want)), (i, j, got[:, i, j], want)
    assert not raw(got[dead]).any() and not raw(zero[dead]).any() and np.isnan(zero[~dead]).all()
    corr = np.zeros((F, 1, 1), np.float32)
    st = np.full(F, -5, np.int32)
    eng.detect_offsets_async(xt, bank, 0, oy0, ox0, 1, 1, mt, 0, corr, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE and list(st) == [1 if d else 0 for d in dead]
    eng.close()
    bank.close()
