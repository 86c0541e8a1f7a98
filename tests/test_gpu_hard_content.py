"""The hard-content families (tests/hard_frames.py) through every path that takes them, against the CPU oracle with the
suite's tolerances (strength rel 1e-4, y 1e-3, u8 <= 1 LSB on <= 0.1 % of the pixels, score 1e-5, Gram rtol 1e-13, u8 Gram
exact) and bit for bit where wm.h promises it: the batched sweeps (mixed batches of F >= 4 frames, f32 and u8, widths a
multiple of 256, 256 k + 4 and -- f32 -- not a multiple of 4, NVF p = 3, 5, 9), wm_compute_mask, the fused one-image calls and
the one-call pair, the Gram hand-over (checked and opt-in), wm_embed_keys / wm_detect_keys with a never-filled key, and row
bands.  Clipped frames make the clamp fire; letterbox bars give exactly flat regions; impulses put max|e| on the seams of the
reductions; singular frames must come back WM_UNSOLVABLE with out == base everywhere; zero-energy frames (u = m W = 0) must
give a = +inf and out == base bit for bit (wm.h wm_embed), and a zero W or key scores NaN."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hard_frames as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

TOL_A, TOL_Y, TOL_CORR = 1e-4, 1e-3, 1e-5
R = 130
MASKS = [("ME", 3), ("NVF", 3), ("NVF", 5), ("NVF", 9)]


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


def omask(name):
    return O.MASK_ME if name == "ME" else O.MASK_NVF


def to_u8(x):
    return np.rint(np.clip(x, 0, 255)).astype(np.uint8)


def mixed_batch(rows, cols, dtype):
    """(names, frames [F, R, C]): one frame of every family; u8 batches round the f32 families"""
    spots = H.impulse_spots(rows, cols, rps=16)
    imp, items = H.impulse(rows, cols, {k: spots[k] for k in ("corner_tl", "strip_c256", "col_C-2", "corner_br")})
    fr = [("clipped", H.clipped(rows, cols)),
          ("letterbox0", H.letterbox(rows, cols, 12, 0)),
          ("pillar16", H.letterbox(rows, cols, 12, 16, pillar=True)),
          ("binary", H.binary(rows, cols)),
          ("near_singular", H.near_singular(rows, cols))]
    fr += [(f"impulse_{n}", x) for x, (n, _, _) in zip(imp, items)]
    fr += [("ramp", H.singular("ramp", rows, cols)), ("rows", H.singular("rows", rows, cols))]
    if dtype == "u8":
        fr += [("flat77", H.flat(rows, cols, 77)), ("flat0", H.flat(rows, cols, 0)), ("flat255", H.flat(rows, cols, 255))]
        fr = [(n, to_u8(x)) for n, x in fr]
    else:
        fr += [("flat77", H.flat(rows, cols, 77.0)), ("flat77.3", H.flat(rows, cols, 77.3))]
    return [n for n, _ in fr], np.stack([x for _, x in fr])


def oracle_embed(x, base, W, p, psnr, mask):
    if x.dtype == np.uint8:
        assert np.array_equal(base, x)  # (the video contract: the frame is its own base)
        return O.embed_u8(x, W, p=p, psnr=psnr, mask=omask(mask))
    return O.embed(x, base, W, p=p, psnr=psnr, mask=omask(mask))


def oracle_detect(y, W, p, mask):
    if y.dtype == np.uint8:
        return O.detect_u8(y, W, p=p, mask=omask(mask))
    return O.detect(y, W, p=p, mask=omask(mask))


def check_embed(tag, y, a, st, x, base, W, p, psnr, mask):
    """one frame's y (numpy), a (float, NaN when untouched) and status against the oracle; returns the oracle's y"""
    so, yo, ao = oracle_embed(x, base, W, p, psnr, mask)
    assert st == so, (tag, st, so)
    if so == O.UNSOLVABLE:
        assert np.isnan(a), (tag, a)                               # strength untouched
        assert np.array_equal(y.view(np.uint8), np.asarray(base).view(np.uint8)), tag
        return yo
    if ao == np.inf:                                               # zero energy: out == base bit for bit
        assert a == np.inf, (tag, a)
        assert np.array_equal(y.view(np.uint8), np.asarray(base).view(np.uint8)), tag
        return yo
    assert a == pytest.approx(ao, rel=TOL_A), (tag, a, ao)
    if y.dtype == np.uint8:
        d = np.abs(y.astype(np.int32) - yo.astype(np.int32))
        assert d.max() <= 1 and (d != 0).mean() <= 1e-3, (tag, d.max(), (d != 0).mean())
    else:
        err = float(np.abs(y - yo).max())
        assert err <= TOL_Y, (tag, err)
    return yo


def check_score(tag, corr, st, y, W, p, mask):
    so, co = oracle_detect(y, W, p, mask)
    assert st == so, (tag, st, so)
    if so == O.UNSOLVABLE:
        assert corr == 0.0, (tag, corr)
    elif np.isnan(co):
        assert np.isnan(corr), (tag, corr)
    else:
        assert corr == pytest.approx(co, abs=TOL_CORR), (tag, corr, co)


def embed_batch(wm, torch, eng, xs_d, base_d, mask, slot=0):
    F = xs_d.shape[0]
    y = torch.empty_like(base_d)
    a = np.full(F, np.nan, np.float32)
    st = np.zeros(F, np.int32)
    eng.embed_async(xs_d, base_d, y, wm.MASK_TYPE[mask], slot, a.ctypes.data_as(C.POINTER(C.c_float)),
                    st.ctypes.data_as(C.POINTER(C.c_int)))
    eng.sync(slot)
    return y, a, st


def detect_batch(wm, eng, img_d, mask, slot=0):
    F = img_d.shape[0]
    corr = np.zeros(F, np.float32)
    st = np.zeros(F, np.int32)
    eng.detect_async(img_d, wm.MASK_TYPE[mask], slot, corr.ctypes.data_as(C.POINTER(C.c_float)),
                     st.ctypes.data_as(C.POINTER(C.c_int)))
    eng.sync(slot)
    return corr, st


def sweeps(wm, rows, cols, W, p, psnr, F, rps=16):
    eng = wm.Watermark(rows, cols, W, p, psnr, max_frames=F)
    eng.set_fused(False)
    if rps:
        eng.set_rows_per_segment(rps)
    return eng


# ---- batched sweeps -------------------------------------------------------------------------------------------------------
SWEEP_CASES = [(dtype, cols, mask, p) for dtype in ("f32", "u8") for cols in ((512, 516, 514) if dtype == "f32" else (512, 516))
               for mask, p in MASKS]


@pytest.mark.parametrize("dtype,cols,mask,p", SWEEP_CASES)
def test_sweeps_mixed_batch(wm, tc, dtype, cols, mask, p):
    """one frame of every family in ONE batch: each frame against the oracle (a zero-energy or unsolvable frame next to
    ordinary ones must touch nothing but itself), then the detector on the oracle's outputs"""
    torch = tc
    names, xs = mixed_batch(R, cols, dtype)
    W = H.watermark(R, cols)
    F = len(names)
    eng = sweeps(wm, R, cols, W, p, 40.0, F)
    xd = dev(torch, xs)
    y, a, st = embed_batch(wm, torch, eng, xd, xd, mask)
    yn = y.cpu().numpy()
    yos = [check_embed(f"{names[f]} {dtype} {cols} {mask}{p}", yn[f], a[f], st[f], xs[f], xs[f], W, p, 40.0, mask) for f in range(F)]
    yo = np.stack(yos)
    corr, cst = detect_batch(wm, eng, dev(torch, yo), mask)
    for f in range(F):
        check_score(f"{names[f]} {dtype} {cols} {mask}{p}", corr[f], cst[f], yo[f], W, p, mask)
    # ... and on the unmarked frames (the singular ones stay singular there under either mask)
    c0, cst0 = detect_batch(wm, eng, xd, mask)
    for f in range(F):
        check_score(f"{names[f]} unmarked {dtype} {cols} {mask}{p}", c0[f], cst0[f], xs[f], W, p, mask)
    # the families kept their promises on this batch
    i = names.index("flat77")
    assert (st[i] == O.UNSOLVABLE) if mask == "ME" else (a[i] == np.inf and st[i] == O.OK)
    for name in ("ramp", "rows"):
        i = names.index(name)
        assert st[i] == (O.UNSOLVABLE if mask == "ME" else O.OK)
        assert cst0[i] == O.UNSOLVABLE and c0[i] == 0.0
    i = names.index("near_singular")
    assert st[i] == O.OK and cst[i] == O.OK and cst0[i] == O.OK
    eng.close()


@pytest.mark.parametrize("psnr", [10.0, 25.0, 40.0, 60.0])
@pytest.mark.parametrize("mask", ["ME", "NVF"])
def test_sweeps_clipped_psnr(wm, tc, psnr, mask):
    """the clamp at every psnr: f32 and u8 batches of clipped frames, and planar-RGB bases with channels at 0 / 255"""
    torch = tc
    cols, F = 516, 4
    W = H.watermark(R, cols)
    eng = sweeps(wm, R, cols, W, 3, psnr, F)
    xs = np.stack([H.clipped(R, cols, frame=f) for f in range(F)])
    xd = dev(torch, xs)
    y, a, st = embed_batch(wm, torch, eng, xd, xd, mask)
    yn = y.cpu().numpy()
    yo = np.stack([check_embed(f"clipped f{f} {psnr}", yn[f], a[f], st[f], xs[f], xs[f], W, 3, psnr, mask) for f in range(F)])
    if psnr == 10.0:
        assert min(H.clamped_fraction(yn[f], xs[f]) for f in range(F)) >= 0.10
    corr, cst = detect_batch(wm, eng, dev(torch, yo), mask)
    for f in range(F):
        check_score(f"clipped f{f} {psnr}", corr[f], cst[f], yo[f], W, 3, mask)
    # u8 (the video contract: the frame is its own base)
    x8 = np.stack([H.clipped(R, cols, frame=f, dtype=np.uint8) for f in range(F)])
    y8, a8, st8 = embed_batch(wm, torch, eng, dev(torch, x8), dev(torch, x8), mask)
    y8n = y8.cpu().numpy()
    for f in range(F):
        check_embed(f"clipped u8 f{f} {psnr}", y8n[f], a8[f], st8[f], x8[f], x8[f], W, 3, psnr, mask)
    # planar RGB base
    gr = [H.clipped_rgb(R, cols, frame=f) for f in range(F)]
    g = np.stack([q[0] for q in gr])
    rgb = np.stack([q[1] for q in gr])
    yr, ar, str_ = embed_batch(wm, torch, eng, dev(torch, g), dev(torch, rgb), mask)
    yrn = yr.cpu().numpy()
    for f in range(F):
        check_embed(f"rgb f{f} {psnr}", yrn[f], ar[f], str_[f], g[f], rgb[f], W, 3, psnr, mask)
    eng.close()


@pytest.mark.parametrize("cols", [512, 516])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_sweeps_impulse_at_every_seam(wm, tc, cols, dtype):
    """one impulse per frame at every structural spot (corners, core edges, strip seams, the shifted last strip's duplicate
    columns, segment seams of 16-row segments): the ME embed against the oracle, and wm_compute_mask's mask planes -- m = 1
    exactly at the planted pixel, e bit-exact given the kernel's coefficients"""
    torch = tc
    spots = H.impulse_spots(R, cols, rps=16)
    xs, items = H.impulse(R, cols, spots, dtype=np.uint8 if dtype == "u8" else np.float32)
    F = len(items)
    W = H.watermark(R, cols)
    eng = sweeps(wm, R, cols, W, 3, 40.0, F)
    xd = dev(torch, xs)
    y, a, st = embed_batch(wm, torch, eng, xd, xd, "ME")
    yn = y.cpu().numpy()
    for f, (name, r, c) in enumerate(items):
        check_embed(f"impulse {name} {dtype} {cols}", yn[f], a[f], st[f], xs[f], xs[f], W, 3, 40.0, "ME")
    m, e, coef, mst = eng.computeMask(xd, wm.MASK_TYPE.ME, want_error_sequence=True)
    mn, en = m.cpu().numpy(), e.cpu().numpy()
    for f, (name, r, c) in enumerate(items):
        xf = xs[f].astype(np.float32)
        so, co, eo, mo, mxo = O.me_mask(xf)
        assert mst[f] == 0 and so == 0
        e_ref = O.error_sequence(xf, coef[f])
        np.testing.assert_array_equal(en[f], e_ref, err_msg=name)
        ae = np.abs(e_ref)
        assert np.unravel_index(np.argmax(ae), ae.shape) == (r, c), name
        np.testing.assert_array_equal(mn[f], ae / ae.max(), err_msg=name)
        assert mn[f][r, c] == 1.0, name
        np.testing.assert_allclose(mn[f], mo, rtol=0, atol=1e-4, err_msg=name)
    eng.close()


@pytest.mark.parametrize("cols", [512, 516, 514])
def test_compute_mask_letterbox(wm, tc, cols):
    """NVF mask planes bit-exact (exactly 0 inside the bars) for p = 3, 5, 9; the ME mask as in the parity suite"""
    torch = tc
    xs = np.stack([H.letterbox(R, cols, 12, lv, pillar=pl) for lv in (0, 16) for pl in (False, True)])
    F = xs.shape[0]
    W = H.watermark(R, cols)
    xd = dev(torch, xs)
    for p in (3, 5, 9):
        eng = sweeps(wm, R, cols, W, p, 40.0, F)
        m, _, _, st = eng.computeMask(xd, wm.MASK_TYPE.NVF)
        mn = m.cpu().numpy()
        for f in range(F):
            np.testing.assert_array_equal(mn[f], O.nvf_mask(xs[f], p))
        assert (mn[[0, 2], :12 - p // 2] == 0).all() and (mn[[1, 3], :, :12 - p // 2] == 0).all()  # inside the bars
        eng.close()
    eng = sweeps(wm, R, cols, W, 3, 40.0, F)
    m, e, coef, st = eng.computeMask(xd, wm.MASK_TYPE.ME, want_error_sequence=True)
    for f in range(F):
        so, co, eo, mo, mxo = O.me_mask(xs[f])
        assert st[f] == 0 and so == 0
        np.testing.assert_array_equal(e[f].cpu().numpy(), O.error_sequence(xs[f], coef[f]))
        np.testing.assert_allclose(m[f].cpu().numpy(), mo, rtol=0, atol=1e-4)
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_gram_binary_and_singular(wm, tc, dtype):
    """Gram sums of binary and singular frames: u8 exact against numpy int64 sums, f32 rtol 1e-13 against the oracle;
    4352 x 256 u8 with 4096 rows per segment reaches the size k_gram's u32 lag-sum accumulators are bounded by"""
    torch = tc
    cols = 516
    fr = [H.binary(R, cols, seed=s) for s in range(3)] + [H.singular(k, R, cols) for k in H.SINGULAR_KINDS]
    if dtype == "u8":
        fr = [to_u8(x) for x in fr if np.array_equal(x, np.rint(x))]
    eng = sweeps(wm, R, cols, H.watermark(R, cols), 3, 40.0, 1, rps=0)
    for x in fr:
        tot = eng.gram_totals(dev(torch, x))
        if dtype == "u8":
            np.testing.assert_array_equal(tot, H.integer_gram(x).astype(np.float64))
        else:
            Rx, rx = O.gram(x)
            iu = np.triu_indices(8)
            np.testing.assert_allclose(tot, np.concatenate([Rx[iu], rx]), rtol=1e-13)
    eng.close()
    if dtype == "u8":
        x = H.binary(4352, 256, p255=0.98, dtype=np.uint8)
        eng = sweeps(wm, 4352, 256, H.watermark(4352, 256), 3, 40.0, 1, rps=4096)
        np.testing.assert_array_equal(eng.gram_totals(dev(torch, x)), H.integer_gram(x).astype(np.float64))
        eng.close()


# ---- fused one-image calls ------------------------------------------------------------------------------------------------
def fused_frames(rows, cols, dtype, tile_rows):
    spots = H.impulse_spots(rows, cols, tile_rows=tile_rows)
    keep = [k for k in spots if k.startswith("tile") or k in ("corner_tl", "corner_br", "strip_c256")]
    imp, items = H.impulse(rows, cols, {k: spots[k] for k in keep})
    fr = [("clipped", H.clipped(rows, cols)), ("letterbox16", H.letterbox(rows, cols, 12, 16)),
          ("pillar0", H.letterbox(rows, cols, 12, 0, pillar=True)), ("binary", H.binary(rows, cols)),
          ("near_singular", H.near_singular(rows, cols)), ("ramp", H.singular("ramp", rows, cols)),
          ("stripes", H.singular("stripes", rows, cols))]
    fr += [(f"impulse_{n}", x) for x, (n, _, _) in zip(imp, items)]
    if dtype == "u8":
        fr = [(n, to_u8(x)) for n, x in fr] + [("flat77", H.flat(rows, cols, 77)), ("flat255", H.flat(rows, cols, 255))]
    else:
        fr += [("flat77", H.flat(rows, cols, 77.0)), ("flat77.3", H.flat(rows, cols, 77.3))]
    return fr


def same_score(c1, c2):
    return (np.isnan(c1) and np.isnan(c2)) or c1 == c2


@pytest.mark.parametrize("one_launch", [0, 1])
@pytest.mark.parametrize("shape", [(R, 516), (1080, 1920)])
@pytest.mark.parametrize("mask", ["ME", "NVF"])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_fused_one_image(wm, tc, dtype, mask, shape, one_launch, monkeypatch):
    """makeWatermark / detectWatermark on the fused kernels against the oracle, and makeAndDetect (both one-launch settings)
    bit for bit equal to the two calls; no launch may have fallen back to the sweeps"""
    torch = tc
    monkeypatch.setenv("WM_FUSED_PAIR", str(one_launch))
    rows, cols = shape
    W = H.watermark(rows, cols)
    mk = wm.MASK_TYPE[mask]
    ef = wm.Watermark(rows, cols, W, 3, 40.0)
    ef.set_fused(True)
    assert ef.fused_info()[0]
    for name, x in fused_frames(rows, cols, dtype, ef.fused_info()[2]):
        if rows > R and not name.startswith(("clipped", "letterbox", "pillar", "impulse_tile", "flat77")):
            continue
        tag = f"{name} {dtype} {mask} {shape}"
        xd = dev(torch, x)
        y, a = ef.makeWatermark(xd, xd, mk)
        yo = check_embed(tag, y.cpu().numpy(), np.nan if a is None else a, 0 if a is not None else 1, x, x, W, 3, 40.0, mask)
        c = ef.detectWatermark(dev(torch, yo), mk)
        so, co = oracle_detect(yo, W, 3, mask)
        check_score(tag, c, so, yo, W, 3, mask)
        cy = ef.detectWatermark(y, mk)
        y1, a1, c1 = ef.makeAndDetect(xd, xd, mk)
        assert (a1 is None and a is None) or a1 == a, (tag, a1, a)
        assert torch.equal(bits(y1), bits(y)) and same_score(c1, cy), (tag, c1, cy)
    assert ef.fused_info()[3] == 0, "a fused launch timed out and fell back to the sweeps"
    ef.close()


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("one_launch", [0, 1])
def test_fused_zero_w(wm, tc, dtype, one_launch, monkeypatch):
    """an engine whose W is all zero: a = +inf, y == base bit for bit, score NaN -- under both masks, a base that is not the
    input included"""
    torch = tc
    monkeypatch.setenv("WM_FUSED_PAIR", str(one_launch))
    rows, cols = R, 516
    Z = H.zero_w(rows, cols)
    ef = wm.Watermark(rows, cols, Z, 3, 40.0)
    assert ef.fused_info()[0]
    x = H.clipped(rows, cols) if dtype == "f32" else H.clipped(rows, cols, dtype=np.uint8)
    b = H.clipped(rows, cols, frame=5) if dtype == "f32" else H.clipped(rows, cols, frame=5, dtype=np.uint8)
    xd, bd = dev(torch, x), dev(torch, b)
    for mask in ("ME", "NVF"):
        mk = wm.MASK_TYPE[mask]
        for base in (xd, bd):
            y, a = ef.makeWatermark(xd, base, mk)
            assert a == np.inf and torch.equal(bits(y), bits(base)), (mask, a)
            y1, a1, c1 = ef.makeAndDetect(xd, base, mk)
            assert a1 == np.inf and torch.equal(bits(y1), bits(base)) and np.isnan(c1), (mask, a1, c1)
        assert np.isnan(ef.detectWatermark(xd, mk))
    assert ef.fused_info()[3] == 0
    ef.close()


def test_fused_4k_clipped(wm, tc):
    torch = tc
    rows, cols = 2160, 3840
    W = H.watermark(rows, cols)
    x = H.clipped(rows, cols)
    ef = wm.Watermark(rows, cols, W, 3, 25.0)
    assert ef.fused_info()[0]
    y, a = ef.makeWatermark(dev(torch, x), dev(torch, x), wm.MASK_TYPE.ME)
    yo = check_embed("4k clipped", y.cpu().numpy(), a, 0, x, x, W, 3, 25.0, "ME")
    so, co = O.detect(yo, W)
    assert ef.detectWatermark(dev(torch, yo), wm.MASK_TYPE.ME) == pytest.approx(co, abs=TOL_CORR)
    assert ef.fused_info()[3] == 0
    ef.close()


# ---- hand-over --------------------------------------------------------------------------------------------------------------
def slot_plane(wm, rows, cols, F):
    return wm.wm_plane(None, rows, cols, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, cols, 0, rows * cols)


HO_CASES = [("clipped", R, 516), ("letterbox", R, 516), ("zero_w", R, 516), ("clipped", 2160, 3840)]


@pytest.mark.parametrize("family,rows,cols", HO_CASES)
@pytest.mark.parametrize("checked", [False, True])
def test_handover(wm, tc, family, rows, cols, checked):
    """ME, f32, F >= 2.  Opt-in hand-over (wm_set_handover): its 44 totals against wm_gram of the same plane; checked
    hand-over (the default): y and a bit-identical to the embed without any hand-over, scores to the Gram grouping's rounding
    (NaN for a zero W).  A singular frame rides along: it passes through and scores 0.0 with WM_UNSOLVABLE"""
    torch = tc
    F = 4 if rows == R else 2
    W = H.zero_w(rows, cols) if family == "zero_w" else H.watermark(rows, cols)
    if family == "letterbox":
        xs = [H.letterbox(rows, cols, 12, lv, frame=f) for f, lv in enumerate((0, 16, 0))]
    else:
        xs = [H.clipped(rows, cols, frame=f) for f in range(F - 1)]
    xs = np.stack(xs + [H.singular("plane", rows, cols)])
    eng = wm.Watermark(rows, cols, W, 3, 25.0, max_frames=F)
    ref = wm.Watermark(rows, cols, W, 3, 25.0, max_frames=F)
    eng.set_fused(False)
    ref.set_fused(False)
    ref.set_checked_handover(False)
    if checked:
        eng.set_checked_handover(True)
    else:
        eng.set_checked_handover(False)
        eng.set_handover(True)
    eng.prof_enable(True)
    xd = dev(torch, xs)
    y, a, st = embed_batch(wm, torch, eng, xd, xd, "ME")
    if not checked:
        buf = (C.c_double * (44 * F))()
        sp = slot_plane(wm, rows, cols, F)
        assert wm.lib().wm_gram(eng._ctx, C.byref(sp), buf, 0) == 0
        tot_ho = np.array(buf[:], np.float64).reshape(F, 44)
        tot_ref = ref.gram_totals(y).reshape(F, 44)
        scale = np.abs(tot_ref).max(axis=1, keepdims=True)
        np.testing.assert_allclose(tot_ho / scale, tot_ref / scale, rtol=0, atol=2e-15)
    sp = slot_plane(wm, rows, cols, F)
    corr = np.zeros(F, np.float32)
    cst = np.zeros(F, np.int32)
    eng.detect_async(sp, wm.MASK_TYPE.ME, 0, corr.ctypes.data_as(C.POINTER(C.c_float)), cst.ctypes.data_as(C.POINTER(C.c_int)))
    eng.sync(0)
    rep = eng.prof_report()
    assert ("k_gram_ho" in rep) or checked, rep
    if checked:
        t, rd = eng.checked_handover_counts()
        assert t >= F - 1 and rd == 0, (t, rd)  # (every solvable frame trusted, none redone)
    y2, a2, st2 = embed_batch(wm, torch, ref, xd, xd, "ME")
    assert torch.equal(bits(y), bits(y2)) and np.array_equal(a.view(np.uint32), a2.view(np.uint32)) and np.array_equal(st, st2)
    c2, cst2 = detect_batch(wm, ref, y2, "ME")
    assert np.array_equal(cst, cst2)
    for f in range(F):
        if np.isnan(c2[f]):
            assert np.isnan(corr[f])
        else:
            assert corr[f] == pytest.approx(c2[f], abs=2e-7)
    assert st[F - 1] == O.UNSOLVABLE and cst[F - 1] == O.UNSOLVABLE and corr[F - 1] == 0.0
    assert torch.equal(bits(y[F - 1]), bits(xd[F - 1]))
    if rows == R:
        yn = y.cpu().numpy()
        for f in range(F):
            yo = check_embed(f"ho {family} f{f}", yn[f], a[f], st[f], xs[f], xs[f], W, 3, 25.0, "ME")
            check_score(f"ho {family} f{f}", corr[f], cst[f], yo, W, 3, "ME")
    eng.close()
    ref.close()


# ---- key banks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("mask,p", [("ME", 3), ("NVF", 3), ("NVF", 5)])
def test_keys_with_a_zero_key(wm, tc, dtype, mask, p):
    """a bank whose key 2 was never filled: wm_embed_keys' copies and strengths bit-identical per key to wm_embed with the key
    as W (the zero key: copies == base, a = +inf), wm_detect_keys' scores bit-identical to wm_detect (the zero key: NaN; an
    unsolvable frame: 0.0 for every key)"""
    torch = tc
    cols = 516
    names, xs = mixed_batch(R, cols, dtype)
    F, K = len(names), 4
    Ws = [H.watermark(R, cols) * (0.5 + k) if k != 2 else None for k in range(K)]
    Ws[1] = np.ascontiguousarray(Ws[1][::-1])
    keys = wm.KeySet(R, cols, K)
    for k in range(K):
        if Ws[k] is not None:
            keys.set(k, Ws[k])
    assert not keys.plane(2).any()
    Ws[2] = H.zero_w(R, cols)
    xd = dev(torch, xs)
    eng = wm.Watermark(R, cols, Ws[0], p, 40.0, max_frames=F)
    copies, a = eng.makeWatermarkKeys(xd, xd, keys, wm.MASK_TYPE[mask])
    mark = copies[:, 0].contiguous()
    scores = eng.detectKeys(mark, keys, wm.MASK_TYPE[mask])
    for k in range(K):
        ek = sweeps(wm, R, cols, Ws[k], p, 40.0, F, rps=0)
        y, ar, st = embed_batch(wm, torch, ek, xd, xd, mask)
        assert torch.equal(bits(copies[:, k]), bits(y)), k
        ok = st == 0
        assert np.array_equal(a[ok, k].view(np.uint32), ar[ok].view(np.uint32)), (k, a[:, k], ar)
        assert np.isnan(a[~ok, k]).all()
        c, cst = detect_batch(wm, ek, mark, mask)
        assert np.array_equal(scores[:, k].view(np.uint32), c.view(np.uint32)), (k, scores[:, k], c)
        if k == 2:
            assert (a[ok, k] == np.inf).all() and torch.equal(bits(copies[:, k]), bits(xd))
            assert np.isnan(c[cst == 0]).all() and (c[cst != 0] == 0.0).all()
        ek.close()
    # the oracle on the copies of one solvable frame per key
    f = names.index("clipped")
    for k in range(K):
        check_embed(f"keys k{k}", copies[f, k].cpu().numpy(), a[f, k], 0, xs[f], xs[f], Ws[k], p, 40.0, mask)
    eng.close()
    keys.close()


# ---- row bands --------------------------------------------------------------------------------------------------------------
def run_bands(wm, torch, x, W, world, mask):
    """the host-exchange band protocol of test_gpu_bands.py on one frame: (status of the solve, stitched y, a, corr)"""
    bands = importlib.import_module("watermarking-gpu_amd.bands")
    rows, cols = x.shape
    mk = wm.MASK_TYPE[mask]
    xd = dev(torch, x)
    engs, views = [], []
    for r in range(world):
        g0, g1, lo, hi = bands.band_with_halo(rows, r, world)
        e = wm.Watermark(g1 - g0, cols, np.ascontiguousarray(W[g0:g1]), 3, 40.0)
        e.band_configure(lo, hi, rows)
        engs.append((e, g0, g1, lo, hi))
        views.append(xd[g0:g1].contiguous())
    try:
        tot = sum(e.gram_totals(v) for (e, *_), v in zip(engs, views))
        if mask == "ME":
            sts = [e.band_solve(tot) for (e, *_) in engs]
            assert len(set(sts)) == 1
            if sts[0] != 0:
                return sts[0], None, None, None
        st = [e.band_stats(v, mk) for (e, *_), v in zip(engs, views)]
        mx, ss = max(s[0] for s in st), sum(s[1] for s in st)
        y = xd.clone()
        a = None
        for (e, g0, g1, lo, hi), v in zip(engs, views):
            out = v.clone()
            a = e.band_embed(v, v, out, mk, mx, ss)
            y[g0 + lo:g0 + hi] = out[lo:hi]
        toty = sum(e.gram_totals(y[g0:g1].contiguous()) for (e, g0, g1, lo, hi) in engs)
        sums = np.zeros(3)
        for (e, g0, g1, lo, hi) in engs:
            if e.band_solve(toty) != 0:
                return 0, y, a, 0.0
            sums += np.array(e.band_detect_sums(y[g0:g1].contiguous(), mk))
        with np.errstate(invalid="ignore"):
            corr = float(np.float32(sums[0]) / np.float32(np.sqrt(sums[2]) * np.sqrt(sums[1])))
        return 0, y, a, corr
    finally:
        for e, *_ in engs:
            e.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mask", ["ME", "NVF"])
def test_bands(wm, tc, world, mask):
    """impulses at the band seams, letterbox bars that fill whole bands (world 3), a zero-energy flat frame (NVF), a singular
    frame (ME: every band's solve says WM_UNSOLVABLE): stitched embed and summed detector sums against the oracle"""
    torch = tc
    bands = importlib.import_module("watermarking-gpu_amd.bands")
    rows, cols = 120, 516
    W = H.watermark(rows, cols)
    seams = [bands.band_rows(rows, r, world)[0] for r in range(1, world)]
    spots = {k: v for k, v in H.impulse_spots(rows, cols, band_rows=seams).items() if k.startswith("band")}
    imp, items = H.impulse(rows, cols, spots)
    cases = [(f"impulse {n}", x) for x, (n, _, _) in zip(imp, items)]
    if world == 3:
        k = bands.band_rows(rows, 0, world)[1]
        cases += [("bars16", H.letterbox(rows, cols, k, 16)), ("bars0", H.letterbox(rows, cols, k, 0))]
    cases += [("flat77", H.flat(rows, cols, 77.0)), ("ramp", H.singular("ramp", rows, cols))]
    for name, x in cases:
        so, yo, ao = O.embed(x, x, W, mask=omask(mask))
        st, y, a, corr = run_bands(wm, torch, x, W, world, mask)
        assert st == so, (name, st, so)
        if so != 0:
            continue
        if ao == np.inf:
            assert a == np.inf and torch.equal(bits(y), bits(dev(torch, x))), (name, a)
        else:
            assert a == pytest.approx(ao, rel=TOL_A), (name, a, ao)
            assert float(np.abs(y.cpu().numpy() - yo).max()) <= TOL_Y, name
        sd, cd = O.detect(y.cpu().numpy(), W, mask=omask(mask))
        if sd != 0:
            assert corr == 0.0, name
        else:
            assert corr == pytest.approx(cd, abs=TOL_CORR), (name, corr, cd)
