"""wm_detect_tiles: the detector's three sums kept per tile of the frame (k_detect_tiles + k_tiles_fold).  Tile scores against the
CPU oracle restated per tile (tests/tiles_model.py, <= 1e-5, the bound of every other detector test), the two outputs against
each other and against wm_detect, the bit equalities the call promises, the splice experiment, the edge cases, the enqueue
semantics and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hard_frames as H
import oracle_lib as O
import tiles_model as TM
from synth import synth_frame, synth_watermark
from test_gpu_offsets import SHAPES as OFFSET_SHAPES, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_SHAPES = [s for _, s in OFFSET_SHAPES]  # (64, 256) twice, (270, 480), (271, 483), (1078, 1918), (2160, 3840)
MASKS = [(0, 3), (1, 3), (1, 5), (1, 9)]
W_SEED = 5100


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames_of(R, Cc, F, dtype, first=0):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def tile_shapes(R, Cc):
    """32x32, 64x128, 128x64 and one tile larger than the plane"""
    return [(32, 32), (64, 128), (128, 64), ((R + 15) // 8 * 8, (Cc + 7) // 4 * 4)]


_model = {}


def model(tag, x, W, p, mask, shapes):
    """{tile shape: (map, sums)} of one frame from the oracle, kept per (tag): the F = 1 and F = 5 cases share frames"""
    if tag not in _model:
        if len(_model) > 64:
            _model.clear()
        st, prod = TM.pixel_products(x, W, p, mask)
        assert st == 0
        _model[tag] = {ts: TM.sums_of(prod, *ts) for ts in shapes}
    return {ts: (TM.score_of(s), s) for ts, s in _model[tag].items()}


def compared_tiles(R, ny, nx):
    """all tiles on shapes of at most 300 rows; the four corner tiles plus one interior tile on the large shapes"""
    if R <= 300:
        return [(i, j) for i in range(ny) for j in range(nx)]
    return sorted({(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (ny // 2, nx // 2)})


PARITY = [(i, mk, p, dt, F) for i in range(len(IMG_SHAPES)) for (mk, p) in MASKS for dt in ("f32", "u8") for F in (1, 5)]


@pytest.mark.parametrize("idx,mask,p,dtype,F", PARITY)
def test_oracle_parity(wm, torch_cuda, idx, mask, p, dtype, F):
    """|map - restatement| <= 1e-5 for the tile shapes 32x32, 64x128, 128x64 and one larger than the plane.  No compared tile is
    NaN and the largest |score| of a case exceeds 1e-4 (the frames are textured everywhere, W is N(0, 1))"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    shapes = tile_shapes(R, Cc)
    W = synth_watermark(R, Cc, W_SEED + idx)
    xs = frames_of(R, Cc, F, dtype, first=idx)
    eng = wm.Watermark(R, Cc, W, p, 40.0, max_frames=F)
    xt = torch.from_numpy(xs).cuda()
    worst, largest, ncmp = 0.0, 0.0, 0
    for ts in shapes:
        got = eng.detectTiles(xt, ts[0], ts[1], wm.MASK_TYPE(mask))
        ny, nx = wm.Watermark.tiles_shape(R, Cc, *ts)
        assert got.shape == (F, ny, nx) and (ny, nx) == TM.tiles_shape(R, Cc, *ts)
        for f in range(F):
            ref = model((idx, mask, p, dtype, idx + f), xs[f], W, p, mask, shapes)[ts][0]
            for (i, j) in compared_tiles(R, ny, nx):
                g, r = float(got[f, i, j]), float(ref[i, j])
                assert np.isfinite(g) and np.isfinite(r), (ts, f, i, j, g, r)
                worst, largest, ncmp = max(worst, abs(g - r)), max(largest, abs(r)), ncmp + 1
                assert abs(g - r) <= TOL, (ts, f, i, j, g, r)
    print(f"{R}x{Cc} mask {mask} p {p} {dtype} F {F}: {ncmp} tiles, worst |diff| {worst:.2e}, largest |score| {largest:.4f}")
    assert ncmp >= F * len(shapes) and largest > 1e-4
    eng.close()


CONSISTENCY = [(i, mk, p, dt) for i in (1, 2, 3, 4) for (mk, p) in ((0, 3), (1, 3), (1, 7)) for dt in ("f32", "u8")]


@pytest.mark.parametrize("idx,mask,p,dtype", CONSISTENCY)
def test_outputs_are_consistent(wm, torch_cuda, idx, mask, p, dtype):
    """map equals the score expression evaluated in numpy from sums_dev to <= 1 ulp of f32 (both sides are correctly rounded
    IEEE operations), and the score formed from the sums added over all tiles agrees with wm_detect on the sweeps to <= 2e-7
    (wm.h: a regrouping of the same sums)"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F = 3
    W = synth_watermark(R, Cc, W_SEED + 40 + idx)
    xt = torch.from_numpy(frames_of(R, Cc, F, dtype, first=7)).cuda()
    eng = wm.Watermark(R, Cc, W, p, 40.0, max_frames=F)
    eng.set_fused(False)
    whole = np.asarray(eng.detectWatermark(xt, wm.MASK_TYPE(mask)), np.float32)
    for ts in tile_shapes(R, Cc):
        m, s = eng.detectTiles(xt, ts[0], ts[1], wm.MASK_TYPE(mask), sums=True)
        assert s.dtype == np.float64 and s.shape == m.shape + (3,)
        again = TM.score_of(s)
        assert np.isfinite(m).all()
        assert np.all(np.abs(m.astype(np.float64) - again.astype(np.float64)) <= np.spacing(np.abs(again))), (ts, m, again)
        total = TM.score_of(s.sum(axis=(1, 2)))
        assert np.all(np.abs(total.astype(np.float64) - whole.astype(np.float64)) <= 2e-7), (ts, total, whole)
    eng.close()


def _bits(m, s):
    return m.view(np.uint32), s.view(np.uint64)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("idx,mask,p,dtype", [(2, 0, 3, "f32"), (3, 0, 3, "f32"), (3, 1, 5, "u8"), (4, 1, 3, "f32"), (5, 0, 3, "u8")])
def test_bit_equalities(wm, torch_cuda, idx, mask, p, dtype):
    """as uint32 / uint64 views: three repeats of one call, a batch of F frames against F one-frame calls, a WM_MEM_HOST plane
    against the same plane on the device"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F = 5
    mt = wm.MASK_TYPE(mask)
    xs = frames_of(R, Cc, F, dtype, first=3)
    xt = torch.from_numpy(xs).cuda()
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, W_SEED + 80 + idx), p, 40.0, max_frames=F)
    for (th, tw) in ((32, 32), (128, 64)):
        a = _bits(*eng.detectTiles(xt, th, tw, mt, sums=True))
        for _ in range(2):
            assert _same(a, _bits(*eng.detectTiles(xt, th, tw, mt, sums=True)))
        for f in range(F):
            one = _bits(*eng.detectTiles(xt[f], th, tw, mt, sums=True))
            assert np.array_equal(one[0], a[0][f]) and np.array_equal(one[1], a[1][f]), (th, tw, f)
        ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
        hx = np.ascontiguousarray(xs)
        ph = wm.wm_plane(hx.ctypes.data, R, Cc, 1, wm.WM_U8 if dtype == "u8" else wm.WM_F32, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
        mh = torch.empty((F, ny, nx), dtype=torch.float32, device="cuda")
        sh = torch.empty((F, ny, nx, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.detect_tiles_async(ph, th, tw, mt, wm.WM_SLOT_SYNC, mh, sh)
        assert _same(a, _bits(mh.cpu().numpy(), sh.cpu().numpy()))
    eng.close()


@pytest.mark.parametrize("idx,mask", [(3, 0), (3, 1), (4, 0)])
def test_host_plane_u8_odd_width(wm, torch_cuda, idx, mask):
    """The one combination test_bit_equalities leaves out, because bit equality is not promised there (wm.h): a u8 plane whose
    width is not a multiple of 4, under ME or NVF p = 3.  On the device its rows are not dword-aligned, so the sweep takes the
    generic strips; the WM_MEM_HOST copy is staged at a pitch rounded up to 4, so it takes the overlapped strips plus one
    generic strip.  The same products are then grouped differently in the lanes that hold the last columns: the two maps agree
    to <= 2e-7, the bound wm.h states for a regrouping of the same sums, and both are within the oracle's bound"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    assert Cc % 4 != 0
    F, th, tw = 2, 32, 32
    mt = wm.MASK_TYPE(mask)
    W = synth_watermark(R, Cc, W_SEED + 100 + idx)
    xs = frames_of(R, Cc, F, "u8", first=9)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, max_frames=F)
    md, sd = eng.detectTiles(torch.from_numpy(xs).cuda(), th, tw, mt, sums=True)
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    hx = np.ascontiguousarray(xs)
    ph = wm.wm_plane(hx.ctypes.data, R, Cc, 1, wm.WM_U8, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
    mh = torch.empty((F, ny, nx), dtype=torch.float32, device="cuda")
    sh = torch.empty((F, ny, nx, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.detect_tiles_async(ph, th, tw, mt, wm.WM_SLOT_SYNC, mh, sh)
    got = mh.cpu().numpy()
    assert np.isfinite(md).all() and float(np.abs(md).max()) > 1e-4
    assert float(np.abs(got.astype(np.float64) - md.astype(np.float64)).max()) <= 2e-7, (got, md)
    assert np.allclose(sh.cpu().numpy()[..., 1:], sd[..., 1:], rtol=1e-5, atol=0.0)  # (the two sums of squares: no cancellation)
    if R <= 300:
        ref = TM.tile_map(xs[1], W, th, tw, 3, mask)[1]
        assert float(np.abs(got[1] - ref).max()) <= TOL and float(np.abs(md[1] - ref).max()) <= TOL
    eng.close()


@pytest.mark.parametrize("idx", [2, 4])
def test_slot_out_and_handover(wm, torch_cuda, idx):
    """WM_MEM_SLOT_OUT after an embed: with the hand-over off the bits are those of the output tensor passed directly; with the
    hand-over on (the Gram sums come from the embed: another summation order) the scores agree to <= 2e-7"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F, th, tw = 2, 64, 128
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, W_SEED + 120 + idx), 3, 40.0, nslots=1, max_frames=F)
    xb = torch.from_numpy(frames_of(R, Cc, F, "f32", first=5)).cuda()
    yb = torch.empty_like(xb)
    ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
    for ho in (False, True):
        eng.set_handover(ho)
        ms = torch.empty((F, ny, nx), dtype=torch.float32, device="cuda")
        ss = torch.empty((F, ny, nx, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
        eng.detect_tiles_async(ps, th, tw, wm.MASK_TYPE.ME, 0, ms, ss)
        eng.sync(0)
        eng.set_handover(False)
        md, sd = eng.detectTiles(yb, th, tw, wm.MASK_TYPE.ME, sums=True)
        got = ms.cpu().numpy()
        assert float(np.abs(md).min()) > 0.3  # (the frames are marked: every tile responds)
        if not ho:
            assert _same(_bits(md, sd), _bits(got, ss.cpu().numpy()))
        else:
            assert float(np.abs(got.astype(np.float64) - md.astype(np.float64)).max()) <= 2e-7, (got, md)
    eng.close()


# the splice: a 360 x 480 rectangle of the unmarked frame pasted into the marked one
SPL_R, SPL_C, SPL_TH, SPL_TW = 1080, 1920, 128, 128
SPL_AT, SPL_SIZE, SPL_SEED = (384, 640), (360, 480), 8100


def splice_classes(R, Cc, th, tw, at, size):
    """boolean [ny, nx]: tiles wholly inside the splice, tiles the splice touches (+-1 pixel)"""
    ny, nx = TM.tiles_shape(R, Cc, th, tw)
    ti, tj = np.indices((ny, nx))
    r_lo, r_hi = ti * th, np.where(ti == ny - 1, R, (ti + 1) * th)
    c_lo, c_hi = tj * tw, np.where(tj == nx - 1, Cc, (tj + 1) * tw)
    (r0, c0), (sr, sc) = at, size
    inside = (r_lo >= r0) & (r_hi <= r0 + sr) & (c_lo >= c0) & (c_hi <= c0 + sc)
    touched = (r_lo < r0 + sr + 1) & (r_hi > r0 - 1) & (c_lo < c0 + sc + 1) & (c_hi > c0 - 1)
    return inside, touched


@pytest.mark.parametrize("mask,dtype", [(0, "f32"), (0, "u8"), (1, "f32"), (1, "u8")])
def test_localises_a_splice(wm, torch_cuda, mask, dtype):
    """A 1080x1920 frame marked with a generated key (psnr 40, p = 3), a 360x480 rectangle of the unmarked frame spliced in at
    (384, 640), the copy floored to u8 in two cases, 128x128 tiles: every tile the splice does not touch (+-1 pixel: 100 of 120)
    scores >= 0.35 (ME) / >= 0.20 (NVF), each of the 6 tiles wholly inside the splice and every tile of the unmarked frame has
    |s| <= 0.10.

    The CPU oracle on these very cases (tests/tiles_model.py; the key from the generator's host twin synth_watermark, the
    embed by the oracle), as whole frame / untouched tiles min .. max / largest |s| inside the splice / largest |s| of the
    unmarked frame:
      ME  f32:  0.5082 / 0.5224 .. 0.5717 / 0.0387 / 0.0450
      ME  u8:   0.5076 / 0.5212 .. 0.5712 / 0.0402 / 0.0461
      NVF f32:  0.2825 / 0.2823 .. 0.3300 / 0.0159 / 0.0266
      NVF u8:   0.2823 / 0.2824 .. 0.3297 / 0.0150 / 0.0266
    so the thresholds leave 1.4x below the weakest untouched tile and 2.1x above the strongest tile without a mark."""
    torch = torch_cuda
    R, Cc, th, tw = SPL_R, SPL_C, SPL_TH, SPL_TW
    (r0, c0), (sr, sc) = SPL_AT, SPL_SIZE
    mt = wm.MASK_TYPE(mask)
    eng = wm.Watermark.generated(R, Cc, SPL_SEED, 3, 40.0)
    xt = torch.from_numpy(synth_frame(R, Cc, frame=mask)).cuda()
    y, a = eng.makeWatermark(xt, xt, mt)
    z = y.clone()
    z[r0:r0 + sr, c0:c0 + sc] = xt[r0:r0 + sr, c0:c0 + sc]
    plain = xt
    if dtype == "u8":
        z, plain = z.to(torch.uint8), xt.to(torch.uint8)  # (truncation of values in [0, 255])
    inside, touched = splice_classes(R, Cc, th, tw, SPL_AT, SPL_SIZE)
    assert int(inside.sum()) == 6 and int((~touched).sum()) == 100
    m = eng.detectTiles(z, th, tw, mt)
    u = eng.detectTiles(plain, th, tw, mt)
    print("untouched", float(m[~touched].min()), float(m[~touched].max()), "inside", float(np.abs(m[inside]).max()), "unmarked", float(np.abs(u).max()))
    assert np.isfinite(m).all() and np.isfinite(u).all()
    assert float(m[~touched].min()) >= (0.35 if mask == 0 else 0.20), m
    assert float(np.abs(m[inside]).max()) <= 0.10, m
    assert float(np.abs(u).max()) <= 0.10, u
    eng.close()


def test_unsolvable_frame_and_zero_w(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, F, th, tw = 270, 480, 5, 32, 64
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 200)
    xs = frames_of(R, Cc, F, "f32")
    xs[2] = 100.0  # constant frame: singular prediction system
    eng = wm.Watermark(R, Cc, W, 3, 40.0, max_frames=F)
    mp = torch.full((F, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    sm = torch.full((F, ny, nx, 3), 7.0, dtype=torch.float64, device="cuda")
    st = np.full(F, -5, np.int32)
    torch.cuda.synchronize()
    eng.detect_tiles_async(torch.from_numpy(xs).cuda(), th, tw, wm.MASK_TYPE.ME, 0, mp, sm, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    m, s = mp.cpu().numpy(), sm.cpu().numpy()
    assert list(st) == [0, 0, 1, 0, 0]
    assert np.all(m[2] == 0.0) and np.all(s[2] == 0.0)
    for f in (1, 3):
        ref = TM.tile_map(xs[f], W, th, tw)[1]
        assert float(np.abs(m[f] - ref).max()) <= TOL
    eng.close()
    # a zero W scores NaN in every tile with status OK: wm_detect's zero-W rule, per tile
    ez = wm.Watermark(R, Cc, H.zero_w(R, Cc), 3, 40.0, max_frames=2)
    mz = torch.zeros((2, ny, nx), dtype=torch.float32, device="cuda")
    sz = np.full(2, -5, np.int32)
    torch.cuda.synchronize()
    ez.detect_tiles_async(torch.from_numpy(xs[:2]).cuda(), th, tw, wm.MASK_TYPE.NVF, 0, mz, None, sz)
    assert ez.sync(0) == wm.WM_OK and list(sz) == [0, 0]
    assert np.isnan(mz.cpu().numpy()).all()
    ez.close()


@pytest.mark.parametrize("mask,dtype", [(0, "f32"), (1, "f32"), (1, "u8")])
def test_flat_patch(wm, torch_cuda, mask, dtype):
    """one flat 64x64 patch at (30, 62) in a textured 270x480 frame, 32x32 tiles.  Under NVF the mask is exactly 0 where the 3x3
    window lies in the patch, so u = 0 there and e_u = 0 one pixel further in: rows 32..91, columns 64..123.  Tile (1, 2) -- rows
    32..63, columns 64..95 -- is the one tile wholly inside: ||e_u||^2 = 0, the score is 0/0 = NaN.  Under ME m = |e_w| is a
    non-zero constant inside the patch (the coefficients do not add up to 1), so no tile is NaN.  Every other tile is finite and
    within the oracle's bound"""
    torch = torch_cuda
    R, Cc, th, tw = 270, 480, 32, 32
    x = synth_frame(R, Cc, frame=4, dtype=np.uint8 if dtype == "u8" else np.float32)
    x[30:94, 62:126] = H.flat(64, 64, 77, dtype=x.dtype)
    W = synth_watermark(R, Cc, W_SEED + 220)
    eng = wm.Watermark(R, Cc, W, 3, 40.0)
    m = eng.detectTiles(torch.from_numpy(x).cuda(), th, tw, wm.MASK_TYPE(mask))
    st, ref, _ = TM.tile_map(x, W, th, tw, 3, mask)
    want_nan = np.zeros(m.shape, bool)
    if mask == 1:
        want_nan[1, 2] = True
    assert st == 0 and np.array_equal(np.isnan(ref), want_nan)
    assert np.array_equal(np.isnan(m), want_nan), m
    assert float(np.abs(m[~want_nan] - ref[~want_nan]).max()) <= TOL
    eng.close()


def test_argument_errors_on_a_device(wm, torch_cuda):
    """the refusals come back before anything is queued: wm_sync then returns WM_OK and the slot stays usable"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc = 64, 256
    W = synth_watermark(R, Cc, W_SEED + 240)
    eng = wm.Watermark(R, Cc, W, 3, 40.0)
    e5 = wm.Watermark(R, Cc, W, 5, 40.0)
    x = synth_frame(R, Cc)
    xt = torch.from_numpy(x).cuda()
    pl = wm.plane_of(xt, 1)
    mp = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pm = C.c_void_p(mp.data_ptr())
    call = lambda th, tw, img=C.byref(pl), m=pm, ctx=eng._ctx, mask=0: L.wm_detect_tiles(ctx, mask, img, th, tw, m, None, None, 0)
    bad = wm.WM_ERR_BAD_ARG
    for (th, tw) in ((24, 32), (36, 32), (32, 28), (32, 34), (0, 32), (32, 0), (-32, 32), (32, -32), (31, 32), (32, 30)):
        assert call(th, tw) == bad, (th, tw)
    assert call(32, 32, img=None) == bad and call(32, 32, m=None) == bad and call(32, 32, mask=2) == bad
    assert call(32, 32, ctx=e5._ctx) == wm.WM_ERR_BAD_P
    assert L.wm_detect_tiles(eng._ctx, 0, C.byref(pl), 32, 32, pm, None, None, 9) == bad  # (no such slot)
    assert eng.sync(0) == wm.WM_OK  # nothing was queued
    assert call(32, 32) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    ref = TM.tile_map(x, W, 32, 32)[1]
    assert float(np.abs(mp.cpu().numpy() - ref).max()) <= TOL
    # NVF takes p = 5
    assert call(32, 32, ctx=e5._ctx, mask=1) == wm.WM_OK and e5.sync(0) == wm.WM_OK
    assert float(np.abs(mp.cpu().numpy() - TM.tile_map(x, W, 32, 32, 5, 1)[1]).max()) <= TOL
    # band mode refuses the call
    eb = wm.Watermark(R, Cc, W, 3, 40.0)
    assert L.wm_band_configure(eb._ctx, 8, 40, 128) == wm.WM_OK
    assert call(32, 32, ctx=eb._ctx) == bad
    for e in (eng, e5, eb):
        e.close()


def test_enqueue_order(wm, torch_cuda):
    """one slot shared with wm_embed, wm_detect and wm_detect_keys in mixed order: one wm_sync delivers every result"""
    torch = torch_cuda
    R, Cc, th, tw = 270, 480, 64, 128
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 260)
    kb = wm.KeySet(R, Cc, 2)
    kb.set(1, W)
    x = synth_frame(R, Cc, frame=2)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2)
    xt = torch.from_numpy(x).cuda()
    y0 = torch.empty_like(xt)
    a0, c_det, c_det2 = (C.c_float * 1)(), (C.c_float * 1)(), (C.c_float * 1)()
    ck = np.zeros(2, np.float32)
    m_x = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    m_y = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    s_y = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
    m_n = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    st_x, st_y = np.full(1, -5, np.int32), np.full(1, -5, np.int32)
    torch.cuda.synchronize()
    eng.detect_tiles_async(xt, th, tw, wm.MASK_TYPE.ME, 0, m_x, None, st_x)  # the unmarked frame first
    eng.embed_async(xt, xt, y0, wm.MASK_TYPE.ME, 0, a0)
    eng.detect_async(y0, wm.MASK_TYPE.ME, 0, c_det)
    eng.detect_tiles_async(y0, th, tw, wm.MASK_TYPE.ME, 0, m_y, s_y, st_y)
    eng.detect_keys_async(y0, kb, wm.MASK_TYPE.ME, 0, ck)
    eng.detect_tiles_async(xt, th, tw, wm.MASK_TYPE.NVF, 1, m_n)  # another slot in between
    eng.detect_async(xt, wm.MASK_TYPE.ME, 0, c_det2)
    assert eng.sync(0) == wm.WM_OK and eng.sync(1) == wm.WM_OK
    assert list(st_x) == [0] and list(st_y) == [0]
    yo = y0.cpu().numpy()
    assert float(np.abs(m_x.cpu().numpy() - TM.tile_map(x, W, th, tw)[1]).max()) <= TOL
    assert float(np.abs(m_y.cpu().numpy() - TM.tile_map(yo, W, th, tw)[1]).max()) <= TOL
    assert float(np.abs(m_n.cpu().numpy() - TM.tile_map(x, W, th, tw, 3, 1)[1]).max()) <= TOL
    assert abs(c_det[0] - O.detect(yo, W)[1]) <= TOL and abs(float(ck[1]) - O.detect(yo, W)[1]) <= TOL
    assert abs(c_det2[0] - O.detect(x, W)[1]) <= TOL and np.isnan(ck[0])
    total = float(TM.score_of(s_y.cpu().numpy().sum(axis=(0, 1))))
    assert abs(total - float(ck[1])) <= 2e-7, (total, ck)
    assert float(m_y.cpu().numpy().min()) > 0.3 > float(np.abs(m_x.cpu().numpy()).max())
    eng.close()
    kb.close()


CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 270, C = 480;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    for (int m = 0; m < 2; ++m) {
        int ny = 0, nx = 0;
        const std::vector<float> s = w.detectTiles(img, 64, 128, m == 0 ? ME : NVF, &ny, &nx);
        if (ny != 4 || nx != 3 || s.size() != 12) return 4;
        for (float v : s) printf("%.9g\n", v);
    }
    if (w.detectTiles(img, 512, 512, ME).size() != 1) return 5;
    try { w.detectTiles(img, 36, 32, ME); return 3; } catch (const std::runtime_error&) {}
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc = 270, 480
    src = tmp_path / "tiles.cpp"
    src.write_text(CPP)
    exe = tmp_path / "tiles"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    x = synth_frame(R, Cc, frame=6)
    xf = tmp_path / "x.f32"
    x.tofile(xf)
    W = synth_watermark(R, Cc, W_SEED + 280)
    wf = tmp_path / "w.dat"
    W.tofile(wf)
    out = subprocess.run([str(exe), str(xf), str(wf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.array([float(v) for v in out.stdout.split()], np.float32).reshape(2, 4, 3)
    eng = wm.Watermark(R, Cc, W, 3, 40.0)
    xt = torch.from_numpy(x).cuda()
    for m, mk in enumerate((wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF)):
        assert np.array_equal(got[m], eng.detectTiles(xt, 64, 128, mk)), (m, got[m])
    eng.close()
