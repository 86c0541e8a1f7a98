"""wm_detect_keys_tiles: the detector's three sums kept per tile of the frame and per key of a bank (k_detect_keys_tiles +
k_keys_tiles_fold).  Key k's map and sums against wm_detect_tiles on an engine whose W is key k (bit for bit), the bit equalities
the call promises, the CPU oracle restated per tile (tests/tiles_model.py, <= 1e-5), the outputs against each other and against
wm_detect_keys, the mosaic experiment, the edge cases, the refusals, the enqueue semantics and the C++ surface."""
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
from test_gpu_tiles import compared_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_SHAPES = [s for _, s in OFFSET_SHAPES]
SMALL = [IMG_SHAPES.index(s) for s in ((64, 256), (270, 480), (271, 483))]
LARGE = IMG_SHAPES.index((1078, 1918))
MASKS = [(0, 3), (1, 3), (1, 5), (1, 9)]
KEY_SEED = 6100


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames_of(R, Cc, F, dtype, first=0):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def keys_of(R, Cc, K, seed):
    return [synth_watermark(R, Cc, seed + k) for k in range(K)]


def bank_of(wm, R, Cc, Ws):
    kb = wm.KeySet(R, Cc, len(Ws))
    for k, W in enumerate(Ws):
        if W is not None:
            kb.set(k, W)
    return kb


def tile_shapes(R, Cc):
    """32x32, 128x64 and one tile larger than the plane"""
    return [(32, 32), (128, 64), ((R + 15) // 8 * 8, (Cc + 7) // 4 * 4)]


def _bits(m, s):
    return np.ascontiguousarray(m).view(np.uint32), np.ascontiguousarray(s).view(np.uint64)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. bit-equal to wm_detect_tiles per key ------------------------------------------------------------------------------------
PER_KEY = [(i, mk, p, dt, F) for i in SMALL for (mk, p) in MASKS for dt in ("f32", "u8") for F in (1, 5)] + [(LARGE, 0, 3, "f32", 1)]


@pytest.mark.parametrize("idx,mask,p,dtype,F", PER_KEY)
def test_equals_detect_tiles_per_key(wm, torch_cuda, idx, mask, p, dtype, F):
    """for each key k of a bank of K = 3 (a short last group), map and sums as uint32 / uint64 views equal wm_detect_tiles on an
    engine created with key k as W"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    K = 3
    mt = wm.MASK_TYPE(mask)
    Ws = keys_of(R, Cc, K, KEY_SEED + 10 * idx)
    kb = bank_of(wm, R, Cc, Ws)
    engs = [wm.Watermark(R, Cc, W, p, 40.0, max_frames=F) for W in Ws]
    xt = torch.from_numpy(frames_of(R, Cc, F, dtype, first=idx)).cuda()
    for (th, tw) in tile_shapes(R, Cc):
        m, s = engs[0].detectKeysTiles(xt, kb, th, tw, mt, sums=True)
        ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
        assert m.shape == (F, K, ny, nx) and m.dtype == np.float32 and s.shape == (F, K, ny, nx, 3) and s.dtype == np.float64
        assert np.isfinite(m).all()
        for k in range(K):
            rm, rs = engs[k].detectTiles(xt, th, tw, mt, sums=True)
            assert _same(_bits(m[:, k], s[:, k]), _bits(rm, rs)), (th, tw, k)
    for e in engs:
        e.close()
    kb.close()


# ---- 2. bit equalities of the call itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,mask,p,dtype", [(SMALL[1], 0, 3, "f32"), (SMALL[2], 0, 3, "f32"), (SMALL[2], 1, 5, "u8"), (SMALL[1], 1, 3, "u8"),
                                              (SMALL[0], 1, 9, "f32")])
def test_bit_equalities(wm, torch_cuda, idx, mask, p, dtype):
    """as uint32 / uint64 views: three repeats of one call; a batch of 5 against 5 one-frame calls; key k in a bank of 5 against a
    bank of 1 that holds only that key (its position in the group, the short last group); a WM_MEM_HOST plane against the same
    plane on the device (f32 planes and widths that are multiples of 4)"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F, K = 5, 5
    mt = wm.MASK_TYPE(mask)
    Ws = keys_of(R, Cc, K, KEY_SEED + 100 + 10 * idx)
    kb = bank_of(wm, R, Cc, Ws)
    singles = [bank_of(wm, R, Cc, [W]) for W in Ws]
    xs = frames_of(R, Cc, F, dtype, first=3)
    xt = torch.from_numpy(xs).cuda()
    eng = wm.Watermark(R, Cc, Ws[0], p, 40.0, max_frames=F)
    for (th, tw) in ((32, 32), (128, 64)):
        a = _bits(*eng.detectKeysTiles(xt, kb, th, tw, mt, sums=True))
        for _ in range(2):
            assert _same(a, _bits(*eng.detectKeysTiles(xt, kb, th, tw, mt, sums=True)))
        for f in range(F):
            one = _bits(*eng.detectKeysTiles(xt[f], kb, th, tw, mt, sums=True))
            assert np.array_equal(one[0], a[0][f]) and np.array_equal(one[1], a[1][f]), (th, tw, f)
        for k in range(K):
            one = _bits(*eng.detectKeysTiles(xt, singles[k], th, tw, mt, sums=True))
            assert np.array_equal(one[0][:, 0], a[0][:, k]) and np.array_equal(one[1][:, 0], a[1][:, k]), (th, tw, k)
        if dtype == "f32" or Cc % 4 == 0:
            ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
            hx = np.ascontiguousarray(xs)
            ph = wm.wm_plane(hx.ctypes.data, R, Cc, 1, wm.WM_U8 if dtype == "u8" else wm.WM_F32, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
            mh = torch.empty((F, K, ny, nx), dtype=torch.float32, device="cuda")
            sh = torch.empty((F, K, ny, nx, 3), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng.detect_keys_tiles_async(ph, kb, th, tw, mt, wm.WM_SLOT_SYNC, mh, sh)
            assert _same(a, _bits(mh.cpu().numpy(), sh.cpu().numpy())), (th, tw)
    eng.close()
    for b in singles + [kb]:
        b.close()


# ---- 3. oracle parity ---------------------------------------------------------------------------------------------------------------
PARITY = [(i, mk, p, dt) for i in SMALL for (mk, p) in MASKS for dt in ("f32", "u8")]


@pytest.mark.parametrize("idx,mask,p,dtype", PARITY)
def test_oracle_parity(wm, torch_cuda, idx, mask, p, dtype):
    """|map - restatement| <= 1e-5 per key for two frames, three keys and the tile shapes 32x32, 128x64 and one larger than the
    plane.  Every compared score is finite and the largest |score| of a case exceeds 1e-4"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F, K = 2, 3
    shapes = tile_shapes(R, Cc)
    Ws = keys_of(R, Cc, K, KEY_SEED + 200 + 10 * idx)
    kb = bank_of(wm, R, Cc, Ws)
    xs = frames_of(R, Cc, F, dtype, first=idx + 1)
    eng = wm.Watermark(R, Cc, Ws[0], p, 40.0, max_frames=F)
    xt = torch.from_numpy(xs).cuda()
    got = {ts: eng.detectKeysTiles(xt, kb, ts[0], ts[1], wm.MASK_TYPE(mask)) for ts in shapes}
    worst, largest, ncmp = 0.0, 0.0, 0
    for f in range(F):
        for k in range(K):
            st, prod = TM.pixel_products(xs[f], Ws[k], p, mask)
            assert st == 0
            for ts in shapes:
                ref = TM.score_of(TM.sums_of(prod, *ts))
                ny, nx = TM.tiles_shape(R, Cc, *ts)
                assert got[ts].shape == (F, K, ny, nx)
                for (i, j) in compared_tiles(R, ny, nx):
                    g, r = float(got[ts][f, k, i, j]), float(ref[i, j])
                    assert np.isfinite(g) and np.isfinite(r), (ts, f, k, i, j, g, r)
                    worst, largest, ncmp = max(worst, abs(g - r)), max(largest, abs(g)), ncmp + 1
                    assert abs(g - r) <= TOL, (ts, f, k, i, j, g, r)
    print(f"{R}x{Cc} mask {mask} p {p} {dtype}: {ncmp} scores, worst |diff| {worst:.2e}, largest |score| {largest:.4f}")
    assert ncmp >= F * K * len(shapes) and largest > 1e-4
    eng.close()
    kb.close()


# ---- 4. consistency -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,mask,p,dtype", [(i, mk, p, dt) for i in SMALL for (mk, p) in ((0, 3), (1, 3), (1, 7)) for dt in ("f32", "u8")])
def test_outputs_are_consistent(wm, torch_cuda, idx, mask, p, dtype):
    """map equals the score expression evaluated in numpy from sums_dev to <= 1 ulp of f32; the score formed from the sums added
    over all tiles agrees with wm_detect_keys on the same bank to <= 2e-7 (a regrouping of the same products); the ||e_w||^2 sums
    do not depend on the key: bit-equal across keys"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F, K = 3, 3
    Ws = keys_of(R, Cc, K, KEY_SEED + 300 + 10 * idx)
    kb = bank_of(wm, R, Cc, Ws)
    xt = torch.from_numpy(frames_of(R, Cc, F, dtype, first=7)).cuda()
    eng = wm.Watermark(R, Cc, Ws[0], p, 40.0, max_frames=F)
    whole = np.asarray(eng.detectKeys(xt, kb, wm.MASK_TYPE(mask)), np.float32)
    assert whole.shape == (F, K)
    for ts in tile_shapes(R, Cc):
        m, s = eng.detectKeysTiles(xt, kb, ts[0], ts[1], wm.MASK_TYPE(mask), sums=True)
        again = TM.score_of(s)
        assert np.isfinite(m).all()
        assert np.all(np.abs(m.astype(np.float64) - again.astype(np.float64)) <= np.spacing(np.abs(again))), (ts, m, again)
        total = TM.score_of(s.sum(axis=(2, 3)))
        assert np.all(np.abs(total.astype(np.float64) - whole.astype(np.float64)) <= 2e-7), (ts, total, whole)
        nw = np.ascontiguousarray(s[..., 2]).view(np.uint64)
        for k in range(1, K):
            assert np.array_equal(nw[:, k], nw[:, 0]), (ts, k)
    eng.close()
    kb.close()


# ---- 5. the mosaic ------------------------------------------------------------------------------------------------------------------
MOS_R, MOS_C, MOS_T = 1080, 1920, 128
MOS_SEEDS = [9100, 9101, 9102, 9103]


@pytest.mark.parametrize("mask,dtype", [(0, "f32"), (0, "u8"), (1, "f32"), (1, "u8")])
def test_mosaic_of_three_colluders(wm, torch_cuda, mask, dtype):
    """A 1080x1920 frame marked once per key of a generated bank of four (psnr 40, p = 3); tile (i, j) of the 128x128 grid of the
    suspect copy is taken from copy (i + 2 j) % 3, key 3 is never used; the copy is floored to u8 in two cases.  In every one of the
    120 tiles the owning key scores >= 0.35 (ME) / >= 0.20 (NVF), every other key -- key 3 included -- has |s| <= 0.10, and the
    argmax over the keys is the tile's source.

    The CPU oracle on these very cases (tests/tiles_model.py; keys from the generator's host twin synth_watermark, the embeds by
    the oracle), as whole frame keys 0..3 / owning key min .. max over the 120 tiles / largest |s| of any other key:
      ME  f32 and u8:  0.195 0.193 0.193 0.005 / 0.506 .. 0.580 / 0.067
      NVF f32 and u8:  0.102 0.102 0.104 0.000 / 0.284 .. 0.332 (u8: 0.331) / 0.044
    so the thresholds leave 1.4x below the weakest owned tile and 1.5x above the strongest foreign one."""
    torch = torch_cuda
    R, Cc, T = MOS_R, MOS_C, MOS_T
    mt = wm.MASK_TYPE(mask)
    kb = wm.KeySet.from_seeds(R, Cc, MOS_SEEDS)
    eng = wm.Watermark.generated(R, Cc, 8100, 3, 40.0)  # (the engine's own W plays no part)
    xt = torch.from_numpy(synth_frame(R, Cc, frame=mask)).cuda()
    copies, a = eng.makeWatermarkKeys(xt, xt, kb, mt)
    ny, nx = wm.Watermark.tiles_shape(R, Cc, T, T)
    assert (ny, nx) == (8, 15) and copies.shape == (4, R, Cc)
    ti = torch.clamp(torch.arange(R, device="cuda") // T, max=ny - 1)[:, None]
    tj = torch.clamp(torch.arange(Cc, device="cuda") // T, max=nx - 1)[None, :]
    src = (ti + 2 * tj) % 3
    z = torch.where(src == 0, copies[0], torch.where(src == 1, copies[1], copies[2]))
    if dtype == "u8":
        z = z.to(torch.uint8)  # (truncation of values in [0, 255])
    m = eng.detectKeysTiles(z, kb, T, T, mt)
    whole = eng.detectKeys(z, kb, mt)
    assert m.shape == (4, ny, nx) and np.isfinite(m).all()
    owner = (np.arange(ny)[:, None] + 2 * np.arange(nx)[None, :]) % 3
    own = np.take_along_axis(m, owner[None], axis=0)[0]
    foreign = np.abs(np.where(np.arange(4)[:, None, None] == owner[None], 0.0, m))
    print("whole frame", whole, "owning key", float(own.min()), "..", float(own.max()), "largest foreign |s|", float(foreign.max()))
    assert float(own.min()) >= (0.35 if mask == 0 else 0.20), own
    assert float(foreign.max()) <= 0.10, foreign
    assert np.array_equal(np.argmax(m, axis=0), owner)
    eng.close()
    kb.close()


# ---- 6. unsolvable frame and zero key -------------------------------------------------------------------------------------------
def test_unsolvable_frame_and_zero_key(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, F, K, th, tw = 270, 480, 5, 3, 32, 64
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    Ws = keys_of(R, Cc, K, KEY_SEED + 400)
    kb = bank_of(wm, R, Cc, Ws)
    xs = frames_of(R, Cc, F, "f32")
    xs[2] = 100.0  # constant frame: singular prediction system
    eng = wm.Watermark(R, Cc, Ws[0], 3, 40.0, max_frames=F)
    mp = torch.full((F, K, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    sm = torch.full((F, K, ny, nx, 3), 7.0, dtype=torch.float64, device="cuda")
    st = np.full(F, -5, np.int32)
    torch.cuda.synchronize()
    eng.detect_keys_tiles_async(torch.from_numpy(xs).cuda(), kb, th, tw, wm.MASK_TYPE.ME, 0, mp, sm, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    m, s = mp.cpu().numpy(), sm.cpu().numpy()
    assert list(st) == [0, 0, 1, 0, 0]
    assert np.all(m[2] == 0.0) and np.all(s[2] == 0.0)
    for f in (1, 3):
        for k in range(K):
            ref = TM.tile_map(xs[f], Ws[k], th, tw)[1]
            assert float(np.abs(m[f, k] - ref).max()) <= TOL, (f, k)
    kb.close()
    # a bank whose key 1 was never set (planes start at zero): NaN for key 1 only, status OK
    kz = bank_of(wm, R, Cc, [Ws[0], None, Ws[2]])
    for mask in (0, 1):
        mz = torch.zeros((2, K, ny, nx), dtype=torch.float32, device="cuda")
        sz = np.full(2, -5, np.int32)
        torch.cuda.synchronize()
        eng.detect_keys_tiles_async(torch.from_numpy(xs[:2]).cuda(), kz, th, tw, wm.MASK_TYPE(mask), 0, mz, None, sz)
        assert eng.sync(0) == wm.WM_OK and list(sz) == [0, 0]
        z = mz.cpu().numpy()
        assert np.isnan(z[:, 1]).all() and np.isfinite(z[:, 0]).all() and np.isfinite(z[:, 2]).all()
        for k in (0, 2):
            assert float(np.abs(z[1, k] - TM.tile_map(xs[1], Ws[k], th, tw, 3, mask)[1]).max()) <= TOL, (mask, k)
    eng.close()
    kz.close()


def test_flat_patch_under_nvf(wm, torch_cuda):
    """test_gpu_tiles.test_flat_patch's frame: under NVF tile (1, 2) of the 32x32 grid lies wholly inside the flat patch, its
    ||e_u||^2 is 0 for EVERY key and its score NaN; every other tile of every key is finite and within the oracle's bound"""
    torch = torch_cuda
    R, Cc, th, tw, K = 270, 480, 32, 32, 3
    x = synth_frame(R, Cc, frame=4)
    x[30:94, 62:126] = H.flat(64, 64, 77, dtype=x.dtype)
    Ws = keys_of(R, Cc, K, KEY_SEED + 420)
    kb = bank_of(wm, R, Cc, Ws)
    eng = wm.Watermark(R, Cc, Ws[0], 3, 40.0)
    m = eng.detectKeysTiles(torch.from_numpy(x).cuda(), kb, th, tw, wm.MASK_TYPE.NVF)
    want_nan = np.zeros(m.shape[1:], bool)
    want_nan[1, 2] = True
    for k in range(K):
        st, ref, _ = TM.tile_map(x, Ws[k], th, tw, 3, 1)
        assert st == 0 and np.array_equal(np.isnan(ref), want_nan)
        assert np.array_equal(np.isnan(m[k]), want_nan), (k, m[k])
        assert float(np.abs(m[k][~want_nan] - ref[~want_nan]).max()) <= TOL
    eng.close()
    kb.close()


# ---- 7. argument errors on a device ---------------------------------------------------------------------------------------------
def test_argument_errors_on_a_device(wm, torch_cuda):
    """the refusals come back before anything is queued: wm_sync then returns WM_OK and the slot stays usable.  (A bank on another
    device needs a second device; the grid beyond 31 bits is test_refuses_a_fold_grid_beyond_31_bits)"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc, K = 64, 256, 3
    Ws = keys_of(R, Cc, K, KEY_SEED + 440)
    kb = bank_of(wm, R, Cc, Ws)
    other = wm.KeySet(R, Cc + 4, 1)
    eng = wm.Watermark(R, Cc, Ws[0], 3, 40.0)
    e5 = wm.Watermark(R, Cc, Ws[0], 5, 40.0)
    x = synth_frame(R, Cc)
    xt = torch.from_numpy(x).cuda()
    pl = wm.plane_of(xt, 1)
    mp = torch.zeros((K, 2, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pm = C.c_void_p(mp.data_ptr())

    def call(th, tw, img=C.byref(pl), keys=kb.handle, m=pm, ctx=eng._ctx, mask=0, slot=0):
        return L.wm_detect_keys_tiles(ctx, mask, img, keys, th, tw, m, None, None, slot)

    bad = wm.WM_ERR_BAD_ARG
    for (th, tw) in ((24, 32), (36, 32), (32, 28), (32, 34), (0, 32), (32, 0), (-32, 32), (32, -32), (31, 32), (32, 30)):
        assert call(th, tw) == bad, (th, tw)
    assert call(32, 32, img=None) == bad and call(32, 32, keys=None) == bad and call(32, 32, m=None) == bad and call(32, 32, mask=2) == bad
    assert call(32, 32, keys=other.handle) == bad  # a bank of another shape
    assert call(32, 32, ctx=e5._ctx) == wm.WM_ERR_BAD_P
    assert call(32, 32, slot=9) == bad and call(32, 32, slot=-3) == bad  # (no such slot)
    if L.wm_device_count() > 1:
        far = wm.KeySet(R, Cc, 1, device=1)
        assert call(32, 32, keys=far.handle) == bad
        far.close()
    eb = wm.Watermark(R, Cc, Ws[0], 3, 40.0)
    assert L.wm_band_configure(eb._ctx, 8, 40, 128) == wm.WM_OK
    assert call(32, 32, ctx=eb._ctx) == bad  # band mode refuses the call
    assert eng.sync(0) == wm.WM_OK  # nothing was queued
    assert call(32, 32) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    got = mp.cpu().numpy()
    for k in range(K):
        assert float(np.abs(got[k] - TM.tile_map(x, Ws[k], 32, 32)[1]).max()) <= TOL
    # NVF takes p = 5
    assert call(32, 32, ctx=e5._ctx, mask=1) == wm.WM_OK and e5.sync(0) == wm.WM_OK
    got = mp.cpu().numpy()
    for k in range(K):
        assert float(np.abs(got[k] - TM.tile_map(x, Ws[k], 32, 32, 5, 1)[1]).max()) <= TOL
    for e in (eng, e5, eb):
        e.close()
    kb.close()
    other.close()


def test_refuses_a_fold_grid_beyond_31_bits(wm, torch_cuda):
    """frames * nkeys * ny * nx beyond 2^31 - 1 is WM_ERR_BAD_ARG before any device work: a 384x352 engine with max_frames = 4096,
    a bank of WM_KEYS_MAX = 4096 keys (2.2 GB of zero planes) and 32x32 tiles (12 x 11 = 132 tiles): 4096 * 4096 * 132 = 2.21e9.
    The sweep's grid for that call (2 strips x 12 segments x 4096 frames x 2048 key groups = 2.0e8) fits, so the fold grid is what
    answers.  wm_sync then returns WM_OK and the slot still works"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc, F, K = 384, 352, 4096, wm.WM_KEYS_MAX
    assert wm.Watermark.tiles_shape(R, Cc, 32, 32) == (12, 11) and F * K * 132 > 2**31 - 1
    big = wm.KeySet(R, Cc, K)
    two = wm.KeySet(R, Cc, 2)
    eng = wm.Watermark.generated(R, Cc, 5, 3, 40.0, nslots=1, max_frames=F)
    xb = torch.empty((F, R, Cc), dtype=torch.uint8, device="cuda")
    xb[0] = torch.from_numpy(synth_frame(R, Cc, dtype=np.uint8)).cuda()
    pl = wm.plane_of(xb, 1)
    mp = torch.zeros((2, 12, 11), dtype=torch.float32, device="cuda")  # (the refused call writes nothing: its map is never touched)
    torch.cuda.synchronize()
    pm = C.c_void_p(mp.data_ptr())
    assert L.wm_detect_keys_tiles(eng._ctx, 0, C.byref(pl), big.handle, 32, 32, pm, None, None, 0) == wm.WM_ERR_BAD_ARG
    assert "31 bits" in L.wm_last_error(eng._ctx).decode()
    assert eng.sync(0) == wm.WM_OK  # nothing was queued
    assert float(mp.abs().max()) == 0.0
    # the slot still works: frame 0 against the bank of two (zero) keys: status OK, NaN everywhere
    st = np.full(1, -5, np.int32)
    eng.detect_keys_tiles_async(xb[0], two, 32, 32, wm.MASK_TYPE.ME, 0, mp, None, st)
    assert eng.sync(0) == wm.WM_OK and list(st) == [0]
    assert np.isnan(mp.cpu().numpy()).all()
    eng.close()
    big.close()
    two.close()


# ---- 8. one slot shared with other calls ----------------------------------------------------------------------------------------
def test_enqueue_order(wm, torch_cuda):
    """one slot shared with wm_embed, wm_detect_keys and wm_detect_tiles in mixed order, a second slot in between: one wm_sync per
    slot delivers every result"""
    torch = torch_cuda
    R, Cc, th, tw = 270, 480, 64, 128
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    Ws = keys_of(R, Cc, 3, KEY_SEED + 460)
    W = Ws[1]
    kb = bank_of(wm, R, Cc, Ws)
    x = synth_frame(R, Cc, frame=2)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2)  # the embeds mark with key 1
    xt = torch.from_numpy(x).cuda()
    y0 = torch.empty_like(xt)
    a0 = (C.c_float * 1)()
    ck = np.zeros(3, np.float32)
    kt_x = torch.zeros((3, ny, nx), dtype=torch.float32, device="cuda")
    kt_y = torch.zeros((3, ny, nx), dtype=torch.float32, device="cuda")
    ks_y = torch.zeros((3, ny, nx, 3), dtype=torch.float64, device="cuda")
    kt_n = torch.zeros((3, ny, nx), dtype=torch.float32, device="cuda")
    t_y = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    t_x = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    st_x, st_y = np.full(1, -5, np.int32), np.full(1, -5, np.int32)
    torch.cuda.synchronize()
    eng.detect_keys_tiles_async(xt, kb, th, tw, wm.MASK_TYPE.ME, 0, kt_x, None, st_x)  # the unmarked frame first
    eng.embed_async(xt, xt, y0, wm.MASK_TYPE.ME, 0, a0)
    eng.detect_tiles_async(y0, th, tw, wm.MASK_TYPE.ME, 0, t_y)
    eng.detect_keys_tiles_async(y0, kb, th, tw, wm.MASK_TYPE.ME, 0, kt_y, ks_y, st_y)
    eng.detect_keys_async(y0, kb, wm.MASK_TYPE.ME, 0, ck)
    eng.detect_keys_tiles_async(xt, kb, th, tw, wm.MASK_TYPE.NVF, 1, kt_n)  # another slot in between
    eng.detect_tiles_async(xt, th, tw, wm.MASK_TYPE.ME, 0, t_x)
    assert eng.sync(0) == wm.WM_OK and eng.sync(1) == wm.WM_OK
    assert list(st_x) == [0] and list(st_y) == [0]
    yo = y0.cpu().numpy()
    for k in range(3):
        assert float(np.abs(kt_x.cpu().numpy()[k] - TM.tile_map(x, Ws[k], th, tw)[1]).max()) <= TOL
        assert float(np.abs(kt_y.cpu().numpy()[k] - TM.tile_map(yo, Ws[k], th, tw)[1]).max()) <= TOL
        assert float(np.abs(kt_n.cpu().numpy()[k] - TM.tile_map(x, Ws[k], th, tw, 3, 1)[1]).max()) <= TOL
    # key 1 is the engine's W: the per-key map's plane 1 is wm_detect_tiles' map of the same plane, bit for bit
    assert np.array_equal(kt_y.cpu().numpy()[1].view(np.uint32), t_y.cpu().numpy().view(np.uint32))
    total = TM.score_of(ks_y.cpu().numpy().sum(axis=(1, 2)))
    assert np.all(np.abs(total.astype(np.float64) - ck.astype(np.float64)) <= 2e-7), (total, ck)
    assert abs(float(ck[1]) - O.detect(yo, W)[1]) <= TOL
    assert float(np.abs(t_x.cpu().numpy() - TM.tile_map(x, W, th, tw)[1]).max()) <= TOL
    m = kt_y.cpu().numpy()
    assert float(m[1].min()) > 0.3 > float(np.abs(m[[0, 2]]).max()) and float(np.abs(kt_x.cpu().numpy()).max()) < 0.3
    eng.close()
    kb.close()


@pytest.mark.parametrize("idx", [SMALL[1], LARGE])
def test_slot_out_and_handover(wm, torch_cuda, idx):
    """WM_MEM_SLOT_OUT after an embed: with the hand-over off the bits are those of the output tensor passed directly; with the
    hand-over on (the Gram sums come from the embed: another summation order) the scores agree to <= 2e-7"""
    torch = torch_cuda
    R, Cc = IMG_SHAPES[idx]
    F, K, th, tw = 2, 3, 64, 128
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    Ws = keys_of(R, Cc, K, KEY_SEED + 480 + idx)
    kb = bank_of(wm, R, Cc, Ws)
    eng = wm.Watermark(R, Cc, Ws[2], 3, 40.0, nslots=1, max_frames=F)
    xb = torch.from_numpy(frames_of(R, Cc, F, "f32", first=5)).cuda()
    yb = torch.empty_like(xb)
    ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
    for ho in (False, True):
        eng.set_handover(ho)
        ms = torch.empty((F, K, ny, nx), dtype=torch.float32, device="cuda")
        ss = torch.empty((F, K, ny, nx, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
        eng.detect_keys_tiles_async(ps, kb, th, tw, wm.MASK_TYPE.ME, 0, ms, ss)
        eng.sync(0)
        eng.set_handover(False)
        md, sd = eng.detectKeysTiles(yb, kb, th, tw, wm.MASK_TYPE.ME, sums=True)
        got = ms.cpu().numpy()
        assert float(md[:, 2].min()) > 0.3  # (the frames are marked with key 2: every tile responds)
        if not ho:
            assert _same(_bits(md, sd), _bits(got, ss.cpu().numpy()))
        else:
            assert float(np.abs(got.astype(np.float64) - md.astype(np.float64)).max()) <= 2e-7, (got, md)
    eng.close()
    kb.close()


# ---- 9. C++ surface -----------------------------------------------------------------------------------------------------------------
CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 270, C = 480, K = 3;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    WatermarkKeys keys(R, C, K);
    for (int k = 0; k < K; ++k) keys.load(k, argv[2 + k]);
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    for (int m = 0; m < 2; ++m) {
        int ny = 0, nx = 0;
        const std::vector<float> s = w.detectKeysTiles(img, keys, 64, 128, m == 0 ? ME : NVF, &ny, &nx);
        if (ny != 4 || nx != 3 || s.size() != (size_t)K * 12) return 4;
        for (float v : s) printf("%.9g\n", v);
    }
    if (w.detectKeysTiles(img, keys, 512, 512, ME).size() != (size_t)K) return 5;
    try { w.detectKeysTiles(img, keys, 36, 32, ME); return 3; } catch (const std::runtime_error&) {}
    WatermarkKeys small(R, C - 4, 1);
    try { w.detectKeysTiles(img, small, 64, 128, ME); return 6; } catch (const std::runtime_error&) {}
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc, K = 270, 480, 3
    src = tmp_path / "keys_tiles.cpp"
    src.write_text(CPP)
    exe = tmp_path / "keys_tiles"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    x = synth_frame(R, Cc, frame=6)
    xf = tmp_path / "x.f32"
    x.tofile(xf)
    Ws = keys_of(R, Cc, K, KEY_SEED + 500)
    files = []
    for k, W in enumerate(Ws):
        files.append(tmp_path / f"w{k}.dat")
        W.tofile(files[-1])
    out = subprocess.run([str(exe), str(xf)] + [str(p) for p in files], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.array([float(v) for v in out.stdout.split()], np.float32).reshape(2, K, 4, 3)
    kb = bank_of(wm, R, Cc, Ws)
    eng = wm.Watermark(R, Cc, Ws[0], 3, 40.0)
    xt = torch.from_numpy(x).cuda()
    for m, mk in enumerate((wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF)):
        assert np.array_equal(got[m], eng.detectKeysTiles(xt, kb, 64, 128, mk)), (m, got[m])
    eng.close()
    kb.close()
