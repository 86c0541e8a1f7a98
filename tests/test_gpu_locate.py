"""wm_locate: the offset of a crop anywhere in its key, by FFT (wm_k_locate.hip, wm_k_fft.hip), against the f64 model of
tests/locate_model.py run with the DEVICE's own coefficients (wm_compute_mask's coef_out on a context of the crop's shape).

Map parity: every map value within 1e-4 sigma_W, sigma_W = ||h||_2 rms(key plane): two orders above an f32 transform's error, below
the 0.06-0.6 sigma_W by which a zero-border adjoint misses, four orders below any misplacement.  The identity on the device:
map[oy][ox] is sums_dev[0] of wm_detect_tiles with one tile on a context whose W is the window, to the same bound.  Finding the crop:
the argmax is the true offset in every marked case, peak and z agree with the model's to 1e-3 relative, and the model itself stays
inside z >= 15 (marked) and z <= 6 (unmarked), so that the inputs stay meaningful.  Then the rules of wm.h: key == image, a zero
key, an unsolvable frame, equal bits over batch and repetition, either output alone, the order of the refusals, the record cap, the
hand-over left as it was.  Measured figures: DESIGN.md section 24."""
import ctypes as C

import numpy as np
import pytest

import hard_frames as H
import layouts as LY
import locate_model as M
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

MAP_BOUND = 1e-4   # of sigma_W
REL_BOUND = 1e-3   # peak and z against the model's
Z_MARKED, Z_UNMARKED = 15.0, 6.0
# (key shape, image shape, true offset)
CASES = [((80, 300), (64, 256), (16, 44)), ((120, 330), (64, 256), (20, 31)), ((270, 480), (200, 384), (37, 53)),
         ((300, 520), (96, 128), (150, 300)), ((301, 523), (271, 483), (0, 0)), ((301, 523), (271, 483), (30, 40)),
         ((70, 4100), (64, 256), (3, 3001)), ((4100, 260), (64, 256), (3001, 2))]
F = 3  # two marked frames and an unmarked one
_keys, _frames = {}, {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def key_of(kshape):
    if kshape not in _keys:
        _keys[kshape] = synth_watermark(*kshape, seed=9100 + 7 * kshape[0] + kshape[1])
    return _keys[kshape]


def frames_of(wm, torch, kshape, shape, at, mask, p, dtype):
    """[F, rows, cols]: frames 0 and 1 marked with the key at its shape (psnr 40) and cropped at `at`, frame 2 the unmarked crop;
    u8: floored"""
    tag = (kshape, shape, at, mask, p)
    if tag not in _frames:
        (r, c), (oy, ox) = shape, at
        emb = wm.Watermark(kshape[0], kshape[1], key_of(kshape), p, 40.0)
        out = []
        for f in range(F):
            xt = torch.from_numpy(synth_frame(*kshape, frame=10 + f)).cuda()
            y = emb.makeWatermark(xt, xt, wm.MASK_TYPE(mask))[0] if f < F - 1 else xt
            out.append(y[oy:oy + r, ox:ox + c].cpu().numpy())
        emb.close()
        _frames.clear()  # (one shape's frames at a time)
        _frames[tag] = np.stack(out)
    x = _frames[tag]
    return np.floor(x).astype(np.uint8) if dtype == "u8" else x


def coefficients(wm, torch, xs):
    """the device's own solve per frame: wm_compute_mask's coef_out under ME on a p = 3 context of the frames' shape"""
    eng = wm.Watermark(xs.shape[1], xs.shape[2], np.ones(xs.shape[1:], np.float32), 3, 40.0, max_frames=len(xs))
    _, _, c, st = eng.computeMask(torch.from_numpy(xs).cuda(), wm.MASK_TYPE.ME)
    eng.close()
    assert list(st) == [0] * len(xs)
    return c


def check_case(wm, torch, kshape, shape, at, mask, p, dtype, nframes=F):
    keys = wm.KeySet(kshape[0], kshape[1], 2)
    keys.set(1, key_of(kshape))
    xs = frames_of(wm, torch, kshape, shape, at, mask, p, dtype)[:nframes]
    xt = torch.from_numpy(xs).cuda()
    eng = wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), p, 40.0, max_frames=F)
    loc, mp = eng.locate(xt, keys, 1, wm.MASK_TYPE(mask), want_map=True)
    mp = mp.cpu().numpy()
    cs = coefficients(wm, torch, xs)
    worst = 0.0
    for f in range(nframes):
        want, (oy, ox, peak, z) = M.locate(xs[f], key_of(kshape), cs[f], mask, p)
        sw = M.sigma_w(xs[f], key_of(kshape), cs[f], mask, p)
        err = float(np.abs(mp[f] - want).max()) / sw
        worst = max(worst, err)
        print(f"{kshape}->{shape}@{at} mask {mask} p {p} {dtype} frame {f}: map error {err:.2e} sigma_W; device {loc[f]} model ({oy}, {ox}, {peak:.6g}, {z:.2f})")
        assert err <= MAP_BOUND
        if f < F - 1:
            assert (oy, ox) == at and z >= Z_MARKED                      # the model: the input is meaningful
            assert (int(loc[f][0]), int(loc[f][1])) == at                # the device finds the crop
        else:
            assert z <= Z_UNMARKED
        if (int(loc[f][0]), int(loc[f][1])) == (oy, ox):
            assert abs(loc[f][2] - peak) <= REL_BOUND * abs(peak) and abs(loc[f][3] - z) <= REL_BOUND * abs(z)
            assert loc[f][2] == mp[f][oy, ox]
    # one frame alone, and the batch again: equal bits
    l1, m1 = eng.locate(xt[0], keys, 1, wm.MASK_TYPE(mask), want_map=True)
    assert np.array_equal(LY.raw(l1), LY.raw(loc[0])) and np.array_equal(LY.raw(m1), LY.raw(mp[0]))
    l2, m2 = eng.locate(xt, keys, 1, wm.MASK_TYPE(mask), want_map=True)
    assert np.array_equal(LY.raw(l2), LY.raw(loc)) and np.array_equal(LY.raw(m2), LY.raw(mp))
    eng.close()
    keys.close()
    return worst


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", CASES)
def test_map_parity_and_finding_the_crop(wm, torch_cuda, kshape, shape, at, mask):
    for dtype in ("f32", "u8"):
        check_case(wm, torch_cuda, kshape, shape, at, mask, 3, dtype)


def test_nvf_window_5(wm, torch_cuda):
    check_case(wm, torch_cuda, (120, 330), (64, 256), (20, 31), 1, 5, "f32")


def test_full_size(wm, torch_cuda):
    """key 2200 x 3900 -> image 2160 x 3840 at (17, 33), f32 ME: a 4096 x 4096 transform against the f64 FFT model"""
    check_case(wm, torch_cuda, (2200, 3900), (2160, 3840), (17, 33), 0, 3, "f32", nframes=1)


def one_tile(n, unit, least=32):
    """a tile size (a multiple of `unit`, >= least) of which an axis of n holds exactly one"""
    t = max(least, (n // 2 // unit + 1) * unit)
    assert n // t == 1 or n < t
    return t


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", [CASES[1], CASES[2], CASES[5]])
def test_identity_on_the_device(wm, torch_cuda, kshape, shape, at, mask):
    """map[oy][ox] = the detector's <e_u, e_w> against the window there (wm_detect_tiles' sums_dev[0] with one tile), at the true
    offset and two others; and wm_detect_offsets with ny = nx = 1 at the found offset gives the detector's score"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    key = key_of(kshape)
    keys = wm.KeySet(kshape[0], kshape[1], 1)
    keys.set(0, key)
    xs = frames_of(wm, torch, kshape, shape, at, mask, 3, "f32")
    xt = torch.from_numpy(xs[0]).cuda()
    eng = wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), 3, 40.0)
    loc, mp = eng.locate(xt, keys, 0, mt, want_map=True)
    mp = mp.cpu().numpy()
    c = coefficients(wm, torch, xs[:1])[0]
    sw = M.sigma_w(xs[0], key, c, mask)
    ny, nx = mp.shape
    for (oy, ox) in (at, (0, 0), (ny - 1, nx - 1)):
        win = np.ascontiguousarray(key[oy:oy + shape[0], ox:ox + shape[1]])
        det = wm.Watermark(shape[0], shape[1], win, 3, 40.0)
        _, sums = det.detectTiles(xt, one_tile(shape[0], 8), one_tile(shape[1], 4), mt, sums=True)
        assert sums.shape == (1, 1, 3)
        print(f"({oy}, {ox}): map {mp[oy, ox]:.9g} <e_u, e_w> {sums[0, 0, 0]:.9g} ({abs(mp[oy, ox] - sums[0, 0, 0]) / sw:.2e} sigma_W)")
        assert abs(mp[oy, ox] - sums[0, 0, 0]) <= MAP_BOUND * sw
        if (oy, ox) == at:
            score = eng.detectOffsets(xt, keys, 0, int(loc[0]), int(loc[1]), 1, 1, mt)
            assert (int(loc[0]), int(loc[1])) == at and abs(float(score[0, 0]) - det.detectWatermark(xt, mt)) <= 1e-5 and score[0, 0] > 0.2
        det.close()
    eng.close()
    keys.close()


def test_layouts_and_host_plane(wm, torch_cuda):
    """a pitched batch (tests/layouts.py) and a host plane give the dense device plane's bits, f32 and u8"""
    torch = torch_cuda
    kshape, shape, at = CASES[1]
    keys = wm.KeySet(kshape[0], kshape[1], 1)
    keys.set(0, key_of(kshape))
    eng = wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), 3, 40.0, max_frames=F)
    for dtype in ("f32", "u8"):
        xs = frames_of(wm, torch, kshape, shape, at, 0, 3, dtype)
        want_l, want_m = eng.locate(torch.from_numpy(xs).cuda(), keys, 0, wm.MASK_TYPE.ME, want_map=True)
        for poison in LY.POISON[dtype]:
            _, view = LY.place(torch, xs, LY.make("pitched", shape[0], shape[1], frames=F), poison)
            l, m = eng.locate(view, keys, 0, wm.MASK_TYPE.ME, want_map=True)
            assert np.array_equal(LY.raw(l), LY.raw(want_l)) and np.array_equal(LY.raw(m), LY.raw(want_m))
        hx = np.ascontiguousarray(xs)
        ph = wm.wm_plane(hx.ctypes.data, shape[0], shape[1], 1, wm.WM_U8 if dtype == "u8" else wm.WM_F32, wm.WM_MEM_HOST, F, shape[1], 0,
                         shape[0] * shape[1])
        l = np.zeros((F, 4), np.float32)
        m = torch.zeros_like(want_m)
        eng.locate_async(ph, keys, 0, wm.MASK_TYPE.ME, wm.WM_SLOT_SYNC, l, m)
        assert np.array_equal(LY.raw(l), LY.raw(want_l)) and np.array_equal(LY.raw(m), LY.raw(want_m))
    eng.close()
    keys.close()


def test_rules(wm, torch_cuda):
    torch = torch_cuda
    kshape, shape, at = CASES[1]
    R, Cc = shape
    xs = frames_of(wm, torch, kshape, shape, at, 0, 3, "f32").copy()
    eng = wm.Watermark(R, Cc, np.zeros(shape, np.float32), 3, 40.0, max_frames=F)
    # key == image: one offset, z NaN, the peak is the numerator of the detector against the whole key
    same = wm.KeySet(R, Cc, 2)  # (key 0 stays zero)
    same.set(1, key_of(kshape)[:R, :Cc])
    loc, mp = eng.locate(torch.from_numpy(xs[0]).cuda(), same, 1, wm.MASK_TYPE.NVF, want_map=True)
    c = coefficients(wm, torch, xs[:1])[0]
    want, (_, _, peak, _) = M.locate(xs[0], key_of(kshape)[:R, :Cc], c, 1)
    assert mp.shape == (1, 1) and loc[0] == 0 and loc[1] == 0 and np.isnan(loc[3])
    assert abs(loc[2] - peak) <= MAP_BOUND * M.sigma_w(xs[0], key_of(kshape)[:R, :Cc], c, 1) and loc[2] == float(mp[0, 0])
    # a zero key: a zero map, the first offset, z NaN
    big = wm.KeySet(kshape[0], kshape[1], 2)
    big.set(1, key_of(kshape))
    loc, mp = eng.locate(torch.from_numpy(xs[0]).cuda(), big, 0, wm.MASK_TYPE.ME, want_map=True)
    assert list(loc[:3]) == [0, 0, 0] and np.isnan(loc[3]) and not mp.cpu().numpy().any()
    # an unsolvable frame: status 1, zeros and a zero map; its neighbours in the batch are what they are alone
    alone = eng.locate(torch.from_numpy(xs[0]).cuda(), big, 1, wm.MASK_TYPE.ME, want_map=True)
    xs[1] = H.singular("ramp", R, Cc)
    xt = torch.from_numpy(xs).cuda()
    ny, nx = kshape[0] - R + 1, kshape[1] - Cc + 1
    l = np.full((F, 4), 7.0, np.float32)
    st = np.full(F, -5, np.int32)
    m = torch.full((F, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    eng.locate_async(xt, big, 1, wm.MASK_TYPE.ME, 0, l, m, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    assert list(st) == [0, 1, 0] and not l[1].any() and not m[1].cpu().numpy().any()
    assert np.array_equal(LY.raw(l[0]), LY.raw(alone[0])) and np.array_equal(LY.raw(m[0]), LY.raw(alone[1]))
    # either output alone
    l_only = np.zeros((F, 4), np.float32)
    eng.locate_async(xt, big, 1, wm.MASK_TYPE.ME, 0, l_only, None)
    m_only = torch.zeros_like(m)
    eng.locate_async(xt, big, 1, wm.MASK_TYPE.ME, 0, None, m_only)
    eng.sync(0)
    assert np.array_equal(LY.raw(l_only), LY.raw(l)) and np.array_equal(LY.raw(m_only), LY.raw(m))
    for k in (same, big):
        k.close()
    eng.close()


def test_refusals_in_order_and_record_cap(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc = 64, 256
    bad, badp, busy = wm.WM_ERR_BAD_ARG, wm.WM_ERR_BAD_P, wm.WM_ERR_BUSY
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=2, max_frames=2)
    e5 = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 5, 40.0)
    keys = wm.KeySet(R + 64, Cc + 64, 1)
    small = wm.KeySet(R - 1, Cc + 64, 1)
    wide = wm.KeySet(R, 8200, 1)
    xt = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=f) for f in range(3)])).cuda()
    pl, pl3 = wm.plane_of(xt[0], 1), wm.plane_of(xt, 1)
    loc = (C.c_float * 16)()

    def call(ctx=eng, mask=0, img=pl, kh=keys, k=0, out=loc, mp=None, slot=0):
        return L.wm_locate(ctx._ctx, mask, C.byref(img) if img is not None else None, kh.handle if kh is not None else None, k, out, mp, None, slot)

    def why(ctx=eng):
        return L.wm_last_error(ctx._ctx).decode()

    assert call() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    # each refusal on its own ...
    assert call(mask=7) == bad and call(ctx=e5) == badp
    assert call(img=None) == bad and call(kh=None) == bad and call(out=None) == bad
    assert call(k=1) == bad and call(k=-1) == bad
    assert call(kh=small) == bad and "at least as large" in why()
    assert call(kh=wide) == bad and "transform" in why()
    assert call(slot=2) == bad and "slot" in why()
    assert call(img=pl3) == bad  # three frames on a context of two
    # ... and in the documented order: the earlier check names the failure
    assert call(ctx=e5, img=None) == badp                      # mask before the pointers
    assert call(img=None, k=5) == bad and "null" in why()      # pointers before k
    assert call(k=5, kh=small) == bad and "key 5" in why()     # k before the bank
    assert call(kh=small, slot=9) == bad and "at least as large" in why()  # the bank before the slot
    assert call(kh=wide, slot=9) == bad and "transform" in why()           # the shape before the slot
    assert call(slot=9, img=pl3) == bad and "slot" in why()    # the slot before the plane
    assert L.wm_band_configure(eng._ctx, 8, 40, 128) == wm.WM_OK
    assert call(slot=9) == bad and "band" in why()             # band mode before the slot
    assert call(kh=wide) == bad and "transform" in why()       # the shape before band mode
    assert L.wm_band_configure(eng._ctx, 0, 0, 0) == wm.WM_OK
    # the record cap: frames x 4 count against the slot's 4096
    cb = np.zeros(4096, np.float32)
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)         # 4032
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 1, 61, wm.MASK_TYPE.ME, 0, cb[4032:])   # 4093
    assert call() == busy and "un-synced" in why()
    eng.sync(0)
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 1, 60, wm.MASK_TYPE.ME, 0, cb[4032:])   # 4092: exactly room for one frame
    assert call() == wm.WM_OK
    eng.sync(0)
    for k in (keys, small, wide):
        k.close()
    eng.close()
    e5.close()


def test_hand_over_left_as_it_was(wm, torch_cuda):
    """a wm_locate of another plane queued between an embed and the detector of its output: the detector's result and the
    hand-over counts are those of the sequence without it, and the location is that of a call on its own"""
    torch = torch_cuda
    kshape, shape, at = CASES[1]
    R, Cc = shape
    keys = wm.KeySet(kshape[0], kshape[1], 1)
    keys.set(0, key_of(kshape))
    crop = torch.from_numpy(frames_of(wm, torch, kshape, shape, at, 0, 3, "f32")[:2].copy()).cuda()
    xb = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=40 + f) for f in range(2)])).cuda()
    res = {}
    for ho in (False, True):
        for with_locate in (False, True):
            eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=2)
            eng.set_handover(ho)
            yb = torch.empty_like(xb)
            corr = (C.c_float * 2)()
            loc = np.zeros((2, 4), np.float32)
            eng.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
            if with_locate:
                eng.locate_async(crop, keys, 0, wm.MASK_TYPE.ME, 0, loc)
            ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, 2, Cc, 0, R * Cc)
            eng.detect_async(ps, wm.MASK_TYPE.ME, 0, corr)
            eng.sync(0)
            res[ho, with_locate] = (np.array(corr[:], np.float32), loc.copy(), yb.cpu().numpy())
            if with_locate:
                assert np.array_equal(LY.raw(loc), LY.raw(eng.locate(crop, keys, 0, wm.MASK_TYPE.ME)))
                assert [tuple(int(v) for v in l[:2]) for l in loc] == [at, at]
            eng.close()
        assert np.array_equal(LY.raw(res[ho, True][0]), LY.raw(res[ho, False][0]))
        assert np.array_equal(LY.raw(res[ho, True][2]), LY.raw(res[ho, False][2]))
    keys.close()


def test_scratch_follows_the_key_shape(wm, torch_cuda):
    """calls with banks of different shapes queued on one slot without a sync between them, and a call behind a reconfiguring call
    (which releases the scratch): every result is that of the call on its own"""
    torch = torch_cuda
    shape = (64, 256)
    banks, crops, want = [], [], []
    for (kshape, sh, at) in (CASES[0], CASES[1], CASES[6]):
        assert sh == shape
        k = wm.KeySet(kshape[0], kshape[1], 1)
        k.set(0, key_of(kshape))
        banks.append(k)
        crops.append(torch.from_numpy(frames_of(wm, torch, kshape, sh, at, 0, 3, "f32")[0].copy()).cuda())
    eng = wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), 3, 40.0, nslots=1)
    for k, x in zip(banks, crops):
        want.append(eng.locate(x, k, 0, wm.MASK_TYPE.ME).copy())
    order = (0, 1, 2, 1, 0)
    got = [np.zeros(4, np.float32) for _ in order]
    for g, i in zip(got, order):
        eng.locate_async(crops[i], banks[i], 0, wm.MASK_TYPE.ME, 0, g)
    eng.sync(0)
    for g, i in zip(got, order):
        assert np.array_equal(LY.raw(g), LY.raw(want[i])), i
    eng.configure(2, 2)
    assert np.array_equal(LY.raw(eng.locate(crops[1], banks[1], 0, wm.MASK_TYPE.ME)), LY.raw(want[1]))
    assert [tuple(int(v) for v in w[:2]) for w in want] == [CASES[0][2], CASES[1][2], CASES[6][2]]
    eng.close()
    for k in banks:
        k.close()
