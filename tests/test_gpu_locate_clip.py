"""wm_clip_pool and the wm_locate_*_pooled calls: a clip's frames pooled on the image side into ONE crop search (wm_k_locate.hip
k_clip_pool; wm.h), against the per-frame calls and the f64 model of tests/locate_clip_model.py run with the
DEVICE's own coefficients.

Bit contract: for a clip of one frame (weights NULL, accumulate 0) the pooled calls' maps and records equal wm_locate's,
wm_locate_bits' and wm_locate_keys' as floats -- k_clip_pool forms h through k_locate_e's and k_locate_h's own helpers, and the tails
are the same launches.  Chunking: the pool's raw bits do not depend on how the clip is cut into calls, on pitch, memory kind or
repetition.  Parity: the pooled map within 1e-4 sigma_W (test_gpu_locate.py's MAP_BOUND) of the model, sigma_W = ||h_pool||_2
rms(key), and within 1e-4 (sigma_W + sum |w_f| sigma_W,f) of the weighted sum of wm_locate's own maps.  The point of it: clips on
which no frame reaches z = 15 and the pooled clip does.  Then the rules of wm.h.  Measured figures: DESIGN.md section 27."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bits_model as B
import hard_frames as H
import layouts as LY
import locate_clip_model as LC
import locate_model as M
import test_gpu_locate as TL
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_BOUND, REL_BOUND = TL.MAP_BOUND, 1e-3
Z_MARKED, Z_UNMARKED = LC.Z_MARKED, LC.Z_UNMARKED
NK, OWNER = 5, 3
# the bit contract's shapes: the table's four, a crop that nearly fills its key, and a crop whose last tile of k_clip_pool (64 columns
# x 16 rows) is two columns and one row: its left halo is the neighbouring tile, its right and lower halos are clamped borders
CONTRACT = LC.CASES + [((301, 523), (271, 483), (30, 40)), ((100, 200), (33, 66), (5, 7))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def keyset(wm, planes):
    ks = wm.KeySet(planes[0].shape[0], planes[0].shape[1], len(planes))
    for k, p in enumerate(planes):
        if p.any():
            ks.set(k, p)
    return ks


def bank_of(kshape):
    """five keys: the shape's key at OWNER, a zero plane at 2, three keys that marked nothing"""
    other = [synth_watermark(*kshape, seed=9500 + 13 * k + kshape[1]) for k in range(NK)]
    other[OWNER] = LC.key_of(kshape)
    other[2] = np.zeros(kshape, np.float32)
    return other


def engine(wm, shape, p=3, **kw):
    return wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), p, 40.0, **kw)


def table_of(kshape, nbits=8):
    ty, tx = LC.LB.tiles_shape(kshape[0], kshape[1], 32, 32)
    return (np.arange(ty * tx) % nbits).astype(np.int32)


def same_floats(a, b):
    """equal as floats (a -0 may have become +0), NaN where the other has NaN"""
    a, b = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def contract_case(wm, torch, kshape, shape, at, mask, p, dtype):
    mt = wm.MASK_TYPE(mask)
    x = LC.clip_of(kshape, shape, at, mask, frames=1)[0]
    xt = torch.from_numpy(x.astype(np.uint8) if dtype == "u8" else x).cuda()
    bank = keyset(wm, bank_of(kshape))
    eng = engine(wm, shape, p)
    tb = table_of(kshape)
    pool, st = eng.poolClip(xt, mt)
    assert list(st) == [0]
    loc, mp = eng.locate(xt, bank, OWNER, mt, want_map=True)
    locp, mpp = eng.locatePooled(pool, bank, OWNER, want_map=True)
    assert same_floats(loc, locp) and same_floats(mp, mpp), (loc, locp)
    assert mp.abs().max() > 0
    want = eng.locate_bits(xt, bank, OWNER, 32, 32, tb, 8, mt, want_energy=True, want_maps=True)
    got = eng.locateBitsPooled(pool, bank, OWNER, 32, 32, tb, 8, want_energy=True, want_maps=True)
    for w, g in zip(want, got):
        assert same_floats(w, g)
    lk, mk = eng.locateKeys(xt, bank, 0, NK, mt, want_maps=True)
    lkp, mkp = eng.locateKeysPooled(pool, bank, 0, NK, want_maps=True)
    assert same_floats(lk, lkp) and same_floats(mk, mkp)
    assert list(lkp[2][:3]) == [0, 0, 0] and np.isnan(lkp[2][3]) and not LY.raw(mkp[2]).any()  # the zero key
    eng.close()
    bank.close()


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", CONTRACT)
def test_bit_contract(wm, torch_cuda, kshape, shape, at, mask):
    for dtype in ("f32", "u8"):
        contract_case(wm, torch_cuda, kshape, shape, at, mask, 3, dtype)


def test_bit_contract_nvf_window_5(wm, torch_cuda):
    contract_case(wm, torch_cuda, (140, 330), (65, 257), (75, 73), 1, 5, "f32")


@pytest.mark.parametrize("mask,dtype", [(0, "f32"), (1, "u8"), (1, "f32")])
def test_chunking(wm, torch_cuda, mask, dtype):
    """the pool of 8 frames by raw bits: one call; 3 + 5 with accumulate; eight calls of one frame; a pitched batch; host planes; the
    batch repeated -- with weights NULL and with 1 / (1 + f)"""
    torch = torch_cuda
    kshape, shape, at = LC.CASES[3]
    mt = wm.MASK_TYPE(mask)
    xs = LC.clip_of(kshape, shape, at, mask)
    xs = xs.astype(np.uint8) if dtype == "u8" else xs
    F = len(xs)
    xt = torch.from_numpy(xs).cuda()
    eng = engine(wm, shape, max_frames=F)
    for w in (None, (1.0 / (1.0 + np.arange(F))).astype(np.float32)):
        cut = (lambda a, b: None) if w is None else (lambda a, b: w[a:b])
        want, st = eng.poolClip(xt, mt, w)
        assert list(st) == [0] * F and want.abs().max() > 0
        want = LY.raw(want)
        p35, _ = eng.poolClip(xt[:3], mt, cut(0, 3))
        p35, _ = eng.poolClip(xt[3:], mt, cut(3, F), p35, accumulate=True)
        assert np.array_equal(LY.raw(p35), want)
        p1 = None
        for f in range(F):
            p1, _ = eng.poolClip(xt[f], mt, cut(f, f + 1), p1, accumulate=f > 0)
        assert np.array_equal(LY.raw(p1), want)
        for poison in LY.POISON[dtype]:
            _, view = LY.place(torch, xs, LY.make("pitched", shape[0], shape[1], frames=F), poison)
            assert np.array_equal(LY.raw(eng.poolClip(view, mt, w)[0]), want)
        hx = np.ascontiguousarray(xs)
        ph = wm.wm_plane(hx.ctypes.data, shape[0], shape[1], 1, wm.WM_U8 if dtype == "u8" else wm.WM_F32, wm.WM_MEM_HOST, F, shape[1], 0,
                         shape[0] * shape[1])
        ph_pool = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
        eng.pool_clip_async(ph, mt, wm.WM_SLOT_SYNC, ph_pool, w)
        assert np.array_equal(LY.raw(ph_pool), want)
        assert np.array_equal(LY.raw(eng.poolClip(xt, mt, w)[0]), want)
    eng.close()


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", [LC.CASES[1], LC.CASES[3]])
def test_parity(wm, torch_cuda, kshape, shape, at, mask):
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    key = LC.key_of(kshape)
    xs = LC.clip_of(kshape, shape, at, mask)
    F = len(xs)
    xt = torch.from_numpy(xs).cuda()
    bank = keyset(wm, [np.zeros(kshape, np.float32), key])
    eng = engine(wm, shape, max_frames=F)
    hs = LC.clip_h(xs, TL.coefficients(wm, torch, xs), mask)
    _, maps = eng.locate(xt, bank, 1, mt, want_map=True)
    maps = maps.cpu().numpy().astype(np.float64)
    for w in (None, (1.0 / (1.0 + np.arange(F))).astype(np.float32)):
        ww = np.ones(F) if w is None else w.astype(np.float64)
        pool, _ = eng.poolClip(xt, mt, w)
        loc, mp = eng.locatePooled(pool, bank, 1, want_map=True)
        mp = mp.cpu().numpy()
        hp = LC.pool(hs, ww)
        want, (oy, ox, peak, z) = LC.locate_pooled(hp, key)
        sw = LC.sigma_w(hp, key)
        err = float(np.abs(mp - want).max()) / sw
        pool_err = float(np.abs(pool.cpu().numpy() - hp).max() / np.abs(hp).max())
        summed = np.tensordot(ww, maps, axes=1)
        sw_sum = sw + sum(abs(wf) * LC.sigma_w(h, key) for wf, h in zip(ww, hs))
        err_sum = float(np.abs(mp - summed).max()) / sw_sum
        print(f"{kshape}->{shape}@{at} mask {mask} weights {'NULL' if w is None else '1/(1+f)'}: pool {pool_err:.2e} of max|h|; map {err:.2e} sigma_W of the "
              f"model, {err_sum:.2e} of the summed wm_locate maps' scale; device {loc} model ({oy}, {ox}, {peak:.6g}, {z:.2f})")
        assert err <= MAP_BOUND and err_sum <= MAP_BOUND
        # per pixel: 4 x what the f32 restatement of ONE frame's h misses the f64 model by on texture (tests/test_locate_model.py)
        assert pool_err <= 4 * H.RESTATEMENT_FIGURES["texture"][0]
        if (int(loc[0]), int(loc[1])) == (oy, ox):
            assert abs(loc[2] - peak) <= REL_BOUND * abs(peak) and abs(loc[3] - z) <= REL_BOUND * abs(z)
        assert loc[2] == mp[int(loc[0]), int(loc[1])]
    eng.close()
    bank.close()


def device_clip(wm, torch, kshape, shape, at, mask, marked=True):
    """LC.clip_of with the frames embedded on the DEVICE: marked at the key's shape at LC.PSNR[mask], floored to 8 bits, cropped"""
    (r, c), (oy, ox) = shape, at
    emb = wm.Watermark(kshape[0], kshape[1], LC.key_of(kshape), 3, LC.PSNR[mask])
    out = []
    for f in range(LC.F_CLIP):
        xt = torch.from_numpy(synth_frame(*kshape, frame=10 + f)).cuda()
        y = emb.makeWatermark(xt, xt, wm.MASK_TYPE(mask))[0] if marked else xt
        out.append(np.floor(y[oy:oy + r, ox:ox + c].cpu().numpy()))
    emb.close()
    return np.stack(out).astype(np.float32)


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", LC.CASES)
def test_pooled_clip_is_found_where_no_frame_is(wm, torch_cuda, kshape, shape, at, mask):
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    key = LC.key_of(kshape)
    xs, xu = device_clip(wm, torch, kshape, shape, at, mask), device_clip(wm, torch, kshape, shape, at, mask, marked=False)
    # the model first: the inputs are meaningful
    hs = LC.clip_h(xs, TL.coefficients(wm, torch, xs), mask)
    hu = LC.clip_h(xu, TL.coefficients(wm, torch, xu), mask)
    zs = [M.fold(M.correlate(h, key))[3] for h in hs]
    _, (oy, ox, _, z) = LC.locate_pooled(LC.pool(hs), key)
    zu = LC.locate_pooled(LC.pool(hu), key)[1][3]
    assert max(zs) < Z_MARKED and (oy, ox) == at and z >= Z_MARKED and zu <= Z_UNMARKED
    # the device
    bank = keyset(wm, bank_of(kshape))
    eng = engine(wm, shape, max_frames=LC.F_CLIP)
    xt = torch.from_numpy(xs).cuda()
    per_frame = eng.locate(xt, bank, OWNER, mt)
    loc, st = eng.locateClip(xt, bank, OWNER, mt)
    pool_u, _ = eng.poolClip(torch.from_numpy(xu).cuda(), mt)
    loc_u = eng.locatePooled(pool_u, bank, OWNER)
    pool, _ = eng.poolClip(xt, mt)
    lk = eng.locateKeysPooled(pool, bank, 0, NK)
    best, z_best, z_next = wm.locate_keys_rank(lk)
    print(f"{kshape}->{shape}@{at} mask {mask}: per-frame z {per_frame[:, 3].min():.1f}-{per_frame[:, 3].max():.1f} (model {min(zs):.1f}-{max(zs):.1f}); "
          f"pooled {loc} (model z {z:.1f}); unmarked clip z {loc_u[3]:.1f} (model {zu:.1f}); owner {best} z {z_best:.1f}, next {z_next:.1f}")
    assert list(st) == [0] * LC.F_CLIP and (per_frame[:, 3] < Z_MARKED).all()
    assert (int(loc[0]), int(loc[1])) == at and loc[3] >= Z_MARKED
    assert loc_u[3] <= Z_UNMARKED
    assert best == OWNER and (int(lk[OWNER][0]), int(lk[OWNER][1])) == at and z_best >= Z_MARKED and z_next <= Z_UNMARKED
    eng.close()
    bank.close()


@pytest.mark.parametrize("mask", [0, 1])
def test_payload_clip_is_read_where_a_frame_is_not(wm, torch_cuda, mask):
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    key = LC.key_of(LC.P_KSHAPE)
    tb, bits = LC.payload_table(), LC.payload_bits()
    (r, c), (oy, ox), (th, tw), nb = LC.P_SHAPE, LC.P_AT, LC.P_TILE, LC.P_NBITS
    emb = wm.Watermark(LC.P_KSHAPE[0], LC.P_KSHAPE[1], key, 3, LC.P_PSNR)
    xs = []
    for f in range(LC.F_CLIP):
        xt = torch.from_numpy(synth_frame(*LC.P_KSHAPE, frame=10 + f)).cuda()
        y = emb.makeWatermarkBits(xt, xt, th, tw, tb, nb, B.pack_bits(bits), mt)[0]
        xs.append(np.floor(y[oy:oy + r, ox:ox + c].cpu().numpy()))
    emb.close()
    xs = np.stack(xs).astype(np.float32)
    # the model first: at least one single frame misreads a bit, the pooled clip reads all eight
    hs = LC.clip_h(xs, TL.coefficients(wm, torch, xs), mask)
    wrong_m = [int(((LC.locate_bits_pooled(h, key, th, tw, tb, nb)[3] > 0) != (bits == 1)).sum()) for h in hs]
    _, _, (my, mx, _, mz), msoft = LC.locate_bits_pooled(LC.pool(hs), key, th, tw, tb, nb)
    assert max(wrong_m) >= 1 and (my, mx) == (oy, ox) and np.array_equal(msoft > 0, bits == 1) and np.abs(msoft).min() >= 3.0
    # the device
    bank = keyset(wm, [np.zeros(LC.P_KSHAPE, np.float32), key])
    eng = engine(wm, LC.P_SHAPE, max_frames=LC.F_CLIP)
    xt = torch.from_numpy(xs).cuda()
    _, soft_f = eng.locate_bits(xt, bank, 1, th, tw, tb, nb, mt)
    wrong = [int(((s > 0) != (bits == 1)).sum()) for s in soft_f]
    pool, _ = eng.poolClip(xt, mt)
    loc, soft = eng.locateBitsPooled(pool, bank, 1, th, tw, tb, nb)
    print(f"mask {mask}: misread bits per frame {wrong} (model {wrong_m}); pooled E {loc} (model z {mz:.1f}), weakest |soft| {np.abs(soft).min():.2f} "
          f"(model {np.abs(msoft).min():.2f})")
    assert max(wrong) >= 1
    assert (int(loc[0]), int(loc[1])) == (oy, ox) and np.array_equal(soft > 0, bits == 1) and np.abs(soft).min() >= 3.0
    eng.close()
    bank.close()


def test_unsolvable_frames_accumulate_and_weights(wm, torch_cuda):
    torch = torch_cuda
    kshape, shape, at = LC.CASES[1]
    R, Cc = shape
    mt = wm.MASK_TYPE.ME
    key = LC.key_of(kshape)
    xs = LC.clip_of(kshape, shape, at, 0)[:4].copy()
    bank = keyset(wm, [key])
    eng = engine(wm, shape, max_frames=4)
    # a flat frame inside the batch: the pool's bits are those of the clip without it, and its status is reported
    absent, _ = eng.poolClip(torch.from_numpy(xs[[0, 2, 3]]).cuda(), mt)
    xf = xs.copy()
    xf[1] = H.flat(R, Cc, 128.0)
    pool = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    st = np.full(4, -5, np.int32)
    eng.pool_clip_async(torch.from_numpy(xf).cuda(), mt, 0, pool, None, False, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE and list(st) == [0, 1, 0, 0]
    assert np.array_equal(LY.raw(pool), LY.raw(absent))
    # an all-unsolvable clip: a zero pool, a zero map, z NaN
    flat = torch.from_numpy(np.stack([H.flat(R, Cc, 100.0 + f) for f in range(3)])).cuda()
    zero, st = eng.poolClip(flat, mt)
    loc, mp = eng.locatePooled(zero, bank, 0, want_map=True)
    assert list(st) == [1, 1, 1] and not LY.raw(zero).any() and not LY.raw(mp).any()
    assert list(loc[:3]) == [0, 0, 0] and np.isnan(loc[3])
    # ... and accumulated onto a plane it leaves the plane as it was
    kept = absent.clone()
    eng.poolClip(flat, mt, None, kept, accumulate=True)
    assert np.array_equal(LY.raw(kept), LY.raw(absent))
    # accumulate onto a caller-filled plane adds to it: fmaf(1, h, fill) per pixel
    fill = torch.from_numpy(synth_frame(R, Cc, frame=77)).cuda()
    h0, _ = eng.poolClip(torch.from_numpy(xs[0]).cuda(), mt)
    got, _ = eng.poolClip(torch.from_numpy(xs[0]).cuda(), mt, None, fill.clone(), accumulate=True)
    want = (h0.cpu().numpy().astype(np.float64) + fill.cpu().numpy().astype(np.float64)).astype(np.float32)  # (one rounding: the fmaf's)
    assert np.array_equal(got.cpu().numpy(), want)
    # a weight of 0 behaves like omission, to the parity tolerance
    w = np.array([1, 0, 1, 1], np.float32)
    p0, _ = eng.poolClip(torch.from_numpy(xs).cuda(), mt, w)
    m0 = eng.locatePooled(p0, bank, 0, want_map=True)[1].cpu().numpy()
    ma = eng.locatePooled(absent, bank, 0, want_map=True)[1].cpu().numpy()
    sw = LC.sigma_w(absent.cpu().numpy(), key)
    assert np.abs(m0.astype(np.float64) - ma).max() <= MAP_BOUND * sw
    # a weight that is not finite is refused, before any device work: the pool is left alone
    for badw in (np.nan, np.inf, -np.inf):
        w = np.array([1, 1, badw, 1], np.float32)
        with pytest.raises(RuntimeError, match="finite"):
            eng.poolClip(torch.from_numpy(xs).cuda(), mt, w, kept, accumulate=True)
    assert np.array_equal(LY.raw(kept), LY.raw(absent))
    eng.close()
    bank.close()


def test_refusals_in_order_and_record_caps(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc = 64, 256
    bad, badp, busy = wm.WM_ERR_BAD_ARG, wm.WM_ERR_BAD_P, wm.WM_ERR_BUSY
    eng = engine(wm, (R, Cc), nslots=2, max_frames=2)
    e5 = engine(wm, (R, Cc), p=5)
    keys = wm.KeySet(R + 64, Cc + 64, 3)
    small = wm.KeySet(R - 1, Cc + 64, 3)
    wide = wm.KeySet(R, 8200, 3)
    xt = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=f) for f in range(3)])).cuda()
    pl, pl2, pl3 = wm.plane_of(xt[0], 1), wm.plane_of(xt[:2], 1), wm.plane_of(xt, 1)
    pool = torch.zeros((R, Cc), dtype=torch.float32, device="cuda")
    pp = C.c_void_p(pool.data_ptr())
    loc, soft = (C.c_float * 4200)(), (C.c_float * 4200)()
    ty, tx = wm.Watermark.tiles_shape(R + 64, Cc + 64, 32, 32)
    tb = (C.c_int32 * (ty * tx))(*([0, 1] * (ty * tx // 2)))
    nanw, okw = (C.c_float * 2)(1.0, float("nan")), (C.c_float * 2)(1.0, 2.0)

    def why(ctx=eng):
        return L.wm_last_error(ctx._ctx).decode()

    def band(on):
        assert L.wm_band_configure(eng._ctx, *((8, 40, 128) if on else (0, 0, 0))) == wm.WM_OK

    # ---- wm_clip_pool: null ctx, mask, pointers, band mode, slot, plane, record room, weights
    def cp(ctx=eng, mask=0, img=pl, w=None, p=pp, acc=0, slot=0):
        return L.wm_clip_pool(ctx._ctx, mask, C.byref(img) if img is not None else None, w, p, acc, None, slot)

    assert cp() == wm.WM_OK and cp(img=pl2, w=okw) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert cp(mask=7) == bad and cp(ctx=e5) == badp and cp(ctx=e5, mask=1) == wm.WM_OK and e5.sync(0) == wm.WM_OK
    assert cp(img=None) == bad and "null" in why() and cp(p=None) == bad and "null" in why()
    assert cp(slot=2) == bad and "slot" in why() and cp(img=pl3) == bad and "max_frames" in why()
    assert cp(img=pl2, w=nanw) == bad and "weights[1]" in why() and "finite" in why()
    assert cp(ctx=e5, img=None) == badp                                   # mask before the pointers
    assert cp(img=None, slot=9) == bad and "null" in why()                # pointers before the slot
    assert cp(slot=9, img=pl3) == bad and "slot" in why()                 # the slot before the plane
    assert cp(img=pl3, w=nanw) == bad and "max_frames" in why()           # the plane before the weights
    band(True)
    assert cp(slot=9) == bad and "band" in why()                          # band mode before the slot
    assert cp(img=None) == bad and "null" in why()                        # pointers before band mode
    band(False)
    one = wm.KeySet(R + 64, Cc + 64, 1)
    cb = np.zeros(4096, np.float32)

    def fill(n):
        """n un-synced records on slot 0"""
        eng.detect_offsets_async(xt[0], one, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)  # 4032
        if n > 4032:
            eng.detect_offsets_async(xt[0], one, 0, 0, 0, 1, n - 4032, wm.MASK_TYPE.ME, 0, cb[4032:])

    fill(4095)
    assert cp(img=pl2) == busy and "un-synced" in why()                   # frames records count against the slot's 4096
    assert cp(img=pl2, w=nanw) == busy                                    # the record room before the weights
    assert cp() == wm.WM_OK and eng.sync(0) == wm.WM_OK

    # ---- wm_locate_pooled: null ctx, pointers, k, the bank, the shape, band mode, slot, record room
    def lp(ctx=eng, p=pp, kh=keys, k=0, out=loc, mp=None, slot=0):
        return L.wm_locate_pooled(ctx._ctx, p, kh.handle if kh is not None else None, k, out, mp, slot)

    assert lp() == wm.WM_OK and lp(ctx=e5) == wm.WM_OK and eng.sync(0) == wm.WM_OK and e5.sync(0) == wm.WM_OK  # (p does not matter)
    assert lp(p=None) == bad and lp(kh=None) == bad and lp(out=None) == bad and "both null" in why()
    assert lp(k=3) == bad and lp(k=-1) == bad and "key -1" in why()
    assert lp(kh=small) == bad and "at least as large" in why() and lp(kh=wide) == bad and "transform" in why()
    assert lp(slot=2) == bad and "slot" in why()
    assert lp(p=None, k=5) == bad and "null" in why()                     # pointers before k
    assert lp(k=5, kh=small) == bad and "key 5" in why()                  # k before the bank
    assert lp(kh=small, slot=9) == bad and "at least as large" in why()   # the bank before the slot
    assert lp(kh=wide, slot=9) == bad and "transform" in why()            # the shape before the slot
    band(True)
    assert lp(slot=9) == bad and "band" in why()                          # band mode before the slot
    assert lp(kh=wide) == bad and "transform" in why()                    # the shape before band mode
    band(False)
    fill(4093)
    assert lp() == busy and "un-synced" in why()
    eng.sync(0)
    fill(4092)
    assert lp() == wm.WM_OK and eng.sync(0) == wm.WM_OK                   # exactly room for the four records

    # ---- wm_locate_bits_pooled: ... record room (4 + nbits), then the tile shape, nbits and the table
    def lb(p=pp, kh=keys, k=0, th=32, tw=32, t=tb, nbits=2, out=loc, so=soft, slot=0):
        return L.wm_locate_bits_pooled(eng._ctx, p, kh.handle if kh is not None else None, k, th, tw, t, nbits, out, so, None, None, slot)

    assert lb() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert lb(p=None) == bad and lb(kh=None) == bad and lb(t=None) == bad and lb(out=None) == bad and lb(so=None) == bad and "null" in why()
    assert lb(k=3) == bad and "key 3" in why() and lb(kh=small) == bad and lb(kh=wide) == bad and lb(slot=2) == bad
    assert lb(th=33) == bad and "tile shape" in why() and lb(nbits=0) == bad and "nbits" in why() and lb(nbits=1) == bad and "tile_bit" in why()
    assert lb(p=None, k=5) == bad and "null" in why()                     # pointers before k
    assert lb(k=5, kh=small) == bad and "key 5" in why()                  # k before the bank
    assert lb(kh=wide, slot=9) == bad and "transform" in why()            # the shape before the slot
    assert lb(slot=9, th=33) == bad and "slot" in why()                   # the slot before the tile shape
    band(True)
    assert lb(slot=9) == bad and "band" in why()
    band(False)
    fill(4091)
    assert lb() == busy and "un-synced" in why()                          # 4 + 2 records do not fit
    assert lb(th=33) == busy                                              # the record room before the tile shape
    eng.sync(0)
    fill(4090)
    assert lb() == wm.WM_OK and eng.sync(0) == wm.WM_OK

    # ---- wm_locate_keys_pooled: ... the key range, the bank, the shape, band mode, slot, record room (4 x keys)
    def lkp(p=pp, kh=keys, k0=0, nk=3, out=loc, mp=None, slot=0):
        return L.wm_locate_keys_pooled(eng._ctx, p, kh.handle if kh is not None else None, k0, nk, out, mp, slot)

    assert lkp() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert lkp(p=None) == bad and lkp(kh=None) == bad and lkp(out=None) == bad and "both null" in why()
    assert lkp(k0=-1) == bad and lkp(nk=0) == bad and lkp(k0=1, nk=3) == bad and lkp(k0=3, nk=1) == bad and "keys 3" in why()
    assert lkp(kh=small) == bad and "at least as large" in why() and lkp(kh=wide) == bad and "transform" in why() and lkp(slot=2) == bad
    assert lkp(p=None, k0=5) == bad and "null" in why()                   # pointers before the key range
    assert lkp(k0=5, kh=small) == bad and "keys 5" in why()               # the key range before the bank
    assert lkp(kh=small, slot=9) == bad and "at least as large" in why()  # the bank before the slot
    band(True)
    assert lkp(slot=9) == bad and "band" in why()
    band(False)
    fill(4085)
    assert lkp() == busy and "un-synced" in why()                         # 3 x 4 records do not fit
    eng.sync(0)
    fill(4084)
    assert lkp() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    for k in (keys, small, wide, one):
        k.close()
    eng.close()
    e5.close()


def test_hand_over_left_as_it_was(wm, torch_cuda):
    """a wm_clip_pool of another plane and a wm_locate_pooled queued between an embed and the detector of its output: the detector's
    result and the output are those of the sequence without them, and the location is that of the calls on their own"""
    torch = torch_cuda
    kshape, shape, at = LC.CASES[1]
    R, Cc = shape
    keys = keyset(wm, [LC.key_of(kshape)])
    crop = torch.from_numpy(TL.frames_of(wm, torch, kshape, shape, at, 0, 3, "f32")[:2].copy()).cuda()
    xb = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=40 + f) for f in range(2)])).cuda()
    res = {}
    for ho in (False, True):
        for with_pool in (False, True):
            eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=2)
            eng.set_handover(ho)
            yb = torch.empty_like(xb)
            corr = (C.c_float * 2)()
            loc = np.zeros(4, np.float32)
            pool = torch.empty(shape, dtype=torch.float32, device="cuda")
            eng.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
            if with_pool:
                eng.pool_clip_async(crop, wm.MASK_TYPE.ME, 0, pool)
                eng.locate_pooled_async(pool, keys, 0, 0, loc)
            ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, 2, Cc, 0, R * Cc)
            eng.detect_async(ps, wm.MASK_TYPE.ME, 0, corr)
            eng.sync(0)
            res[ho, with_pool] = (np.array(corr[:], np.float32), yb.cpu().numpy())
            if with_pool:
                alone = eng.locatePooled(eng.poolClip(crop, wm.MASK_TYPE.ME)[0], keys, 0)
                assert np.array_equal(LY.raw(loc), LY.raw(alone)) and (int(loc[0]), int(loc[1])) == at
            eng.close()
        assert np.array_equal(LY.raw(res[ho, True][0]), LY.raw(res[ho, False][0])) and (res[ho, True][0] > 0.2).all()
        assert np.array_equal(LY.raw(res[ho, True][1]), LY.raw(res[ho, False][1]))
    keys.close()


def test_scratch_follows_the_key_shape(wm, torch_cuda):
    """the three pooled calls and their per-frame calls with banks of two shapes queued on one slot without a sync between them, and
    behind a reconfiguring call (which releases the scratch): every result is that of the call on its own"""
    torch = torch_cuda
    shape = (64, 256)
    mt = wm.MASK_TYPE.ME
    eng = engine(wm, shape, nslots=1, max_frames=2)
    jobs = []
    for (kshape, sh, at) in (LC.CASES[0], LC.CASES[1]):
        assert sh == shape
        xt = torch.from_numpy(LC.clip_of(kshape, sh, at, 0)[:2].copy()).cuda()
        jobs.append((keyset(wm, [LC.key_of(kshape), LC.key_of(kshape, other=True)]), xt, eng.poolClip(xt, mt)[0], table_of(kshape, 4)))

    def run(kind, i, slot, outs):
        keys, xt, pool, tb = jobs[i]
        if kind == "one":
            eng.locate_pooled_async(pool, keys, 0, slot, outs[0])
        elif kind == "keys":
            eng.locate_keys_pooled_async(pool, keys, 0, 2, slot, outs[0])
        elif kind == "bits":
            eng.locate_bits_pooled_async(pool, keys, 0, 32, 32, tb, 4, slot, outs[0], outs[1])
        else:  # the per-frame call of two frames: its scratch changes layout between its turns and the pooled call's
            eng.locate_keys_async(xt, keys, 0, 2, mt, slot, outs[0])

    def outs_of(kind):
        return (np.zeros({"one": (4,), "keys": (2, 4), "bits": (4,), "frames": (2, 2, 4)}[kind], np.float32), np.zeros(4, np.float32))

    kinds = ("one", "keys", "bits", "frames")
    want = {}
    for kind in kinds:
        for i in (0, 1):
            want[kind, i] = outs_of(kind)
            run(kind, i, wm.WM_SLOT_SYNC, want[kind, i])
    order = [(k, i) for i in (0, 1, 0) for k in kinds] + [(k, i) for i in (1, 0) for k in reversed(kinds)]
    got = [outs_of(k) for (k, i) in order]
    for (k, i), o in zip(order, got):
        run(k, i, 0, o)
    assert eng.sync(0) == wm.WM_OK
    for (k, i), o in zip(order, got):
        assert np.array_equal(LY.raw(o[0]), LY.raw(want[k, i][0])) and np.array_equal(LY.raw(o[1]), LY.raw(want[k, i][1])), (k, i)
    eng.configure(2, 2)
    again = outs_of("keys")
    run("keys", 1, wm.WM_SLOT_SYNC, again)
    assert np.array_equal(LY.raw(again[0]), LY.raw(want["keys", 1][0]))
    assert (int(want["one", 0][0][0]), int(want["one", 0][0][1])) == LC.CASES[0][2]
    eng.close()
    for j in jobs:
        j[0].close()


def test_table_that_fills_the_arena(wm, torch_cuda):
    """wm_locate_bits_pooled on a slot that has taken no table room yet, with a table of 16384 entries (a 4096 x 4096 key in 32 x 32
    tiles): the table alone fills the first arena of 65536 bytes, so the zero status word must come out of the SAME request -- a
    second request would move the arenas from under the table.  Records and soft values equal wm_locate_bits' as floats"""
    torch = torch_cuda
    kshape, shape, at, nbits = (4096, 4096), (64, 256), (1000, 2000), 2
    key = synth_watermark(*kshape, seed=77)
    tb = (np.arange(128 * 128) % nbits).astype(np.int32)
    assert wm.Watermark.tiles_shape(kshape[0], kshape[1], 32, 32) == (128, 128) and tb.size * 4 == 65536
    bank = keyset(wm, [key])
    x = synth_frame(*shape, frame=3) + 8.0 * key[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]]
    xt = torch.from_numpy(x.astype(np.float32)).cuda()
    eng = engine(wm, shape, nslots=2)
    pool = torch.empty(shape, dtype=torch.float32, device="cuda")
    eng.pool_clip_async(xt, wm.MASK_TYPE.ME, 1, pool)   # (slot 1: slot 0 stays without a table arena)
    assert eng.sync(1) == wm.WM_OK
    loc, soft = np.zeros(4, np.float32), np.zeros(nbits, np.float32)
    eng.locate_bits_pooled_async(pool, bank, 0, 32, 32, tb, nbits, 0, loc, soft)
    assert eng.sync(0) == wm.WM_OK
    want_loc, want_soft = eng.locate_bits(xt, bank, 0, 32, 32, tb, nbits, wm.MASK_TYPE.ME)
    print(f"pooled {loc} {soft}; per frame {want_loc} {want_soft}")
    assert same_floats(loc, want_loc) and same_floats(soft, want_soft)
    assert (int(loc[0]), int(loc[1])) == at
    eng.close()
    bank.close()


@pytest.mark.parametrize("mask,p", [(0, 3), (1, 3), (1, 7)])
def test_yardstick_routes_have_equal_bits(wm, mask, p):
    """wm_clip_pool_bench: the LDS-tile kernel and the direct gather it is held against give the same pool, bit for bit, on a shape
    one past a tile edge on both axes"""
    us, equal = wm.clip_pool_bench(65, 257, 3, mask, p, iters=2)
    assert equal and us["lds_tile"] > 0 and us["gather"] > 0


def test_locate_clip_chunks_by_max_frames(wm, torch_cuda):
    """locateClip cuts by the engine's max_frames, a copy()'s included: the pool calls it makes are counted"""
    torch = torch_cuda
    kshape, shape, at = LC.CASES[0]
    bank = keyset(wm, [LC.key_of(kshape)])
    xt = torch.from_numpy(LC.clip_of(kshape, shape, at, 0)).cuda()
    eng = engine(wm, shape, max_frames=4)
    for e in (eng, eng.copy()):
        calls = []
        inner = e.poolClip
        e.poolClip = lambda frames, *a, **kw: (calls.append(frames.shape[0]), inner(frames, *a, **kw))[1]
        loc, st = e.locateClip(xt, bank, 0)
        assert calls == [4, 4] and list(st) == [0] * 8 and (int(loc[0]), int(loc[1])) == at
        e.close()
    bank.close()


def test_tool_smoke_run(tmp_path):
    """tools/locate_clip_bench.py on the smallest clip of the table, in a child process under a time limit: it finds the crop by both
    routes (it asserts so itself) and writes its JSON"""
    out = str(tmp_path / "clip.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "locate_clip_bench.py"), "--key", "80x300", "--crop", "64x256", "--at", "16,44",
                        "--frames", "2", "--iters", "2", "--rounds", "2", "--json", out], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    with open(out) as f:
        res = json.load(f)
    assert [r["F"] for r in res["results"]] == [2, 2] and all(r["found_pooled"] == [16, 44] for r in res["results"])
    assert len(res["clip_pool_alone"]) == 2 and len(res["other_tails"]) == 2
