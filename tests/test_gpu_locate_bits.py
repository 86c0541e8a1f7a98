"""wm_locate_bits: a cropped, payload-marked copy found in its key without a hint, and read (wm_k_locate.hip, wm_k_fft.hip), against
the f64 model of tests/locate_bits_model.py run with the DEVICE's own coefficients.

Parity: every per-bit map within 1e-4 sigma_W of the model (sigma_W and the bound are test_gpu_locate.py's), E within what follows
from it, sum_b (2 |map_b| d + d^2) with d = 1e-4 sigma_W; on a case without a -1 tile the maps add up to wm_locate's map and each
equals wm_locate on a bank holding key_b, both to 2e-4 sigma_W (the two bounds added).  Finding and reading: the model first (the
input is meaningful: true offset, z(E) >= 60 marked and <= 15 unmarked, wm_locate's own map below z 10 on the payload copies), then
the device: the true offset, loc and soft within 1e-3 max(1, |.|) of the model's, peak == E[oy][ox] bit for bit, every bit with
>= 512 px in the window decoded.  The payloads are balanced (as many set as clear pixels, nearly): a lopsided payload leaves a net
mark that wm_locate finds.  Then the rules of wm.h.  Measured figures: DESIGN.md section 25."""
import ctypes as C

import numpy as np
import pytest

import bits_model as B
import hard_frames as H
import layouts as LY
import locate_bits_model as LB
import locate_model as M
import test_gpu_locate as TL
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

MAP_BOUND, REL_BOUND = TL.MAP_BOUND, 1e-3
Z_MARKED, Z_UNMARKED, Z_WHOLE = 60.0, 15.0, 10.0
MIN_COVER = 512
F = 3  # two payload copies with different payloads and an unmarked crop


def own_table(T, holes, counts, seed):
    """a table of the caller's own: bit b on counts[b] tiles drawn by a seeded shuffle, the tiles `holes` on none"""
    free = [t for t in np.random.default_rng(seed).permutation(T) if t not in holes]
    tb = np.full(T, -1, np.int32)
    tb[free] = np.repeat(np.arange(len(counts)), counts)
    return tb


class Case:
    def __init__(self, kshape, shape, at, tile, nbits, holes=(), counts=None, payloads=None):
        self.kshape, self.shape, self.at, self.tile, self.nbits = kshape, shape, at, tile, nbits
        self.ny, self.nx = LB.tiles_shape(kshape[0], kshape[1], *tile)
        if counts:
            self.tb = own_table(self.ny * self.nx, holes, counts, 5)
        else:
            self.tb = B.layout(self.ny, self.nx, nbits, 5)
            for t in holes:
                self.tb[t] = -1
        self.payloads = payloads or [LB.balanced_payload(nbits, 1000 * f + nbits) for f in range(F - 1)]
        self.cover = LB.cover(shape, kshape, tile[0], tile[1], self.tb, nbits, *at)


# 5 bits cannot be balanced on tiles of equal count: bits 0-1 on 24 tiles each, bits 2-4 on 16 each, two tiles on none
CASES = {
    "120x330_8": Case((120, 330), (64, 256), (20, 31), (32, 32), 8),
    "270x480_16": Case((270, 480), (200, 384), (37, 53), (32, 32), 16),
    "270x480_15": Case((270, 480), (200, 384), (37, 53), (32, 32), 15),
    "301x523_5": Case((301, 523), (271, 483), (30, 40), (40, 36), 5, holes=(11, 60), counts=(24, 24, 16, 16, 16),
                      payloads=[np.array([1, 1, 0, 0, 0]), np.array([0, 0, 1, 1, 1])]),
    "70x4100_7": Case((70, 4100), (64, 256), (3, 3001), (32, 32), 7),
}
_frames, _model = {}, {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames_of(wm, torch, name, mask, p, dtype, payloads=None):
    """[F, rows, cols]: frames 0 and 1 marked with the case's payloads at the key's shape (psnr 40) and cropped, frame 2 the unmarked
    crop; u8: floored"""
    cs = CASES[name]
    tag = (name, mask, p, None if payloads is None else tuple(map(tuple, payloads)))
    if tag not in _frames:
        (r, c), (oy, ox) = cs.shape, cs.at
        emb = wm.Watermark(cs.kshape[0], cs.kshape[1], TL.key_of(cs.kshape), p, 40.0)
        out = []
        for f in range(F):
            xt = torch.from_numpy(synth_frame(*cs.kshape, frame=10 + f)).cuda()
            y = xt
            if f < F - 1:
                y = emb.makeWatermarkBits(xt, xt, cs.tile[0], cs.tile[1], cs.tb, cs.nbits, B.pack_bits((payloads or cs.payloads)[f]), wm.MASK_TYPE(mask))[0]
            out.append(y[oy:oy + r, ox:ox + c].cpu().numpy())
        emb.close()
        _frames[tag] = np.stack(out)
    x = _frames[tag]
    return np.floor(x).astype(np.uint8) if dtype == "u8" else x


def model_of(wm, torch, name, mask, p, dtype):
    """the model of every frame with the device's own coefficients, computed once: [(maps, E, loc, soft, sigma_W, whole-map z)]"""
    tag = (name, mask, p, dtype)
    if tag not in _model:
        cs = CASES[name]
        xs = frames_of(wm, torch, name, mask, p, dtype)
        key = TL.key_of(cs.kshape)
        out = []
        for x, c in zip(xs, TL.coefficients(wm, torch, xs)):
            mp, E, loc, soft = LB.locate_bits(x, key, c, mask, cs.tile[0], cs.tile[1], cs.tb, cs.nbits, p)
            out.append((mp, E, loc, soft, M.sigma_w(x, key, c, mask, p), M.fold(mp.sum(axis=0))[3] if not (cs.tb < 0).any() else
                        M.locate(x, key, c, mask, p)[1][3]))
        _model[tag] = out
    return _model[tag]


def close(got, want):
    return abs(got - want) <= REL_BOUND * max(1.0, abs(want))


def check_case(wm, torch, name, mask, p, dtype):
    cs = CASES[name]
    mt = wm.MASK_TYPE(mask)
    keys = wm.KeySet(cs.kshape[0], cs.kshape[1], 2)
    keys.set(1, TL.key_of(cs.kshape))  # (the key is not key 0 of its bank)
    xs = frames_of(wm, torch, name, mask, p, dtype)
    xt = torch.from_numpy(xs).cuda()
    eng = wm.Watermark(cs.shape[0], cs.shape[1], np.zeros(cs.shape, np.float32), p, 40.0, max_frames=F)
    args = (keys, 1, cs.tile[0], cs.tile[1], cs.tb, cs.nbits, mt)
    loc, soft, en, mp = eng.locate_bits(xt, *args, want_energy=True, want_maps=True)
    whole = eng.locate(xt, keys, 1, mt)
    en_h, mp_h = en.cpu().numpy(), mp.cpu().numpy()
    read = cs.cover >= MIN_COVER
    assert read.sum() >= cs.nbits - 1
    for f, (want_mp, want_E, (oy, ox, peak, z), want_soft, sw, z_whole) in enumerate(model_of(wm, torch, name, mask, p, dtype)):
        d = MAP_BOUND * sw
        err = float(np.abs(mp_h[f] - want_mp).max())
        e_excess = float((np.abs(en_h[f] - want_E) - (2 * np.abs(want_mp) * d + d * d).sum(axis=0)).max())
        print(f"{name} mask {mask} p {p} {dtype} frame {f}: map error {err / sw:.2e} sigma_W; device {loc[f]} model ({oy}, {ox}, {peak:.6g}, {z:.2f}); "
              f"wm_locate's z {whole[f][3]:.2f} (model {z_whole:.2f}); weakest covered |soft| {np.abs(soft[f][read]).min():.2f}")
        assert err <= d and e_excess <= 0.0
        if f < F - 1:
            assert (oy, ox) == cs.at and z >= Z_MARKED and z_whole <= Z_WHOLE   # the model: the input is meaningful
            assert (int(loc[f][0]), int(loc[f][1])) == cs.at                    # the device finds the crop ...
            assert whole[f][3] < Z_WHOLE                                         # ... where wm_locate's own map has no peak
            assert np.array_equal((soft[f] > 0)[read], cs.payloads[f][read] == 1)
        else:
            assert z <= Z_UNMARKED and loc[f][3] <= Z_UNMARKED
        if (int(loc[f][0]), int(loc[f][1])) == (oy, ox):
            assert close(loc[f][2], peak) and close(loc[f][3], z)
            assert loc[f][2] == en_h[f][oy, ox]
            for b in range(cs.nbits):
                assert close(soft[f][b], want_soft[b]), (b, soft[f][b], want_soft[b])
    # one frame alone, and the batch again: equal bits; without maps_dev and energy_dev: the same numbers
    one = eng.locate_bits(xt[0], *args, want_energy=True, want_maps=True)
    again = eng.locate_bits(xt, *args, want_energy=True, want_maps=True)
    for a, b1, bF in zip((loc, soft, en, mp), one, again):
        assert np.array_equal(LY.raw(b1), LY.raw(a[0])) and np.array_equal(LY.raw(bF), LY.raw(a))
    l0, s0 = eng.locate_bits(xt, *args)
    assert np.array_equal(LY.raw(l0), LY.raw(loc)) and np.array_equal(LY.raw(s0), LY.raw(soft))
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_parity_finding_and_reading(wm, torch_cuda, name, mask):
    for dtype in ("f32", "u8"):
        check_case(wm, torch_cuda, name, mask, 3, dtype)


def test_nvf_window_5(wm, torch_cuda):
    check_case(wm, torch_cuda, "120x330_8", 1, 5, "f32")


@pytest.mark.parametrize("mask", [0, 1])
def test_maps_against_wm_locate(wm, torch_cuda, mask):
    """no -1 tile: the maps add up to wm_locate's map of the whole key, and map b is wm_locate's map on a bank that holds key_b"""
    torch = torch_cuda
    name = "120x330_8"
    cs = CASES[name]
    mt = wm.MASK_TYPE(mask)
    key = TL.key_of(cs.kshape)
    bank = wm.KeySet(cs.kshape[0], cs.kshape[1], cs.nbits + 1)
    for b in range(cs.nbits):
        bank.set(b, LB.key_b(key, cs.tile[0], cs.tile[1], cs.tb, b).astype(np.float32))
    bank.set(cs.nbits, key)
    xs = frames_of(wm, torch, name, mask, 3, "f32")
    xt = torch.from_numpy(xs).cuda()
    eng = wm.Watermark(cs.shape[0], cs.shape[1], np.zeros(cs.shape, np.float32), 3, 40.0, max_frames=F)
    _, _, mp = eng.locate_bits(xt, bank, cs.nbits, cs.tile[0], cs.tile[1], cs.tb, cs.nbits, mt, want_maps=True)
    mp = mp.cpu().numpy().astype(np.float64)
    sw = np.array([m[4] for m in model_of(wm, torch, name, mask, 3, "f32")])[:, None, None]
    whole = eng.locate(xt, bank, cs.nbits, mt, want_map=True)[1].cpu().numpy()
    assert (np.abs(mp.sum(axis=1) - whole) <= 2 * MAP_BOUND * sw).all()
    for b in range(cs.nbits):
        single = eng.locate(xt, bank, b, mt, want_map=True)[1].cpu().numpy()
        assert (np.abs(mp[:, b] - single) <= 2 * MAP_BOUND * sw).all(), b
    eng.close()
    bank.close()


@pytest.mark.parametrize("mask", [0, 1])
def test_one_bit_on_every_tile_is_wm_locate_bit_for_bit(wm, torch_cuda, mask):
    """one payload bit whose table takes every tile masks nothing: its map is wm_locate's map of the key bit for bit -- the lay pass,
    the transforms and the map value are the same code --, and the energy map is that map squared in f32 (the missing second bit of
    the pair adds an exact zero)"""
    torch = torch_cuda
    name = "120x330_8"
    cs = CASES[name]
    mt = wm.MASK_TYPE(mask)
    keys = wm.KeySet(cs.kshape[0], cs.kshape[1], 2)
    keys.set(1, TL.key_of(cs.kshape))
    xt = torch.from_numpy(frames_of(wm, torch, name, mask, 3, "f32")).cuda()
    eng = wm.Watermark(cs.shape[0], cs.shape[1], np.zeros(cs.shape, np.float32), 3, 40.0, max_frames=F)
    every = np.zeros(cs.ny * cs.nx, np.int32)
    _, _, en, mp = eng.locate_bits(xt, keys, 1, cs.tile[0], cs.tile[1], every, 1, mt, want_energy=True, want_maps=True)
    whole = eng.locate(xt, keys, 1, mt, want_map=True)[1]
    assert mp.shape[:2] == (F, 1) and float(whole.abs().max()) > 0.0
    assert torch.equal(mp[:, 0].view(torch.int32), whole.view(torch.int32))
    assert torch.equal(en.view(torch.int32), (mp[:, 0] * mp[:, 0]).view(torch.int32))
    eng.close()
    keys.close()


def test_layouts_and_host_plane(wm, torch_cuda):
    """a pitched batch (tests/layouts.py) and a host plane give the dense device plane's bits, f32 and u8"""
    torch = torch_cuda
    name = "120x330_8"
    cs = CASES[name]
    (R, Cc), n = cs.shape, cs.nbits
    keys = wm.KeySet(cs.kshape[0], cs.kshape[1], 1)
    keys.set(0, TL.key_of(cs.kshape))
    eng = wm.Watermark(R, Cc, np.zeros(cs.shape, np.float32), 3, 40.0, max_frames=F)
    args = (keys, 0, 32, 32, cs.tb, n, wm.MASK_TYPE.ME)
    for dtype in ("f32", "u8"):
        xs = frames_of(wm, torch, name, 0, 3, dtype)
        want = eng.locate_bits(torch.from_numpy(xs).cuda(), *args, want_energy=True, want_maps=True)
        for poison in LY.POISON[dtype]:
            _, view = LY.place(torch, xs, LY.make("pitched", R, Cc, frames=F), poison)
            got = eng.locate_bits(view, *args, want_energy=True, want_maps=True)
            assert all(np.array_equal(LY.raw(g), LY.raw(w)) for g, w in zip(got, want))
        hx = np.ascontiguousarray(xs)
        ph = wm.wm_plane(hx.ctypes.data, R, Cc, 1, wm.WM_U8 if dtype == "u8" else wm.WM_F32, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
        l, s = np.zeros((F, 4), np.float32), np.zeros((F, n), np.float32)
        e, m = torch.zeros_like(want[2]), torch.zeros_like(want[3])
        eng.locate_bits_async(ph, *args, wm.WM_SLOT_SYNC, l, s, e, m)
        assert all(np.array_equal(LY.raw(g), LY.raw(w)) for g, w in zip((l, s, e, m), want))
    eng.close()
    keys.close()


def test_rules(wm, torch_cuda):
    torch = torch_cuda
    name = "120x330_8"
    cs = CASES[name]
    (R, Cc), n, key = cs.shape, cs.nbits, TL.key_of(cs.kshape)
    ny, nx = cs.kshape[0] - R + 1, cs.kshape[1] - Cc + 1
    xs = frames_of(wm, torch, name, 0, 3, "f32").copy()
    keys = wm.KeySet(cs.kshape[0], cs.kshape[1], 1)
    keys.set(0, key)
    eng = wm.Watermark(R, Cc, np.zeros(cs.shape, np.float32), 3, 40.0, max_frames=F)
    args = (keys, 0, 32, 32, cs.tb, n, wm.MASK_TYPE.ME)
    alone = eng.locate_bits(torch.from_numpy(xs[0]).cuda(), *args, want_energy=True, want_maps=True)
    # a bit without a tile: NaN and a zero map; the other bits read as before, the crop is found as before
    tb3 = np.where(cs.tb == 3, -1, cs.tb).astype(np.int32)
    l3, s3, m3 = eng.locate_bits(torch.from_numpy(xs[0]).cuda(), keys, 0, 32, 32, tb3, n, wm.MASK_TYPE.ME, want_maps=True)
    assert np.isnan(s3[3]) and not m3[3].cpu().numpy().any() and (int(l3[0]), int(l3[1])) == cs.at
    assert all(close(s3[b], alone[1][b]) for b in range(n) if b != 3)
    assert (np.abs(m3.cpu().numpy() - alone[3].cpu().numpy())[np.arange(n) != 3] <= 2 * MAP_BOUND * model_of(wm, torch, name, 0, 3, "f32")[0][4]).all()
    # a zero key: zero maps, the first offset, NaN everywhere
    zero = wm.KeySet(cs.kshape[0], cs.kshape[1], 1)
    lz, sz, ez = eng.locate_bits(torch.from_numpy(xs[0]).cuda(), zero, 0, 32, 32, cs.tb, n, wm.MASK_TYPE.ME, want_energy=True)
    assert list(lz[:3]) == [0, 0, 0] and np.isnan(lz[3]) and np.isnan(sz).all() and not ez.cpu().numpy().any()
    # a flat frame: unsolvable, zeros; its neighbours in the batch are what they are alone
    xs[1] = H.singular("ramp", R, Cc)
    xt = torch.from_numpy(xs).cuda()
    l, s, st = np.full((F, 4), 7.0, np.float32), np.full((F, n), 7.0, np.float32), np.full(F, -5, np.int32)
    e = torch.full((F, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    m = torch.full((F, n, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    eng.locate_bits_async(xt, *args, 0, l, s, e, m, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    assert list(st) == [0, 1, 0] and not l[1].any() and not s[1].any() and not e[1].cpu().numpy().any() and not m[1].cpu().numpy().any()
    assert all(np.array_equal(LY.raw(g[0]), LY.raw(w)) for g, w in zip((l, s, e, m), alone))
    # a plainly marked copy (payload all ones): found, every covered bit reads as set
    ones = frames_of(wm, torch, name, 0, 3, "f32", payloads=[np.ones(n, np.int64)] * 2)
    lp, sp = eng.locate_bits(torch.from_numpy(ones[0]).cuda(), *args)
    assert (int(lp[0]), int(lp[1])) == cs.at and lp[3] >= Z_MARKED and (sp[cs.cover >= MIN_COVER] > 0).all()
    for k in (keys, zero):
        k.close()
    eng.close()


def test_refusals_in_order_and_record_cap(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc, n = 64, 256, 8
    bad, badp, busy = wm.WM_ERR_BAD_ARG, wm.WM_ERR_BAD_P, wm.WM_ERR_BUSY
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=2, max_frames=2)
    e5 = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 5, 40.0)
    keys = wm.KeySet(R + 64, Cc + 64, 1)   # 128 x 320: 4 x 10 tiles of 32 x 32
    small = wm.KeySet(R - 1, Cc + 64, 1)
    wide = wm.KeySet(R, 8200, 1)
    xt = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=f) for f in range(3)])).cuda()
    pl, pl3 = wm.plane_of(xt[0], 1), wm.plane_of(xt, 1)
    loc, soft = (C.c_float * 16)(), (C.c_float * 8192)()
    tb = B.layout(4, 10, n, 5)

    def call(ctx=eng, mask=0, img=pl, kh=keys, k=0, th=32, tw=32, table=tb, nbits=n, out=loc, sout=soft, slot=0):
        return L.wm_locate_bits(ctx._ctx, mask, C.byref(img) if img is not None else None, kh.handle if kh is not None else None, k, th, tw,
                                table.ctypes.data_as(C.c_void_p) if table is not None else None, nbits, out, sout, None, None, None, slot)

    def why(ctx=eng):
        return L.wm_last_error(ctx._ctx).decode()

    assert call() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    # each refusal on its own ...
    assert call(mask=7) == bad and call(ctx=e5) == badp
    assert call(img=None) == bad and call(kh=None) == bad and call(table=None) == bad and call(out=None) == bad and call(sout=None) == bad
    assert call(k=1) == bad and call(k=-1) == bad
    assert call(kh=small) == bad and "at least as large" in why()
    assert call(kh=wide) == bad and "transform" in why()
    assert call(slot=2) == bad and "slot" in why()
    assert call(img=pl3) == bad  # three frames on a context of two
    assert call(th=30) == bad and "tile shape" in why() and call(tw=34) == bad and "tile shape" in why()
    assert call(nbits=0) == bad and "nbits" in why() and call(nbits=-3) == bad and "nbits" in why()
    assert call(nbits=n - 1) == bad and "tile_bit" in why()   # an entry n - 1 needs nbits >= n
    assert call(table=np.where(tb == 2, -2, tb).astype(np.int32)) == bad and "tile_bit" in why()
    # ... and in the documented order: the earlier check names the failure
    assert call(ctx=e5, img=None) == badp                      # mask before the pointers
    assert call(img=None, k=5) == bad and "null" in why()      # pointers before k
    assert call(k=5, kh=small) == bad and "key 5" in why()     # k before the bank
    assert call(kh=small, slot=9) == bad and "at least as large" in why()  # the bank before the slot
    assert call(kh=wide, slot=9) == bad and "transform" in why()           # the shape before the slot
    assert call(slot=9, img=pl3) == bad and "slot" in why()    # the slot before the plane
    assert call(img=pl3, th=30) == bad and "tile shape" not in why()       # the plane before the tiles
    assert call(th=30, nbits=0) == bad and "tile shape" in why()           # the tile shape before nbits
    assert call(nbits=4093) == busy and "un-synced" in why()   # the record room before nbits: 4 + 4093 records
    assert L.wm_band_configure(eng._ctx, 8, 40, 128) == wm.WM_OK
    assert call(slot=9) == bad and "band" in why()             # band mode before the slot
    assert call(kh=wide) == bad and "transform" in why()       # the shape before band mode
    assert L.wm_band_configure(eng._ctx, 0, 0, 0) == wm.WM_OK
    # the record cap: frames x (4 + nbits) count against the slot's 4096
    cb = np.zeros(4096, np.float32)
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)         # 4032
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 1, 53, wm.MASK_TYPE.ME, 0, cb[4032:])   # 4085: 12 more do not fit
    assert call() == busy and "un-synced" in why()
    assert call(th=30) == busy                                 # the record room before the tiles
    eng.sync(0)
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)
    eng.detect_offsets_async(xt[0], keys, 0, 0, 0, 1, 52, wm.MASK_TYPE.ME, 0, cb[4032:])   # 4084: exactly room for one frame
    assert call() == wm.WM_OK
    eng.sync(0)
    for k in (keys, small, wide):
        k.close()
    eng.close()
    e5.close()


def test_hand_over_left_as_it_was(wm, torch_cuda):
    """a wm_locate_bits of another plane queued between an embed and the detector of its output: the detector's result is that of
    the sequence without it, and the location and bits are those of a call on its own"""
    torch = torch_cuda
    name = "120x330_8"
    cs = CASES[name]
    (R, Cc), n = cs.shape, cs.nbits
    keys = wm.KeySet(cs.kshape[0], cs.kshape[1], 1)
    keys.set(0, TL.key_of(cs.kshape))
    args = (keys, 0, 32, 32, cs.tb, n, wm.MASK_TYPE.ME)
    crop = torch.from_numpy(frames_of(wm, torch, name, 0, 3, "f32")[:2].copy()).cuda()
    xb = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=40 + f) for f in range(2)])).cuda()
    res = {}
    for ho in (False, True):
        for with_locate in (False, True):
            eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=2)
            eng.set_handover(ho)
            yb = torch.empty_like(xb)
            corr = (C.c_float * 2)()
            loc, soft = np.zeros((2, 4), np.float32), np.zeros((2, n), np.float32)
            eng.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
            if with_locate:
                eng.locate_bits_async(crop, *args, 0, loc, soft)
            ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, 2, Cc, 0, R * Cc)
            eng.detect_async(ps, wm.MASK_TYPE.ME, 0, corr)
            eng.sync(0)
            res[ho, with_locate] = (np.array(corr[:], np.float32), yb.cpu().numpy())
            if with_locate:
                want = eng.locate_bits(crop, *args)
                assert np.array_equal(LY.raw(loc), LY.raw(want[0])) and np.array_equal(LY.raw(soft), LY.raw(want[1]))
                assert [tuple(int(v) for v in l[:2]) for l in loc] == [cs.at, cs.at]
            eng.close()
        assert np.array_equal(LY.raw(res[ho, True][0]), LY.raw(res[ho, False][0])) and (res[ho, True][0] > 0.2).all()
        assert np.array_equal(LY.raw(res[ho, True][1]), LY.raw(res[ho, False][1]))
    keys.close()


def test_scratch_follows_the_key_shape_and_nbits(wm, torch_cuda):
    """calls with banks of different shapes and tables of different nbits queued on one slot without a sync between them, with and
    without the caller's own maps, and a call behind a reconfiguring call (which releases the scratch): every result is that of the
    call on its own"""
    torch = torch_cuda
    shape = (64, 256)
    jobs = []  # (bank, crop, table, nbits)
    for name, nbits in (("120x330_8", 8), ("70x4100_7", 7), ("120x330_8", 5)):
        cs = CASES[name]
        assert cs.shape == shape
        k = wm.KeySet(cs.kshape[0], cs.kshape[1], 1)
        k.set(0, TL.key_of(cs.kshape))
        tb = cs.tb if nbits == cs.nbits else (cs.tb % nbits).astype(np.int32)
        jobs.append((k, torch.from_numpy(frames_of(wm, torch, name, 0, 3, "f32")[0].copy()).cuda(), tb, nbits))
    eng = wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), 3, 40.0, nslots=1)
    want = [eng.locate_bits(x, k, 0, 32, 32, tb, nb, wm.MASK_TYPE.ME) for (k, x, tb, nb) in jobs]
    order = (0, 1, 2, 1, 0, 0)
    got = [(np.zeros(4, np.float32), np.zeros(jobs[i][3], np.float32)) for i in order]
    ny, nx, _, _ = wm.locate_shape(shape[0], shape[1], 120, 330)
    own = torch.zeros((8, ny, nx), dtype=torch.float32, device="cuda")
    for j, ((l, s), i) in enumerate(zip(got, order)):
        k, x, tb, nb = jobs[i]
        eng.locate_bits_async(x, k, 0, 32, 32, tb, nb, wm.MASK_TYPE.ME, 0, l, s, None, own if j == len(order) - 1 else None)
    eng.sync(0)
    for (l, s), i in zip(got, order):
        assert np.array_equal(LY.raw(l), LY.raw(want[i][0])) and np.array_equal(LY.raw(s), LY.raw(want[i][1])), i
    eng.configure(2, 2)
    k, x, tb, nb = jobs[0]
    again = eng.locate_bits(x, k, 0, 32, 32, tb, nb, wm.MASK_TYPE.ME)
    assert np.array_equal(LY.raw(again[0]), LY.raw(want[0][0])) and np.array_equal(LY.raw(again[1]), LY.raw(want[0][1]))
    assert [tuple(int(v) for v in w[0][:2]) for w in want[:2]] == [CASES["120x330_8"].at, CASES["70x4100_7"].at]
    eng.close()
    for j in jobs:
        j[0].close()
