"""wm_locate_keys: whose key is in a crop, and where, two keys per transform (wm_k_locate.hip, wm_k_fft.hip), against the f64 model of
tests/locate_keys_model.py run with the DEVICE's own coefficients (as test_gpu_locate.py obtains them).

Bounds are the project's (test_gpu_locate.py): every (frame, key) map within MAP_BOUND = 1e-4 sigma_W of the model, sigma_W =
||h||_2 rms(that key); peak and z within REL_BOUND = 1e-3 of the model's wherever the argmax agrees; the model itself is asserted
first on every input (owner: the true offset and z >= 15; every other (frame, key): z <= 6), so the inputs stay meaningful.  Two
device maps of the same (frame, key) -- wm_locate's, or the call's own under another partner -- are each within MAP_BOUND of the
model, hence within 2 MAP_BOUND of each other.  Then the rules of wm.h: zero keys, equal bits, layouts, either output, an unsolvable
frame, the order of the refusals, the record cap, the hand-over, a slot shared with wm_locate and wm_locate_bits.
Measured figures: DESIGN.md section 26."""
import ctypes as C

import numpy as np
import pytest

import bits_model as B
import hard_frames as H
import layouts as LY
import locate_keys_model as LK
import locate_model as M
import test_gpu_locate as TL
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

MAP_BOUND, REL_BOUND = TL.MAP_BOUND, TL.REL_BOUND
Z_MARKED, Z_UNMARKED = TL.Z_MARKED, TL.Z_UNMARKED
F, NK = len(LK.OWNER), LK.NKEYS
LONG = [((70, 4100), (64, 256), (3, 3001)), ((4100, 260), (64, 256), (3001, 2))]
_model = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def keyset(wm, bank):
    ks = wm.KeySet(bank.shape[1], bank.shape[2], len(bank))
    for k, w in enumerate(bank):
        ks.set(k, w)
    return ks


def engine(wm, shape, p=3, **kw):
    return wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), p, 40.0, **kw)


def model_of(wm, torch, kshape, shape, at, mask, p, dtype, owners=LK.OWNER, nkeys=NK):
    """the model of every frame against the whole bank with the device's own coefficients, computed once and left unchanged:
    (frames, [(maps [nk, ny, nx], loc [nk, 4], sigma_W [nk])]); asserted here, before the device is asked"""
    tag = (kshape, shape, at, mask, p, dtype, tuple(owners), nkeys)
    if tag not in _model:
        bank = LK.bank_of(kshape, nkeys)
        xs = LK.frames_of(kshape, shape, at, mask, dtype, owners, bank)
        out = []
        for f, (x, c) in enumerate(zip(xs, TL.coefficients(wm, torch, xs))):
            maps, loc = LK.locate_keys(x, bank, c, mask, p)
            for k in range(nkeys):
                if k == owners[f]:
                    assert (int(loc[k][0]), int(loc[k][1])) == at and loc[k][3] >= Z_MARKED, (f, k, loc[k])
                else:
                    assert loc[k][3] <= Z_UNMARKED, (f, k, loc[k])
            out.append((maps, loc, np.array([M.sigma_w(x, w, c, mask, p) for w in bank])))
        _model[tag] = (xs, out)
    return _model[tag]


def check_maps(got, model, what, factor=1.0):
    """every (frame, key) map of `got` [F, nk, ny, nx] within factor * MAP_BOUND sigma_W of the model's; returns the worst ratio"""
    worst = 0.0
    for f, (maps, _, sw) in enumerate(model):
        for j in range(got.shape[1]):
            err = float(np.abs(got[f][j] - maps[j]).max()) / sw[j]
            worst = max(worst, err)
            assert err <= factor * MAP_BOUND, (what, f, j, err)
    return worst


def check_case(wm, torch, kshape, shape, at, mask, p, dtype):
    xs, model = model_of(wm, torch, kshape, shape, at, mask, p, dtype)
    keys = keyset(wm, LK.bank_of(kshape))
    eng = engine(wm, shape, p, max_frames=F)
    loc, maps = eng.locateKeys(torch.from_numpy(xs).cuda(), keys, 0, NK, wm.MASK_TYPE(mask), want_maps=True)
    maps = maps.cpu().numpy()
    assert loc.shape == (F, NK, 4) and maps.shape[:2] == (F, NK)
    worst = check_maps(maps, model, (kshape, mask, dtype))
    print(f"{kshape}->{shape}@{at} mask {mask} p {p} {dtype}: worst map error {worst:.2e} sigma_W; device z {np.round(loc[:, :, 3], 2).tolist()}")
    for f, (_, want, _) in enumerate(model):
        for j in range(NK):
            oy, ox, peak, z = want[j]
            if j == LK.OWNER[f]:
                assert (int(loc[f][j][0]), int(loc[f][j][1])) == at                # the device finds the owner's crop
            gy, gx = int(loc[f][j][0]), int(loc[f][j][1])
            assert loc[f][j][2] == maps[f][j][gy, gx]                              # the peak is the map's value, bit for bit
            if (gy, gx) == (int(oy), int(ox)):
                assert abs(loc[f][j][2] - peak) <= REL_BOUND * abs(peak) and abs(loc[f][j][3] - z) <= REL_BOUND * abs(z), (f, j, loc[f][j], want[j])
        if LK.OWNER[f] is not None:
            best, z_best, z_next = wm.locate_keys_rank(loc[f])
            assert best == LK.OWNER[f] and z_best >= Z_MARKED and z_next <= Z_UNMARKED
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", LK.CASES)
def test_parity_and_finding(wm, torch_cuda, kshape, shape, at, mask):
    for dtype in ("f32", "u8"):
        check_case(wm, torch_cuda, kshape, shape, at, mask, 3, dtype)


def test_nvf_window_5(wm, torch_cuda):
    check_case(wm, torch_cuda, *LK.CASES[1], 1, 5, "f32")


@pytest.mark.parametrize("kshape,shape,at", LONG)
def test_long_rows_and_long_columns(wm, torch_cuda, kshape, shape, at):
    """an 8192-point row transform carries a complex pair: map parity and the owner's offset"""
    torch = torch_cuda
    xs, model = model_of(wm, torch, kshape, shape, at, 0, 3, "f32", owners=(1,), nkeys=2)
    keys = keyset(wm, LK.bank_of(kshape, 2))
    eng = engine(wm, shape)
    loc, maps = eng.locateKeys(torch.from_numpy(xs).cuda(), keys, 0, 2, wm.MASK_TYPE.ME, want_maps=True)
    worst = check_maps(maps.cpu().numpy(), model, kshape)
    print(f"{kshape}->{shape}@{at}: worst map error {worst:.2e} sigma_W; device {loc[0].tolist()}")
    assert (int(loc[0][1][0]), int(loc[0][1][1])) == at
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask", [0, 1])
def test_against_wm_locate_and_another_partner(wm, torch_cuda, mask):
    """wm_locate per key, and the same keys under (k0 = 1, nk = 4), where every key has another partner or another half: the same
    offset for the owners, maps within 2 MAP_BOUND sigma_W of each other"""
    torch = torch_cuda
    kshape, shape, at = LK.CASES[1]
    mt = wm.MASK_TYPE(mask)
    xs, model = model_of(wm, torch, kshape, shape, at, mask, 3, "f32")
    xt = torch.from_numpy(xs).cuda()
    keys = keyset(wm, LK.bank_of(kshape))
    eng = engine(wm, shape, max_frames=F)
    loc, maps = eng.locateKeys(xt, keys, 0, NK, mt, want_maps=True)
    loc1, maps1 = eng.locateKeys(xt, keys, 1, NK - 1, mt, want_maps=True)
    maps, maps1 = maps.cpu().numpy().astype(np.float64), maps1.cpu().numpy().astype(np.float64)
    differ = 0
    for k in range(NK):
        l, m = eng.locate(xt, keys, k, mt, want_map=True)
        m = m.cpu().numpy()
        for f in range(F):
            sw = model[f][2][k]
            assert np.abs(maps[f][k] - m[f]).max() <= 2 * MAP_BOUND * sw, (f, k)
            if k >= 1:
                assert np.abs(maps[f][k] - maps1[f][k - 1]).max() <= 2 * MAP_BOUND * sw, (f, k)
                differ += int(not np.array_equal(maps[f][k], maps1[f][k - 1]))
            if k == LK.OWNER[f]:
                assert tuple(int(v) for v in l[f][:2]) == at == tuple(int(v) for v in loc[f][k][:2]) == tuple(int(v) for v in loc1[f][k - 1][:2])
    print(f"mask {mask}: {differ} of {F * (NK - 1)} maps differ in some bit under another partner")
    eng.close()
    keys.close()


# 1037 x 1045 offsets make 265 block records: the one shape here where a thread of the record fold takes more than one
MANY_RECORDS = ((1100, 1300), (64, 256), (500, 600))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", [LK.CASES[0], LK.CASES[2], MANY_RECORDS])
def test_one_key_is_wm_locate_bit_for_bit(wm, torch_cuda, kshape, shape, at, mask):
    """a range of ONE key is wm_locate of that key: locateKeys(x, keys, k, 1) gives locate(x, keys, k)'s records and map bit for bit,
    for every key of the bank and the three frames (two owners, one unmarked), and locateKeysPooled(pool, keys, k, 1) gives
    locatePooled(pool, keys, k)'s -- the map pass, the record fold and the z rule are the same code"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    xt = torch.from_numpy(LK.frames_of(kshape, shape, at, mask)).cuda()
    keys = keyset(wm, LK.bank_of(kshape))
    eng = engine(wm, shape, max_frames=F)
    pool, status = eng.poolClip(xt, mt)
    assert not status.any()
    for k in range(NK):
        loc, m = eng.locate(xt, keys, k, mt, want_map=True)
        lock, mk = eng.locateKeys(xt, keys, k, 1, mt, want_maps=True)
        assert lock.shape == (F, 1, 4) and np.array_equal(bits(lock[:, 0]), bits(loc)), (k, loc, lock)
        assert torch.equal(mk[:, 0].view(torch.int32), m.view(torch.int32)), k
        if k == LK.OWNER[0]:
            assert (int(loc[0][0]), int(loc[0][1])) == at  # (the inputs mean something: frame 0's owner is found)
        locp, mp = eng.locatePooled(pool, keys, k, want_map=True)
        lockp, mkp = eng.locateKeysPooled(pool, keys, k, 1, want_maps=True)
        assert np.array_equal(bits(lockp[0]), bits(locp)), (k, locp, lockp)
        assert torch.equal(mkp[0].view(torch.int32), mp.view(torch.int32)), k
    eng.close()
    keys.close()


def is_zero_record(rec):
    return list(rec[:3]) == [0, 0, 0] and np.isnan(rec[3])


def test_zero_keys(wm, torch_cuda):
    """a key plane that is all zero: an exact zero map and {0, 0, 0, NaN}, whichever half it rides in; its partner is unaffected"""
    torch = torch_cuda
    kshape, shape, at = LK.CASES[1]
    xs, model = model_of(wm, torch, kshape, shape, at, 0, 3, "f32")
    bank = LK.bank_of(kshape)
    xt = torch.from_numpy(xs[0]).cuda()
    eng = engine(wm, shape)
    # key 0 stays zero beside the owner as key 1: the zero key in the real half
    ks = wm.KeySet(kshape[0], kshape[1], 2)
    ks.set(1, bank[1])
    loc, maps = eng.locateKeys(xt, ks, 0, 2, wm.MASK_TYPE.ME, want_maps=True)
    maps = maps.cpu().numpy()
    assert is_zero_record(loc[0]) and not LY.raw(maps[0]).any()
    assert np.abs(maps[1] - model[0][0][1]).max() <= MAP_BOUND * model[0][2][1] and tuple(int(v) for v in loc[1][:2]) == at
    ks.close()
    # the owner first, a zero key in the imaginary half, and a zero key as the odd last key
    ks = wm.KeySet(kshape[0], kshape[1], 3)
    ks.set(0, bank[1])
    loc, maps = eng.locateKeys(xt, ks, 0, 3, wm.MASK_TYPE.ME, want_maps=True)
    maps = maps.cpu().numpy()
    assert is_zero_record(loc[1]) and is_zero_record(loc[2]) and not LY.raw(maps[1:]).any()
    assert np.abs(maps[0] - model[0][0][1]).max() <= MAP_BOUND * model[0][2][1] and tuple(int(v) for v in loc[0][:2]) == at
    assert wm.locate_keys_rank(loc)[0] == 0 and np.isnan(wm.locate_keys_rank(loc)[2])
    # ... and alone: nk = 1 on the zero key, then on the owner
    l1 = eng.locateKeys(xt, ks, 2, 1, wm.MASK_TYPE.ME)
    assert l1.shape == (1, 4) and is_zero_record(l1[0])
    l1 = eng.locateKeys(xt, ks, 0, 1, wm.MASK_TYPE.ME)
    assert tuple(int(v) for v in l1[0][:2]) == at and l1[0][3] >= Z_MARKED
    ks.close()
    # a bank that is all zero (a new bank's planes are)
    ks = wm.KeySet(kshape[0], kshape[1], 3)
    loc, maps = eng.locateKeys(xt, ks, 0, 3, wm.MASK_TYPE.NVF, want_maps=True)
    assert all(is_zero_record(r) for r in loc) and not LY.raw(maps).any() and wm.locate_keys_rank(loc)[0] == -1
    # a key set after a call on the zero bank is seen: the flags are cleared and raised per call
    ks.set(2, bank[1])
    loc = eng.locateKeys(xt, ks, 0, 3, wm.MASK_TYPE.ME)
    assert is_zero_record(loc[0]) and is_zero_record(loc[1]) and tuple(int(v) for v in loc[2][:2]) == at
    ks.close()
    eng.close()


def test_equal_bits_layouts_and_outputs(wm, torch_cuda):
    """one frame alone, the batch and the batch again; a pitched batch (tests/layouts.py) and a host plane, f32 and u8; either output
    alone: equal bits throughout"""
    torch = torch_cuda
    kshape, shape, at = LK.CASES[1]
    mt = wm.MASK_TYPE.ME
    keys = keyset(wm, LK.bank_of(kshape))
    eng = engine(wm, shape, max_frames=F)
    for dtype in ("f32", "u8"):
        xs, _ = model_of(wm, torch, kshape, shape, at, 0, 3, dtype)
        xt = torch.from_numpy(xs).cuda()
        want = eng.locateKeys(xt, keys, 0, NK, mt, want_maps=True)
        one = eng.locateKeys(xt[1], keys, 0, NK, mt, want_maps=True)
        again = eng.locateKeys(xt, keys, 0, NK, mt, want_maps=True)
        for w, o, a in zip(want, one, again):
            assert np.array_equal(LY.raw(o), LY.raw(w[1])) and np.array_equal(LY.raw(a), LY.raw(w))
        for poison in LY.POISON[dtype]:
            _, view = LY.place(torch, xs, LY.make("pitched", shape[0], shape[1], frames=F), poison)
            got = eng.locateKeys(view, keys, 0, NK, mt, want_maps=True)
            assert all(np.array_equal(LY.raw(g), LY.raw(w)) for g, w in zip(got, want))
        hx = np.ascontiguousarray(xs)
        ph = wm.wm_plane(hx.ctypes.data, shape[0], shape[1], 1, wm.WM_U8 if dtype == "u8" else wm.WM_F32, wm.WM_MEM_HOST, F, shape[1], 0,
                         shape[0] * shape[1])
        l, m = np.zeros((F, NK, 4), np.float32), torch.zeros_like(want[1])
        eng.locate_keys_async(ph, keys, 0, NK, mt, wm.WM_SLOT_SYNC, l, m)
        assert np.array_equal(LY.raw(l), LY.raw(want[0])) and np.array_equal(LY.raw(m), LY.raw(want[1]))
        # either output alone, queued behind each other
        l_only, m_only = np.zeros((F, NK, 4), np.float32), torch.zeros_like(want[1])
        eng.locate_keys_async(xt, keys, 0, NK, mt, 0, l_only, None)
        eng.locate_keys_async(xt, keys, 0, NK, mt, 0, None, m_only)
        assert eng.sync(0) == wm.WM_OK
        assert np.array_equal(LY.raw(l_only), LY.raw(want[0])) and np.array_equal(LY.raw(m_only), LY.raw(want[1]))
    eng.close()
    keys.close()


def test_unsolvable_frame(wm, torch_cuda):
    torch = torch_cuda
    kshape, shape, at = LK.CASES[1]
    R, Cc = shape
    xs = model_of(wm, torch, kshape, shape, at, 0, 3, "f32")[0].copy()
    keys = keyset(wm, LK.bank_of(kshape))
    eng = engine(wm, shape, max_frames=F)
    alone = [eng.locateKeys(torch.from_numpy(xs[f]).cuda(), keys, 0, NK, wm.MASK_TYPE.ME, want_maps=True) for f in (0, 2)]
    xs[1] = H.singular("ramp", R, Cc)
    ny, nx = kshape[0] - R + 1, kshape[1] - Cc + 1
    l, st = np.full((F, NK, 4), 7.0, np.float32), np.full(F, -5, np.int32)
    m = torch.full((F, NK, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    eng.locate_keys_async(torch.from_numpy(xs).cuda(), keys, 0, NK, wm.MASK_TYPE.ME, 0, l, m, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    assert list(st) == [0, 1, 0] and not LY.raw(l[1]).any() and not LY.raw(m[1]).any()
    for f, (al, am) in zip((0, 2), alone):
        assert np.array_equal(LY.raw(l[f]), LY.raw(al)) and np.array_equal(LY.raw(m[f]), LY.raw(am))
    eng.close()
    keys.close()


def test_refusals_in_order_and_record_cap(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc = 64, 256
    bad, badp, busy = wm.WM_ERR_BAD_ARG, wm.WM_ERR_BAD_P, wm.WM_ERR_BUSY
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, nslots=2, max_frames=2)
    e5 = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 5, 40.0)
    keys = wm.KeySet(R + 64, Cc + 64, 3)
    small = wm.KeySet(R - 1, Cc + 64, 3)
    wide = wm.KeySet(R, 8200, 3)
    xt = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=f) for f in range(3)])).cuda()
    pl, pl2, pl3 = wm.plane_of(xt[0], 1), wm.plane_of(xt[:2], 1), wm.plane_of(xt, 1)
    loc = (C.c_float * 4200)()
    mp = torch.zeros((3, 65, 65), dtype=torch.float32, device="cuda")

    def call(ctx=eng, mask=0, img=pl, kh=keys, k0=0, nk=3, out=loc, maps=None, slot=0):
        return L.wm_locate_keys(ctx._ctx, mask, C.byref(img) if img is not None else None, kh.handle if kh is not None else None, k0, nk, out,
                                C.c_void_p(maps.data_ptr()) if maps is not None else None, None, slot)

    def why(ctx=eng):
        return L.wm_last_error(ctx._ctx).decode()

    assert call() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert call(out=None, maps=mp) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    # each refusal on its own ...
    assert call(mask=7) == bad and call(ctx=e5) == badp
    assert call(img=None) == bad and call(kh=None) == bad and call(out=None) == bad and "both null" in why()
    assert call(k0=-1) == bad and call(nk=0) == bad and call(nk=-2) == bad and call(k0=1, nk=3) == bad and call(k0=3, nk=1) == bad and "keys 3" in why()
    assert call(k0=2, nk=1) == wm.WM_OK and call(k0=1, nk=2) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert call(kh=small) == bad and "at least as large" in why()
    assert call(kh=wide) == bad and "transform" in why()
    assert call(slot=2) == bad and "slot" in why()
    assert call(img=pl3) == bad  # three frames on a context of two
    # ... and in the documented order: the earlier check names the failure
    assert call(ctx=e5, img=None) == badp                      # mask before the pointers
    assert call(img=None, k0=5) == bad and "null" in why()     # pointers before the key range
    assert call(k0=5, kh=small) == bad and "keys 5" in why()   # the key range before the bank
    assert call(kh=small, slot=9) == bad and "at least as large" in why()  # the bank before the slot
    assert call(kh=wide, slot=9) == bad and "transform" in why()           # the shape before the slot
    assert call(slot=9, img=pl3) == bad and "slot" in why()    # the slot before the plane
    assert L.wm_band_configure(eng._ctx, 8, 40, 128) == wm.WM_OK
    assert call(slot=9) == bad and "band" in why()             # band mode before the slot
    assert call(kh=wide) == bad and "transform" in why()       # the shape before band mode
    assert L.wm_band_configure(eng._ctx, 0, 0, 0) == wm.WM_OK
    # the record cap: frames x nk x 4 count against the slot's 4096
    cb = np.zeros(4096, np.float32)
    one = wm.KeySet(R + 64, Cc + 64, 1)
    eng.detect_offsets_async(xt[0], one, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)           # 4032
    eng.detect_offsets_async(xt[0], one, 0, 0, 0, 1, 41, wm.MASK_TYPE.ME, 0, cb[4032:])     # 4073: 2 x 3 x 4 = 24 more do not fit
    assert call(img=pl2) == busy and "un-synced" in why()
    assert call(img=pl3) == bad                                # the plane before the record room
    assert call() == wm.WM_OK                                  # one frame: 12 records, 4085
    eng.sync(0)
    eng.detect_offsets_async(xt[0], one, 0, 0, 0, 64, 63, wm.MASK_TYPE.ME, 0, cb)
    eng.detect_offsets_async(xt[0], one, 0, 0, 0, 1, 40, wm.MASK_TYPE.ME, 0, cb[4032:])     # 4072: exactly room for two frames
    assert call(img=pl2) == wm.WM_OK
    eng.sync(0)
    # an empty slot: 1025 keys of one frame are 4100 records, 1024 keys fill the slot exactly (and use every non-zero flag)
    many = wm.KeySet(R + 4, Cc + 4, 1025)   # (5 x 5 offsets: 16 of them outside the 3 x 3 block)
    many.set(1023, synth_watermark(R + 4, Cc + 4))
    assert call(kh=many, nk=1025) == busy and "un-synced" in why()
    assert call(kh=many, nk=1024) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    got = np.array(loc[:4096], np.float32).reshape(1024, 4)
    assert all(is_zero_record(r) for r in got[:1023]) and not np.isnan(got[1023][3]) and got[1023][2] != 0
    for k in (keys, small, wide, one, many):
        k.close()
    eng.close()
    e5.close()


def test_hand_over_left_as_it_was(wm, torch_cuda):
    """a wm_locate_keys of another plane queued between an embed and the detector of its output: the detector's result and the
    output are those of the sequence without it, and the records are those of a call on its own"""
    torch = torch_cuda
    kshape, shape, at = LK.CASES[1]
    R, Cc = shape
    keys = keyset(wm, LK.bank_of(kshape))
    crop = torch.from_numpy(model_of(wm, torch, kshape, shape, at, 0, 3, "f32")[0][:2].copy()).cuda()
    xb = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=40 + f) for f in range(2)])).cuda()
    res = {}
    for ho in (False, True):
        for with_locate in (False, True):
            eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=1, max_frames=2)
            eng.set_handover(ho)
            yb = torch.empty_like(xb)
            corr = (C.c_float * 2)()
            loc = np.zeros((2, NK, 4), np.float32)
            eng.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
            if with_locate:
                eng.locate_keys_async(crop, keys, 0, NK, wm.MASK_TYPE.ME, 0, loc)
            ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, 2, Cc, 0, R * Cc)
            eng.detect_async(ps, wm.MASK_TYPE.ME, 0, corr)
            eng.sync(0)
            res[ho, with_locate] = (np.array(corr[:], np.float32), yb.cpu().numpy())
            if with_locate:
                assert np.array_equal(LY.raw(loc), LY.raw(eng.locateKeys(crop, keys, 0, NK, wm.MASK_TYPE.ME)))
                assert [tuple(int(v) for v in loc[f][LK.OWNER[f]][:2]) for f in range(2)] == [at, at]
            eng.close()
        assert np.array_equal(LY.raw(res[ho, True][0]), LY.raw(res[ho, False][0])) and (res[ho, True][0] > 0.2).all()
        assert np.array_equal(LY.raw(res[ho, True][1]), LY.raw(res[ho, False][1]))
    keys.close()


def test_slot_shared_with_locate_and_locate_bits(wm, torch_cuda):
    """wm_locate_keys, wm_locate and wm_locate_bits queued on one slot in every order, with banks of two shapes and two batch sizes so
    that each call's scratch changes layout between its turns, and behind a reconfiguring call: every result is that of the call on its
    own"""
    torch = torch_cuda
    shape = (64, 256)
    mt = wm.MASK_TYPE.ME
    jobs = []
    for (kshape, sh, at) in (LK.CASES[0], LK.CASES[1]):
        assert sh == shape
        xs = model_of(wm, torch, kshape, sh, at, 0, 3, "f32")[0]
        ty, tx = wm.Watermark.tiles_shape(kshape[0], kshape[1], 32, 32)
        jobs.append((keyset(wm, LK.bank_of(kshape)), torch.from_numpy(xs).cuda(), B.layout(ty, tx, 4, 5)))
    eng = engine(wm, shape, nslots=1, max_frames=F)

    def run(kind, i, slot, outs):
        keys, xt, tb = jobs[i]
        x = xt if i == 0 else xt[0]   # (job 0: the batch of three; job 1: one frame)
        if kind == "keys":
            eng.locate_keys_async(x, keys, 0, NK, mt, slot, outs[0])
        elif kind == "one":
            eng.locate_async(x, keys, 1, mt, slot, outs[0])
        else:
            eng.locate_bits_async(x, keys, 1, 32, 32, tb, 4, mt, slot, outs[0], outs[1])

    def outs_of(kind, i):
        n = F if i == 0 else 1
        return (np.zeros((n, NK, 4) if kind == "keys" else (n, 4), np.float32), np.zeros((n, 4), np.float32))

    kinds = ("keys", "one", "bits")
    want = {}
    for kind in kinds:
        for i in (0, 1):
            want[kind, i] = outs_of(kind, i)
            run(kind, i, wm.WM_SLOT_SYNC, want[kind, i])
    order = [(k, i) for i in (0, 1, 0) for k in kinds] + [(k, i) for i in (1, 0) for k in reversed(kinds)] + [("keys", 0), ("bits", 0), ("keys", 1), ("one", 1), ("keys", 0)]
    got = [outs_of(k, i) for (k, i) in order]
    for (k, i), o in zip(order, got):
        run(k, i, 0, o)
    assert eng.sync(0) == wm.WM_OK
    for (k, i), o in zip(order, got):
        assert np.array_equal(LY.raw(o[0]), LY.raw(want[k, i][0])) and np.array_equal(LY.raw(o[1]), LY.raw(want[k, i][1])), (k, i)
    eng.configure(2, F)
    again = outs_of("keys", 0)
    run("keys", 0, wm.WM_SLOT_SYNC, again)
    assert np.array_equal(LY.raw(again[0]), LY.raw(want["keys", 0][0]))
    assert [tuple(int(v) for v in want["keys", 0][0][f][LK.OWNER[f]][:2]) for f in range(2)] == [LK.CASES[0][2]] * 2
    eng.close()
    for j in jobs:
        j[0].close()
