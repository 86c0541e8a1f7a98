"""The crop-search family (wm_locate, wm_locate_keys, wm_locate_bits, wm_clip_pool and the pooled tails; wm_k_locate.hip) on the hard
crops of tests/hard_frames.py: clipped, letterboxed, pillarboxed, binary, near-singular, low-contrast and impulse crops at three
geometries that between them hold every tile edge of k_clip_pool, under ME p = 3 and NVF p = 3, 5, 9, f32 and u8.

h per pixel: a one-frame wm_clip_pool with weights NULL and accumulate 0 returns fmaf(1, h, 0) = h, which is held against the
oracle's restatement wmo_locate_h run with the DEVICE's coefficients -- equal as floats (-0 == +0): every operation of the image
side is single-rounded and written out, so nothing less is promised.

The map, against two references, in sigma_W = ||h||_2 rms(key): (1) locate_model.correlate of the device's OWN h in f64 at MAP_BOUND
= 1e-4 -- the transform alone; (2) the full f64 model at 1e-4 + the family's figure of the restatement against the f64 model
(hard_frames.RESTATEMENT_FIGURES, asserted by tests/test_locate_model.py) -- the transform's share plus the f32 image side's.

Records: a crop tests/test_hard_content.py found in the model is found on the device, peak and z to 1e-3 relative; the others are
compared where the argmax agrees.  One mixed batch with unsolvable frames in it; the siblings on three of the crops.
Measured figures: DESIGN.md sections 24 and 27."""
import numpy as np
import pytest

import hard_frames as H
import layouts as LY
import locate_bits_model as LB
import locate_clip_model as LC
import locate_model as M
import oracle_lib as O
import test_gpu_locate as TL
from synth import synth_watermark

pytestmark = pytest.mark.gpu

MAP_BOUND, REL_BOUND = TL.MAP_BOUND, TL.REL_BOUND
BATCH = 14
NK, OWNER = 5, 3
TH, TW, NBITS = 32, 32, 8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def engine(wm, shape, p, **kw):
    return wm.Watermark(shape[0], shape[1], np.zeros(shape, np.float32), p, 40.0, **kw)


def cases_of(kshape, shape, at, mask, p):
    """[(name, family, frame, found)]: every hard crop marked and unmarked (f32 and u8) and every impulse crop (f32 and u8); found:
    tests/test_hard_content.py holds the model to the true offset with z >= 10 there"""
    out = []
    for name, (marked, plain) in H.locate_crops(kshape, shape, at, mask, p).items():
        fam = H.locate_family(name)
        out.append((name + "/marked", fam, marked, H.LOCATE_FAMILIES[fam][0]))
        out.append((name + "/plain", fam, plain, False))
    for dtype in (np.float32, np.uint8):
        xs, items = H.locate_impulses(kshape, shape, at, dtype)
        out += [(f"impulse_{n}{'_u8' if dtype == np.uint8 else ''}", "impulse", x, False) for x, (n, _, _) in zip(xs, items)]
    return out


def batches(cases):
    """the cases cut into batches of one dtype, BATCH frames at the most"""
    for dtype in (np.float32, np.uint8):
        sel = [c for c in cases if c[2].dtype == dtype]
        for i in range(0, len(sel), BATCH):
            yield sel[i:i + BATCH], np.stack([c[2] for c in sel[i:i + BATCH]])


def restated_h(x, c, mask, p):
    return O.locate_h(np.asarray(x, np.float32), c, mask, p)[3]


def assert_same_h(got, want, what):
    """equal as floats; names the first pixel that differs"""
    bad = np.argwhere(~(got == want))
    assert bad.size == 0, (what, f"{len(bad)} pixels differ, the first at (row, column) {tuple(bad[0])}: device {got[tuple(bad[0])]!r} "
                                 f"restatement {want[tuple(bad[0])]!r}; columns {sorted(set(bad[:, 1].tolist()))[:8]}")


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
@pytest.mark.parametrize("kshape,shape,at", H.LOCATE_GEOMS)
def test_h_per_pixel(wm, torch_cuda, kshape, shape, at, mask, p):
    """a one-frame wm_clip_pool == wmo_locate_h with the device's coefficients, as floats, on every hard crop; inside the bars the
    pool is exactly 0 under NVF"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    eng = engine(wm, shape, p, max_frames=BATCH)
    for group, xs in batches(cases_of(kshape, shape, at, mask, p)):
        cs = TL.coefficients(wm, torch, xs)
        xt = torch.from_numpy(xs).cuda()
        for f, (name, fam, x, _) in enumerate(group):
            pool, st = eng.poolClip(xt[f], mt)
            got = pool.cpu().numpy()
            assert list(st) == [0] and np.isfinite(got).all() and np.abs(got).max() > 0, name
            assert_same_h(got, restated_h(x, cs[f], mask, p), name)
            zero = H.locate_bar_zero(name.split("/")[0], shape, p, name.endswith("/marked")) if mask == 1 and "/" in name else None
            if zero is not None:
                assert zero.sum() > 0 and not got[zero].any(), name
    eng.close()


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
@pytest.mark.parametrize("kshape,shape,at", H.LOCATE_GEOMS)
def test_two_frame_pool(wm, torch_cuda, kshape, shape, at, mask, p):
    """an impulse frame and a clipped frame with weights (1, 0.5), in two calls with accumulate, and in one: fmaf(0.5, h_1,
    fmaf(1, h_0, 0)) formed on the host in f32 (0.5 h_1 is exact, so the sum's one rounding is the fmaf's)"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    xs = np.stack([H.locate_impulses(kshape, shape, at)[0][3], H.locate_crops(kshape, shape, at, mask, p)["clipped"][0]])
    cs = TL.coefficients(wm, torch, xs)
    h0, h1 = (restated_h(xs[f], cs[f], mask, p) for f in (0, 1))
    want = np.float32(0.5) * h1 + (h0 + np.float32(0.0))
    eng = engine(wm, shape, p, max_frames=2)
    xt = torch.from_numpy(xs).cuda()
    pool, _ = eng.poolClip(xt[0], mt, np.array([1.0], np.float32))
    pool, st = eng.poolClip(xt[1], mt, np.array([0.5], np.float32), pool, accumulate=True)
    assert list(st) == [0]
    assert_same_h(pool.cpu().numpy(), want, "two calls")
    both, st = eng.poolClip(xt, mt, np.array([1.0, 0.5], np.float32))
    assert list(st) == [0, 0]
    assert_same_h(both.cpu().numpy(), want, "one call")
    eng.close()


def check_map(mp, hdev, x, c, key, mask, p, fam, what, sigma_key=None):
    """the device's map against the f64 correlation of the device's own h (the transform alone: MAP_BOUND) and against the full f64
    model (MAP_BOUND + the family's restatement figure); returns the model's map, its fold and the two errors in sigma_W.
    sigma_key: the key plane of sigma_W where `key` is one bit's share of it (test_gpu_locate_bits.py's scale)"""
    mp = np.asarray(mp, np.float64)
    sigma_key = key if sigma_key is None else sigma_key
    sw_dev = LC.sigma_w(hdev, sigma_key)
    e1 = float(np.abs(mp - M.correlate(np.asarray(hdev, np.float64), key)).max()) / sw_dev
    want, rec = M.locate(np.asarray(x, np.float32), key, c, mask, p)
    e2 = float(np.abs(mp - want).max()) / M.sigma_w(np.asarray(x, np.float32), sigma_key, c, mask, p)
    print(f"{what}: map {e1:.2e} sigma_W of the device's own h, {e2:.2e} of the f64 model")
    assert e1 <= MAP_BOUND, what
    assert e2 <= MAP_BOUND + H.RESTATEMENT_FIGURES[fam][1], what
    return want, rec, e1, e2


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
@pytest.mark.parametrize("kshape,shape,at", H.LOCATE_GEOMS)
def test_maps_and_records(wm, torch_cuda, kshape, shape, at, mask, p):
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    key = H.locate_key(kshape)
    bank = wm.KeySet(kshape[0], kshape[1], 2)
    bank.set(1, key)
    eng = engine(wm, shape, p, max_frames=BATCH)
    worst = {}
    for group, xs in batches(cases_of(kshape, shape, at, mask, p)):
        cs = TL.coefficients(wm, torch, xs)
        xt = torch.from_numpy(xs).cuda()
        loc, maps = eng.locate(xt, bank, 1, mt, want_map=True)
        maps = maps.cpu().numpy()
        for f, (name, fam, x, found) in enumerate(group):
            hdev = eng.poolClip(xt[f], mt)[0].cpu().numpy()
            what = f"{kshape}->{shape}@{at} mask {mask} p {p} {name}"
            _, (oy, ox, peak, z), e1, e2 = check_map(maps[f], hdev, x, cs[f], key, mask, p, fam, what)
            w = worst.setdefault(fam, [0.0, 0.0])
            w[0], w[1] = max(w[0], e1), max(w[1], e2)
            dev = (int(loc[f][0]), int(loc[f][1]))
            print(f"    device {loc[f]} model ({oy}, {ox}, {peak:.6g}, {z:.2f})")
            if found:
                assert (oy, ox) == at and z >= 10.0, what   # (the model with the device's coefficients: the input is meaningful)
                assert dev == at, what
            if dev == (oy, ox):
                assert abs(loc[f][2] - peak) <= REL_BOUND * abs(peak) and abs(loc[f][3] - z) <= REL_BOUND * abs(z), what
            assert loc[f][2] == maps[f][dev], what
    for fam, (e1, e2) in worst.items():
        print(f"{kshape}->{shape} mask {mask} p {p} {fam}: worst map error {e1:.2e} sigma_W (own h), {e2:.2e} (f64 model)")
    eng.close()
    bank.close()


def mixed_frames(kshape, shape, at, mask, dtype):
    """one frame of every family, with a ramp, a row-constant frame and an integer-flat frame among them: (frames, unsolvable)"""
    crops = H.locate_crops(kshape, shape, at, mask, 3)
    sfx = "_u8" if dtype == np.uint8 else ""
    fams = [f for f, (_, has_u8) in H.LOCATE_FAMILIES.items() if has_u8 or dtype == np.float32]
    xs = [crops[f + sfx][0] for f in fams]
    xs.insert(2, np.floor(H.singular("ramp", *shape)).astype(dtype))
    xs.append(H.locate_impulses(kshape, shape, at, dtype)[0][0])
    xs.insert(5, np.floor(H.singular("rows", *shape)).astype(dtype))
    xs.append(H.flat(shape[0], shape[1], 77, dtype))
    return np.stack(xs), (2, 5, len(xs) - 1)


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_mixed_batch(wm, torch_cuda, mask, dtype):
    """every family in one wm_locate call: each frame's records and map are the bits of the frame alone; each unsolvable frame -- a
    flat frame is one -- has status WM_UNSOLVABLE, four zeros (z = 0, not NaN) and a zero map"""
    torch = torch_cuda
    kshape, shape, at = H.LOCATE_GEOMS[1]
    mt = wm.MASK_TYPE(mask)
    xs, dead = mixed_frames(kshape, shape, at, mask, dtype)
    F = len(xs)
    assert F <= BATCH
    bank = wm.KeySet(kshape[0], kshape[1], 1)
    bank.set(0, H.locate_key(kshape))
    eng = engine(wm, shape, 3, max_frames=F)
    xt = torch.from_numpy(xs).cuda()
    ny, nx = kshape[0] - shape[0] + 1, kshape[1] - shape[1] + 1
    loc = np.full((F, 4), 7.0, np.float32)
    st = np.full(F, -5, np.int32)
    maps = torch.full((F, ny, nx), 7.0, dtype=torch.float32, device="cuda")
    eng.locate_async(xt, bank, 0, mt, 0, loc, maps, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    assert list(st) == [1 if f in dead else 0 for f in range(F)]
    for f in range(F):
        l1 = np.full((1, 4), 7.0, np.float32)
        s1 = np.full(1, -5, np.int32)
        m1 = torch.full((1, ny, nx), 7.0, dtype=torch.float32, device="cuda")
        eng.locate_async(xt[f], bank, 0, mt, 0, l1, m1, s1)
        assert eng.sync(0) == (wm.WM_UNSOLVABLE if f in dead else wm.WM_OK)
        assert s1[0] == st[f]
        assert np.array_equal(LY.raw(l1[0]), LY.raw(loc[f])) and np.array_equal(LY.raw(m1[0]), LY.raw(maps[f])), f
        if f in dead:
            assert not LY.raw(loc[f]).any() and not LY.raw(maps[f]).any(), f   # (+0 bits: z = 0, not NaN)
        else:
            assert np.isfinite(loc[f]).all() and LY.raw(maps[f]).any(), f
    eng.close()
    bank.close()


def bank_of(kshape):
    """five keys: the shape's key at OWNER, a zero plane at 2, three keys that marked nothing"""
    planes = [synth_watermark(*kshape, seed=9700 + 13 * k + kshape[1]) for k in range(NK)]
    planes[OWNER] = H.locate_key(kshape)
    planes[2] = np.zeros(kshape, np.float32)
    return planes


def sibling_crops(kshape, shape, at, mask, p):
    crops = H.locate_crops(kshape, shape, at, mask, p)
    return [("clipped_u8", "clipped", crops["clipped_u8"][0], True), ("letterbox", "letterbox", crops["letterbox"][0], True),
            ("impulse_corner_tl", "impulse", H.locate_impulses(kshape, shape, at)[0][0], False)]


def same_floats(a, b):
    a, b = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
def test_locate_keys_and_pooled_tails(wm, torch_cuda, mask, p):
    """wm_locate_keys on a bank of five with a zero key at 2 and the owner at 3: the owner is found, the zero key gives {0, 0, 0, NaN}
    and a zero map, every map lies within the two bounds; the one-frame pooled tails equal the per-frame calls as floats"""
    torch = torch_cuda
    kshape, shape, at = H.LOCATE_GEOMS[0]
    mt = wm.MASK_TYPE(mask)
    planes = bank_of(kshape)
    bank = wm.KeySet(kshape[0], kshape[1], NK)
    for k, pl in enumerate(planes):
        if pl.any():
            bank.set(k, pl)
    eng = engine(wm, shape, p)
    for name, fam, x, found in sibling_crops(kshape, shape, at, mask, p):
        c = TL.coefficients(wm, torch, x[None])[0]
        xt = torch.from_numpy(x).cuda()
        pool, _ = eng.poolClip(xt, mt)
        hdev = pool.cpu().numpy()
        lk, mk = eng.locateKeys(xt, bank, 0, NK, mt, want_maps=True)
        assert list(lk[2][:3]) == [0, 0, 0] and np.isnan(lk[2][3]) and not LY.raw(mk[2]).any(), name
        for k in (0, 1, OWNER, 4):
            _, (oy, ox, peak, z), _, _ = check_map(mk[k].cpu().numpy(), hdev, x, c, planes[k], mask, p, fam, f"mask {mask} p {p} {name} key {k}")
            if (int(lk[k][0]), int(lk[k][1])) == (oy, ox):
                assert abs(lk[k][2] - peak) <= REL_BOUND * abs(peak) and abs(lk[k][3] - z) <= REL_BOUND * abs(z), (name, k)
        best, z_best, z_next = wm.locate_keys_rank(lk)
        print(f"mask {mask} p {p} {name}: owner {best} z {z_best:.1f}, next {z_next:.1f}")
        if found:
            assert best == OWNER and (int(lk[OWNER][0]), int(lk[OWNER][1])) == at and z_best >= 10.0 and z_next <= 6.0, name
        # the pooled tails of a one-frame pool
        lkp, mkp = eng.locateKeysPooled(pool, bank, 0, NK, want_maps=True)
        assert same_floats(lk, lkp) and same_floats(mk, mkp), name
        l1, m1 = eng.locate(xt, bank, OWNER, mt, want_map=True)
        l1p, m1p = eng.locatePooled(pool, bank, OWNER, want_map=True)
        assert same_floats(l1, l1p) and same_floats(m1, m1p) and same_floats(l1, lk[OWNER]) and same_floats(m1, mk[OWNER]), name
    eng.close()
    bank.close()


def payload_crop(kshape, shape, at, fam, mask, p, tb, bits, dtype):
    """locate_clip_model.payload_clip's construction on a hard frame: +key where the tile's bit is set, -key where not, psnr 40"""
    import np_restatement as NP
    key = H.locate_key(kshape)
    s = LB.signs_plane(kshape, TH, TW, tb, bits)
    x = H.locate_base(fam, kshape, shape, at)
    name = "ME" if mask == 0 else "NVF"
    yp, ym = NP.embed(x, x, key, p, H.locate_psnr(shape), name)[0], NP.embed(x, x, -key, p, H.locate_psnr(shape), name)[0]
    y = np.where(s > 0, yp, np.where(s < 0, ym, x))[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]]
    return np.floor(y).astype(np.uint8) if dtype == np.uint8 else np.ascontiguousarray(y, np.float32)


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
def test_locate_bits(wm, torch_cuda, mask, p):
    """wm_locate_bits with 32 x 32 tiles and 8 bits on payload-marked clipped (u8) and letterboxed crops: found at the true offset,
    every covered bit read, every bit's map within the two bounds; on a corner impulse the maps alone; the pooled tail equals the
    per-frame call as floats"""
    torch = torch_cuda
    kshape, shape, at = H.LOCATE_GEOMS[0]
    mt = wm.MASK_TYPE(mask)
    key = H.locate_key(kshape)
    ty, tx = LB.tiles_shape(kshape[0], kshape[1], TH, TW)
    tb = (np.arange(ty * tx) % NBITS).astype(np.int32)
    bits = LB.balanced_payload(NBITS, 5)
    bank = wm.KeySet(kshape[0], kshape[1], 1)
    bank.set(0, key)
    eng = engine(wm, shape, p)
    cover = wm.locate_bits_cover(shape[0], shape[1], kshape[0], kshape[1], TH, TW, tb, NBITS, at[0], at[1])
    crops = [("clipped_u8", "clipped", payload_crop(kshape, shape, at, "clipped", mask, p, tb, bits, np.uint8), True),
             ("letterbox", "letterbox", payload_crop(kshape, shape, at, "letterbox", mask, p, tb, bits, np.float32), True),
             ("impulse_corner_tl", "impulse", H.locate_impulses(kshape, shape, at)[0][0], False)]
    for name, fam, x, found in crops:
        c = TL.coefficients(wm, torch, x[None])[0]
        xt = torch.from_numpy(x).cuda()
        pool, _ = eng.poolClip(xt, mt)
        hdev = pool.cpu().numpy()
        loc, soft, en, maps = eng.locate_bits(xt, bank, 0, TH, TW, tb, NBITS, mt, want_energy=True, want_maps=True)
        mmaps, mE, (oy, ox, _, z), msoft = LB.locate_bits(x.astype(np.float32), key, c, mask, TH, TW, tb, NBITS, p)
        for b in range(NBITS):
            check_map(maps[b].cpu().numpy(), hdev, x, c, LB.key_b(key, TH, TW, tb, b), mask, p, fam, f"mask {mask} p {p} {name} bit {b}",
                      sigma_key=key)
        print(f"mask {mask} p {p} {name}: device {loc} soft {soft}; model ({oy}, {ox}) z {z:.1f} soft {msoft}")
        if found:
            assert (oy, ox) == at and z >= 10.0 and np.array_equal(msoft[cover > 0] > 0, bits[cover > 0] == 1), name   # (the model)
            assert (int(loc[0]), int(loc[1])) == at, name
            assert np.array_equal(soft[cover > 0] > 0, bits[cover > 0] == 1), name
        got = eng.locateBitsPooled(pool, bank, 0, TH, TW, tb, NBITS, want_energy=True, want_maps=True)
        for w, g in zip((loc, soft, en, maps), got):
            assert same_floats(w, g), name
    eng.close()
    bank.close()
