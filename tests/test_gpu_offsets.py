"""wm_detect_offsets: one image scored against a rectangle of window offsets into one key plane that is larger than the image
(k_detect_offsets).  Bit equality with wm_detect_keys on a bank that holds every window copied out (and with wm_detect on the
batched sweeps), independence from everything outside a window, scores against the CPU oracle (<= 1e-5, the bound of the other
detector tests), finding a crop, and the enqueue / error / determinism / C++ cases of tests/test_gpu_keys.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
KBANK = 2  # keys per searched bank: the LAST one is searched (its far-corner window ends at the allocation's last float)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames_of(R, Cc, F, dtype, first=0):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def window(key, R, Cc, oy, ox):
    return np.ascontiguousarray(key[oy:oy + R, ox:ox + Cc])


def rectangles(wm, KR, KC, R, Cc):
    """(oy0, ox0, ny, nx): ox0 covers the four residues mod 4; nx is 1, a non-multiple of the group size G above it, G + 1 and
    2 (below every G); ny is 1 and 3; the last two end at the far corner of the key plane"""
    dy, dx = KR - R, KC - Cc
    if dy == 0 and dx == 0:
        return [(0, 0, 1, 1)]
    G = wm.lib().wm_detect_offsets_group()
    odd = next(n for n in (7, 11, 13) if all(n % g for g in (2, 3, 4)) and n > G)  # (a non-multiple of any group size)
    assert dy >= 4 and dx >= 16 and dx % 4 == 0
    rs = [(1, 0, 1, 1), (2, 5, 3, G + 1), (0, 2, 1, odd),
          (dy - 2, dx - 5, 3, 6),   # ox0 = 3 mod 4, ends at the far corner
          (dy, dx - 1, 1, 2)]       # nx < G, ends at the far corner
    assert sorted(r[1] % 4 for r in rs[:4]) == [0, 1, 2, 3]
    return rs


SHAPES = [((64, 256), (64, 256)), ((80, 300), (64, 256)), ((300, 520), (270, 480)), ((301, 523), (271, 483)),
          ((1100, 1950), (1078, 1918)), ((2200, 3900), (2160, 3840))]
_cache = {}


def banks_for(wm, kshape, shape):
    """the searched bank (KBANK generated keys, the last one searched) and, for every offset of the shape's rectangles, the
    window copied out into a rows x cols bank; kept for the cases of one shape"""
    tag = (kshape, shape)
    if _cache.get("tag") != tag:
        for b in _cache.get("banks", ()):
            b.close()
        _cache.clear()
        (KR, KC), (R, Cc) = kshape, shape
        keys = wm.KeySet.from_seeds(KR, KC, [4100 + 13 * k for k in range(KBANK)])
        key = keys.plane(KBANK - 1)
        rects = rectangles(wm, KR, KC, R, Cc)
        offs = [(oy0 + i, ox0 + j) for (oy0, ox0, ny, nx) in rects for i in range(ny) for j in range(nx)]
        wins = wm.KeySet(R, Cc, len(offs))
        for n, (oy, ox) in enumerate(offs):
            wins.set(n, window(key, R, Cc, oy, ox))
        _cache.update(tag=tag, banks=(keys, wins), key=key, rects=rects, offs=offs)
    return _cache["banks"][0], _cache["banks"][1], _cache["key"], _cache["rects"], _cache["offs"]


BIT_CASES = [(ks, s, mk, p, dt, F) for ks, s in SHAPES for (mk, p) in ((0, 3), (1, 3), (1, 5), (1, 9)) for dt in ("f32", "u8") for F in (1, 5)]


@pytest.mark.parametrize("kshape,shape,mask,p,dtype,F", BIT_CASES)
def test_bit_equal_to_detect_keys(wm, torch_cuda, kshape, shape, mask, p, dtype, F):
    """every score equals, as uint32, wm_detect_keys' on a rows x cols bank filled with the window copied out; the far-corner
    window of the bank's last key also equals wm_detect on the batched sweeps with that window as W.  Key == image shape: the
    single offset (0, 0) equals detectKeys on the very same bank"""
    torch = torch_cuda
    (KR, KC), (R, Cc) = kshape, shape
    keys, wins, key, rects, offs = banks_for(wm, kshape, shape)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype, first=2)).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0, max_frames=F)
    mt = wm.MASK_TYPE(mask)
    ref = np.asarray(eng.detectKeys(xs, wins, mt)).reshape(F, len(offs))
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) > 1e-4
    n0 = 0
    for (oy0, ox0, ny, nx) in rects:
        got = np.asarray(eng.detectOffsets(xs, keys, KBANK - 1, oy0, ox0, ny, nx, mt)).reshape(F, ny * nx)
        want = ref[:, n0:n0 + ny * nx]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ((oy0, ox0, ny, nx), got, want)
        n0 += ny * nx
    if (KR, KC) == (R, Cc):
        same = np.asarray(eng.detectKeys(xs, keys, mt)).reshape(F, KBANK)[:, KBANK - 1]
        got = np.asarray(eng.detectOffsets(xs, keys, KBANK - 1, 0, 0, 1, 1, mt)).reshape(F)
        assert np.array_equal(got.view(np.uint32), same.view(np.uint32))
    # wm_detect (fused kernels off) with the far-corner window as W
    oy, ox = KR - R, KC - Cc
    ek = wm.Watermark(R, Cc, window(key, R, Cc, oy, ox), p, 40.0, max_frames=F)
    ek.set_fused(False)
    one = np.asarray(ek.detectWatermark(xs, mt), np.float32).reshape(F)
    got = np.asarray(eng.detectOffsets(xs, keys, KBANK - 1, oy, ox, 1, 1, mt)).reshape(F)
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), (got, one)
    ek.close()
    eng.close()


# (key shape, image shape, rectangles (oy0, ox0, ny, nx)): with groups of 4, nx = 7 is a full shared group and a three-column
# remainder that runs as a group moved left, nx = 5 a one-column remainder in a launch of its own
SHARED_ROW_SHAPES = [((80, 300), (64, 256), [(3, 5, 2, 7), (1, 2, 2, 5)]), ((301, 523), (271, 483), [(3, 5, 2, 7)])]
SHARED_ROW_CASES = [(ks, s, rs, mk, dt, F) for ks, s, rs in SHARED_ROW_SHAPES for mk in (0, 1) for dt in ("f32", "u8") for F in (1, 5)]


@pytest.mark.parametrize("kshape,shape,rects,mask,dtype,F", SHARED_ROW_CASES)
def test_every_score_bit_equal_to_wm_detect(wm, torch_cuda, kshape, shape, rects, mask, dtype, F):
    """wm_detect_offsets and wm_detect_keys run one march (group_march), so their equality does not anchor the shared W row to
    independent code: every score of a rectangle equals, as uint32, wm_detect on the batched sweeps (fused kernels off:
    detect_march) with that window copied out as W.  p = 3; the aligned overlapped strips (256 columns) and the generic / split
    ones (483), the record per wave (F = 5) and per block (F = 1), the full, the moved-left and the one-column-tail groups"""
    torch = torch_cuda
    (KR, KC), (R, Cc) = kshape, shape
    keys = wm.KeySet.from_seeds(KR, KC, [4100 + 13 * k for k in range(KBANK)])
    key = keys.plane(KBANK - 1)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype, first=2)).cuda()
    mt = wm.MASK_TYPE(mask)
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    one = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    for (oy0, ox0, ny, nx) in rects:
        got = np.asarray(eng.detectOffsets(xs, keys, KBANK - 1, oy0, ox0, ny, nx, mt)).reshape(F, ny, nx)
        want = np.empty((F, ny, nx), np.float32)
        for i in range(ny):
            for j in range(nx):
                one.reinitialize(window(key, R, Cc, oy0 + i, ox0 + j), R, Cc)
                one.set_fused(False)
                want[:, i, j] = np.asarray(one.detectWatermark(xs, mt), np.float32).reshape(F)
        assert np.isfinite(want).all() and float(np.abs(want).max()) > 1e-4
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ((oy0, ox0, ny, nx), got, want)
    one.close()
    eng.close()
    keys.close()


@pytest.mark.parametrize("kshape,shape", SHAPES[1:4])
@pytest.mark.parametrize("mask,p", [(0, 3), (1, 3), (1, 7)])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_nothing_outside_the_window_counts(wm, torch_cuda, kshape, shape, mask, p, dtype):
    """two key planes that agree on the searched window and differ everywhere else -- zero outside, noise outside -- give
    identical bits for a one-offset search (the replicate border of u is the window's edge)"""
    torch = torch_cuda
    (KR, KC), (R, Cc) = kshape, shape
    rng = np.random.default_rng(11)
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0)
    x = torch.from_numpy(frames_of(R, Cc, 1, dtype, first=4)[0]).cuda()
    for (oy, ox) in ((0, 0), (3, 5), (KR - R, KC - Cc), (0, KC - Cc), (KR - R, 2)):
        w = rng.standard_normal((R, Cc)).astype(np.float32)
        noise = (100.0 * rng.standard_normal((KR, KC))).astype(np.float32)
        zero = np.zeros((KR, KC), np.float32)
        noise[oy:oy + R, ox:ox + Cc] = w
        zero[oy:oy + R, ox:ox + Cc] = w
        bank = wm.KeySet(KR, KC, 2)
        bank.set(0, zero)
        bank.set(1, noise)
        a = eng.detectOffsets(x, bank, 0, oy, ox, 1, 1, wm.MASK_TYPE(mask))
        b = eng.detectOffsets(x, bank, 1, oy, ox, 1, 1, wm.MASK_TYPE(mask))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ((oy, ox), a, b)
        assert abs(float(a[0, 0])) > 1e-5
        bank.close()
    eng.close()


def oracle_score(x, W, p, mask):
    if x.dtype == np.uint8:
        return O.detect_u8(x, W, p=p, mask=mask)[1]
    return O.detect(x, W, p=p, mask=mask)[1]


@pytest.mark.parametrize("kshape,shape", SHAPES)
@pytest.mark.parametrize("mask,p", [(0, 3), (1, 3), (1, 5)])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_oracle_parity(wm, torch_cuda, kshape, shape, mask, p, dtype):
    """|score - oracle.detect(image, window)| <= 1e-5: every offset on the small shapes, the corners of the rectangle on the
    large ones"""
    torch = torch_cuda
    (KR, KC), (R, Cc) = kshape, shape
    large = R > 300
    keys = wm.KeySet.from_seeds(KR, KC, [91, 92])
    key = keys.plane(1)
    x = frames_of(R, Cc, 1, dtype, first=1)[0]
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0)
    if (KR, KC) == (R, Cc):
        oy0, ox0, ny, nx = 0, 0, 1, 1
    else:
        ny, nx = 3, 6
        oy0, ox0 = KR - R - (ny - 1), KC - Cc - (nx - 1)
    got = eng.detectOffsets(torch.from_numpy(x).cuda(), keys, 1, oy0, ox0, ny, nx, wm.MASK_TYPE(mask))
    assert got.shape == (ny, nx)
    for i in range(ny):
        for j in range(nx):
            if large and not (i in (0, ny - 1) and j in (0, nx - 1)):
                continue
            ref = oracle_score(x, window(key, R, Cc, oy0 + i, ox0 + j), p, mask)
            assert abs(float(got[i, j]) - ref) <= TOL, ((i, j), float(got[i, j]), ref)
    keys.close()
    eng.close()


# (key shape, crop shape, true offset, frame, mask, dtype of the crop)
CROPS = [((270, 480), (200, 384), (37, 53), 0, 0, "f32"), ((270, 480), (200, 384), (37, 53), 1, 1, "f32"),
         ((270, 480), (200, 384), (37, 53), 2, 0, "u8"),
         ((2200, 3900), (2160, 3840), (17, 33), 0, 0, "f32"), ((2200, 3900), (2160, 3840), (17, 33), 1, 1, "f32")]
CROP_SEEDS = [7000 + 31 * k for k in range(3)]
CROP_KEY = 1


@pytest.mark.parametrize("kshape,shape,at,frame,mask,dtype", CROPS)
def test_finds_the_crop(wm, torch_cuda, kshape, shape, at, frame, mask, dtype):
    """A frame marked with key 1 of 3 (psnr 40, p = 3) at the key's shape, cropped at an offset with odd ox (floored to u8 in one
    case) and searched over the 7x7 offsets around the truth: the argmax is the true offset, the peak is >= 1.4x every other
    score (the +-1 neighbours: the prediction filter smears the peak over 3x3) and >= 3x every score at Chebyshev distance >= 2.
    The unmarked 200x384 crop scores below 0.05 at every offset.

    The CPU oracle on these very cases (keys from the device generator's host twin wm_genw, the embed by the oracle), as
    peak / best +-1 neighbour / best at distance >= 2 / largest |score| of the unmarked crop:
      270x480  -> 200x384   ME  f32  frame 0:  0.5484 / 0.1159 (4.73x) / 0.0339 (16.2x) / 0.0199
      270x480  -> 200x384   NVF f32  frame 1:  0.2979 / 0.1090 (2.73x) / 0.0394 (7.6x) / 0.0126
      270x480  -> 200x384   ME  u8   frame 2:  0.5405 / 0.1060 (5.10x) / 0.0249 (21.7x) / 0.0257
      2200x3900 -> 2160x3840 ME  f32 frame 0:  0.5457 / 0.0997 (5.47x) / 0.0231 (23.6x) / -
      2200x3900 -> 2160x3840 NVF f32 frame 1:  0.3062 / 0.1081 (2.83x) / 0.0357 (8.6x) / -"""
    torch = torch_cuda
    (KR, KC), (R, Cc), (oy, ox) = kshape, shape, at
    assert ox % 2 == 1
    mt = wm.MASK_TYPE(mask)
    keys = wm.KeySet.from_seeds(KR, KC, CROP_SEEDS)
    x = synth_frame(KR, KC, frame=frame)
    xt = torch.from_numpy(x).cuda()
    emb = wm.Watermark.generated(KR, KC, CROP_SEEDS[CROP_KEY], 3, 40.0)
    y, a = emb.makeWatermark(xt, xt, mt)
    emb.close()
    crop = y[oy:oy + R, ox:ox + Cc].contiguous()
    plain = xt[oy:oy + R, ox:ox + Cc].contiguous()
    if dtype == "u8":
        crop = crop.to(torch.uint8)  # (truncation of values in [0, 255])
        plain = plain.to(torch.uint8)
    det = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0)
    s = det.detectOffsets(crop, keys, CROP_KEY, oy - 3, ox - 3, 7, 7, mt)
    print("scores around the truth:\n", s[2:5, 2:5], "\nbest at distance >= 2:", _far(s).max())
    assert np.unravel_index(int(np.argmax(s)), s.shape) == (3, 3), s
    peak = float(s[3, 3])
    others = s.copy()
    others[3, 3] = -np.inf
    assert peak >= 1.4 * float(others.max()), (peak, float(others.max()))
    assert peak >= 3.0 * float(_far(s).max()), (peak, float(_far(s).max()))
    if (R, Cc) == (200, 384):
        u = det.detectOffsets(plain, keys, CROP_KEY, oy - 3, ox - 3, 7, 7, mt)
        print("unmarked crop, largest |score|:", float(np.abs(u).max()))
        assert float(np.abs(u).max()) < 0.05, u
    det.close()
    keys.close()


def _far(s):
    i, j = np.indices(s.shape)
    return s[np.maximum(np.abs(i - 3), np.abs(j - 3)) >= 2]


def test_unsolvable_frame_and_zero_key(wm, torch_cuda):
    torch = torch_cuda
    (KR, KC), (R, Cc), F = (300, 520), (270, 480), 5
    keys = wm.KeySet(KR, KC, 2)  # key 0 stays zero
    gen = wm.KeySet.from_seeds(KR, KC, [5])
    keys.set(1, gen.plane(0))
    xs = frames_of(R, Cc, F, "f32")
    xs[2] = 100.0  # constant frame: singular prediction system
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    ny, nx = 2, 5
    corr = np.full(F * ny * nx, 7.0, np.float32)
    st = np.full(F, -5, np.int32)
    eng.detect_offsets_async(torch.from_numpy(xs).cuda(), keys, 1, 4, 9, ny, nx, wm.MASK_TYPE.ME, 0, corr, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    corr = corr.reshape(F, ny, nx)
    assert list(st) == [0, 0, 1, 0, 0]
    assert np.all(corr[2] == 0.0)
    key = keys.plane(1)
    for f in (1, 3):
        for (i, j) in ((0, 0), (1, 4)):
            assert abs(float(corr[f, i, j]) - O.detect(xs[f], window(key, R, Cc, 4 + i, 9 + j))[1]) <= TOL
    # a key that is all zero scores NaN, as in wm_detect_keys
    z = eng.detectOffsets(torch.from_numpy(xs[:2]).cuda(), keys, 0, 0, 0, 2, 5, wm.MASK_TYPE.NVF)
    assert z.shape == (2, 2, 5) and np.isnan(z).all()


def test_enqueue_semantics(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    (KR, KC), (R, Cc) = (300, 520), (270, 480)
    keys = wm.KeySet.from_seeds(KR, KC, [300, 317])
    key = keys.plane(1)
    oy, ox = 11, 23
    W0 = window(key, R, Cc, oy, ox)
    kb = wm.KeySet(R, Cc, 2)
    kb.set(1, W0)
    x = synth_frame(R, Cc, frame=2)
    eng = wm.Watermark(R, Cc, W0, 3, 40.0, nslots=2)
    xt = torch.from_numpy(x).cuda()
    y0, y1 = torch.empty_like(xt), torch.empty_like(xt)
    a0, a1 = (C.c_float * 1)(), (C.c_float * 1)()
    c_det = (C.c_float * 1)()
    ck = np.zeros(2, np.float32)
    co0 = np.zeros((3, 5), np.float32)
    co1 = np.zeros((1, 6), np.float32)
    torch.cuda.synchronize()
    # slot 0: embed, detect_offsets of its output, detect, detect_keys; slot 1: detect_offsets first, then an embed; one sync each
    eng.embed_async(xt, xt, y0, wm.MASK_TYPE.ME, 0, a0)
    eng.detect_offsets_async(y0, keys, 1, oy - 1, ox - 2, 3, 5, wm.MASK_TYPE.ME, 0, co0)
    eng.detect_offsets_async(xt, keys, 1, oy, ox, 1, 6, wm.MASK_TYPE.NVF, 1, co1)
    eng.detect_async(y0, wm.MASK_TYPE.ME, 0, c_det)
    eng.detect_keys_async(y0, kb, wm.MASK_TYPE.ME, 0, ck)
    eng.embed_async(xt, xt, y1, wm.MASK_TYPE.NVF, 1, a1)
    eng.sync(1)
    eng.sync(0)
    yo = y0.cpu().numpy()
    for i in range(3):
        for j in range(5):
            assert abs(float(co0[i, j]) - O.detect(yo, window(key, R, Cc, oy - 1 + i, ox - 2 + j))[1]) <= TOL
    for j in range(6):
        assert abs(float(co1[0, j]) - O.detect(x, window(key, R, Cc, oy, ox + j), mask=1)[1]) <= TOL
    assert np.unravel_index(int(np.argmax(co0)), co0.shape) == (1, 2)
    assert co0[1, 2].view(np.uint32) == ck[1].view(np.uint32) and abs(c_det[0] - float(ck[1])) <= 2e-7
    # WM_MEM_HOST input
    hx = np.ascontiguousarray(x)
    ph = wm.wm_plane(hx.ctypes.data, R, Cc, 1, wm.WM_F32, wm.WM_MEM_HOST, 1, Cc, 0, 0)
    ch = np.zeros((2, 5), np.float32)
    eng.detect_offsets_async(ph, keys, 1, 3, 7, 2, 5, wm.MASK_TYPE.ME, wm.WM_SLOT_SYNC, ch)
    assert np.array_equal(ch, eng.detectOffsets(xt, keys, 1, 3, 7, 2, 5, wm.MASK_TYPE.ME))
    # WM_MEM_SLOT_OUT after an embed, hand-over off and on (2 frames: the hand-over applies to batched embeds)
    F = 2
    engb = wm.Watermark(R, Cc, W0, 3, 40.0, nslots=1, max_frames=F)
    xb = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    yb = torch.empty_like(xb)
    for ho in (False, True):
        engb.set_handover(ho)
        engb.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
        ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
        cs = np.zeros((F, 1, 5), np.float32)
        engb.detect_offsets_async(ps, keys, 1, oy, ox - 2, 1, 5, wm.MASK_TYPE.ME, 0, cs)
        engb.sync(0)
        ys = yb.cpu().numpy()
        for f in range(F):
            for j in (0, 2, 4):
                assert abs(float(cs[f, 0, j]) - O.detect(ys[f], window(key, R, Cc, oy, ox - 2 + j))[1]) <= TOL, (ho, f, j)
            assert int(np.argmax(cs[f, 0])) == 2
    # result capacity: frames x ny x nx count against 4096 un-synced results per slot
    big = wm.KeySet(R + 64, Cc + 64, 1)
    cb = np.zeros(4096, np.float32)
    eng.detect_async(xt, wm.MASK_TYPE.ME, 0, c_det)
    with pytest.raises(RuntimeError, match="un-synced"):
        eng.detect_offsets_async(xt, big, 0, 0, 0, 64, 64, wm.MASK_TYPE.ME, 0, cb)  # 1 + 4096 results
    assert L.wm_detect_offsets(eng._ctx, 0, C.byref(wm.plane_of(xt, 1)), big.handle, 0, 0, 0, 64, 64, cb.ctypes.data_as(C.POINTER(C.c_float)), None,
                               0) == wm.WM_ERR_BUSY
    eng.sync(0)
    eng.detect_offsets_async(xt, big, 0, 0, 0, 64, 64, wm.MASK_TYPE.ME, 0, cb)  # exactly the capacity: accepted
    eng.sync(0)
    assert np.isnan(cb).all()  # (a zero key)
    big.close()


def test_argument_errors_on_a_device(wm, torch_cuda):
    """the refusals of tests/test_offsets_abi.py through wm_detect_offsets itself: nothing is queued, the slot stays usable"""
    torch = torch_cuda
    L = wm.lib()
    (KR, KC), (R, Cc) = (80, 300), (64, 256)
    keys = wm.KeySet.from_seeds(KR, KC, [1, 2])
    small = wm.KeySet(R - 1, KC, 1)
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0)
    e5 = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 5, 40.0)
    xt = torch.from_numpy(synth_frame(R, Cc)).cuda()
    pl = wm.plane_of(xt, 1)
    out = np.zeros(17 * 45, np.float32)
    po = out.ctypes.data_as(C.POINTER(C.c_float))
    call = lambda k, oy0, ox0, ny, nx, kh=keys.handle, img=C.byref(pl), o=po: L.wm_detect_offsets(eng._ctx, 0, img, kh, k, oy0, ox0, ny, nx, o, None, 0)
    bad = wm.WM_ERR_BAD_ARG
    for args in ((0, -1, 0, 1, 1), (0, 0, -1, 1, 1), (0, 17, 0, 1, 1), (0, 0, 45, 1, 1), (0, 0, 0, 18, 1), (0, 0, 0, 1, 46), (0, 1, 0, 17, 1),
                 (0, 0, 1, 1, 45), (0, 0, 0, 0, 1), (0, 0, 0, 1, 0), (2, 0, 0, 1, 1), (-1, 0, 0, 1, 1)):
        assert call(*args) == bad, args
    assert call(0, 0, 0, 1, 1, kh=None) == bad and call(0, 0, 0, 1, 1, img=None) == bad and call(0, 0, 0, 1, 1, o=None) == bad
    assert call(0, 0, 0, 1, 1, kh=small.handle) == bad
    assert L.wm_detect_offsets(e5._ctx, 0, C.byref(pl), keys.handle, 0, 0, 0, 1, 1, po, None, 0) == wm.WM_ERR_BAD_P
    assert eng.sync(0) == wm.WM_OK  # nothing was queued
    assert call(1, 0, 0, 17, 45) == wm.WM_OK and eng.sync(0) == wm.WM_OK  # the whole rectangle
    key = keys.plane(1)
    x = synth_frame(R, Cc)
    for (i, j) in ((0, 0), (16, 44), (0, 44), (16, 0), (7, 21)):
        assert abs(float(out[i * 45 + j]) - O.detect(x, window(key, R, Cc, i, j))[1]) <= TOL, (i, j)


def test_deterministic(wm, torch_cuda):
    torch = torch_cuda
    (KR, KC), (R, Cc), F = (1100, 1950), (1078, 1918), 4
    keys = wm.KeySet.from_seeds(KR, KC, [8, 9])
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    for mk in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        a = eng.detectOffsets(xs, keys, 1, 5, 9, 3, 7, mk)
        b = eng.detectOffsets(xs, keys, 1, 5, 9, 3, 7, mk)
        c = eng.detectOffsets(xs, keys, 1, 5, 9, 3, 7, mk)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))


CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 270, C = 480, KR = 300, KC = 520;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    WatermarkKeys keys(KR, KC, 2);
    for (int k = 0; k < 2; ++k) keys.generate(k, 1000 + 17 * k);
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    for (int m = 0; m < 2; ++m) {
        const std::vector<float> s = w.detectOffsets(img, keys, 1, 7, 13, 3, 6, m == 0 ? ME : NVF);
        if (s.size() != 18) return 4;
        for (float v : s) printf("%.9g\n", v);
    }
    try { w.detectOffsets(img, keys, 1, 29, 0, 3, 1, ME); return 3; } catch (const std::runtime_error&) {}
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc, KR, KC = 270, 480, 300, 520
    src = tmp_path / "offsets.cpp"
    src.write_text(CPP)
    exe = tmp_path / "offsets"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    x = synth_frame(R, Cc, frame=6)
    xf = tmp_path / "x.f32"
    x.tofile(xf)
    wf = tmp_path / "w.dat"
    np.zeros((R, Cc), np.float32).tofile(wf)
    out = subprocess.run([str(exe), str(xf), str(wf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.array([float(v) for v in out.stdout.split()], np.float32).reshape(2, 3, 6)
    keys = wm.KeySet.from_seeds(KR, KC, [1000, 1017])
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0)
    xt = torch.from_numpy(x).cuda()
    for m, mk in enumerate((wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF)):
        assert np.array_equal(got[m], eng.detectOffsets(xt, keys, 1, 7, 13, 3, 6, mk)), (m, got[m])
