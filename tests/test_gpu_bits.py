"""A payload in the mark: wm_embed_signs / wm_embed_bits (k_embed_signs) and wm_detect_bits (k_bits_fold).  The embed against
wm_embed with W, -W and a zero W bit for bit, its queueing, edge cases and hand-over hygiene; the fold against wm_detect_tiles'
sums added sequentially bit for bit; soft values against the CPU oracle (tests/bits_model.py, <= 1e-5, the bound of every
detector test); the round trip of five cases; the capacity of the result records; the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bits_model as BM
import hard_frames as H
import tiles_model as TM
from synth import synth_frame, synth_watermark
from test_gpu_offsets import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_SEED = 6100


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames_of(R, Cc, F, dtype, first=0):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def raw(a):
    """the bits of an array: f32 as uint32, u8 as it is"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def random_signs(F, ny, nx, seed):
    return np.random.default_rng(seed).integers(-1, 2, (F, ny, nx)).astype(np.int8)


def select_frames(signs, th, tw, yp, yn, yz):
    """per frame and tile the pixels of the three reference outputs [F, (3,) R, C]"""
    return np.stack([BM.select(signs[f], th, tw, yp[f], yn[f], yz[f]) for f in range(len(signs))])


def host_plane(wm, a, channels=1):
    F, R, Cc = a.shape[0], a.shape[-2], a.shape[-1]
    return wm.wm_plane(a.ctypes.data, R, Cc, channels, wm.WM_U8 if a.dtype == np.uint8 else wm.WM_F32, wm.WM_MEM_HOST, F, Cc, R * Cc, channels * R * Cc)


# (R, C, tile_rows, tile_cols, mask, p, dtype, F, variant, rows per segment)
#   variants: grey = a grey base that is another picture; rgb = a planar-RGB base; input = the base is in_gray; inplace = input,
#   base and output are one plane; host = WM_MEM_HOST in and out.  F = 5 takes the quad mapping (one table per frame).
#   272 x 484 and 72 x 260: one tile larger than the plane.  The widths 483 take the generic strip at the right edge (f32) or the
#   generic strips throughout (u8); 24 rows per segment against tile_rows 40: segments straddle tile rows
EMBED_CASES = [
    (64, 256, 32, 32, 0, 3, "f32", 1, "input", 0),
    (64, 256, 32, 32, 1, 3, "u8", 5, "grey", 0),
    (64, 256, 72, 260, 0, 3, "f32", 1, "grey", 0),
    (270, 480, 32, 32, 0, 3, "f32", 5, "input", 0),
    (270, 480, 32, 32, 1, 5, "f32", 5, "input", 0),
    (270, 480, 40, 36, 0, 3, "u8", 1, "grey", 0),
    (270, 480, 40, 36, 0, 3, "f32", 5, "grey", 24),
    (270, 480, 64, 128, 1, 5, "f32", 1, "rgb", 0),
    (270, 480, 64, 128, 0, 3, "u8", 5, "rgb", 0),
    (270, 480, 32, 32, 0, 3, "u8", 5, "inplace", 0),
    (270, 480, 40, 36, 0, 3, "f32", 5, "host", 0),
    (270, 480, 272, 484, 1, 5, "u8", 5, "grey", 0),
    (271, 483, 32, 32, 0, 3, "f32", 5, "grey", 0),
    (271, 483, 40, 36, 1, 9, "f32", 1, "input", 0),
    (271, 483, 40, 36, 0, 3, "u8", 5, "input", 0),
    (271, 483, 64, 128, 1, 3, "f32", 5, "inplace", 0),
    (271, 483, 32, 32, 1, 3, "u8", 1, "host", 0),
    (271, 483, 64, 128, 1, 9, "u8", 5, "grey", 0),
]


@pytest.mark.parametrize("R,Cc,th,tw,mask,p,dtype,F,variant,rps", EMBED_CASES)
def test_embed_bit_equal_to_wm_embed(wm, torch_cuda, R, Cc, th, tw, mask, p, dtype, F, variant, rps):
    """wm_embed_signs with a random {-1, 0, +1} table equals, as bits, the per-tile selection of wm_embed's outputs on three
    contexts with W, -W and a zero W (fused off); `a` equals the W context's; an all-+1 table equals wm_embed outright"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + R + th)
    engs = [wm.Watermark(R, Cc, w, p, 40.0, nslots=1, max_frames=F) for w in (W, -W, H.zero_w(R, Cc))]
    for e in engs:
        e.set_fused(False)
        if rps:
            e.set_rows_per_segment(rps)
    xs = frames_of(R, Cc, F, dtype, first=2)
    if variant == "rgb":
        base = np.stack([frames_of(R, Cc, 3, dtype, first=20 + 3 * f) for f in range(F)])  # [F, 3, R, C]
    elif variant == "grey":
        base = frames_of(R, Cc, F, dtype, first=40)
    else:
        base = xs
    signs = random_signs(F, ny, nx, 1000 * R + th + 7 * mask)
    assert {-1, 0, 1} <= set(signs.ravel().tolist()) or ny * nx < 3

    def run(e, call):
        """one embed on slot 0 of `e`, waited for: call(in, base, out, a_out, status_out) -> (output as numpy, a)"""
        a = np.full(F, np.nan, np.float32)
        st = np.full(F, -5, np.int32)
        if variant == "host":
            hin, hout = np.ascontiguousarray(xs), np.empty_like(base)
            pin = host_plane(wm, hin)
            call(pin, pin, host_plane(wm, hout), a, st)
        else:
            tin = torch.from_numpy(xs).cuda()
            if variant == "inplace":
                tbase = tout = tin
            else:
                tbase = tin if variant == "input" else torch.from_numpy(base).cuda()
                tout = torch.empty_like(tbase)
            torch.cuda.synchronize()
            call(tin, tbase, tout, a, st)
        assert e.sync(0) == wm.WM_OK and list(st) == [0] * F
        return (hout if variant == "host" else tout.cpu().numpy()), a

    outs = []
    for e in engs:
        outs.append(run(e, lambda i, b, o, a_, s_, e=e: e.embed_async(i, b, o, mt, 0, a_.ctypes.data_as(C.POINTER(C.c_float)), s_.ctypes.data_as(C.POINTER(C.c_int)))))
    (yp, ap), (yn, an), (yz, az) = outs
    assert np.array_equal(raw(ap), raw(an)) and np.all(np.isinf(az)) and np.array_equal(raw(yz), raw(base))
    assert not np.array_equal(raw(yp), raw(yn))

    eng = engs[0]
    for table, want in ((signs, select_frames(signs, th, tw, yp, yn, yz)), (np.ones_like(signs), yp)):
        got, a = run(eng, lambda i, b, o, a_, s_: eng.embed_signs_async(i, b, o, th, tw, table, mt, 0, a_, s_))
        assert np.array_equal(raw(a), raw(ap)), (a, ap)
        diff = raw(got) != raw(want)
        assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4])
    for e in engs:
        e.close()


def test_queueing_keeps_each_table(wm, torch_cuda):
    """two un-synced calls on one slot with different tables, the caller's array overwritten between and after the calls: each
    output matches its own table"""
    torch = torch_cuda
    R, Cc, th, tw, F = 270, 480, 32, 32, 2
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 1)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    eng.set_fused(False)
    xt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=3)).cuda()
    t1, t2 = random_signs(F, ny, nx, 11), random_signs(F, ny, nx, 12)
    want = []
    for t in (t1, t2):
        y = torch.empty_like(xt)
        torch.cuda.synchronize()
        eng.embed_signs_async(xt, xt, y, th, tw, t.copy(), wm.MASK_TYPE.ME, 0)
        eng.sync(0)
        want.append(y.cpu().numpy())
    assert not np.array_equal(want[0], want[1])
    table = t1.copy()
    y1, y2 = torch.empty_like(xt), torch.empty_like(xt)
    torch.cuda.synchronize()
    eng.embed_signs_async(xt, xt, y1, th, tw, table, wm.MASK_TYPE.ME, 0)
    table[...] = t2
    eng.embed_signs_async(xt, xt, y2, th, tw, table, wm.MASK_TYPE.ME, 0)
    table[...] = 0
    assert eng.sync(0) == wm.WM_OK
    assert np.array_equal(raw(y1.cpu().numpy()), raw(want[0])) and np.array_equal(raw(y2.cpu().numpy()), raw(want[1]))
    eng.close()


def test_embed_edge_cases(wm, torch_cuda):
    """a flat frame under ME: status 1, out == base, `a` untouched; a zero W: a = +inf, out == base; a bad sign value or tile
    shape: WM_ERR_BAD_ARG with nothing queued; ME needs p = 3; band mode refuses the call"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc, th, tw, F = 64, 256, 32, 32, 2
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 2)
    signs = random_signs(F, ny, nx, 21)
    xs = frames_of(R, Cc, F, "f32", first=1)
    xs[1] = H.flat(R, Cc, 100)
    base = torch.from_numpy(frames_of(R, Cc, F, "f32", first=9)).cuda()
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    a, st = np.full(F, 123.0, np.float32), np.full(F, -5, np.int32)
    y = torch.zeros_like(base)
    torch.cuda.synchronize()
    eng.embed_signs_async(torch.from_numpy(xs).cuda(), base, y, th, tw, signs, wm.MASK_TYPE.ME, 0, a, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE and list(st) == [0, 1]
    assert a[1] == 123.0 and np.isfinite(a[0]) and a[0] != 123.0
    assert np.array_equal(raw(y[1].cpu().numpy()), raw(base[1].cpu().numpy())) and not np.array_equal(y[0].cpu().numpy(), base[0].cpu().numpy())
    # a zero W
    ez = wm.Watermark(R, Cc, H.zero_w(R, Cc), 3, 40.0, nslots=1, max_frames=F)
    for mt in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        xt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=1)).cuda()
        yz, az = ez.makeWatermarkSigns(xt, base, th, tw, signs, mt)
        assert all(np.isposinf(v) for v in az) and np.array_equal(raw(yz.cpu().numpy()), raw(base.cpu().numpy()))
    ez.close()
    # refusals: nothing is queued
    xt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=1)).cuda()
    pl = wm.plane_of(xt, 1)
    po = wm.plane_of(y, 1)
    torch.cuda.synchronize()
    sp = lambda s: s.ctypes.data_as(C.c_void_p)
    call = lambda t=signs, a_=th, b_=tw, ctx=eng._ctx, mask=0, i=C.byref(pl): L.wm_embed_signs(ctx, mask, i, C.byref(pl), C.byref(po), a_, b_, sp(t) if t is not None else None,
                                                                                           None, None, 0)
    bad = wm.WM_ERR_BAD_ARG
    for v in (2, -2, 127, -128):
        t = signs.copy()
        t[1, ny - 1, nx - 1] = v
        assert call(t) == bad, v
    for (a_, b_) in ((36, 32), (24, 32), (32, 30), (32, 28), (0, 32), (32, 0)):
        assert call(a_=a_, b_=b_) == bad, (a_, b_)
    assert call(t=None) == bad and call(i=None) == bad and call(mask=2) == bad
    e5 = wm.Watermark(R, Cc, W, 5, 40.0, nslots=1, max_frames=F)
    assert call(ctx=e5._ctx) == wm.WM_ERR_BAD_P
    assert call(ctx=e5._ctx, mask=1) == wm.WM_OK and e5.sync(0) == wm.WM_OK
    eb = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    assert L.wm_band_configure(eb._ctx, 8, 40, 128) == wm.WM_OK
    assert call(ctx=eb._ctx) == bad
    assert eng.sync(0) == wm.WM_OK  # nothing was queued
    assert call() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    # wm_embed_bits: nbits and the table's entries
    tb = wm.Watermark.bits_layout(ny, nx, 4, 1)
    pay = np.zeros(F, np.uint8)
    bits = lambda t=tb, n=4: L.wm_embed_bits(eng._ctx, 0, C.byref(pl), C.byref(pl), C.byref(po), th, tw, sp(t), n, sp(pay), None, None, 0)
    over, under = tb.copy(), tb.copy()
    over[3], under[5] = 4, -2
    assert bits(n=0) == bad and bits(n=4097) == bad and bits(over) == bad and bits(under) == bad
    assert eng.sync(0) == wm.WM_OK
    assert bits() == wm.WM_OK and eng.sync(0) == wm.WM_OK
    for e in (eng, e5, eb):
        e.close()


def test_leaves_no_handover(wm, torch_cuda):
    """after wm_embed_signs on F = 2 grey f32 aligned planes, wm_detect of the output agrees with a fresh context's wm_detect of
    a copy to <= 1.2e-7 and leaves the checked hand-over's counts unchanged -- also when an ordinary wm_embed into the same plane
    left a hand-over just before"""
    torch = torch_cuda
    R, Cc, th, tw, F = 270, 480, 32, 32, 2
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 3)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    xt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=4)).cuda()
    y = torch.empty_like(xt)
    corr = np.zeros(F, np.float32)
    torch.cuda.synchronize()
    before = eng.checked_handover_counts()
    eng.embed_async(xt, xt, y, wm.MASK_TYPE.ME, 0)
    eng.embed_signs_async(xt, xt, y, th, tw, random_signs(F, ny, nx, 31), wm.MASK_TYPE.ME, 0)
    eng.detect_async(y, wm.MASK_TYPE.ME, 0, corr.ctypes.data_as(C.POINTER(C.c_float)))
    assert eng.sync(0) == wm.WM_OK
    assert eng.checked_handover_counts() == before
    fresh = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    fresh.set_fused(False)
    ref = np.asarray(fresh.detectWatermark(y.clone(), wm.MASK_TYPE.ME), np.float32)
    assert float(np.abs(corr.astype(np.float64) - ref.astype(np.float64)).max()) <= 1.2e-7, (corr, ref)
    eng.close()
    fresh.close()


def table_with_gaps(ny, nx, nbits, seed):
    """wm_bits_layout's table with the tiles of the LAST bit left unmarked (-1): that bit has no tile and scores NaN"""
    tb = BM.layout(ny, nx, nbits, seed)
    tb[tb == nbits - 1] = -1
    return tb


FOLD_CASES = [(64, 256, 32, 32, 16, 0, 3, "f32", 1), (270, 480, 32, 32, 48, 0, 3, "u8", 5), (270, 480, 40, 36, 7, 1, 3, "f32", 5),
              (271, 483, 40, 36, 32, 1, 5, "u8", 1), (271, 483, 64, 128, 5, 0, 3, "f32", 5), (270, 480, 272, 484, 1, 1, 3, "u8", 5),
              (270, 480, 32, 32, 100, 0, 3, "f32", 1)]


@pytest.mark.parametrize("R,Cc,th,tw,nbits,mask,p,dtype,F", FOLD_CASES)
def test_fold_bit_equal_to_sequential_sum(wm, torch_cuda, R, Cc, th, tw, nbits, mask, p, dtype, F):
    """soft equals, as uint32, the score expression over detectTiles(..., sums=True) added per bit one after the other in
    ascending tile index; a bit without a tile is NaN; a frame's values do not depend on the batch or on repetition"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, W_SEED + 4), p, 40.0, nslots=1, max_frames=F)
    xt = torch.from_numpy(frames_of(R, Cc, F, dtype, first=5)).cuda()
    for tb in (BM.layout(ny, nx, nbits, 12345), table_with_gaps(ny, nx, nbits, 777)):
        _, s = eng.detectTiles(xt, th, tw, mt, sums=True)
        payload, soft = eng.detectBits(xt, th, tw, tb, nbits, mt)
        assert soft.shape == (F, nbits) and len(payload) == F
        want = np.stack([BM.soft_of_sums(s[f], tb, nbits) for f in range(F)])
        empty = np.array([not (tb == b).any() for b in range(nbits)])
        assert np.array_equal(np.isnan(soft), np.broadcast_to(empty, soft.shape)) and np.array_equal(np.isnan(want), np.isnan(soft))
        assert np.array_equal(raw(soft[:, ~empty]), raw(want[:, ~empty])), (soft, want)
        assert payload == [BM.pack_bits(soft[f] > 0) for f in range(F)]
        assert np.array_equal(raw(eng.detectBits(xt, th, tw, tb, nbits, mt)[1]), raw(soft))
        one = eng.detectBits(xt[F - 1], th, tw, tb, nbits, mt)[1]
        assert np.array_equal(raw(one), raw(soft[F - 1]))
    eng.close()


PARITY_CASES = [(64, 256, 32, 32, 16, 0, 3, "u8"), (64, 256, 32, 32, 16, 1, 3, "f32"), (270, 480, 32, 32, 48, 0, 3, "f32"),
                (270, 480, 64, 128, 6, 1, 5, "u8"), (271, 483, 40, 36, 32, 0, 3, "u8"), (271, 483, 40, 36, 32, 1, 9, "f32"),
                (271, 483, 272, 484, 1, 0, 3, "f32")]


@pytest.mark.parametrize("R,Cc,th,tw,nbits,mask,p,dtype", PARITY_CASES)
def test_oracle_parity(wm, torch_cuda, R, Cc, th, tw, nbits, mask, p, dtype):
    """planes composed on the CPU from the oracle's embed with W and -W: |soft - restatement| <= 1e-5"""
    torch = torch_cuda
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 5)
    tb = BM.layout(ny, nx, nbits, 12345)
    bits = np.random.default_rng(9).integers(0, 2, nbits)
    x = synth_frame(R, Cc, frame=3)
    st, y, _ = BM.compose(x, W, th, tw, BM.signs_of(tb, BM.pack_bits(bits), nbits), p=p, mask=mask)
    if dtype == "u8":
        y = np.floor(y).astype(np.uint8)
    st, ref = BM.soft(y, W, th, tw, tb, nbits, p=p, mask=mask)
    assert st == 0
    eng = wm.Watermark(R, Cc, W, p, 40.0)
    payload, soft = eng.detectBits(torch.from_numpy(y).cuda(), th, tw, tb, nbits, wm.MASK_TYPE(mask))
    worst = float(np.abs(soft.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{R}x{Cc} {th}x{tw} {nbits} bits mask {mask} p {p} {dtype}: worst |diff| {worst:.2e}, min |soft| {float(np.abs(ref).min()):.4f}")
    assert np.isfinite(soft).all() and worst <= TOL, (soft, ref)
    eng.close()


# the five cases of the round trip: (R, C, tile_rows, tile_cols, nbits, u8, the top-left quarter replaced by frame 7).  Layout seed
# 12345, synth_frame(frame=1), synth_watermark(seed 777), payload from default_rng(9), psnr 40, p = 3.
# The CPU oracle on them (tests/bits_model.py), min |soft| of the marked frame / max |soft| of the unmarked frame, ME and NVF:
#   64x256    32x32 16 bits u8          0.416 / 0.134   0.160 / 0.121
#   270x480   32x32 48 bits u8          0.422 / 0.133   0.254 / 0.084
#   270x480   32x32 24 bits u8 spliced  0.244 / 0.090   0.124 / 0.058
#   271x483   40x36 32 bits f32         0.508 / 0.081   0.266 / 0.043
#   1078x1918 64x64 64 bits u8 spliced  0.231 / 0.033   0.122 / 0.021
ROUND_TRIP = [(64, 256, 32, 32, 16, True, False), (270, 480, 32, 32, 48, True, False), (270, 480, 32, 32, 24, True, True),
              (271, 483, 40, 36, 32, False, False), (1078, 1918, 64, 64, 64, True, True)]
_oracle = {}


def oracle_case(case, mask):
    """(tile_bit, payload, the oracle's min |soft| of the marked frame) -- recomputed here, not copied from the table above"""
    if (case, mask) not in _oracle:
        R, Cc, th, tw, nbits, u8, splice = case
        ny, nx = TM.tiles_shape(R, Cc, th, tw)
        tb = BM.layout(ny, nx, nbits, 12345)
        bits = np.random.default_rng(9).integers(0, 2, nbits)
        payload = BM.pack_bits(bits)
        x, W = synth_frame(R, Cc, frame=1), synth_watermark(R, Cc, 777)
        st, y, _ = BM.compose(x, W, th, tw, BM.signs_of(tb, payload, nbits), mask=mask)
        if splice:
            y[:R // 2, :Cc // 2] = synth_frame(R, Cc, frame=7)[:R // 2, :Cc // 2]
        if u8:
            y = np.floor(y).astype(np.uint8)
        st, s = BM.soft(y, W, th, tw, tb, nbits, mask=mask)
        assert st == 0 and np.array_equal(s > 0, bits == 1)
        _oracle[(case, mask)] = (tb, payload, float(np.abs(s).min()))
    return _oracle[(case, mask)]


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("case", ROUND_TRIP)
def test_round_trip(wm, torch_cuda, case, mask):
    """wm_embed_bits -> wm_detect_bits on the GPU: the decoded payload is the payload and min |soft| is at least half the oracle's
    figure for the case (a sanity floor: the GPU's y differs from the oracle's by <= 1e-3 per pixel, which moves a score by about
    1e-4).  Once on the device plane -- spliced and floored to u8 where the case says so -- and once as WM_MEM_SLOT_OUT after a
    host-staged embed in the case's element type (the slot's output as it is: the splice belongs to the first leg only)"""
    torch = torch_cuda
    R, Cc, th, tw, nbits, u8, splice = case
    mt = wm.MASK_TYPE(mask)
    tb, payload, floor = oracle_case(case, mask)
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, 777), 3, 40.0, nslots=1)
    x = synth_frame(R, Cc, frame=1)
    xt = torch.from_numpy(x).cuda()
    y, a = eng.makeWatermarkBits(xt, xt, th, tw, tb, nbits, payload, mt)
    assert a is not None and np.isfinite(a)
    if splice:
        y[:R // 2, :Cc // 2] = torch.from_numpy(synth_frame(R, Cc, frame=7)[:R // 2, :Cc // 2]).cuda()
    if u8:
        y = y.to(torch.uint8)  # (truncation of values in [0, 255])
    got, soft = eng.detectBits(y, th, tw, tb, nbits, mt)
    print(f"{case} mask {mask}: device plane min |soft| {float(np.abs(soft).min()):.4f}, oracle {floor:.4f}")
    assert got == payload, (soft, BM.payload_bits(payload, nbits))
    assert float(np.abs(soft).min()) >= 0.5 * floor
    # host-staged embed, then the slot's output
    hx = np.ascontiguousarray(synth_frame(R, Cc, frame=1, dtype=np.uint8) if u8 else x)[None]
    hy = np.empty_like(hx)
    pin = host_plane(wm, hx)
    s2 = np.zeros(nbits, np.float32)
    eng.embed_bits_async(pin, pin, host_plane(wm, hy), th, tw, tb, nbits, payload, mt, 0)
    ps = wm.wm_plane(None, R, Cc, 1, wm.WM_U8 if u8 else wm.WM_F32, wm.WM_MEM_SLOT_OUT, 1, Cc, 0, R * Cc)
    eng.detect_bits_async(ps, th, tw, tb, nbits, mt, 0, s2)
    assert eng.sync(0) == wm.WM_OK
    print(f"{case} mask {mask}: slot output min |soft| {float(np.abs(s2).min()):.4f}")
    assert BM.pack_bits(s2 > 0) == payload and float(np.abs(s2).min()) >= 0.5 * floor
    # the staged output is the plane the detector read: the same bits where both take the same strips (wm.h wm_detect_tiles: f32
    # planes and widths that are multiples of 4), else a regrouping of the same sums (<= 2e-7)
    again = eng.detectBits(torch.from_numpy(hy[0]).cuda(), th, tw, tb, nbits, mt)[1]
    if not u8 or Cc % 4 == 0:
        assert np.array_equal(raw(again), raw(s2))
    else:
        assert float(np.abs(again.astype(np.float64) - s2.astype(np.float64)).max()) <= 2e-7
    eng.close()


def test_capacity_and_unsolvable(wm, torch_cuda):
    """frames * nbits results count against the slot's 4096 records: beyond them WM_ERR_BUSY, nothing queued; exactly 4096 fit.
    An unsolvable frame: 0.0f for every bit and status WM_UNSOLVABLE"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc, th, tw, F = 64, 256, 32, 32, 2
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, W_SEED + 6), 3, 40.0, nslots=1, max_frames=F)
    xs = frames_of(R, Cc, F, "f32", first=2)
    xs[0] = H.flat(R, Cc, 100)
    xt = torch.from_numpy(xs).cuda()
    pl = wm.plane_of(xt, 1)
    tb = (np.arange(ny * nx) % 8).astype(np.int32)
    torch.cuda.synchronize()
    soft = np.full((F, 2049), 7.0, np.float32)
    call = lambda n: L.wm_detect_bits(eng._ctx, 0, C.byref(pl), th, tw, tb.ctypes.data_as(C.c_void_p), n, soft.ctypes.data_as(C.POINTER(C.c_float)), None, 0)
    assert call(2049) == wm.WM_ERR_BUSY and call(4097) == wm.WM_ERR_BAD_ARG and call(0) == wm.WM_ERR_BAD_ARG
    assert eng.sync(0) == wm.WM_OK and np.all(soft == 7.0)
    assert call(2048) == wm.WM_OK
    assert call(8) == wm.WM_ERR_BUSY  # (the slot is full until its sync)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    got = soft.reshape(-1)[:F * 2048].reshape(F, 2048)
    assert np.all(got[0] == 0.0) and np.isfinite(got[1, :8]).all() and np.isnan(got[1, 8:]).all()
    st = np.full(F, -5, np.int32)
    s8 = np.zeros((F, 8), np.float32)
    eng.detect_bits_async(xt, th, tw, tb, 8, wm.MASK_TYPE.ME, 0, s8, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE and list(st) == [1, 0]
    assert np.array_equal(raw(s8[1]), raw(got[1, :8])) and np.all(s8[0] == 0.0)
    eng.close()


CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 270, C = 480, NB = 24;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    const std::vector<int32_t> tb = Watermark::bitsLayout(8, 15, NB, 12345);
    if (tb.size() != 120) return 4;
    const std::vector<uint8_t> payload = {0xA5, 0x3C, 0x0F};
    for (int m = 0; m < 2; ++m) {
        float a = -1.0f;
        const wm::Image y = w.makeWatermarkBits(img, img, a, 32, 32, tb, NB, payload, m == 0 ? ME : NVF);
        std::vector<uint8_t> back;
        const std::vector<float> soft = w.detectBits(y, 32, 32, tb, NB, m == 0 ? ME : NVF, &back);
        if (soft.size() != (size_t)NB || back != payload || !(a > 0.0f)) return 5;
        printf("%.9g\n", a);
        for (float v : soft) printf("%.9g\n", v);
    }
    std::vector<int8_t> signs(120, 1);
    float a1 = 0.0f, a2 = 0.0f;
    const wm::Image y1 = w.makeWatermarkSigns(img, img, a1, 32, 32, signs, ME);
    signs[7] = 3;
    try { w.makeWatermarkSigns(img, img, a2, 32, 32, signs, ME); return 3; } catch (const std::runtime_error&) {}
    try { Watermark::bitsLayout(8, 15, 121, 1); return 6; } catch (const std::runtime_error&) {}
    printf("%.9g\n", a1);
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc, nbits = 270, 480, 24
    src = tmp_path / "bits.cpp"
    src.write_text(CPP)
    exe = tmp_path / "bits"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    x = synth_frame(R, Cc, frame=6)
    xf = tmp_path / "x.f32"
    x.tofile(xf)
    W = synth_watermark(R, Cc, W_SEED + 7)
    wf = tmp_path / "w.dat"
    W.tofile(wf)
    out = subprocess.run([str(exe), str(xf), str(wf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.array([float(v) for v in out.stdout.split()], np.float32)
    assert got.size == 2 * (1 + nbits) + 1
    eng = wm.Watermark(R, Cc, W, 3, 40.0)
    eng.set_fused(False)
    xt = torch.from_numpy(x).cuda()
    tb = wm.Watermark.bits_layout(8, 15, nbits, 12345)
    payload = bytes([0xA5, 0x3C, 0x0F])
    for m, mk in enumerate((wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF)):
        y, a = eng.makeWatermarkBits(xt, xt, 32, 32, tb, nbits, payload, mk)
        back, soft = eng.detectBits(y, 32, 32, tb, nbits, mk)
        part = got[m * (1 + nbits):(m + 1) * (1 + nbits)]
        assert back == payload and np.array_equal(raw(part[1:]), raw(soft)) and raw(part[:1])[0] == raw(np.float32(a).reshape(1))[0]
    assert raw(got[-1:])[0] == raw(np.float32(eng.makeWatermark(xt, xt, wm.MASK_TYPE.ME)[1]).reshape(1))[0]
    eng.close()
