"""One frame, many payload copies: wm_embed_signs_multi / wm_embed_bits_multi (k_embed_signs_multi).  Every copy and the frame's
strength against wm_embed_signs on the same context bit for bit -- full, ragged and several copy groups, both masks and element
types, the quad mapping, grey / RGB / input bases, aligned and generic strips, host input, an output with padded rows and gapped
frames behind which nothing may be written --, the round trip of K payloads, unsolvable and zero-energy frames, the refusals, the
queueing and hand-over hygiene, and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bits_model as BM
import hard_frames as H
from synth import synth_frame, synth_watermark
from test_gpu_bits import frames_of, host_plane, raw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_SEED = 6300


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def G(wm):
    return wm.lib().wm_embed_signs_group()


def random_signs(F, K, ny, nx, seed):
    return np.random.default_rng(seed).integers(-1, 2, (F, K, ny, nx)).astype(np.int8)


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


POISON = {"f32": -777.25, "u8": 0xAB}


class Gapped:
    """a device buffer of n frames whose rows are padded to a wider pitch and whose frames lie a gap apart, poisoned, with a poison
    band of `guard` frames behind the last frame (a store one copy group too far stays inside the buffer and is seen): the plane
    for the library and, after the call, the frames and everything that is NOT a frame"""

    def __init__(self, wm, torch, n, R, Cc, dtype, guard, channels=1):
        self.n, self.R, self.Cc, self.ch = n, R, Cc, channels
        self.pitch = Cc + 16
        self.cstride = R * self.pitch + 4 * self.pitch
        self.fstride = channels * self.cstride + 8 * self.pitch
        self.total = (n + guard) * self.fstride
        tdt = torch.float32 if dtype == "f32" else torch.uint8
        self.poison = POISON[dtype]
        self.buf = torch.full((self.total,), self.poison, dtype=tdt, device="cuda")
        self.plane = wm.wm_plane(self.buf.data_ptr(), R, Cc, channels, wm.WM_F32 if dtype == "f32" else wm.WM_U8, wm.WM_MEM_DEVICE, n, self.pitch,
                                 self.cstride, self.fstride)

    def split(self):
        """(frames [n, (ch,) R, C], everything else as one flat array)"""
        h = self.buf.cpu().numpy()
        inside = np.zeros(self.total, bool)
        out = np.empty((self.n, self.ch, self.R, self.Cc), h.dtype)
        for f in range(self.n):
            for c in range(self.ch):
                o = f * self.fstride + c * self.cstride
                v = np.lib.stride_tricks.as_strided(h[o:], (self.R, self.Cc), (self.pitch * h.itemsize, h.itemsize))
                out[f, c] = v
                np.lib.stride_tricks.as_strided(inside[o:], (self.R, self.Cc), (self.pitch, 1))[...] = True
        return (out[:, 0] if self.ch == 1 else out), h[~inside]


# (R, C, tile_rows, tile_cols, mask, p, dtype, F, variant, rows per segment, which K of (1, G, G + 1, 2 G + 1))
#   variants: input = the base is in_gray; grey = a grey base that is another picture; rgb = a planar-RGB base; host = a WM_MEM_HOST
#   in_gray that is the base as well; gapped = a grey base and an `out` with padded rows and gapped frames (class Gapped).
#   F = 5 takes the quad mapping.  Width 480: the aligned path; 483: the generic strip at the right edge (f32) or the generic strips
#   throughout (u8).  24 rows per segment against tile_rows 40: segments straddle tile rows.  272 x 484: one tile
CASES = [
    (64, 256, 32, 32, 0, 3, "f32", 1, "input", 0, 0),
    (64, 256, 32, 32, 1, 3, "u8", 5, "grey", 0, 1),
    (270, 480, 32, 32, 0, 3, "f32", 5, "input", 0, 2),
    (270, 480, 32, 32, 1, 5, "f32", 5, "input", 0, 3),
    (270, 480, 40, 36, 0, 3, "u8", 1, "grey", 0, 2),
    (270, 480, 40, 36, 0, 3, "f32", 5, "grey", 24, 3),
    (270, 480, 64, 128, 1, 5, "f32", 1, "rgb", 0, 1),
    (270, 480, 64, 128, 0, 3, "u8", 5, "rgb", 0, 2),
    (270, 480, 40, 36, 0, 3, "f32", 5, "host", 0, 2),
    (270, 480, 272, 484, 1, 5, "u8", 5, "grey", 0, 1),
    (270, 480, 32, 32, 0, 3, "f32", 2, "gapped", 0, 2),
    (271, 483, 32, 32, 0, 3, "f32", 5, "grey", 0, 3),
    (271, 483, 40, 36, 1, 9, "f32", 1, "input", 0, 2),
    (271, 483, 40, 36, 0, 3, "u8", 5, "input", 0, 1),
    (271, 483, 64, 128, 1, 9, "u8", 5, "grey", 0, 2),
    (271, 483, 32, 32, 1, 3, "u8", 1, "gapped", 0, 3),
]


@pytest.mark.parametrize("R,Cc,th,tw,mask,p,dtype,F,variant,rps,kidx", CASES)
def test_bit_equal_to_wm_embed_signs(wm, torch_cuda, G, R, Cc, th, tw, mask, p, dtype, F, variant, rps, kidx):
    """copy (f, k) and a[f] equal, as raw bits, the output and strength of wm_embed_signs on the same context (fused off) with the
    table signs[f][k]; the last copy's table repeats the first one's (two copies with equal tables are the same bits); an all-+1
    table gives wm_embed's output for every copy; a gapped `out` keeps its poison everywhere outside the copies"""
    torch = torch_cuda
    mt = wm.MASK_TYPE(mask)
    K = (1, G, G + 1, 2 * G + 1)[kidx]
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, W_SEED + R + th), p, 40.0, nslots=1, max_frames=F)
    eng.set_fused(False)
    if rps:
        eng.set_rows_per_segment(rps)
    xs = frames_of(R, Cc, F, dtype, first=2)
    ch = 3 if variant == "rgb" else 1
    if variant == "rgb":
        base = np.stack([frames_of(R, Cc, 3, dtype, first=20 + 3 * f) for f in range(F)])  # [F, 3, R, C]
    elif variant in ("grey", "gapped"):
        base = frames_of(R, Cc, F, dtype, first=40)
    else:
        base = xs
    dev = [torch.from_numpy(xs).cuda(), torch.from_numpy(base).cuda()]  # (kept alive: a wm_plane holds no reference to its tensor)
    if variant == "host":
        hin = np.ascontiguousarray(xs)
        tin = tbase = host_plane(wm, hin)
    else:
        tin = wm.plane_of(dev[0], 1)
        tbase = tin if variant == "input" else wm.plane_of(dev[1], ch)
    signs = random_signs(F, K, ny, nx, 1000 * R + th + 7 * mask + K)
    if K > 1:
        signs[:, K - 1] = signs[:, 0]
    assert {-1, 0, 1} <= set(signs.ravel().tolist()) or ny * nx * K < 6

    def single(call):
        """one embed of the F frames on slot 0, waited for: (output as numpy, a)"""
        a, st = np.full(F, np.nan, np.float32), np.full(F, -5, np.int32)
        out = torch.empty((F,) + base.shape[1:], dtype=dev[1].dtype, device="cuda")
        torch.cuda.synchronize()
        call(wm.plane_of(out, ch), a, st)
        assert eng.sync(0) == wm.WM_OK and list(st) == [0] * F
        return out.cpu().numpy(), a

    def multi(table):
        a, st = np.full(F, np.nan, np.float32), np.full(F, -5, np.int32)
        if variant == "gapped":
            gp = Gapped(wm, torch, F * K, R, Cc, dtype, G)
            pout = gp.plane
        else:
            out = torch.empty((F * K,) + base.shape[1:], dtype=dev[1].dtype, device="cuda")
            pout = wm.plane_of(out, ch)
        torch.cuda.synchronize()
        eng.embed_signs_multi_async(tin, tbase, pout, th, tw, K, table, mt, 0, a, st)
        assert eng.sync(0) == wm.WM_OK and list(st) == [0] * F
        if variant == "gapped":
            got, rest = gp.split()
            assert np.all(rest == np.asarray(gp.poison, rest.dtype)), "written outside the copies"
        else:
            got = out.cpu().numpy()
        return got.reshape((F, K) + base.shape[1:]), a

    want = [single(lambda o, a, s, k=k: eng.embed_signs_async(tin, tbase, o, th, tw, signs[:, k].copy(), mt, 0, a, s)) for k in range(K)]
    got, a = multi(signs)
    for k in range(K):
        yk, ak = want[k]
        assert np.array_equal(raw(a), raw(ak)), (k, a, ak)
        diff = raw(got[:, k]) != raw(yk)
        assert not diff.any(), (k, int(diff.sum()), np.argwhere(diff)[:4])
    if K > 1:
        assert np.array_equal(raw(got[:, K - 1]), raw(got[:, 0])) and not np.array_equal(raw(got[:, 1 if K > 2 else 0]), raw(dev[1].cpu().numpy()))
    # an all-+1 table: wm_embed's output, K times
    yp, ap = single(lambda o, a_, s: eng.embed_async(tin, tbase, o, mt, 0, fp(a_), ip(s)))
    got, a = multi(np.ones_like(signs))
    assert np.array_equal(raw(a), raw(ap))
    for k in range(K):
        assert np.array_equal(raw(got[:, k]), raw(yp)), k
    eng.close()


@pytest.mark.parametrize("mask", [0, 1])
def test_bits_multi_round_trip(wm, torch_cuda, mask):
    """wm_embed_bits_multi with K = 5 distinct payloads, then wm_detect_bits on each copy returns that copy's payload; copy k
    equals wm_embed_bits with payload k bit for bit"""
    torch = torch_cuda
    R, Cc, th, tw, nbits, K = 270, 480, 32, 32, 48, 5
    mt = wm.MASK_TYPE(mask)
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    tb = BM.layout(ny, nx, nbits, 12345)
    payloads = np.random.default_rng(9).integers(0, 256, (K, nbits // 8)).astype(np.uint8)
    assert len({p.tobytes() for p in payloads}) == K
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc, 777), 3, 40.0, nslots=1)
    xt = torch.from_numpy(synth_frame(R, Cc, frame=1, dtype=np.uint8)).cuda()
    copies, a = eng.makeWatermarkBitsMulti(xt, xt, th, tw, tb, nbits, payloads, mt)
    assert tuple(copies.shape) == (K, R, Cc) and a.shape == (1,) and np.isfinite(a[0])
    for k in range(K):
        back, soft = eng.detectBits(copies[k], th, tw, tb, nbits, mt)
        print(f"mask {mask} copy {k}: min |soft| {float(np.abs(soft).min()):.4f}")
        assert back == payloads[k].tobytes(), (k, soft)
        y1, a1 = eng.makeWatermarkBits(xt, xt, th, tw, tb, nbits, payloads[k].tobytes(), mt)
        assert np.array_equal(y1.cpu().numpy(), copies[k].cpu().numpy()) and raw(np.float32(a1).reshape(1))[0] == raw(a)[0]
    eng.close()


def test_unsolvable_and_zero_energy(wm, torch_cuda):
    """F = 3, K = 3 under ME with a singular frame 1: its status is WM_UNSOLVABLE, its copies equal base bit for bit and a_out[1] is
    untouched, the neighbouring frames are what they are without it; on a zero-W context a = +inf and every copy equals base"""
    torch = torch_cuda
    R, Cc, th, tw, F, K = 64, 256, 32, 32, 3, 3
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 2)
    signs = random_signs(F, K, ny, nx, 21)
    xs = frames_of(R, Cc, F, "f32", first=1)
    good = xs.copy()
    xs[1] = H.singular("ramp", R, Cc)
    base = torch.from_numpy(frames_of(R, Cc, F, "f32", first=9)).cuda()
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    eng.set_fused(False)

    def run(x):
        a, st = np.full(F, 123.0, np.float32), np.full(F, -5, np.int32)
        y = torch.zeros((F * K, R, Cc), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.embed_signs_multi_async(torch.from_numpy(x).cuda(), base, y, th, tw, K, signs, wm.MASK_TYPE.ME, 0, a, st)
        rc = eng.sync(0)
        return rc, y.cpu().numpy().reshape(F, K, R, Cc), a, st

    rc, y, a, st = run(xs)
    assert rc == wm.WM_UNSOLVABLE and list(st) == [0, 1, 0]
    assert a[1] == 123.0 and np.isfinite(a[[0, 2]]).all() and 123.0 not in (a[0], a[2])
    hb = base.cpu().numpy()
    for k in range(K):
        assert np.array_equal(raw(y[1, k]), raw(hb[1])), k
    rc, y2, a2, st2 = run(good)
    assert rc == wm.WM_OK and list(st2) == [0, 0, 0]
    for f in (0, 2):
        assert np.array_equal(raw(y[f]), raw(y2[f])) and raw(a)[f] == raw(a2)[f] and not np.array_equal(y[f, 0], hb[f])
    eng.close()
    ez = wm.Watermark(R, Cc, H.zero_w(R, Cc), 3, 40.0, nslots=1, max_frames=F)
    for mt in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        yz, az = ez.makeWatermarkSignsMulti(torch.from_numpy(good).cuda(), base, th, tw, signs, mt)
        assert tuple(yz.shape) == (F, K, R, Cc) and np.all(np.isposinf(az))
        for k in range(K):
            assert np.array_equal(raw(yz[:, k].cpu().numpy()), raw(hb)), k
    ez.close()


def test_refusals(wm, torch_cuda):
    """WM_ERR_BAD_ARG with `out` unchanged (a poison fill) and nothing queued: a host out, a wrong out->frames, an out that overlaps
    in_gray or base, ncopies 0 and 4097, a sign of 2 at a late index, a bad tile shape, band mode; ME with p = 5 is WM_ERR_BAD_P"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc, th, tw, F, K = 64, 256, 32, 32, 2, 3
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 3)
    signs = random_signs(F, 4097, ny, nx, 31)  # (room for every ncopies below)
    xt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=1)).cuda()
    bt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=9)).cuda()
    x0, b0 = xt.cpu().numpy(), bt.cpu().numpy()
    out = torch.full((F * K, R, Cc), -777.25, dtype=torch.float32, device="cuda")
    hout = np.full((F * K, R, Cc), -777.25, np.float32)
    pin, pbase, pout = wm.plane_of(xt, 1), wm.plane_of(bt, 1), wm.plane_of(out, 1)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    e5 = wm.Watermark(R, Cc, W, 5, 40.0, nslots=1, max_frames=F)
    eb = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    assert L.wm_band_configure(eb._ctx, 8, 40, 128) == wm.WM_OK
    torch.cuda.synchronize()
    sp = lambda s: s.ctypes.data_as(C.c_void_p)

    def call(ctx=eng, mask=0, o=pout, n=K, t=signs, a_=th, b_=tw, i=pin, b=pbase):
        return L.wm_embed_signs_multi(ctx._ctx, mask, C.byref(i), C.byref(b), C.byref(o), a_, b_, n, sp(t), None, None, 0)

    def frames(pl, n):
        q = wm.wm_plane(pl.data, R, Cc, 1, pl.dtype, pl.mem, n, pl.pitch, pl.channel_stride, pl.frame_stride)
        return q

    bad = wm.WM_ERR_BAD_ARG
    assert call(o=host_plane(wm, hout)) == bad
    assert call(o=frames(pout, F * K - 1)) == bad and call(o=frames(pout, F)) == bad
    assert call(o=frames(pin, F), n=1) == bad                # out is in_gray
    assert call(o=frames(pbase, F), n=1) == bad              # out is base
    assert call(n=0) == bad and call(n=4097) == bad and call(n=-1) == bad
    late = signs[:, :K].copy()
    late[F - 1, K - 1, ny - 1, nx - 1] = 2
    assert call(t=late) == bad
    assert "index " + str(late.size - 1) in L.wm_last_error(eng._ctx).decode()
    for (a_, b_) in ((36, 32), (32, 30), (0, 32)):
        assert call(a_=a_, b_=b_) == bad, (a_, b_)
    assert call(ctx=eb) == bad
    assert call(ctx=e5) == wm.WM_ERR_BAD_P
    for e in (eng, e5, eb):
        assert e.sync(0) == wm.WM_OK  # nothing was queued
    assert np.all(out.cpu().numpy() == np.float32(-777.25)) and np.all(hout == np.float32(-777.25))
    assert np.array_equal(xt.cpu().numpy(), x0) and np.array_equal(bt.cpu().numpy(), b0)
    # the neighbours that are allowed
    assert call(t=signs[:, :K].copy()) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert call(ctx=e5, mask=1, t=signs[:, :K].copy()) == wm.WM_OK and e5.sync(0) == wm.WM_OK
    assert not np.any(out.cpu().numpy() == np.float32(-777.25))
    for e in (eng, e5, eb):
        e.close()


def test_queueing_and_hygiene(wm, torch_cuda, G):
    """two un-synced calls on one slot keep their own tables; a multi call over a wm_embed output ends that embed's hand-over; it
    does not change what WM_MEM_SLOT_OUT names; three repeats are the same bits"""
    torch = torch_cuda
    R, Cc, th, tw, F, K = 270, 480, 32, 32, 2, G + 1
    ME = wm.MASK_TYPE.ME
    ny, nx = wm.Watermark.tiles_shape(R, Cc, th, tw)
    W = synth_watermark(R, Cc, W_SEED + 4)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    eng.set_fused(False)
    xt = torch.from_numpy(frames_of(R, Cc, F, "f32", first=3)).cuda()
    t1, t2 = random_signs(F, K, ny, nx, 11), random_signs(F, K, ny, nx, 12)
    want = []
    for t in (t1, t2):
        reps = []
        for _ in range(3 if t is t1 else 1):
            y = torch.empty((F * K, R, Cc), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.embed_signs_multi_async(xt, xt, y, th, tw, K, t.copy(), ME, 0)
            assert eng.sync(0) == wm.WM_OK
            reps.append(y.cpu().numpy())
        assert all(np.array_equal(raw(r), raw(reps[0])) for r in reps)
        want.append(reps[0])
    assert not np.array_equal(want[0], want[1])
    table = t1.copy()
    y1, y2 = torch.empty((F * K, R, Cc), dtype=torch.float32, device="cuda"), torch.empty((F * K, R, Cc), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.embed_signs_multi_async(xt, xt, y1, th, tw, K, table, ME, 0)
    table[...] = t2
    eng.embed_signs_multi_async(xt, xt, y2, th, tw, K, table, ME, 0)
    table[...] = 0
    assert eng.sync(0) == wm.WM_OK
    assert np.array_equal(raw(y1.cpu().numpy()), raw(want[0])) and np.array_equal(raw(y2.cpu().numpy()), raw(want[1]))
    # a multi call (one copy per frame) over the plane a wm_embed just wrote: the detector scores the plane as it is
    y = torch.empty_like(xt)
    corr = np.zeros(F, np.float32)
    torch.cuda.synchronize()
    before = eng.checked_handover_counts()
    eng.embed_async(xt, xt, y, ME, 0)
    eng.embed_signs_multi_async(xt, xt, y, th, tw, 1, t1[:, :1].copy(), ME, 0)
    eng.detect_async(y, ME, 0, fp(corr))
    assert eng.sync(0) == wm.WM_OK
    assert eng.checked_handover_counts()[0] == before[0]  # no trusted frame
    fresh = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=F)
    fresh.set_fused(False)
    ref = np.asarray(fresh.detectWatermark(y.clone(), ME), np.float32)
    assert float(np.abs(corr.astype(np.float64) - ref.astype(np.float64)).max()) <= 1.2e-7, (corr, ref)
    assert np.array_equal(raw(y.cpu().numpy()), raw(want[0].reshape(F, K, R, Cc)[:, 0]))
    # WM_MEM_SLOT_OUT still names the last wm_embed output after a multi call into another buffer
    ye = torch.empty_like(xt)
    c1, c2 = np.zeros(F, np.float32), np.zeros(F, np.float32)
    torch.cuda.synchronize()
    eng.embed_async(xt, xt, ye, ME, 0)
    eng.embed_signs_multi_async(xt, xt, y1, th, tw, K, t2, ME, 0)
    ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
    eng.detect_async(ps, ME, 0, fp(c1))
    assert eng.sync(0) == wm.WM_OK
    eng.detect_async(ye, ME, 0, fp(c2))
    assert eng.sync(0) == wm.WM_OK
    assert float(np.abs(c1.astype(np.float64) - c2.astype(np.float64)).max()) <= 1.2e-7 and np.all(c1 > 0.1), (c1, c2)
    eng.close()
    fresh.close()


CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 64, C = 256, NB = 8;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    const std::vector<int32_t> tb = Watermark::bitsLayout(2, 8, NB, 12345);
    const std::vector<std::vector<uint8_t>> payloads = {{0xA5}, {0x3C}, {0x0F}};
    float a = -1.0f;
    const std::vector<wm::Image> copies = w.makeWatermarkBitsMulti(img, img, a, 32, 32, tb, NB, payloads, ME);
    if (copies.size() != 3 || !(a > 0.0f)) return 3;
    printf("%.9g\n", a);
    for (const wm::Image& y : copies) {
        const std::vector<float> soft = w.detectBits(y, 32, 32, tb, NB, ME);
        if (soft.size() != (size_t)NB) return 4;
        for (float v : soft) printf("%d\n", v > 0.0f ? 1 : 0);
    }
    std::vector<std::vector<int8_t>> signs(2, std::vector<int8_t>(16, 1));
    float a1 = 0.0f;
    if (w.makeWatermarkSignsMulti(img, img, a1, 32, 32, signs, ME).size() != 2 || a1 != a) return 5;
    signs[1][7] = 3;
    try { w.makeWatermarkSignsMulti(img, img, a1, 32, 32, signs, ME); return 6; } catch (const std::runtime_error&) {}
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    """makeWatermarkBitsMulti with K = 3 on 64 x 256 from C++: the signs detectBits prints for every copy are its payload's bits"""
    R, Cc, nbits = 64, 256, 8
    src = tmp_path / "multi.cpp"
    src.write_text(CPP)
    exe = tmp_path / "multi"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    xf = tmp_path / "x.f32"
    synth_frame(R, Cc, frame=6).tofile(xf)
    wf = tmp_path / "w.dat"
    synth_watermark(R, Cc, W_SEED + 7).tofile(wf)
    out = subprocess.run([str(exe), str(xf), str(wf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = out.stdout.split()
    assert len(vals) == 1 + 3 * nbits and float(vals[0]) > 0
    got = np.array([int(v) for v in vals[1:]]).reshape(3, nbits)
    want = np.array([[(b >> i) & 1 for i in range(nbits)] for b in (0xA5, 0x3C, 0x0F)])
    assert np.array_equal(got, want), (got, want)
