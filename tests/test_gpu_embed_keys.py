"""wm_embed_keys: one image marked with every key of a bank in one call (k_stats_keys, k_embed_keys_fold, k_embed_keys).  Bit
equality of every copy and strength with wm_embed on a context whose W is the key (fused kernels off), parity with the CPU
oracle, the round trip through wm_detect_keys, unsolvable frames, every input kind and refusal, hand-over safety, enqueue
semantics, determinism and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ME, NVF = 0, 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def seeds_for(K, base=2000):
    return [base + 31 * k for k in range(K)]


def frames_of(R, Cc, F, dtype, first=0):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def bits(t):
    """a tensor's bytes as an integer tensor (bit-for-bit comparisons on the device)"""
    import torch
    return t.contiguous().view(torch.uint8)


def make_base(torch, xs, kind):
    """xs: [F, R, C] device tensor.  kind: 'grey' (another grey plane), 'rgb' ([F, 3, R, C]) or 'in' (the input itself)"""
    if kind == "in":
        return xs
    if kind == "grey":
        return (xs.flip(-1) if xs.dtype == torch.uint8 else xs.flip(-1) * 0.5 + 20.0).contiguous()
    ch = [xs, xs.flip(-2), xs.flip(-1)]
    return torch.stack(ch, 1).contiguous()


def reference_embed(wm, torch, R, Cc, p, seed, xs, base, mask, F):
    """wm_embed with W = the generated key, on the batched sweeps: (y [F, ...], a float32 [F], status)"""
    ek = wm.Watermark.generated(R, Cc, seed, p, 40.0, max_frames=F)
    ek.set_fused(False)
    y = torch.empty_like(base)
    torch.cuda.synchronize()
    a = np.full(F, np.nan, np.float32)
    st = np.zeros(F, np.int32)
    ek.embed_async(xs, base, y, wm.MASK_TYPE(mask), wm.WM_SLOT_SYNC, a.ctypes.data_as(C.POINTER(C.c_float)),
                   st.ctypes.data_as(C.POINTER(C.c_int)))
    ek.close()
    return y, a, st


SHAPES = [(1, 1), (5, 7), (64, 256), (270, 480), (271, 483), (1078, 1918), (2160, 3840)]
MASKS = [(ME, 3), (NVF, 3), (NVF, 5), (NVF, 9)]
CASES = []
for i, shape in enumerate(SHAPES):
    for j, (mk, p) in enumerate(MASKS):
        for d, dtype in enumerate(("f32", "u8")):
            base = ("grey", "rgb", "in")[(i + j + d) % 3]
            F = (1, 5)[(i + j + 2 * d) % 2] if shape != (2160, 3840) else (1, 5)[(j + d) % 2]
            K = (1, 3, 8)[(i + 2 * j + d) % 3]
            CASES.append((shape, mk, p, dtype, base, F, K))


@pytest.mark.parametrize("shape,mask,p,dtype,base_kind,F,K", CASES)
def test_bit_equal_to_wm_embed(wm, torch_cuda, shape, mask, p, dtype, base_kind, F, K):
    torch = torch_cuda
    R, Cc = shape
    sd = seeds_for(K)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype, first=1)).cuda()
    base = make_base(torch, xs, base_kind)
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0, max_frames=F)
    copies, a = eng.makeWatermarkKeys(xs, base, keys, wm.MASK_TYPE(mask))
    assert tuple(copies.shape) == (F, K) + tuple(base.shape[1:]) and a.shape == (F, K) and a.dtype == np.float32
    for k in range(K):
        y, ar, st = reference_embed(wm, torch, R, Cc, p, sd[k], xs, base, mask, F)
        assert torch.equal(bits(copies[:, k]), bits(y)), (k, shape, mask, p, dtype, base_kind)
        ok = st == 0
        assert np.array_equal(a[ok, k].view(np.uint32), ar[ok].view(np.uint32)), (k, a[:, k], ar)
    eng.close()
    keys.close()


@pytest.mark.parametrize("shape", [(1078, 1918), (2160, 3840)])
@pytest.mark.parametrize("base_kind", ["grey", "rgb"])
def test_full_key_groups_base_stream_quad(wm, torch_cuda, shape, base_kind):
    """the f32 ME instance with a base stream (no BX) with two full key groups, four frames per block, at 1080p (aligned + generic
    strips) and 4K (shifted strips): every copy bit-equal to wm_embed, and three repeated calls bit-identical to the first"""
    torch = torch_cuda
    R, Cc = shape
    F, K = 5, 8
    sd = seeds_for(K, base=4100)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32", first=2)).cuda()
    base = make_base(torch, xs, base_kind)
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    copies, a = eng.makeWatermarkKeys(xs, base, keys, wm.MASK_TYPE.ME)
    assert not np.any(np.isnan(a))
    for k in range(K):
        y, ar, st = reference_embed(wm, torch, R, Cc, 3, sd[k], xs, base, ME, F)
        assert np.all(st == 0)
        assert torch.equal(bits(copies[:, k]), bits(y)), (k, shape, base_kind)
        assert np.array_equal(a[:, k].view(np.uint32), ar.view(np.uint32)), (k, a[:, k], ar)
        del y
    again = torch.empty_like(copies)
    for _ in range(3):
        _, a2 = eng.makeWatermarkKeys(xs, base, keys, wm.MASK_TYPE.ME, out=again)
        assert torch.equal(bits(again), bits(copies)) and np.array_equal(a2.view(np.uint32), a.view(np.uint32))
    eng.close()
    keys.close()


PARITY = [((64, 256), ME, 3, "f32", "grey"), ((270, 480), ME, 3, "u8", "in"), ((271, 483), NVF, 3, "f32", "rgb"),
          ((270, 480), NVF, 5, "u8", "in"), ((271, 483), NVF, 9, "f32", "in"), ((1078, 1918), ME, 3, "f32", "in")]


@pytest.mark.parametrize("shape,mask,p,dtype,base_kind", PARITY)
def test_oracle_parity(wm, torch_cuda, shape, mask, p, dtype, base_kind):
    torch = torch_cuda
    R, Cc = shape
    K = 3
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K, base=90))
    x = frames_of(R, Cc, 1, dtype, first=4)[0]
    xt = torch.from_numpy(x).cuda()
    bt = make_base(torch, xt[None], base_kind)[0]
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0)
    copies, a = eng.makeWatermarkKeys(xt, bt, keys, wm.MASK_TYPE(mask))
    assert tuple(copies.shape) == (K,) + tuple(bt.shape) and a.shape == (K,)
    b = bt.cpu().numpy()
    for k in range(K):
        W = keys.plane(k)
        if dtype == "u8":
            assert base_kind == "in"
            st, yo, ao = O.embed_u8(x, W, p=p, mask=mask)
            diff = np.abs(copies[k].cpu().numpy().astype(np.int32) - yo.astype(np.int32))
            assert int(diff.max()) <= 1, k
        else:
            st, yo, ao = O.embed(x, b, W, p=p, mask=mask)
            assert float(np.abs(copies[k].cpu().numpy() - yo).max()) <= 1e-3, k
        assert st == 0 and abs(float(a[k]) - ao) <= 1e-4 * abs(ao), (k, a[k], ao)
    eng.close()
    keys.close()


def test_round_trip_4k(wm, torch_cuda):
    """8 copies of a 4K frame: wm_detect_keys on copy k scores highest at key k, with wm_detect's score (W = key k) bit for bit"""
    torch = torch_cuda
    R, Cc, K = 2160, 3840, 8
    sd = seeds_for(K, base=7000)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    xt = torch.from_numpy(synth_frame(R, Cc, frame=3)).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=K)
    copies, a = eng.makeWatermarkKeys(xt, xt, keys, wm.MASK_TYPE.ME)
    s = np.asarray(eng.detectKeys(copies, keys, wm.MASK_TYPE.ME)).reshape(K, K)
    for k in range(K):
        assert int(np.argmax(s[k])) == k, (k, s[k])
        assert s[k, k] > 4 * float(np.abs(np.delete(s[k], k)).max()), (k, s[k])
        # wm_detect with W = key k over the same batch of copies (the same sweep geometry): copy k's score bit for bit
        ek = wm.Watermark.generated(R, Cc, sd[k], 3, 40.0, max_frames=K)
        ek.set_fused(False)
        c = np.asarray(ek.detectWatermark(copies, wm.MASK_TYPE.ME), np.float32)[k]
        assert c.view(np.uint32) == s[k, k].view(np.uint32), (k, c, s[k, k])
        ek.close()
    eng.close()
    keys.close()


def test_unsolvable_frame_in_batch(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, F, K = 270, 480, 5, 3
    sd = seeds_for(K)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    xs = frames_of(R, Cc, F, "f32")
    xs[2] = 100.0  # constant frame: singular prediction system
    xt = torch.from_numpy(xs).cuda()
    base = make_base(torch, xt, "grey")
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    out = torch.full((F * K, R, Cc), -1.0, device="cuda")
    a = np.full(F * K, 7.0, np.float32)
    st = np.full(F, -5, np.int32)
    torch.cuda.synchronize()
    eng.embed_keys_async(xt, base, out, keys, wm.MASK_TYPE.ME, 0, a, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    a = a.reshape(F, K)
    out = out.view(F, K, R, Cc)
    assert list(st) == [0, 0, 1, 0, 0]
    assert np.all(a[2] == 7.0)
    for k in range(K):
        assert torch.equal(bits(out[2, k]), bits(base[2]))
        y, ar, str_ = reference_embed(wm, torch, R, Cc, 3, sd[k], xt, base, ME, F)
        assert list(str_) == [0, 0, 1, 0, 0]
        for f in (0, 1, 3, 4):
            assert torch.equal(bits(out[f, k]), bits(y[f])) and a[f, k].view(np.uint32) == ar[f].view(np.uint32), (f, k)
    # the Python surface: NaN strengths and the base for the unsolvable frame
    copies, a2 = eng.makeWatermarkKeys(xt, base, keys, wm.MASK_TYPE.ME)
    assert np.all(np.isnan(a2[2])) and not np.any(np.isnan(a2[[0, 1, 3, 4]]))
    assert torch.equal(bits(copies[2, 1]), bits(base[2]))
    eng.close()
    keys.close()


def test_inputs_host_and_slot_out(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc, F, K = 270, 483, 2, 3
    sd = seeds_for(K, base=400)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    xs = frames_of(R, Cc, F, "f32", first=5)
    xt = torch.from_numpy(xs).cuda()
    bt = make_base(torch, xt, "grey")
    eng = wm.Watermark(R, Cc, keys.plane(0), 3, 40.0, max_frames=F)  # (its own W marks the WM_MEM_SLOT_OUT input below)
    torch.cuda.synchronize()
    ref, aref = eng.makeWatermarkKeys(xt, bt, keys, wm.MASK_TYPE.ME)
    # host-staged in_gray and base: pageable numpy arrays, then pinned memory (wm_host_alloc)
    bh = np.ascontiguousarray(bt.cpu().numpy())
    nbytes = xs.nbytes
    pin_x, pin_b = L.wm_host_alloc(nbytes), L.wm_host_alloc(nbytes)
    try:
        C.memmove(pin_x, xs.ctypes.data, nbytes)
        C.memmove(pin_b, bh.ctypes.data, nbytes)
        for px, pb in ((xs.ctypes.data, bh.ctypes.data), (pin_x, pin_b)):
            pin = wm.wm_plane(px, R, Cc, 1, wm.WM_F32, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
            pbase = wm.wm_plane(pb, R, Cc, 1, wm.WM_F32, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
            out = torch.empty((F * K, R, Cc), device="cuda")
            a = np.zeros(F * K, np.float32)
            torch.cuda.synchronize()
            eng.embed_keys_async(pin, pbase, out, keys, wm.MASK_TYPE.ME, wm.WM_SLOT_SYNC, a)
            assert torch.equal(bits(out.view(F, K, R, Cc)), bits(ref)) and np.array_equal(a.reshape(F, K), aref)
        # host in_gray that is also the base (base == in_gray)
        pin = wm.wm_plane(pin_x, R, Cc, 1, wm.WM_F32, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)
        out = torch.empty((F * K, R, Cc), device="cuda")
        eng.embed_keys_async(pin, pin, out, keys, wm.MASK_TYPE.ME, wm.WM_SLOT_SYNC)
        ref_in, _ = eng.makeWatermarkKeys(xt, xt, keys, wm.MASK_TYPE.ME)
        assert torch.equal(bits(out.view(F, K, R, Cc)), bits(ref_in))
    finally:
        L.wm_host_free(pin_x)
        L.wm_host_free(pin_b)
    # WM_MEM_SLOT_OUT as in_gray: the slot's last wm_embed output
    yb = torch.empty_like(xt)
    eng.embed_async(xt, xt, yb, wm.MASK_TYPE.ME, 0)
    ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
    out = torch.empty((F * K, R, Cc), device="cuda")
    a = np.zeros(F * K, np.float32)
    eng.embed_keys_async(ps, wm.plane_of(bt), out, keys, wm.MASK_TYPE.ME, 0, a)
    eng.sync(0)
    ref_s, aref_s = eng.makeWatermarkKeys(yb, bt, keys, wm.MASK_TYPE.ME)
    assert not np.any(np.isnan(aref_s))
    assert torch.equal(bits(out.view(F, K, R, Cc)), bits(ref_s)) and np.array_equal(a.reshape(F, K), aref_s)
    eng.close()
    keys.close()


def test_refusals_and_capacity(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc, K = 64, 256, 2
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K))
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=2)
    x = torch.from_numpy(synth_frame(R, Cc)).cuda()
    big = torch.zeros((4, R, Cc), device="cuda")
    torch.cuda.synchronize()
    pin = wm.plane_of(x)
    pout = wm.plane_of(big[:K])
    a = (C.c_float * K)()
    call = lambda i, b, ks, o, mask=ME: L.wm_embed_keys(eng._ctx, mask, C.byref(i), C.byref(b), ks, C.byref(o), a, None, wm.WM_SLOT_SYNC)
    assert call(pin, pin, keys.handle, pout) == wm.WM_OK
    # host out
    host = np.zeros((K, R, Cc), np.float32)
    ph = wm.wm_plane(host.ctypes.data, R, Cc, 1, wm.WM_F32, wm.WM_MEM_HOST, K, Cc, 0, R * Cc)
    assert call(pin, pin, keys.handle, ph) == wm.WM_ERR_BAD_ARG
    # out overlapping in_gray, or base
    pin_big = wm.plane_of(big[1])
    assert call(pin_big, pin_big, keys.handle, pout) == wm.WM_ERR_BAD_ARG
    assert call(pin, wm.plane_of(big[0]), keys.handle, pout) == wm.WM_ERR_BAD_ARG
    assert call(pin, pin, keys.handle, wm.plane_of(big[2:4])) == wm.WM_OK
    # wrong out->frames
    assert call(pin, pin, keys.handle, wm.plane_of(big[:3])) == wm.WM_ERR_BAD_ARG
    assert call(pin, pin, keys.handle, wm.plane_of(big[0])) == wm.WM_ERR_BAD_ARG
    # a bank of another shape; a null bank; a bad mask; NVF is fine, and with p = 5 ME is WM_ERR_BAD_P (wm_embed's code)
    other = wm.KeySet(R + 1, Cc, K)
    assert call(pin, pin, other.handle, pout) == wm.WM_ERR_BAD_ARG
    assert call(pin, pin, None, pout) == wm.WM_ERR_BAD_ARG
    assert call(pin, pin, keys.handle, pout, mask=2) == wm.WM_ERR_BAD_ARG
    assert call(pin, pin, keys.handle, pout, mask=NVF) == wm.WM_OK
    e5 = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 5, 40.0)
    assert L.wm_embed_keys(e5._ctx, ME, C.byref(pin), C.byref(pin), keys.handle, C.byref(pout), a, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_P
    # the Python surface: a wrong `out` shape
    with pytest.raises(RuntimeError, match="out must be"):
        eng.makeWatermarkKeys(x, x, keys, wm.MASK_TYPE.ME, out=big[:3])
    # result capacity: frames x keys count against 4096 un-synced results per slot
    r2, c2 = 16, 16
    bank = wm.KeySet(r2, c2, 4096)
    e2 = wm.Watermark(r2, c2, np.zeros((r2, c2), np.float32), 3, 40.0)
    x2 = torch.from_numpy(synth_frame(r2, c2)).cuda()
    o2 = torch.empty((4096, r2, c2), device="cuda")
    c_det = (C.c_float * 1)()
    torch.cuda.synchronize()
    e2.detect_async(x2, wm.MASK_TYPE.ME, 0, c_det)
    with pytest.raises(RuntimeError, match="un-synced"):
        e2.embed_keys_async(x2, x2, o2, bank, wm.MASK_TYPE.ME, 0)
    e2.sync(0)
    e2.embed_keys_async(x2, x2, o2, bank, wm.MASK_TYPE.ME, 0)  # (4096 fit on an empty slot)
    e2.sync(0)
    for obj in (bank, e2, e5, other, eng, keys):
        obj.close()


def test_handover_safety(wm, torch_cuda):
    """an embed under wm_set_handover leaves the Gram sums of its output B; wm_embed_keys then overwrites B: the detector on
    WM_MEM_SLOT_OUT must read B as it now is (the hand-over ended), not the sums of the old plane"""
    torch = torch_cuda
    R, Cc, F = 270, 480, 2
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(2, base=55))
    W = synth_frame(R, Cc, frame=9) - 128.0
    eng = wm.Watermark(R, Cc, W, 3, 40.0, max_frames=F)
    eng.set_handover(True)
    xb = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    B = torch.empty_like(xb)
    torch.cuda.synchronize()
    eng.embed_async(xb, xb, B, wm.MASK_TYPE.ME, 0)
    eng.sync(0)
    x1 = torch.from_numpy(synth_frame(R, Cc, frame=11)).cuda()
    torch.cuda.synchronize()
    eng.embed_keys_async(x1, x1, B, keys, wm.MASK_TYPE.ME, 0)
    ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
    cs = (C.c_float * F)()
    eng.detect_async(ps, wm.MASK_TYPE.ME, 0, cs)
    eng.sync(0)
    plain = wm.Watermark(R, Cc, W, 3, 40.0, max_frames=F)
    plain.set_fused(False)
    plain.set_checked_handover(False)
    ref = np.asarray(plain.detectWatermark(B, wm.MASK_TYPE.ME), np.float32)
    assert np.array_equal(np.asarray(list(cs), np.float32), ref), (list(cs), ref)
    for obj in (plain, eng, keys):
        obj.close()


def test_enqueue_semantics(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, K = 270, 480, 3
    sd = seeds_for(K, base=600)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    W0 = keys.plane(1)
    eng = wm.Watermark(R, Cc, W0, 3, 40.0, nslots=2)
    x = torch.from_numpy(synth_frame(R, Cc, frame=2)).cuda()
    x2 = torch.from_numpy(synth_frame(R, Cc, frame=8)).cuda()
    y0 = torch.empty_like(x)
    o0 = torch.empty((K, R, Cc), device="cuda")
    o1 = torch.empty((K, R, Cc), device="cuda")
    o2 = torch.empty((K, R, Cc), device="cuda")
    a0, c0 = (C.c_float * 1)(), (C.c_float * 1)()
    ak0, ak1, ak2 = (np.zeros(K, np.float32) for _ in range(3))
    ck = np.zeros(K, np.float32)
    torch.cuda.synchronize()
    # slot 0: embed, embed_keys, detect of the embed's output, detect_keys of copy 1 -- one wm_sync
    eng.embed_async(x, x, y0, wm.MASK_TYPE.ME, 0, a0)
    eng.embed_keys_async(x, x, o0, keys, wm.MASK_TYPE.ME, 0, ak0)
    eng.detect_async(y0, wm.MASK_TYPE.ME, 0, c0)
    eng.detect_keys_async(o0[1], keys, wm.MASK_TYPE.ME, 0, ck)
    # slot 1 at the same time: two embed_keys calls
    eng.embed_keys_async(x2, x2, o1, keys, wm.MASK_TYPE.NVF, 1, ak1)
    eng.embed_keys_async(x, x, o2, keys, wm.MASK_TYPE.ME, 1, ak2)
    eng.sync(1)
    eng.sync(0)
    r0, ra0 = eng.makeWatermarkKeys(x, x, keys, wm.MASK_TYPE.ME)
    r1, ra1 = eng.makeWatermarkKeys(x2, x2, keys, wm.MASK_TYPE.NVF)
    assert torch.equal(bits(o0), bits(r0)) and np.array_equal(ak0, ra0)
    assert torch.equal(bits(o2), bits(r0)) and np.array_equal(ak2, ra0)
    assert torch.equal(bits(o1), bits(r1)) and np.array_equal(ak1, ra1)
    # the engine's own W is key 1: its embed equals copy 1
    assert torch.equal(bits(y0), bits(o0[1])) and np.float32(a0[0]) == ak0[1]
    assert np.array_equal(ck, eng.detectKeys(r0[1], keys, wm.MASK_TYPE.ME)) and int(np.argmax(ck)) == 1
    assert abs(c0[0] - float(ck[1])) <= 2e-7
    eng.close()
    keys.close()


def test_deterministic(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, F, K = 1078, 1918, 4, 5
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K))
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    for mk in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        y1, a1 = eng.makeWatermarkKeys(xs, xs, keys, mk)
        y2, a2 = eng.makeWatermarkKeys(xs, xs, keys, mk)
        assert torch.equal(bits(y1), bits(y2)) and np.array_equal(a1.view(np.uint32), a2.view(np.uint32))
    eng.close()
    keys.close()


CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 270, C = 480, K = 5;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    WatermarkKeys keys(R, C, K);
    for (int k = 0; k < K; ++k) keys.generate(k, 2000 + 31 * k);
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    FILE* o = fopen(argv[3], "wb");
    for (int m = 0; m < 2; ++m) {
        std::vector<float> a;
        const std::vector<wm::Image> copies = w.makeWatermarkKeys(img, img, keys, a, m == 0 ? ME : NVF);
        if ((int)copies.size() != K || (int)a.size() != K) return 4;
        for (float v : a) printf("%.9g\n", v);
        std::vector<float> y((size_t)R * C);
        for (const wm::Image& c : copies) { c.host(y.data()); fwrite(y.data(), 4, y.size(), o); }
    }
    fclose(o);
    // an unsolvable image: every copy is the base itself, the strengths stay untouched
    const wm::Image flat = wm::Image::fromHost(std::vector<float>((size_t)R * C, 100.0f).data(), R, C);
    std::vector<float> a2(1, 7.0f);
    const std::vector<wm::Image> c2 = w.makeWatermarkKeys(flat, flat, keys, a2, ME);
    if ((int)c2.size() != K || !c2[K - 1].same_buffer(flat) || a2.size() != 1 || a2[0] != 7.0f) return 5;
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc, K = 270, 480, 5
    src = tmp_path / "ekeys.cpp"
    src.write_text(CPP)
    exe = tmp_path / "ekeys"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    x = synth_frame(R, Cc, frame=6)
    xf = tmp_path / "x.f32"
    x.tofile(xf)
    wf = tmp_path / "w.dat"
    np.zeros((R, Cc), np.float32).tofile(wf)
    yf = tmp_path / "y.f32"
    out = subprocess.run([str(exe), str(xf), str(wf), str(yf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    got_a = np.array([float(v) for v in out.stdout.split()], np.float32).reshape(2, K)
    got_y = np.fromfile(yf, np.float32).reshape(2, K, R, Cc)
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K))
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0)
    xt = torch.from_numpy(x).cuda()
    for m, mk in enumerate((wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF)):
        y, a = eng.makeWatermarkKeys(xt, xt, keys, mk)
        assert np.array_equal(got_a[m], a), (m, got_a[m], a)
        assert np.array_equal(got_y[m].view(np.uint32), y.cpu().numpy().view(np.uint32)), m
    eng.close()
    keys.close()
