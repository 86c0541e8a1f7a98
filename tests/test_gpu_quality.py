"""wm_quality on the device (wm.h): PSNR and SSIM of a marked copy against its base.

Every expectation comes from tests/quality_model.py, the numpy float64 restatement of wm.h's definitions, never from the library.
Tolerances, each derived (N = a tile's pixel count, n = its window count):
  sse       u8 against u8: an integer below 2^53 -- equal.  Otherwise relative error <= N * 2^-52: twice the worst-case bound of a
            sequential float64 summation of N terms, whatever the order.
  npix, nwin, max|d|: bit for bit (max|d| is one IEEE subtraction and a max).
  ssim_sum  |delta| <= n * 1e-10: the model's two evaluation orders differ by <= 3e-13 per window on frames like these and by
            65025 * 2^-52 * O(10) / C2 ~ 2e-12 on a bright flat patch (tests/test_quality_model.py); 1e-10 leaves a 50x margin.
  q_out     mse within relative 2^-23 of (float) of the model's; ssim within 1.2e-7 (two f32 ulps in [0.5, 1)); max|d| bit-equal.
Shapes: (11, 11) one window; (12, 13); (10, 40) and (40, 10) no window; (43, 67) ragged in both axes; (70, 130) in 32 x 32 tiles (ny = 2,
nx = 4, remainder tiles, windows across tile and block seams); (64, 300) more than four 64-column strips; (270, 480), F = 3, 64 x 128."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layouts as LY
import oracle_lib as O
import quality_model as Q
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "watermarking-gpu_amd", "wm_app")
# shape -> (frames, channels, tile)
CASES = {(11, 11): (1, 1, (0, 0)), (12, 13): (1, 3, (0, 0)), (10, 40): (1, 1, (0, 0)), (40, 10): (1, 1, (0, 0)), (43, 67): (1, 3, (32, 32)),
         (70, 130): (1, 1, (32, 32)), (64, 300): (2, 1, (0, 0)), (270, 480): (3, 1, (64, 128))}
MIXES = [("f32", "f32"), ("f32", "u8"), ("u8", "f32"), ("u8", "u8")]
NP_OF = {"f32": np.float32, "u8": np.uint8}


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_ENGINES = {}


def engine(wm, shape, F=1):
    key = (shape, F)
    if key not in _ENGINES:
        _ENGINES[key] = wm.Watermark(shape[0], shape[1], synth_watermark(*shape), 3, 40.0, nslots=2, max_frames=F)
    return _ENGINES[key]


_DATA = {}


def content(shape, F=3):
    """(base, marked): [F, 3, R, C] float32 each -- synth frames and their oracle-embedded copies (40 dB, ME); where the oracle cannot
    solve a plane this small, the frame plus noise of the same size.  Read-only, computed once per shape"""
    if shape not in _DATA:
        R, Cc = shape
        W = synth_watermark(R, Cc)
        rng = np.random.default_rng(1000 * R + Cc)
        x = np.stack([np.stack([synth_frame(R, Cc, frame=3 * f + c) for c in range(3)]) for f in range(F)])
        y = np.empty_like(x)
        for f in range(F):
            for c in range(3):
                st, yo, a = O.embed(x[f, c], x[f, c], W) if min(shape) >= 32 else (1, None, None)
                assert st == 0 or min(shape) < 43
                y[f, c] = yo if st == 0 else np.clip(x[f, c] + 2.55 * rng.standard_normal(shape), 0, 255)
        assert (x != y).any()
        x.setflags(write=False); y.setflags(write=False)
        _DATA[shape] = (x, y)
    return _DATA[shape]


def as_kind(a, kind):
    return np.ascontiguousarray(a.astype(NP_OF[kind]))  # (u8: truncation, what a u8 plane or wm_pack_rgb8 holds)


_MODEL = {}


def model(ref, test, tile, key=None):
    """[F, ch, ny, nx, 5] of arrays [F, ch, R, C]"""
    if key is not None and key in _MODEL:
        return _MODEL[key]
    m = np.stack([np.stack([Q.tile_sums(ref[f, c], test[f, c], *tile) for c in range(ref.shape[1])]) for f in range(ref.shape[0])])
    if key is not None:
        _MODEL[key] = m
    return m


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_sums(got, want, exact_sse, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(-1, 5), want.reshape(-1, 5)
    for i in range(w.shape[0]):
        sse, npix, ssum, nwin, mx = w[i]
        print(f"{what} tile {i}: sse {g[i, 0]!r} / {sse!r}  ssim_sum {g[i, 2]!r} / {ssum!r}  nwin {nwin}  max {g[i, 4]!r}")
        if exact_sse:
            assert g[i, 0] == sse, (what, i)
        else:
            assert abs(g[i, 0] - sse) <= npix * 2.0 ** -52 * sse, (what, i, g[i, 0], sse)
        assert bits(g[i, [1, 3, 4]]).tolist() == bits(w[i, [1, 3, 4]]).tolist(), (what, i, g[i], w[i])
        assert abs(g[i, 2] - ssum) <= nwin * 1e-10, (what, i, g[i, 2], ssum)


def check_q(q, want, what):
    """q [F, ch, 3] float32 against the model's tile sums [F, ch, ny, nx, 5]"""
    for f in range(want.shape[0]):
        for c in range(want.shape[1]):
            mse, ssim, mx = Q.plane_values(want[f, c])
            print(f"{what} f={f} c={c}: mse {q[f, c, 0]!r} / {mse!r}  ssim {q[f, c, 1]!r} / {ssim!r}  max {q[f, c, 2]!r} / {mx!r}")
            assert abs(float(q[f, c, 0]) - float(np.float32(mse))) <= 2.0 ** -23 * float(np.float32(mse)), (what, f, c)
            if np.isnan(ssim):
                assert np.isnan(q[f, c, 1]), (what, f, c)
            else:
                assert abs(float(q[f, c, 1]) - ssim) <= 1.2e-7, (what, f, c)
            assert bits(q[f, c, 2:3])[0] == bits(np.float32([mx]))[0], (what, f, c)


def run(wm, tc, eng, ref, test, tile, channels, slot=None, want_q=True, want_sums=True):
    """one wm_quality call on planes (tensors, arrays or wm_planes): (q [F, ch, 3] float32, sums [F, ch, ny, nx, 5] float64)"""
    slot = wm.WM_SLOT_SYNC if slot is None else slot
    pr = ref if isinstance(ref, wm.wm_plane) else wm.plane_u8f32(ref, channels)
    F, R, Cc = pr.frames, pr.rows, pr.cols
    ny, nx = Q.tiles_shape(R, Cc, *tile)
    q = np.full((F, channels, 3), -7.0, np.float32) if want_q else None
    sums = tc.full((F, channels, ny, nx, 5), -7.0, dtype=tc.float64, device="cuda") if want_sums else None
    tc.cuda.synchronize()
    eng.quality_async(ref, test, slot, q, tile[0], tile[1], sums, channels)
    if slot != wm.WM_SLOT_SYNC:
        assert eng.sync(slot) == wm.WM_OK
    return q, (sums.cpu().numpy() if want_sums else None)


def squeeze(a, F, channels):
    a = a[:F, :channels] if channels == 3 else a[:F, 0]
    return a if F > 1 else a[0]


# ---- shapes x sample types --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", MIXES, ids=lambda m: m[0] + "-" + m[1])
@pytest.mark.parametrize("shape", list(CASES))
def test_shapes_and_sample_types(wm, tc, shape, mix):
    F, ch, tile = CASES[shape]
    eng = engine(wm, shape, F)
    x, y = content(shape)
    ref, test = as_kind(x[:F, :ch], mix[0]), as_kind(y[:F, :ch], mix[1])
    want = model(ref, test, tile, (shape, mix, tile))
    rd, td = tc.from_numpy(squeeze(ref, F, ch).copy()).cuda(), tc.from_numpy(squeeze(test, F, ch).copy()).cuda()
    q, sums = run(wm, tc, eng, rd, td, tile, ch)
    what = f"{shape} {mix} tile={tile}"
    check_sums(sums, want, mix == ("u8", "u8"), what)
    check_q(q, want, what)
    if min(shape) < 11:
        assert np.isnan(q[..., 1]).all() and (sums[..., 3] == 0).all() and (q[..., 0] > 0).all()
    # one tile per plane and q_out alone, sums alone: the same values
    q1, _ = run(wm, tc, eng, rd, td, (0, 0), ch, slot=1, want_sums=False)
    check_q(q1, model(ref, test, (0, 0), (shape, mix, (0, 0))), what + " q_out alone")
    _, s2 = run(wm, tc, eng, rd, td, tile, ch, slot=1, want_q=False)
    assert (bits(s2) == bits(sums)).all()
    # the Python surface: the same figures, psnr from wm_psnr_from_mse
    mse, psnr, ssim, mx, st = eng.quality(rd, td, tile=tile if tile != (0, 0) else None, sums=True, channels=ch)
    assert mse.shape == (F, ch) and (bits(st) == bits(sums)).all()
    assert (mse == q[..., 0]).all() and (mx == q[..., 2]).all() and (bits(ssim.astype(np.float32)) == bits(q[..., 1])).all()
    assert psnr.reshape(-1).tolist() == pytest.approx([Q.psnr_from_mse(float(v)) for v in mse.reshape(-1)], abs=1e-12)


# ---- content ----------------------------------------------------------------------------------------------------------------------------
def test_marked_copy_has_the_requested_psnr(wm, tc):
    """the oracle's copy at 40 dB: the device's figure for the f32 copy is 40 dB up to the clamp, its u8 truncation lies below"""
    shape = (270, 480)
    eng = engine(wm, shape, 3)
    x, y = content(shape)
    mse, psnr, ssim, mx = eng.quality(tc.from_numpy(x[0, 0].copy()).cuda(), tc.from_numpy(y[0, 0].copy()).cuda())
    assert abs(psnr[0, 0] - 40.0) < 0.1 and 0.9 < ssim[0, 0] < 1.0
    mse8, psnr8, ssim8, mx8 = eng.quality(tc.from_numpy(x[0, 0].copy()).cuda(), tc.from_numpy(as_kind(y[0, 0], "u8")).cuda())
    assert psnr8[0, 0] < psnr[0, 0] and mx8[0, 0] >= 1.0


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_identical_planes(wm, tc, kind):
    shape = (70, 130)
    eng = engine(wm, shape)
    a = tc.from_numpy(as_kind(content(shape)[0][0, 0], kind)).cuda()
    for test in (a, a.clone()):  # the same plane, and a copy of it
        q, sums = run(wm, tc, eng, a, test, (32, 32), 1)
        assert q[0, 0].tolist() == [0.0, 1.0, 0.0]
        assert (sums[..., 0] == 0).all() and (sums[..., 4] == 0).all() and (sums[..., 2] == sums[..., 3]).all() and sums[..., 3].sum() == 60 * 120
    assert np.isinf(eng.quality(a, a)[1][0, 0])


@pytest.mark.parametrize("c1,c2", [(255, 0), (0, 255), (100, 101)])
def test_flat_against_flat(wm, tc, c1, c2):
    shape = (43, 67)
    eng = engine(wm, shape)
    a, b = np.full(shape, c1, np.uint8), np.full(shape, c2, np.float32)
    q, sums = run(wm, tc, eng, tc.from_numpy(a).cuda(), tc.from_numpy(b).cuda(), (0, 0), 1)
    want = (2.0 * c1 * c2 + Q.C1) / (c1 * c1 + c2 * c2 + Q.C1)
    n = 33 * 57
    assert sums[0, 0, 0, 0, [0, 1, 3, 4]].tolist() == [43 * 67 * (c1 - c2) ** 2, 43 * 67, n, abs(c1 - c2)]
    assert abs(sums[0, 0, 0, 0, 2] - n * want) <= n * 1e-10
    check_q(q, model(a[None, None], b[None, None], (0, 0)), f"flat {c1} {c2}")


def test_one_changed_pixel(wm, tc):
    """max|d| is that pixel's; exactly the windows that contain it -- 121 here, in the four tiles around the seam -- differ from 1"""
    shape = (70, 130)
    eng = engine(wm, shape)
    x = content(shape)[0][0, 0].copy()
    x[33, 62] = 100.0
    y = x.copy()
    y[33, 62] = 109.0
    want = model(x[None, None], y[None, None], (32, 32))
    q, sums = run(wm, tc, eng, tc.from_numpy(x.copy()).cuda(), tc.from_numpy(y).cuda(), (32, 32), 1)
    check_sums(sums, want, False, "one pixel")
    check_q(q, want, "one pixel")
    assert q[0, 0, 2] == 9.0 and sums[..., 4].max() == 9.0 and (sums[..., 4] != 0).sum() == 1
    touched = sums[0, 0, :, :, 2] != sums[0, 0, :, :, 3]  # tiles whose windows are not all exactly 1
    assert touched.sum() == 4 and touched[0:2, 1:3].all()
    assert (Q.ssim_map(x, y) != 1.0).sum() == 121


# ---- layouts and memory kinds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layouts", [("dense", "odd"), ("odd", "pitched"), ("pitched", "dense")], ids=lambda l: l[0] + "-" + l[1])
def test_layouts_and_poison(wm, tc, layouts, channels, pi):
    """the planes in poisoned buffers (both poisons of layouts.POISON): the bits of the dense planes, whatever fills the padding"""
    shape, F, tile = (43, 67), 2, (32, 32)
    R, Cc = shape
    eng = engine(wm, shape, 3)
    x, y = content(shape)
    for mix in (("f32", "u8"), ("u8", "f32")):
        ref, test = squeeze(as_kind(x, mix[0]), F, channels), squeeze(as_kind(y, mix[1]), F, channels)
        q0, s0 = run(wm, tc, eng, tc.from_numpy(ref.copy()).cuda(), tc.from_numpy(test.copy()).cuda(), tile, channels)
        want = model(ref.reshape(F, channels, R, Cc), test.reshape(F, channels, R, Cc), tile)
        check_sums(s0, want, False, f"dense {mix}")
        la, lb = LY.make(layouts[0], R, Cc, channels, F), LY.make(layouts[1], R, Cc, channels, F)
        abuf, av = LY.place(tc, ref, la, LY.POISON[mix[0]][pi], channels)
        bbuf, bv = LY.place(tc, test, lb, LY.POISON[mix[1]][pi], channels)
        q, s = run(wm, tc, eng, av, bv, tile, channels)
        assert (bits(s) == bits(s0)).all() and (bits(q) == bits(q0)).all(), (layouts, mix)
        assert (LY.raw(abuf) == LY.raw(LY.expect(ref, la, LY.POISON[mix[0]][pi], channels))).all()  # (both planes are only read)
        assert (LY.raw(bbuf) == LY.raw(LY.expect(test, lb, LY.POISON[mix[1]][pi], channels))).all()
        # the same buffers as WM_MEM_HOST planes
        ha, hb = LY.expect(ref, la, LY.POISON[mix[0]][pi], channels), LY.expect(test, lb, LY.POISON[mix[1]][pi], channels)
        hp = lambda buf, lay, kind: wm.wm_plane(buf.ctypes.data + lay.offset * buf.itemsize, R, Cc, channels, wm.WM_F32 if kind == "f32" else wm.WM_U8,
                                                wm.WM_MEM_HOST, F, lay.pitch, lay.channel_stride if channels > 1 else 0, lay.frame_stride)
        qh, sh = run(wm, tc, eng, hp(ha, la, mix[0]), hp(hb, lb, mix[1]), tile, channels, slot=1)
        assert (bits(sh) == bits(s0)).all() and (bits(qh) == bits(q0)).all(), (layouts, mix, "host")
        # ... and one host plane against one device plane
        qm, sm = run(wm, tc, eng, hp(ha, la, mix[0]), bv, tile, channels, slot=1)
        assert (bits(sm) == bits(s0)).all() and (bits(qm) == bits(q0)).all(), (layouts, mix, "host ref, device test")


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("channels", [1, 3])
def test_slot_out_after_an_embed_with_host_output(wm, tc, channels, kind):
    """test = WM_MEM_SLOT_OUT after wm_embed(host in, host out): the figures of the output that embed delivered to the host"""
    shape = (70, 130)
    R, Cc = shape
    eng = engine(wm, shape)
    x = content(shape)[0][0]
    gray = as_kind(x[0], kind)
    base = as_kind(x, kind) if channels == 3 else gray
    out_h = np.zeros_like(base)
    dt = wm.WM_F32 if kind == "f32" else wm.WM_U8
    host = lambda arr, ch: wm.wm_plane(arr.ctypes.data, R, Cc, ch, dt, wm.WM_MEM_HOST, 1, Cc, R * Cc if ch > 1 else 0, 0)
    named = wm.wm_plane(None, R, Cc, channels, dt, wm.WM_MEM_SLOT_OUT, 1, Cc, R * Cc if channels > 1 else 0, 0)
    a, st = (C.c_float * 1)(), (C.c_int * 1)()
    q = np.zeros((1, channels, 3), np.float32)
    eng.embed_async(host(gray, 1), host(base, channels), host(out_h, channels), wm.MASK_TYPE.NVF, 1, a, st)
    eng.quality_async(host(base, channels), named, 1, q, channels=channels)
    assert eng.sync(1) == wm.WM_OK and st[0] == 0 and (out_h != base).any()
    want = model(base.reshape(1, channels, R, Cc), out_h.reshape(1, channels, R, Cc), (0, 0))
    check_q(q, want, f"SLOT_OUT ch={channels} {kind}")
    # the name still means that output: a second call, and the packers' matching rule
    q2, s2 = run(wm, tc, eng, host(base, channels), named, (32, 32), channels, slot=1)
    want32 = model(base.reshape(1, channels, R, Cc), out_h.reshape(1, channels, R, Cc), (32, 32))
    check_sums(s2, want32, kind == "u8", "SLOT_OUT again")
    check_q(q2, want32, "SLOT_OUT again")
    other = wm.wm_plane(None, R, Cc, channels, wm.WM_U8 if kind == "f32" else wm.WM_F32, wm.WM_MEM_SLOT_OUT, 1, Cc, R * Cc if channels > 1 else 0, 0)
    assert wm.lib().wm_quality(eng._ctx, C.byref(host(base, channels)), C.byref(other), 0, 0, q.ctypes.data_as(C.POINTER(C.c_float)), None, 1) == wm.WM_ERR_BAD_ARG


# ---- invariance -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [("f32", "f32"), ("u8", "f32")], ids=lambda m: m[0] + "-" + m[1])
def test_a_frames_sums_do_not_depend_on_the_batch_or_on_repetition(wm, tc, mix):
    shape, tile = (270, 480), (64, 128)
    eng = engine(wm, shape, 3)
    x, y = content(shape)
    ref, test = tc.from_numpy(as_kind(x[:, 0], mix[0])).cuda(), tc.from_numpy(as_kind(y[:, 0], mix[1])).cuda()
    q3, s3 = run(wm, tc, eng, ref, test, tile, 1)
    q3b, s3b = run(wm, tc, eng, ref, test, tile, 1, slot=1)
    assert (bits(s3) == bits(s3b)).all() and (bits(q3) == bits(q3b)).all()
    for f in range(3):
        q1, s1 = run(wm, tc, eng, ref[f], test[f], tile, 1, slot=f % 2)
        assert (bits(s1[0]) == bits(s3[f])).all() and (bits(q1[0]) == bits(q3[f])).all(), f


# ---- no side effects --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["checked", "promised"])
def test_no_side_effects_on_the_slot(wm, tc, mode):
    """wm_embed, wm_quality(base, SLOT_OUT), wm_detect: the score's bits and the checked hand-over's counts of the sequence without the
    quality call -- under the checked hand-over (the detector names the pointer) and under wm_set_handover (it names SLOT_OUT)"""
    shape, F = (64, 256), 2
    R, Cc = shape
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=2, max_frames=F)
    if mode == "promised":
        eng.set_handover(True)
    x = tc.from_numpy(np.stack([synth_frame(R, Cc, frame=5 + f) for f in range(F)])).cuda()
    y = tc.empty_like(x)
    named = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
    seen = y if mode == "checked" else named
    c0, c1, c2 = (C.c_float * F)(), (C.c_float * F)(), (C.c_float * F)()
    q = np.zeros((F, 1, 3), np.float32)
    tc.cuda.synchronize()
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    eng.detect_async(seen, wm.MASK_TYPE.ME, 0, c0)
    eng.sync(0)
    counts0 = eng.checked_handover_counts()
    y0 = y.clone()
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    eng.quality_async(x, named, 0, q)
    eng.detect_async(seen, wm.MASK_TYPE.ME, 0, c1)
    eng.sync(0)
    counts1 = eng.checked_handover_counts()
    eng.detect_async(named, wm.MASK_TYPE.ME, 0, c2)  # (the name still means the embed's output)
    eng.sync(0)
    assert bits(np.array(c1[:], np.float32)).tolist() == bits(np.array(c0[:], np.float32)).tolist()
    assert all(abs(c2[f] - c0[f]) <= 2e-7 and c0[f] > 0.3 for f in range(F))
    assert counts0 == ((F, 0) if mode == "checked" else (0, 0)) and counts1 == (2 * counts0[0], 0)
    assert tc.equal(y, y0)
    check_q(q, model(x.cpu().numpy()[:, None], y.cpu().numpy()[:, None], (0, 0)), mode)
    eng.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_order_and_the_record_cap(wm, tc):
    shape, F = (43, 67), 3
    R, Cc = shape
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=2, max_frames=F)
    L, ctx, byref = wm.lib(), eng._ctx, C.byref

    def refused(rc, text, code=wm.WM_ERR_BAD_ARG):
        assert rc == code, (rc, text)
        msg = L.wm_last_error(ctx).decode()
        assert text in msg, (text, msg)

    def plane(src, **kw):
        p = wm.wm_plane.from_buffer_copy(src)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    a_t = tc.zeros((F, 3, R, Cc), dtype=tc.float32, device="cuda")
    b_t = tc.ones((F, 3, R, Cc), dtype=tc.uint8, device="cuda")
    tc.cuda.synchronize()
    a, b = wm.plane_of(a_t[0, 0]), wm.plane_of(b_t[0, 0])
    qbuf = (C.c_float * (F * 3 * 3))()
    sums = tc.zeros(F * 3 * 5 * 4, dtype=tc.float64, device="cuda")
    sp = C.c_void_p(sums.data_ptr())
    BAD_SLOT = 2
    wrong = dict(rows=R + 1)
    two = dict(frames=2, frame_stride=3 * R * Cc)
    three_ch = dict(channels=3, channel_stride=R * Cc)
    named = plane(b, data=None, mem=wm.WM_MEM_SLOT_OUT)  # (no embed has run on this engine)
    Q_ = lambda r, t, th, tw, q, s, slot: L.wm_quality(ctx, r, t, th, tw, q, s, slot)

    assert Q_(byref(a), byref(b), 0, 0, qbuf, sp, wm.WM_SLOT_SYNC) == wm.WM_OK  # the arguments the cases are built from are accepted
    assert Q_(byref(a), byref(a), 32, 32, qbuf, None, 1) == wm.WM_OK and eng.sync(1) == wm.WM_OK
    # 1. null pointers, or both outputs null -- each with a later step wrong as well
    assert Q_(None, byref(b), 0, 0, qbuf, None, 0) == wm.WM_ERR_BAD_ARG
    assert L.wm_quality(None, byref(a), byref(b), 0, 0, qbuf, None, 0) == wm.WM_ERR_BAD_ARG
    refused(Q_(None, byref(plane(b, **wrong)), 0, 0, qbuf, None, 0), "null plane")
    refused(Q_(byref(plane(a, **wrong)), None, 0, 0, qbuf, None, 0), "null plane")
    refused(Q_(byref(plane(a, data=None)), byref(plane(b, **wrong)), 0, 0, qbuf, None, 0), "null plane")
    refused(Q_(byref(plane(a, **wrong)), byref(plane(b, data=None)), 0, 0, qbuf, None, 0), "null plane")
    refused(Q_(byref(plane(a, data=None, mem=wm.WM_MEM_SLOT_OUT)), byref(b), 0, 0, qbuf, None, 0), "null plane")
    refused(Q_(byref(plane(a, **wrong)), byref(b), 0, 0, None, None, 0), "both null")
    # 2. shapes
    refused(Q_(byref(plane(a, **wrong)), byref(plane(b, dtype=wm.WM_U16)), 0, 0, qbuf, None, 0), "ref: plane is")
    refused(Q_(byref(plane(a, dtype=wm.WM_U16)), byref(plane(b, cols=Cc - 1)), 0, 0, qbuf, None, 0), "test: plane is")
    refused(Q_(byref(a), byref(plane(named, **wrong)), 0, 0, qbuf, None, 0), "test: plane is")
    # 3. each plane's own rules
    refused(Q_(byref(plane(a, dtype=wm.WM_U16)), byref(plane(b, **three_ch)), 0, 0, qbuf, None, 0), "ref: bad dtype")
    refused(Q_(byref(plane(a, channels=2)), byref(plane(b, **three_ch)), 0, 0, qbuf, None, 0), "ref: channels must be 1 or 3")
    refused(Q_(byref(plane(a, mem=wm.WM_MEM_SLOT_OUT)), byref(plane(b, **three_ch)), 0, 0, qbuf, None, 0), "ref: WM_MEM_SLOT_OUT is valid for")
    refused(Q_(byref(plane(a, frames=F + 1, frame_stride=R * Cc)), byref(plane(b, **three_ch)), 0, 0, qbuf, None, 0), "ref: frames=4 exceeds")
    refused(Q_(byref(a), byref(plane(b, pitch=Cc - 1, **three_ch)), 0, 0, qbuf, None, 0), "test: pitch < cols")
    refused(Q_(byref(a), byref(plane(b, mem=7, **three_ch)), 0, 0, qbuf, None, 0), "test: bad mem")
    refused(Q_(byref(a), byref(plane(b, channels=3, channel_stride=R * Cc - 1)), 0, 0, qbuf, None, 0), "test: channel_stride too small")
    # 4. channel counts, 5. frame counts, 6. tile shape, 7. band mode, 8. slot, 9. the WM_MEM_SLOT_OUT match
    refused(Q_(byref(a), byref(plane(b, frames=2, frame_stride=3 * R * Cc, **three_ch)), 0, 0, qbuf, None, 0), "channel count mismatch")
    refused(Q_(byref(plane(a, **three_ch)), byref(b), 0, 0, qbuf, None, 0), "channel count mismatch")
    refused(Q_(byref(a), byref(plane(b, **two)), 16, 16, qbuf, None, 0), "frame count mismatch")
    for th, tw in ((16, 16), (32, 0), (0, 32), (36, 32), (32, 34), (-32, 32)):
        refused(Q_(byref(a), byref(b), th, tw, qbuf, None, BAD_SLOT), "wm_quality: tile shape")
    assert L.wm_band_configure(ctx, 2, R - 2, 4 * R) == wm.WM_OK
    refused(Q_(byref(a), byref(b), 0, 0, qbuf, None, BAD_SLOT), "wm_quality: not in band mode")
    assert L.wm_band_configure(ctx, 0, 0, 0) == wm.WM_OK
    refused(Q_(byref(a), byref(named), 0, 0, qbuf, None, BAD_SLOT), "bad slot")
    refused(Q_(byref(a), byref(named), 0, 0, qbuf, None, -2), "bad slot")
    refused(Q_(byref(a), byref(named), 0, 0, qbuf, None, 1), "WM_MEM_SLOT_OUT: no matching embed output")
    assert eng.sync(0) == wm.WM_OK and eng.sync(1) == wm.WM_OK  # nothing above left work or results behind
    # record room, after all of these: F * 3 channels * 3 = 27 records a call, 151 calls fit the slot's 4096
    a3, b3 = wm.plane_of(a_t, 3), wm.plane_of(b_t, 3)
    for i in range(151):
        assert Q_(byref(a3), byref(b3), 0, 0, qbuf, None, 1) == wm.WM_OK, i
    refused(Q_(byref(a3), byref(b3), 0, 0, qbuf, None, 1), "too many un-synced results", wm.WM_ERR_BUSY)
    refused(Q_(byref(a3), byref(plane(named, frames=F, frame_stride=3 * R * Cc, **three_ch)), 0, 0, qbuf, None, 1), "WM_MEM_SLOT_OUT: no matching embed output")
    assert Q_(byref(a3), byref(b3), 0, 0, None, sp, 1) == wm.WM_OK            # no q_out: no records
    assert Q_(byref(a), byref(b), 0, 0, qbuf, None, 1) == wm.WM_OK            # 3 records still fit (4077 + 3)
    assert Q_(byref(a3), byref(b3), 0, 0, qbuf, None, 0) == wm.WM_OK          # the other slot has its own 4096
    assert eng.sync(1) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert Q_(byref(a3), byref(b3), 0, 0, qbuf, None, 1) == wm.WM_OK and eng.sync(1) == wm.WM_OK
    assert [qbuf[0], qbuf[1] != qbuf[1] or qbuf[1] < 1.0, qbuf[2]] == [1.0, True, 1.0]  # zeros against ones
    eng.close()


# ---- wm_app ------------------------------------------------------------------------------------------------------------------------------
def write_ini(path, image, wfile, extra):
    path.write_text(f"""[paths]
image = {image}
watermark = {wfile}

[options]
opencl_device = 0
save_watermarked_files_to_disk = false
execution_time_in_fps = true
{extra}

[parameters]
p = 3
psnr = 40.0
loops_for_test = 2
""")


def run_app(ini):
    r = subprocess.run([APP, str(ini)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def untimed(text):
    """the app's output without the lines that hold a measured time (they differ between any two runs)"""
    return [ln for ln in text.splitlines() if not ln.startswith("FPS:") and not ln.startswith("Time to load") and not ln.endswith(" seconds")]


def test_app_reports_quality(wm, tc, tmp_path, golden):
    from conftest import GOLDEN
    info = golden["512"]["files"]
    rgb8 = np.fromfile(os.path.join(GOLDEN, info["rgb"]), np.uint8)[-512 * 512 * 3:].reshape(512, 512, 3)
    img = tmp_path / "512.ppm"
    with open(img, "wb") as f:
        f.write(b"P6\n512 512\n255\n" + rgb8.tobytes())
    wfile = os.path.join(GOLDEN, info["w"])
    ini = tmp_path / "settings.ini"
    write_ini(ini, img, wfile, "")
    plain = run_app(ini)
    write_ini(ini, img, wfile, "report_quality = false")
    off = run_app(ini)
    write_ini(ini, img, wfile, "report_quality = true")
    on = run_app(ini)
    assert "Quality" not in plain and untimed(off) == untimed(plain)
    lines = untimed(on)
    at = [i for i, ln in enumerate(lines) if ln.startswith("Quality [")]
    assert len(at) == 2 and lines[at[0] - 1].startswith("Correlation [ME]:") and at[1] == at[0] + 1
    assert [ln for ln in lines if not ln.startswith("Quality [")] == untimed(plain)  # everything else byte for byte
    # the same planes through the Python surface: the unquantised marked RGB image against the RGB input
    eng = wm.Watermark(512, 512, np.fromfile(wfile, np.float32).reshape(512, 512), 3, 40.0)
    rgb = tc.from_numpy(np.ascontiguousarray(rgb8.transpose(2, 0, 1)).astype(np.float32)).cuda()
    gray = eng.rgb2gray(rgb)
    for k, name in enumerate(("NVF", "ME")):
        y, a = eng.makeWatermark(gray, rgb, wm.MASK_TYPE[name])
        mse, psnr, ssim, mx = eng.quality(rgb, y, channels=3)
        want = "Quality [%s]: PSNR %.4f SSIM %.6f" % (name, wm.psnr_from_mse(float(mse[0].mean())), float(ssim[0].mean()))
        assert lines[at[k]] == want, (lines[at[k]], want)
        assert 39.0 < wm.psnr_from_mse(float(mse[0].mean())) < 42.0 and 0.9 < ssim[0].mean() < 1.0
    eng.close()
