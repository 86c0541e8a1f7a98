"""Samples of 9 to 16 bits on the device (wm.h wm_unpack16, wm_pack16, wm_embed16, wm_detect16) and wm_app's high-depth video mode.

Expectations come from tests/depth_model.py (the numpy restatement of wm.h's arithmetic) and the CPU oracle, never from the library.
Conversions are compared bit for bit (integer views, so a NaN equals itself) and as whole BUFFERS: tests/layouts.py's scheme -- the
plane in a poisoned buffer, and after the call the buffer holds the expected elements in place and poison everywhere else.  u16
layouts (elements): `dense`; `oddpitch` (an odd pitch: rows alternate between 4- and 2-byte alignment, the per-pixel path); `offset1`
(even pitch and strides, base one element in: 2-byte but not 4-byte aligned, per pixel); `padded` (base, pitch and strides padded but
even: the 8-byte path).  The f32 side takes layouts.py's `dense`, `odd` (base one element in, pitch cols + 5) and `pitched`.
Shapes (5, 3), (7, 67), (33, 258), (8, 1030): narrower than one lane, ragged tails of 3 and 2 pixels, more than one block per row."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_model as D
import layouts as LY
import oracle_lib as O
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "watermarking-gpu_amd", "wm_app")
SHAPES = [(5, 3), (7, 67), (33, 258), (8, 1030)]
LAYOUTS16 = ["dense", "oddpitch", "offset1", "padded"]
F32_OF = {"dense": "dense", "oddpitch": "odd", "offset1": "pitched", "padded": "dense"}  # the f32 layout that goes with a u16 layout here
POISON16 = np.uint16(0xA5A5)
POISON32 = LY.POISON["f32"][0]


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


def raw(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = raw(got) != raw(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {int(np.argmax(bad))}"


def layout16(name, rows, cols, channels, frames):
    if name == "dense":
        return LY.make("dense", rows, cols, channels, frames)
    if name == "oddpitch":
        off, pitch = 0, cols + 1 + cols % 2
        cs = rows * pitch + 1
        fs = channels * cs + 3
    elif name == "offset1":
        off, pitch = 1, cols + cols % 2 + 2
        cs = rows * pitch + 2
        fs = channels * cs + 4
    else:  # padded
        off, pitch = 2, LY.roundup4(cols) + 4
        cs = rows * pitch + 6
        fs = channels * cs + 10
    lay = LY.Layout(off, pitch, cs, fs, 0)
    return lay._replace(length=LY.extent(lay, rows, cols, channels, frames) + 5)


def to_dev16(tc, a):
    """a numpy uint16 array on the device as an int16 tensor (the 16-bit pattern is the sample)"""
    return tc.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def from_dev16(t):
    return t.cpu().numpy().view(np.uint16)


def squeeze(a, F, channels):
    a = a if channels == 3 else a[:, 0]
    return a if F > 1 else a[0]


def plane_of_buf(wm, ptr, itemsize, lay, rows, cols, channels, frames, dtype, mem):
    return wm.wm_plane(ptr + lay.offset * itemsize, rows, cols, channels, dtype, mem, frames, lay.pitch, lay.channel_stride if channels > 1 else 0,
                       lay.frame_stride if frames > 1 else 0)


_DATA = {}


def samples(shape, F, bits):
    """[F, 3, R, C] uint16: random codes up to a little above full scale (the clamp), 0 and full scale among them; read-only"""
    key = (shape, F, bits)
    if key not in _DATA:
        rng = np.random.default_rng(100 * shape[0] + shape[1] + 7 * F + bits)
        m = D.maxv(bits)
        v = rng.integers(0, min(65536, m + m // 8 + 2), (F, 3) + shape, dtype=np.uint16)
        v.reshape(-1)[:3] = (0, m, min(65535, m + 1))
        v.setflags(write=False)
        _DATA[key] = v
    return _DATA[key]


def values(shape, F, bits):
    """[F, 3, R, C] float32 for wm_pack16: random in [-8, 263], the special values in the first and last elements; read-only"""
    key = (shape, F, bits, "f")
    if key not in _DATA:
        rng = np.random.default_rng(100 * shape[0] + shape[1] + 7 * F + bits + 1)
        x = (rng.random((F, 3) + shape) * 271 - 8).astype(np.float32)
        sp = specials(bits)[: min(len(specials(bits)), x[0, 0].size)]
        x[0, 0].reshape(-1)[: len(sp)] = sp
        x[-1, -1].reshape(-1)[-len(sp):] = sp[::-1]
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def specials(bits):
    g, _ = D.tie_inputs(bits)
    return np.concatenate([np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 255.0, np.nextafter(np.float32(255), np.float32(np.inf)), 1e9], np.float32), g])


# ---- every code -------------------------------------------------------------------------------------------------------------------------
ALL = np.arange(65536, dtype=np.uint16).reshape(256, 256)


@pytest.mark.parametrize("msb", [0, 1])
@pytest.mark.parametrize("bits", D.BITS)
def test_every_code(wm, tc, bits, msb):
    eng = engine(wm, (256, 256))
    v = to_dev16(tc, ALL)
    x = tc.empty((256, 256), dtype=tc.float32, device="cuda")
    back = tc.zeros((256, 256), dtype=tc.int16, device="cuda")
    tc.cuda.synchronize()
    eng.unpack16_async(v, bits, x, 0, msb)
    eng.pack16_async(x, back, bits, 0, msb)
    eng.sync(0)
    assert_bits(x.cpu().numpy(), D.unpack(ALL, bits, msb), f"unpack d={bits} msb={msb}")
    sh = 16 - bits
    want = ((ALL >> sh) << sh) if msb else np.minimum(ALL, D.maxv(bits))
    assert_bits(from_dev16(back), want.astype(np.uint16), f"pack(unpack) d={bits} msb={msb}")
    assert_bits(from_dev16(back), D.pack(D.unpack(ALL, bits, msb), bits, msb), "... and the model's")


# ---- pack semantics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msb", [0, 1])
@pytest.mark.parametrize("bits", D.BITS)
def test_pack_semantics(wm, tc, bits, msb):
    """NaN, +-inf, -1, -0.0, 255, the float above 255, 1e9 and exact ties k + 0.5 for even and odd k, in a vector lane at the start of
    the plane and in the ragged tail at its end"""
    shape = (7, 67)
    g, k = D.tie_inputs(bits)
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    x = np.array(values(shape, 1, bits)[0, 0])
    sp = specials(bits)
    x.reshape(-1)[-len(sp):] = sp[::-1]
    assert np.isnan(x[0, 0]) and np.isnan(x[-1, -1]) and (x.reshape(-1)[8:8 + len(g)] == g).all()
    out = eng_pack(wm, tc, shape, x, bits, msb)
    assert_bits(out, D.pack(x, bits, msb), f"pack specials d={bits} msb={msb}")
    # (what the model says of them, spelled out once)
    m, sh = D.maxv(bits), (16 - bits) * msb
    assert (out.reshape(-1)[:8] >> sh).tolist() == [0, m, 0, 0, 0, m, m, m]
    assert ((out.reshape(-1)[8:8 + len(k)] >> sh) == np.where(k % 2 == 0, k, k + 1)).all()


def eng_pack(wm, tc, shape, x, bits, msb):
    eng = engine(wm, shape)
    out = tc.zeros(shape, dtype=tc.int16, device="cuda")
    xd = tc.from_numpy(np.array(x)).cuda()
    tc.cuda.synchronize()
    eng.pack16_async(xd, out, bits, wm.WM_SLOT_SYNC, msb)
    return from_dev16(out)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS16)
@pytest.mark.parametrize("shape", SHAPES)
def test_layouts_device(wm, tc, shape, layout, channels, F):
    R, Cc = shape
    eng = engine(wm, shape, F)
    lay16 = layout16(layout, R, Cc, channels, F)
    lay32 = LY.make(F32_OF[layout], R, Cc, channels, F)
    for bits, msb in ((10, 0), (12, 1)):
        what = f"{shape} {layout} ch={channels} F={F} d={bits} msb={msb}"
        v = squeeze(samples(shape, F, bits), F, channels)
        vbuf = to_dev16(tc, LY.expect(v, lay16, POISON16, channels))
        xbuf = tc.from_numpy(np.full(lay32.length, POISON32, np.float32)).cuda()
        tc.cuda.synchronize()
        eng.unpack16_async(LY.view_of(vbuf, lay16, v.shape, channels), bits, LY.view_of(xbuf, lay32, v.shape, channels), wm.WM_SLOT_SYNC, msb, channels)
        assert_bits(xbuf.cpu().numpy(), LY.expect(D.unpack(v, bits, msb), lay32, POISON32, channels), "unpack " + what)
        assert_bits(from_dev16(vbuf), LY.expect(v, lay16, POISON16, channels), "unpack leaves its source: " + what)
        x = squeeze(values(shape, F, bits), F, channels)
        _, xin = LY.place(tc, x, lay32, POISON32, channels)
        obuf = to_dev16(tc, np.full(lay16.length, POISON16, np.uint16))
        tc.cuda.synchronize()
        eng.pack16_async(xin, LY.view_of(obuf, lay16, x.shape, channels), bits, wm.WM_SLOT_SYNC, msb, channels)
        assert_bits(from_dev16(obuf), LY.expect(D.pack(x, bits, msb), lay16, POISON16, channels), "pack " + what)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", ["oddpitch", "padded"])
@pytest.mark.parametrize("shape", SHAPES)
def test_layouts_host(wm, tc, shape, layout, channels):
    """WM_MEM_HOST planes on both sides, F = 3 with padded frame strides: staged both ways, the host outputs' padding untouched; then
    the synchronous methods on dense arrays"""
    R, Cc = shape
    F, bits = 3, 10
    eng = engine(wm, shape, F)
    lay16 = layout16(layout, R, Cc, channels, F)
    lay32 = LY.make(F32_OF[layout], R, Cc, channels, F)
    v = squeeze(samples(shape, F, bits), F, channels)
    x = squeeze(values(shape, F, bits), F, channels)
    hv = LY.expect(v, lay16, POISON16, channels)
    hx_out = np.full(lay32.length, POISON32, np.float32)
    hx = LY.expect(x, lay32, POISON32, channels)
    hv_out = np.full(lay16.length, POISON16, np.uint16)
    p = lambda buf, lay, dt: plane_of_buf(wm, buf.ctypes.data, buf.itemsize, lay, R, Cc, channels, F, dt, wm.WM_MEM_HOST)
    eng.unpack16_async(p(hv, lay16, wm.WM_U16), bits, p(hx_out, lay32, wm.WM_F32), 1, 0, channels)
    eng.pack16_async(p(hx, lay32, wm.WM_F32), p(hv_out, lay16, wm.WM_U16), bits, 1, 0, channels)
    eng.sync(1)
    assert_bits(hx_out, LY.expect(D.unpack(v, bits), lay32, POISON32, channels), f"unpack host {shape} {layout} ch={channels}")
    assert_bits(hv_out, LY.expect(D.pack(x, bits), lay16, POISON16, channels), f"pack host {shape} {layout} ch={channels}")
    if layout == "padded":
        got = eng.unpack16(np.ascontiguousarray(v), bits, channels=channels)
        assert_bits(got.cpu().numpy(), D.unpack(v, bits), "Watermark.unpack16")
        assert_bits(eng.pack16(tc.from_numpy(np.array(x)).cuda(), bits, channels=channels), D.pack(x, bits), "Watermark.pack16")


@pytest.mark.parametrize("channels", [1, 3])
def test_pack16_from_slot_out(wm, tc, channels):
    """wm_pack16 of WM_MEM_SLOT_OUT after a host-staged wm_embed = wm_pack16 of the output that embed delivered to the host"""
    shape, bits = (33, 258), 10
    R, Cc = shape
    eng = engine(wm, shape, 1)
    gray = np.ascontiguousarray(D.unpack(samples(shape, 1, bits)[0, 0], bits))
    base = np.ascontiguousarray(D.unpack(samples(shape, 1, bits)[0], bits)) if channels == 3 else gray
    out_h = np.full(base.shape, np.float32(-1e30), np.float32)
    a, st = (C.c_float * 1)(), (C.c_int * 1)()
    host = lambda arr, ch: wm.wm_plane(arr.ctypes.data, R, Cc, ch, wm.WM_F32, wm.WM_MEM_HOST, 1, Cc, R * Cc if ch > 1 else 0, 0)
    slot_out = wm.wm_plane(None, R, Cc, channels, wm.WM_F32, wm.WM_MEM_SLOT_OUT, 1, Cc, R * Cc if channels > 1 else 0, 0)
    from_slot = tc.zeros(base.shape, dtype=tc.int16, device="cuda")
    tc.cuda.synchronize()
    eng.embed_async(host(gray, 1), host(base, channels), host(out_h, channels), wm.MASK_TYPE.NVF, 1, a, st)
    eng.pack16_async(slot_out, from_slot, bits, 1, 0, channels)
    eng.sync(1)
    assert st[0] == 0 and not (out_h == np.float32(-1e30)).any()
    from_host = np.zeros(base.shape, np.uint16)
    eng.pack16_async(host(out_h, channels), from_host, bits, 1, 0, channels)
    eng.sync(1)
    assert_bits(from_dev16(from_slot), from_host, f"pack16 of SLOT_OUT, channels={channels}")
    assert_bits(from_host, D.pack(out_h, bits), "... which is the model's pack of the output")
    assert (from_host != D.pack(base, bits)).any()  # (the embed did mark the plane)


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def frames16(shape, F, bits):
    return np.stack([D.quantise(synth_frame(shape[0], shape[1], frame=f + 1), bits) for f in range(F)])


_COMP = {}


def comp_engine(wm, shape, F):
    key = (shape, F)
    if key not in _COMP:
        eng = wm.Watermark(shape[0], shape[1], synth_watermark(shape[0], shape[1], 777), 3, 40.0, nslots=2, max_frames=F)
        eng.set_fused(False)
        _COMP[key] = eng
    return _COMP[key]


@pytest.mark.parametrize("bits", [10, 12])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("mask", ["ME", "NVF"])
@pytest.mark.parametrize("shape", [(64, 256), (130, 522)])
def test_embed16_and_detect16_are_their_three_calls(wm, tc, shape, mask, F, bits):
    R, Cc = shape
    mt = wm.MASK_TYPE[mask]
    eng = comp_engine(wm, shape, F)
    v = frames16(shape, F, bits)
    vd = to_dev16(tc, v)
    X, Y = tc.empty((F, R, Cc), dtype=tc.float32, device="cuda"), tc.empty((F, R, Cc), dtype=tc.float32, device="cuda")
    ref = tc.zeros((F, R, Cc), dtype=tc.int16, device="cuda")
    a_ref, st_ref, c_ref = (C.c_float * F)(), (C.c_int * F)(), (C.c_float * F)()
    tc.cuda.synchronize()
    eng.unpack16_async(vd, bits, X, 0)
    eng.embed_async(X, X, Y, mt, 0, a_ref, st_ref)
    eng.pack16_async(Y, ref, bits, 0)
    eng.sync(0)
    want = from_dev16(ref)
    assert list(st_ref) == [0] * F and all(np.isfinite(a_ref[f]) and a_ref[f] > 0 for f in range(F))
    assert (want != v).any()
    # out of place, on the device
    out = tc.zeros((F, R, Cc), dtype=tc.int16, device="cuda")
    a, st = (C.c_float * F)(), (C.c_int * F)()
    tc.cuda.synchronize()
    eng.embed16_async(vd, out, bits, mt, 0, False, a, st)
    # ... afterwards WM_MEM_SLOT_OUT names an f32 grey plane wm_detect accepts: Y
    c_slot = (C.c_float * F)()
    eng.detect_async(wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc), mt, 0, c_slot)
    eng.sync(0)
    assert_bits(from_dev16(out), want, f"embed16 out of place {shape} {mask} F={F} d={bits}")
    assert_bits(np.array(a[:], np.float32), np.array(a_ref[:], np.float32), "strength")
    assert list(st) == [0] * F
    assert_bits(from_dev16(vd), v, "the input is left as it was")
    eng.detect_async(Y, mt, 0, c_ref)
    eng.sync(0)
    assert_bits(np.array(c_slot[:], np.float32), np.array(c_ref[:], np.float32), "wm_detect of WM_MEM_SLOT_OUT = wm_detect of Y")
    # in place, on a host plane, synchronous
    hv = np.array(v)
    a2, st2 = (C.c_float * F)(), (C.c_int * F)()
    eng.embed16_async(hv, hv, bits, mt, wm.WM_SLOT_SYNC, False, a2, st2)
    assert_bits(hv, want, "embed16 in place (host, synchronous)")
    assert_bits(np.array(a2[:], np.float32), np.array(a_ref[:], np.float32), "strength (in place)")
    # in place on the device
    vd2 = to_dev16(tc, v)
    tc.cuda.synchronize()
    eng.embed16_async(vd2, vd2, bits, mt, 1)
    eng.sync(1)
    assert_bits(from_dev16(vd2), want, "embed16 in place (device)")
    # wm_detect16 = wm_detect(wm_unpack16(v)), on the marked samples
    c16, c3 = (C.c_float * F)(), (C.c_float * F)()
    eng.detect16_async(out, bits, mt, 0, False, c16)
    eng.sync(0)
    eng.unpack16_async(out, bits, X, 0)
    eng.detect_async(X, mt, 0, c3)
    eng.sync(0)
    assert_bits(np.array(c16[:], np.float32), np.array(c3[:], np.float32), "detect16")
    assert all(abs(c) > 0.1 for c in c16)
    if F == 1:  # the synchronous methods
        y2, a_m = eng.makeWatermark16(v[0], bits, mt)
        assert_bits(y2, want[0], "Watermark.makeWatermark16")
        assert np.float32(a_m) == np.float32(a_ref[0])
        assert np.float32(eng.detectWatermark16(y2, bits, mt)) == np.float32(c16[0])


def test_embed16_unsolvable_frame(wm, tc):
    """a flat frame between two ordinary ones: its prediction system cannot be solved (status 1, WM_UNSOLVABLE from the sync, `a`
    untouched) and it comes back equal to its input -- wm_embed's rule for Y, and pack(unpack(v)) == v"""
    shape, F, bits = (64, 256), 3, 10
    eng = comp_engine(wm, shape, F)
    v = np.array(frames16(shape, F, bits))
    v[1] = 517
    vd = to_dev16(tc, v)
    out = tc.zeros(v.shape, dtype=tc.int16, device="cuda")
    a, st = (C.c_float * F)(-7.0, -7.0, -7.0), (C.c_int * F)(9, 9, 9)
    tc.cuda.synchronize()
    eng.embed16_async(vd, out, bits, wm.MASK_TYPE.ME, 0, False, a, st)
    rc = wm.lib().wm_sync(eng._ctx, 0)
    got = from_dev16(out)
    assert_bits(got[1], v[1], "the flat frame comes back as it went in")
    assert (got[0] != v[0]).any() and (got[2] != v[2]).any()
    assert rc == wm.WM_UNSOLVABLE and list(st) == [0, 1, 0] and a[1] == -7.0 and a[0] > 0 and a[2] > 0
    # in place and synchronous: the call itself reports it
    hv = np.array(v)
    a2, st2 = (C.c_float * F)(-7.0, -7.0, -7.0), (C.c_int * F)(9, 9, 9)
    assert wm.lib().wm_embed16(eng._ctx, 0, C.byref(wm.plane_any(hv)), C.byref(wm.plane_any(hv)), bits, 0, a2, st2, wm.WM_SLOT_SYNC) == wm.WM_UNSOLVABLE
    assert_bits(hv, got, "in place on the host")
    assert list(st2) == [0, 1, 0] and a2[1] == -7.0


# ---- oracle parity and round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["ME", "NVF"])
def test_oracle_parity_and_round_trip(wm, tc, mask):
    R, Cc, bits = 270, 480, 10
    mt, om = wm.MASK_TYPE[mask], (O.MASK_ME if mask == "ME" else O.MASK_NVF)
    W = synth_watermark(R, Cc, 777)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=1)
    v = D.quantise(synth_frame(R, Cc, frame=1), bits)
    x = D.unpack(v, bits)
    # the oracle's own figure for the same route: embed the unpacked plane, requantise, detect the unpacked result
    st, yo, ao = O.embed(x, x, W, psnr=40.0, mask=om)
    floor = O.detect(D.unpack(D.pack(yo.astype(np.float32), bits), bits), W, mask=om)[1]
    marked, a = eng.makeWatermark16(v, bits, mt)
    assert a == pytest.approx(ao, rel=1e-4)
    c = eng.detectWatermark16(marked, bits, mt)
    co = O.detect(D.unpack(marked, bits), W, mask=om)[1]
    c0 = eng.detectWatermark16(v, bits, mt)
    print(f"{mask}: marked {c:.6f} (oracle on the same samples {co:.6f}; oracle's own route {floor:.6f}), unmarked {c0:.6f}")
    assert abs(c - co) <= 1e-5
    assert c >= 0.5 * floor and floor > 0.1
    assert abs(c0) < 0.1
    assert abs(c0 - O.detect(x, W, mask=om)[1]) <= 1e-5
    # the requantised plane keeps its PSNR: 40 dB against peak 255 on the [0, 255] scale
    mse = float(np.mean((D.unpack(marked, bits).astype(np.float64) - x) ** 2))
    assert abs(10 * np.log10(255.0 ** 2 / mse) - 40.0) < 0.1
    eng.close()


# ---- hand-over --------------------------------------------------------------------------------------------------------------------------
def test_unpack16_and_pack16_end_a_handover(wm, tc):
    """a batched grey f32 ME embed leaves a checked hand-over of its output y.  wm_unpack16 INTO y ends it: the detector of the pointer
    takes the ordinary path on the new pixels and no frame is counted as trusted or redone.  wm_pack16 into memory that overlaps y
    (a u16 plane laid over the first frame's bytes) ends it the same way"""
    shape, F, bits = (64, 256), 2, 10
    R, Cc = shape
    W = synth_watermark(R, Cc)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2, max_frames=F)
    plain = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2, max_frames=F)
    plain.set_checked_handover(False)
    v = frames16(shape, F, bits)
    x = tc.from_numpy(np.stack([synth_frame(R, Cc, frame=5 + f) for f in range(F)])).cuda()
    y = tc.empty_like(x)
    vd = to_dev16(tc, v)
    c, c_plain = (C.c_float * F)(), (C.c_float * F)()
    tc.cuda.synchronize()
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    eng.unpack16_async(vd, bits, y, 0)
    eng.detect_async(y, wm.MASK_TYPE.ME, 0, c)
    eng.sync(0)
    new_pixels = D.unpack(v, bits)
    assert_bits(y.cpu().numpy(), new_pixels, "the plane holds the unpacked samples")
    plain.detect_async(tc.from_numpy(new_pixels).cuda(), wm.MASK_TYPE.ME, 0, c_plain)
    plain.sync(0)
    assert_bits(np.array(c[:], np.float32), np.array(c_plain[:], np.float32), "score of the new pixels on the ordinary path")
    assert eng.checked_handover_counts() == (0, 0)
    # wm_pack16 whose u16 output lies over y's first bytes (2 frames of u16 = 1 frame of f32)
    src = tc.from_numpy(new_pixels).cuda()
    over = wm.wm_plane(y.data_ptr(), R, Cc, 1, wm.WM_U16, wm.WM_MEM_DEVICE, F, Cc, 0, R * Cc)
    tc.cuda.synchronize()
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    eng.pack16_async(src, over, bits, 0)
    eng.detect_async(y, wm.MASK_TYPE.ME, 0, c)
    eng.sync(0)
    assert eng.checked_handover_counts() == (0, 0)
    assert_bits(y[0].cpu().numpy().view(np.uint16).reshape(F, R, Cc), D.pack(new_pixels, bits), "the packed samples lie over y's first frame")
    # (the hand-over itself works on this engine: without the write in between the frames are trusted)
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    eng.detect_async(y, wm.MASK_TYPE.ME, 0, c)
    eng.sync(0)
    assert eng.checked_handover_counts() == (F, 0)
    eng.close(); plain.close()


# ---- error precedence: null pointers, shapes, one plane's own rules, channels / frames between the planes, overlap, slot, depth, SLOT_OUT
def test_error_precedence(wm, tc):
    shape, F = (7, 67), 3
    R, Cc = shape
    eng = engine(wm, shape, F)
    L = wm.lib()
    ctx = eng._ctx
    byref = C.byref

    def refused(rc, text, code=wm.WM_ERR_BAD_ARG, at=None):
        assert rc == code, (rc, text)
        msg = L.wm_last_error(ctx if at is None else at).decode()
        assert text in msg, (text, msg)

    u_t = tc.zeros((R, Cc + 1), dtype=tc.int16, device="cuda")[:, :Cc]
    f_t = tc.zeros((R, Cc), dtype=tc.float32, device="cuda")
    tc.cuda.synchronize()
    u, f = wm.plane_any(u_t), wm.plane_any(f_t)

    def plane(src, **kw):
        p = wm.wm_plane.from_buffer_copy(src)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    BAD_SLOT = 2
    wrong = dict(rows=R + 1)
    two = dict(frames=2, frame_stride=R * (Cc + 1))
    three_ch = dict(channels=3, channel_stride=R * (Cc + 1))
    u_over_f = plane(u, data=f.data)                      # a u16 plane over f's bytes
    f_over_u = plane(f, data=u.data, pitch=Cc)            # an f32 plane over u's bytes
    slot_out = plane(f, data=None, mem=wm.WM_MEM_SLOT_OUT)  # (no embed has run on this engine's slot 1)
    a, st = (C.c_float * F)(), (C.c_int * F)()

    # the arguments these cases are built from are accepted as they stand
    assert L.wm_unpack16(ctx, byref(u), 10, 0, byref(f), wm.WM_SLOT_SYNC) == wm.WM_OK
    assert L.wm_pack16(ctx, byref(f), byref(u), 10, 1, wm.WM_SLOT_SYNC) == wm.WM_OK
    assert L.wm_embed16(ctx, 1, byref(u), byref(u), 10, 0, a, st, wm.WM_SLOT_SYNC) in (wm.WM_OK, wm.WM_UNSOLVABLE)
    assert L.wm_detect16(ctx, 1, byref(u), 10, 0, a, st, wm.WM_SLOT_SYNC) in (wm.WM_OK, wm.WM_UNSOLVABLE)

    # wm_unpack16: each case reaches a call that would also fail a later step
    refused(L.wm_unpack16(ctx, byref(plane(u, **wrong)), 10, 0, None, 0), "null plane")
    refused(L.wm_unpack16(ctx, byref(plane(u, data=None)), 10, 0, byref(plane(f, **wrong)), 0), "null plane")
    refused(L.wm_unpack16(ctx, byref(plane(u, dtype=wm.WM_U8)), 10, 0, byref(plane(f, **wrong)), 0), "out_f32: plane is")
    refused(L.wm_unpack16(ctx, byref(plane(u, **wrong)), 10, 0, byref(plane(f, dtype=wm.WM_U8)), 0), "src16: plane is")
    refused(L.wm_unpack16(ctx, byref(plane(u, dtype=wm.WM_U8)), 10, 0, byref(plane(f, **two)), 0), "src16: must be a WM_U16 plane")
    refused(L.wm_unpack16(ctx, byref(plane(u, dtype=wm.WM_F32)), 10, 0, byref(plane(f, **two)), 0), "src16: must be a WM_U16 plane")
    refused(L.wm_unpack16(ctx, byref(plane(u, data=u.data + 1)), 10, 0, byref(plane(f, **two)), 0), "src16: data must be 2-byte aligned")
    refused(L.wm_unpack16(ctx, byref(plane(u, pitch=Cc - 1)), 10, 0, byref(plane(f, **two)), 0), "src16: pitch < cols")
    refused(L.wm_unpack16(ctx, byref(u), 10, 0, byref(plane(f, dtype=wm.WM_U16, **two)), 0), "out_f32: must be a WM_F32 plane")
    refused(L.wm_unpack16(ctx, byref(u), 10, 0, byref(plane(f, mem=wm.WM_MEM_SLOT_OUT, **two)), 0), "out_f32: WM_MEM_SLOT_OUT is valid for")
    refused(L.wm_unpack16(ctx, byref(plane(u, **three_ch)), 10, 0, byref(plane(f, **two)), 0), "channel count mismatch")
    refused(L.wm_unpack16(ctx, byref(u), 10, 0, byref(plane(f_over_u, **two)), 0), "frame count mismatch")
    refused(L.wm_unpack16(ctx, byref(u), 10, 0, byref(f_over_u), BAD_SLOT), "out_f32 overlaps src16")
    refused(L.wm_unpack16(ctx, byref(u), 8, 0, byref(f), BAD_SLOT), "bad slot")
    refused(L.wm_unpack16(ctx, byref(u), 8, 0, byref(f), 1), "bits=8")
    refused(L.wm_unpack16(ctx, byref(u), 17, 0, byref(f), 1), "bits=17")
    refused(L.wm_unpack16(ctx, byref(u), 10, 2, byref(f), 1), "msb_aligned must be 0 or 1")
    refused(L.wm_unpack16(ctx, byref(u), 10, -1, byref(f), 1), "msb_aligned must be 0 or 1")

    # wm_pack16
    refused(L.wm_pack16(ctx, byref(plane(f, **wrong)), None, 10, 0, 0), "null plane")
    refused(L.wm_pack16(ctx, byref(plane(f, channels=2)), byref(plane(u, **wrong)), 10, 0, 0), "out16: plane is")
    refused(L.wm_pack16(ctx, byref(plane(f, dtype=wm.WM_U8)), byref(plane(u, **two)), 10, 0, 0), "src_f32: must be a WM_F32 plane")
    refused(L.wm_pack16(ctx, byref(plane(f, channels=2)), byref(plane(u, **two)), 10, 0, 0), "src_f32: channels must be 1 or 3")
    refused(L.wm_pack16(ctx, byref(f), byref(plane(u, dtype=wm.WM_F32, **two)), 10, 0, 0), "out16: must be a WM_U16 plane")
    refused(L.wm_pack16(ctx, byref(f), byref(plane(u, **three_ch)), 10, 0, BAD_SLOT), "channel count mismatch")
    refused(L.wm_pack16(ctx, byref(f), byref(plane(u_over_f, **two)), 10, 0, 0), "frame count mismatch")
    refused(L.wm_pack16(ctx, byref(f), byref(u_over_f), 10, 0, BAD_SLOT), "out16 overlaps src_f32")
    refused(L.wm_pack16(ctx, byref(slot_out), byref(u), 8, 0, BAD_SLOT), "bad slot")
    refused(L.wm_pack16(ctx, byref(slot_out), byref(u), 8, 0, 1), "bits=8")
    refused(L.wm_pack16(ctx, byref(slot_out), byref(u), 10, 3, 1), "msb_aligned must be 0 or 1")
    refused(L.wm_pack16(ctx, byref(slot_out), byref(u), 10, 0, 1), "WM_MEM_SLOT_OUT: no matching f32 embed output")

    # the host layers: their own refusals, and the masks' rule
    refused(L.wm_embed16(ctx, 1, byref(u), None, 10, 0, a, st, 0), "null plane")
    refused(L.wm_embed16(ctx, 7, byref(u), byref(u), 8, 0, a, st, BAD_SLOT), "bad mask type")
    refused(L.wm_embed16(ctx, 1, byref(plane(u, **three_ch)), byref(u), 8, 0, a, st, BAD_SLOT), "grey planes only")
    refused(L.wm_embed16(ctx, 1, byref(u), byref(u), 8, 0, a, st, BAD_SLOT), "bad slot")
    refused(L.wm_embed16(ctx, 1, byref(u), byref(plane(u, dtype=wm.WM_U8)), 8, 0, a, st, 1), "bits=8")
    refused(L.wm_embed16(ctx, 1, byref(u), byref(plane(u, dtype=wm.WM_U8)), 10, 0, a, st, 1), "out16: must be a WM_U16 plane")
    refused(L.wm_embed16(ctx, 1, byref(u), byref(plane(u, **two)), 10, 0, a, st, 1), "grey plane with in16's frame count")
    refused(L.wm_detect16(ctx, 1, None, 10, 0, a, st, 0), "null plane")
    refused(L.wm_detect16(ctx, 1, byref(plane(u, dtype=wm.WM_U8)), 8, 0, a, st, BAD_SLOT), "img16: must be a WM_U16 plane")
    refused(L.wm_detect16(ctx, 1, byref(u), 17, 0, a, st, BAD_SLOT), "bad slot")
    refused(L.wm_detect16(ctx, 1, byref(u), 17, 0, a, st, 1), "bits=17")

    # every other entry point keeps refusing the dtype
    refused(L.wm_detect(ctx, 1, byref(u), a, st, 0), "bad dtype")
    refused(L.wm_embed(ctx, 1, byref(u), byref(u), byref(u), a, st, 0), "bad dtype")

    # band mode refuses the host layers; a p = 5 engine refuses ME
    assert L.wm_band_configure(ctx, 2, R - 2, 4 * R) == wm.WM_OK
    refused(L.wm_embed16(ctx, 1, byref(u), byref(u), 10, 0, a, st, 0), "wm_embed16: not in band mode")
    refused(L.wm_detect16(ctx, 1, byref(u), 10, 0, a, st, 0), "wm_detect16: not in band mode")
    assert L.wm_band_configure(ctx, 0, 0, 0) == wm.WM_OK
    p5 = wm.Watermark(R, Cc, synth_watermark(R, Cc), 5, 40.0)
    assert L.wm_embed16(p5._ctx, 0, byref(u), byref(u), 10, 0, a, st, 0) == wm.WM_ERR_BAD_P
    assert L.wm_detect16(p5._ctx, 0, byref(u), 10, 0, a, st, 0) == wm.WM_ERR_BAD_P
    p5.close()

    # the refusals of the two conversions that no case above reaches
    refused(L.wm_pack16(ctx, byref(plane(f, **wrong)), byref(plane(u, dtype=wm.WM_F32)), 10, 0, 0), "src_f32: plane is")
    refused(L.wm_pack16(ctx, byref(plane(f, mem=wm.WM_MEM_SLOT_OUT, channels=2)), byref(plane(u, **two)), 10, 0, 0), "src_f32: channels must be 1 or 3")
    refused(L.wm_unpack16(ctx, byref(plane(u, mem=wm.WM_MEM_SLOT_OUT)), 10, 0, byref(plane(f, **two)), 0), "src16: WM_MEM_SLOT_OUT is valid for")
    refused(L.wm_unpack16(ctx, byref(u), 10, 0, byref(plane(f, pitch=Cc - 1, **two)), 0), "out_f32: pitch < cols")
    # (the launch grid's refusals cannot be reached: wm_create stops at 32768 rows and wm_configure at 4096 frames, the grid at 65535)

    # nothing above left work or results behind
    assert eng.sync(0) == wm.WM_OK and eng.sync(1) == wm.WM_OK

    # what needs an embed's output on the slot: a WM_MEM_SLOT_OUT input that does not match it, and an output laid over it
    R2, C2 = 33, 258
    eng2 = wm.Watermark(R2, C2, synth_watermark(R2, C2), 3, 40.0, nslots=2, max_frames=2)
    ctx2 = eng2._ctx
    x = tc.from_numpy(np.ascontiguousarray(D.unpack(samples((R2, C2), 1, 10)[0, 0], 10))).cuda()
    y = tc.empty((2, R2, C2), dtype=tc.float32, device="cuda")[0]  # (room for the two frames one case below asks for)
    free16 = tc.zeros((2, R2, C2), dtype=tc.int16, device="cuda")
    tc.cuda.synchronize()
    eng2.embed_async(x, x, y, wm.MASK_TYPE.NVF, 1)
    assert eng2.sync(1) == wm.WM_OK
    named = wm.wm_plane(None, R2, C2, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, 1, C2, 0, 0)
    u_free = wm.plane_any(free16[0])
    u_over_y = plane(u_free, data=y.data_ptr())
    assert L.wm_pack16(ctx2, byref(named), byref(u_free), 10, 0, 1) == wm.WM_OK
    no_match = "WM_MEM_SLOT_OUT: no matching f32 embed output"
    refused(L.wm_pack16(ctx2, byref(plane(named, frames=2, frame_stride=R2 * C2)), byref(wm.plane_any(free16)), 10, 0, 1), no_match, at=ctx2)
    refused(L.wm_pack16(ctx2, byref(plane(named, channels=3, channel_stride=R2 * C2)), byref(plane(u_over_y, channels=3, channel_stride=R2 * C2)), 10, 0, 1), no_match, at=ctx2)
    refused(L.wm_pack16(ctx2, byref(named), byref(u_over_y), 8, 0, 1), "bits=8", at=ctx2)
    refused(L.wm_pack16(ctx2, byref(named), byref(u_over_y), 10, 0, 1), "wm_pack16: out16 overlaps src_f32 (the slot's last output)", at=ctx2)
    assert eng2.sync(1) == wm.WM_OK
    eng2.close()


# ---- wm_app: a C420p10 y4m ---------------------------------------------------------------------------------------------------------------
def write_ini(path, video, wfile, interval, out, detection):
    path.write_text(f"""[paths]
watermark = {wfile}
video = {video}

[options]
opencl_device = 0

[parameters]
p = 3
psnr = 40.0

[parameters_video]
watermark_interval = {interval}
encode_watermark_file_path = {out}
watermark_detection = {detection}
""")


def run_app(ini):
    r = subprocess.run([APP, str(ini)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("size", [(96, 160), (98, 158)])
def test_app_video_mode_10_bit(wm, tc, tmp_path, size):
    R, Cc = size
    NF, interval, bits = 3, 2, 10
    W = synth_watermark(R, Cc)
    wfile = tmp_path / "w.dat"
    W.tofile(wfile)
    header = b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420p10 XYSCSS=420P10\n" % (Cc, R)
    nuv = 2 * (R // 2) * (Cc // 2)
    ys = [D.quantise(synth_frame(R, Cc, frame=k), bits) for k in range(NF)]
    uvs = [((np.arange(nuv) * (k + 3)) % 1021).astype("<u2") for k in range(NF)]
    src = tmp_path / "in.y4m"
    with open(src, "wb") as f:
        f.write(header)
        for y, uv in zip(ys, uvs):
            f.write(b"FRAME\n" + y.astype("<u2").tobytes() + uv.tobytes())
    dst, ini = tmp_path / "out.y4m", tmp_path / "settings.ini"
    write_ini(ini, src, wfile, interval, dst, "false")
    run_app(ini)
    data = dst.read_bytes()
    assert data[: len(header)] == header
    fsz = 6 + 2 * R * Cc + 2 * nuv
    assert len(data) == len(header) + NF * fsz
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=3)
    marked = {}
    for k in range(NF):
        fr = data[len(header) + k * fsz: len(header) + (k + 1) * fsz]
        assert fr[:6] == b"FRAME\n"
        y = np.frombuffer(fr[6: 6 + 2 * R * Cc], "<u2").reshape(R, Cc)
        assert fr[6 + 2 * R * Cc:] == uvs[k].tobytes(), "chroma passes through"
        if k % interval == 0:
            want = np.array(ys[k])
            eng.embed16_async(want, want, bits, wm.MASK_TYPE.ME, 0)
            eng.sync(0)
            assert_bits(y.astype(np.uint16), want, f"frame {k}: the Y plane is wm_embed16's")
            assert (want != ys[k]).any()
            marked[k] = want
        else:
            assert_bits(y.astype(np.uint16), ys[k], f"frame {k} is not marked")
    # detect mode over the marked stream: the printed correlations are wm_detect16's (printed with 6 significant digits)
    write_ini(ini, dst, wfile, interval, "", "true")
    found = {int(m.group(1)): m.group(2) for m in re.finditer(r"Correlation for frame: (\d+): ([-0-9.e+]+)", run_app(ini))}
    assert sorted(found) == sorted(marked)
    for k, text in found.items():
        c = eng.detectWatermark16(marked[k], bits, wm.MASK_TYPE.ME)
        assert float(text) == float("%g" % c), (k, text, c)
        assert c > 0.3
    eng.close()


def test_app_video_mode_other_420_tags_stay_8_bit(wm, tc, tmp_path):
    """C420jpeg (and C420paldv, C420mpeg2): one byte per sample, the Y plane through wm_embed on u8 host planes as before"""
    R, Cc, NF = 96, 160, 2
    W = synth_watermark(R, Cc)
    wfile = tmp_path / "w.dat"
    W.tofile(wfile)
    nuv = 2 * (R // 2) * (Cc // 2)
    ys = [synth_frame(R, Cc, frame=k, dtype=np.uint8) for k in range(NF)]
    uv = (np.arange(nuv) % 251).astype(np.uint8)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=3)
    for tag in (b"C420jpeg", b"C420paldv"):
        header = b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 %s\n" % (Cc, R, tag)
        src = tmp_path / "in8.y4m"
        with open(src, "wb") as f:
            f.write(header)
            for y in ys:
                f.write(b"FRAME\n" + y.tobytes() + uv.tobytes())
        dst, ini = tmp_path / "out8.y4m", tmp_path / "settings.ini"
        write_ini(ini, src, wfile, 1, dst, "false")
        run_app(ini)
        data = dst.read_bytes()
        fsz = 6 + R * Cc + nuv
        assert data[: len(header)] == header and len(data) == len(header) + NF * fsz
        for k in range(NF):
            fr = data[len(header) + k * fsz: len(header) + (k + 1) * fsz]
            want = np.array(ys[k])
            pl = wm.wm_plane(want.ctypes.data, R, Cc, 1, wm.WM_U8, wm.WM_MEM_HOST, 1, Cc, 0, 0)
            eng.embed_async(pl, pl, pl, wm.MASK_TYPE.ME, 0)
            eng.sync(0)
            assert fr[:6] == b"FRAME\n" and fr[6: 6 + R * Cc] == want.tobytes() and fr[6 + R * Cc:] == uv.tobytes(), (tag, k)
    eng.close()
