"""The pixel-format front on the device (wm.h wm_rgb2gray, wm_unpack_rgb8, wm_pack_rgb8).

Expectations come from the oracle (oracle_lib.rgb2gray = wmo_rgb2gray) and numpy, never from the library; every comparison is bit
for bit (uint32 views of f32, so a NaN equals itself), and every output is compared as a whole BUFFER: tests/layouts.py puts the
plane into a poisoned buffer, and the buffer after the call must hold the expected pixels in place and poison everywhere else.
Shapes (5, 64), (7, 67), (33, 258), (3, 1029): one partial vector, a right-edge tail of 1, 2 and 3 pixels, more than one wave per
row, and a 1024-pixel block boundary plus tail.  Planar layouts: `dense`, `pitched` (aligned padding) and `odd` (pitch = cols + 5,
padded channel and frame strides, base one element off: u8 planes leave the vector path, f32 rows are 4-byte aligned only).
Packed rows: 3 * cols bytes, 3 * cols + 1 (unaligned rows: the per-pixel path) and a 4-aligned padded pitch; F = 3 with a padded
frame stride.  Custom weights are held against (w0 * R + w1 * G) + w2 * B evaluated on numpy float32 arrays, which equals the oracle
bit for bit with the default weights (asserted here, on the CPU, for every frame the tests use)."""
import ctypes as C

import numpy as np
import pytest

import layouts as LY
import oracle_lib as O
from synth import synth_watermark

pytestmark = pytest.mark.gpu

SHAPES = [(5, 64), (7, 67), (33, 258), (3, 1029)]
DTYPES = ["f32", "u8"]
POISON8 = np.uint8(0xA5)
PITCHES = ["tight", "odd", "padded"]                     # packed rows
PLANAR_OF = {"tight": "dense", "odd": "odd", "padded": "pitched"}  # the planar layout that goes with a packed pitch in these tests
DEFAULT_W = (0.299, 0.587, 0.114)
OTHER_W = (0.2126, 0.7152, 0.0722)


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


def rgb_frames(shape, F, dtype):
    """[F, 3, R, C]: rng.random * 255 as f32, or random bytes; read-only and shared"""
    key = (shape, F, dtype)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * shape[0] + shape[1] + 7 * F + (dtype == "u8"))
        a = (rng.random((F, 3) + shape) * 255).astype(np.float32) if dtype == "f32" else rng.integers(0, 256, (F, 3) + shape, dtype=np.uint8)
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def gray_np(rgb, w=DEFAULT_W):
    """(w0 * R + w1 * G) + w2 * B on float32 arrays, every product and sum rounded to f32"""
    x = np.asarray(rgb).astype(np.float32)
    w = np.asarray(w, np.float32)
    return (w[0] * x[..., 0, :, :] + w[1] * x[..., 1, :, :]) + w[2] * x[..., 2, :, :]


_GRAY = {}


def gray_oracle(rgb, key=None):
    """oracle_lib.rgb2gray frame by frame; the numpy restatement is held to it bit for bit on the way"""
    x = np.asarray(rgb)
    batched = x.ndim == 4
    key = None if key is None else key + (batched,)
    if key is not None and key in _GRAY:
        return _GRAY[key]
    fr = x if batched else x[None]
    g = np.stack([O.rgb2gray(np.ascontiguousarray(f).astype(np.float32)) for f in fr])
    assert (g.view(np.uint32) == gray_np(fr).view(np.uint32)).all(), "the numpy restatement left the oracle"
    g = g if batched else g[0]
    g.setflags(write=False)
    if key is not None:
        _GRAY[key] = g
    return g


def squeeze(a, F):
    return a if F > 1 else a[0]


def npdt(dtype):
    return np.float32 if dtype == "f32" else np.uint8


def poison_of(dtype):
    return LY.POISON[dtype][0]


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = LY.raw(got) != LY.raw(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {int(np.argmax(bad))}"


def assert_buffer(buf, arr, lay, poison, channels, what):
    assert_bits(buf.cpu().numpy(), LY.expect(arr, lay, poison, channels), what)


def out_buffer(tc, lay, shape, dtype, channels):
    """a poisoned device buffer and the view of it that the call writes"""
    buf = tc.from_numpy(np.full(lay.length, poison_of(dtype), npdt(dtype))).cuda()
    return buf, LY.view_of(buf, lay, shape, channels)


# ---- packed buffers as data: byte offset of pixel (f, r, c) = off + f * fstride + r * pitch + 3 * c ------------------------------
def packed_strides(kind, rows, cols, frames):
    tight = 3 * cols
    if kind == "tight":
        pitch, off = tight, 0
        fs = rows * pitch
    elif kind == "odd":
        pitch, off = tight + 1, 0
        fs = rows * pitch + 7
    else:
        pitch, off = (tight + 3) // 4 * 4 + 8, 4
        fs = rows * pitch + 8
    return off, pitch, fs, off + (frames - 1) * fs + rows * pitch


def packed_indices(kind, rows, cols, frames):
    off, pitch, fs, _ = packed_strides(kind, rows, cols, frames)
    f = np.arange(frames, dtype=np.int64)[:, None, None, None] * fs
    r = np.arange(rows, dtype=np.int64)[None, :, None, None] * pitch
    c = np.arange(cols, dtype=np.int64)[None, None, :, None] * 3
    return off + f + r + c + np.arange(3, dtype=np.int64)[None, None, None, :]


def packed_expect(px, kind):
    """the host image of a packed buffer: px [F, R, C, 3] in place, 0xA5 everywhere else"""
    F, R, Cc, _ = px.shape
    buf = np.full(packed_strides(kind, R, Cc, F)[3], POISON8, np.uint8)
    buf[packed_indices(kind, R, Cc, F).reshape(-1)] = px.reshape(-1)
    return buf


def packed_desc(wm, data_ptr, kind, rows, cols, frames, mem):
    off, pitch, fs, _ = packed_strides(kind, rows, cols, frames)
    return wm.wm_packed(data_ptr + off, rows, cols, mem, frames, pitch, fs if frames > 1 else 0)


def packed_pixels(shape, F):
    """[F, R, C, 3] random bytes"""
    return np.ascontiguousarray(rgb_frames(shape, F, "u8").transpose(0, 2, 3, 1))


def host_plane(wm, buf, lay, rows, cols, channels, dtype, frames):
    return wm.wm_plane(buf.ctypes.data + lay.offset * buf.itemsize, rows, cols, channels, wm.WM_F32 if dtype == "f32" else wm.WM_U8, wm.WM_MEM_HOST,
                       frames, lay.pitch, lay.channel_stride if channels > 1 else 0, lay.frame_stride if frames > 1 else 0)


# ---- wm_rgb2gray ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "odd"])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rgb2gray_default_weights(wm, tc, shape, dtype, F, layout):
    eng = engine(wm, shape, F)
    x = squeeze(rgb_frames(shape, F, dtype), F)
    want = gray_oracle(x, (shape, F, dtype))
    lay_in = LY.make(layout, shape[0], shape[1], 3, F)
    lay_out = LY.make(layout, shape[0], shape[1], 1, F)
    _, xin = LY.place(tc, x, lay_in, poison_of(dtype), 3)
    obuf, out = out_buffer(tc, lay_out, want.shape, "f32", 1)
    tc.cuda.synchronize()
    eng.rgb2gray_async(xin, out, wm.WM_SLOT_SYNC)
    assert_buffer(obuf, want, lay_out, poison_of("f32"), 1, f"rgb2gray {shape} {dtype} F={F} {layout}")
    if layout == "dense":  # the synchronous method, on the same data
        assert_bits(eng.rgb2gray(xin).cpu().numpy(), want, "Watermark.rgb2gray")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rgb2gray_host_planes(wm, tc, shape, dtype):
    """WM_MEM_HOST input (odd layout) and output (pitched layout), F = 3: staged both ways, padding of the host output untouched"""
    F = 3
    eng = engine(wm, shape, F)
    x = rgb_frames(shape, F, dtype)
    want = gray_oracle(x, (shape, F, dtype))
    lay_in = LY.make("odd", shape[0], shape[1], 3, F)
    lay_out = LY.make("pitched", shape[0], shape[1], 1, F)
    hin = LY.expect(x, lay_in, poison_of(dtype), 3)
    hout = np.full(lay_out.length, poison_of("f32"), np.float32)
    pin = host_plane(wm, hin, lay_in, shape[0], shape[1], 3, dtype, F)
    pout = host_plane(wm, hout, lay_out, shape[0], shape[1], 1, "f32", F)
    eng.rgb2gray_async(pin, pout, 1)
    eng.sync(1)
    assert_bits(hout, LY.expect(want, lay_out, poison_of("f32"), 1), f"rgb2gray host planes {shape} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rgb2gray_custom_weights(wm, tc, shape, dtype):
    eng = engine(wm, shape, 1)
    x = rgb_frames(shape, 1, dtype)[0]
    gray_oracle(x, (shape, 1, dtype))  # (holds the restatement to the oracle on this very frame)
    want = gray_np(x, OTHER_W)
    got = eng.rgb2gray(tc.from_numpy(np.array(x)).cuda(), weights=OTHER_W)
    assert_bits(got.cpu().numpy(), want, f"rgb2gray weights {shape} {dtype}")


# ---- wm_unpack_rgb8 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_unpack_rgb8(wm, tc, shape, pitch, dtype, F):
    """planes = packed.transpose exactly, grey = the oracle's of them; both outputs, then each alone (the other NULL)"""
    eng = engine(wm, shape, F)
    R, Cc = shape
    px = packed_pixels(shape, F)
    planar = np.ascontiguousarray(px.transpose(0, 3, 1, 2)).astype(npdt(dtype))
    gray = gray_oracle(planar, (shape, F, "u8"))
    pbuf = tc.from_numpy(packed_expect(px, pitch)).cuda()
    pk = packed_desc(wm, pbuf.data_ptr(), pitch, R, Cc, F, wm.WM_MEM_DEVICE)
    name = PLANAR_OF[pitch]
    lay_rgb, lay_g = LY.make(name, R, Cc, 3, F), LY.make(name, R, Cc, 1, F)
    tc.cuda.synchronize()
    for want_rgb, want_gray in ((True, True), (True, False), (False, True)):
        rbuf, rgb_out = out_buffer(tc, lay_rgb, squeeze(planar, F).shape, dtype, 3)
        gbuf, gray_out = out_buffer(tc, lay_g, squeeze(gray, F).shape, "f32", 1)
        tc.cuda.synchronize()
        eng.unpack_rgb8_async(pk, rgb_out if want_rgb else None, gray_out if want_gray else None, wm.WM_SLOT_SYNC)
        what = f"unpack {shape} {pitch} {dtype} F={F} rgb={want_rgb} gray={want_gray}"
        if want_rgb:
            assert_buffer(rbuf, squeeze(planar, F), lay_rgb, poison_of(dtype), 3, what + ": planes")
        else:
            assert (LY.raw(rbuf) == LY.raw(np.full(1, poison_of(dtype)))[0]).all(), what + ": rgb_out is NULL, nothing may be written"
        if want_gray:
            assert_buffer(gbuf, squeeze(gray, F), lay_g, poison_of("f32"), 1, what + ": grey")
        else:
            assert (LY.raw(gbuf) == LY.raw(np.full(1, poison_of("f32")))[0]).all(), what + ": gray_out is NULL, nothing may be written"
    assert_bits(pbuf.cpu().numpy(), packed_expect(px, pitch), "the source is left as it was")


@pytest.mark.parametrize("F,pitch", [(1, "tight"), (3, "odd"), (3, "padded")])
@pytest.mark.parametrize("shape", SHAPES)
def test_unpack_rgb8_host_input(wm, tc, shape, F, pitch):
    eng = engine(wm, shape, F)
    R, Cc = shape
    px = packed_pixels(shape, F)
    planar = np.ascontiguousarray(px.transpose(0, 3, 1, 2)).astype(np.float32)
    gray = gray_oracle(planar, (shape, F, "u8"))
    hbuf = packed_expect(px, pitch)
    pk = packed_desc(wm, hbuf.ctypes.data, pitch, R, Cc, F, wm.WM_MEM_HOST)
    rgb_out = tc.empty(squeeze(planar, F).shape, dtype=tc.float32, device="cuda")
    gray_out = tc.empty(squeeze(gray, F).shape, dtype=tc.float32, device="cuda")
    eng.unpack_rgb8_async(pk, rgb_out, gray_out, 0)
    eng.sync(0)
    assert_bits(rgb_out.cpu().numpy(), squeeze(planar, F), f"unpack host {shape} F={F} {pitch}: planes")
    assert_bits(gray_out.cpu().numpy(), squeeze(gray, F), f"unpack host {shape} F={F} {pitch}: grey")
    if F == 1:  # the synchronous method on a CPU tensor
        r2, g2 = eng.unpackRgb8(tc.from_numpy(px[0]), tc.float32)
        assert_bits(r2.cpu().numpy(), planar[0], "Watermark.unpackRgb8: planes")
        assert_bits(g2.cpu().numpy(), gray[0], "Watermark.unpackRgb8: grey")


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_rgb8_host_outputs(wm, tc, dtype):
    """WM_MEM_HOST outputs, F = 2 at (7, 67) -- the staged pitch is 68, so the staged frame and channel strides differ from the
    planes' own: both outputs on the host (staged side by side), then each with the other on the device.  rgb_out in the odd layout,
    gray_out in the pitched one: the pixels in place, the padding of host and device buffers untouched"""
    shape, F = (7, 67), 2
    R, Cc = shape
    eng = engine(wm, shape, F)
    px = packed_pixels(shape, F)
    planar = np.ascontiguousarray(px.transpose(0, 3, 1, 2)).astype(npdt(dtype))
    gray = gray_oracle(planar, (shape, F, "u8"))
    pbuf = tc.from_numpy(packed_expect(px, "padded")).cuda()
    pk = packed_desc(wm, pbuf.data_ptr(), "padded", R, Cc, F, wm.WM_MEM_DEVICE)
    lay_rgb, lay_g = LY.make("odd", R, Cc, 3, F), LY.make("pitched", R, Cc, 1, F)
    want_rgb, want_g = LY.expect(planar, lay_rgb, poison_of(dtype), 3), LY.expect(gray, lay_g, poison_of("f32"), 1)
    for host_rgb, host_gray in ((True, True), (True, False), (False, True)):
        hr = np.full(lay_rgb.length, poison_of(dtype), npdt(dtype))
        hg = np.full(lay_g.length, poison_of("f32"), np.float32)
        rbuf, rgb_dev = out_buffer(tc, lay_rgb, planar.shape, dtype, 3)
        gbuf, gray_dev = out_buffer(tc, lay_g, gray.shape, "f32", 1)
        tc.cuda.synchronize()
        eng.unpack_rgb8_async(pk, host_plane(wm, hr, lay_rgb, R, Cc, 3, dtype, F) if host_rgb else rgb_dev,
                              host_plane(wm, hg, lay_g, R, Cc, 1, "f32", F) if host_gray else gray_dev, 1)
        eng.sync(1)
        what = f"unpack host outputs {dtype} rgb_out={'host' if host_rgb else 'device'} gray_out={'host' if host_gray else 'device'}"
        got_rgb, idle_rgb = (hr, rbuf.cpu().numpy()) if host_rgb else (rbuf.cpu().numpy(), hr)
        got_g, idle_g = (hg, gbuf.cpu().numpy()) if host_gray else (gbuf.cpu().numpy(), hg)
        assert_bits(got_rgb, want_rgb, what + ": planes")
        assert_bits(got_g, want_g, what + ": grey")
        assert (LY.raw(idle_rgb) == LY.raw(np.full(1, poison_of(dtype)))[0]).all(), what + ": the rgb buffer the call was not given"
        assert (LY.raw(idle_g) == LY.raw(np.full(1, poison_of("f32")))[0]).all(), what + ": the grey buffer the call was not given"
    assert_bits(pbuf.cpu().numpy(), packed_expect(px, "padded"), "the source is left as it was")


# ---- wm_pack_rgb8 --------------------------------------------------------------------------------------------------------------------
SPECIALS =np.array([0.0, 255.0, 254.999, 255.5, -0.5, -3.0, 1e9, np.nan], np.float32)


def pack_input(shape, F, dtype):
    """f32: the random frames with the special values at the start of the first row (a vector lane) and, reversed, at the end of the
    last row of the last channel of the last frame (the tail); want: np.clip(...).astype(uint8) with 0 for the NaN"""
    x = np.array(rgb_frames(shape, F, dtype))
    if dtype == "u8":
        return x, x
    x[0, 0, 0, :8] = SPECIALS
    x[-1, -1, -1, -8:] = SPECIALS[::-1]
    want = np.clip(np.where(np.isnan(x), np.float32(0), x), 0, 255).astype(np.uint8)
    assert want[0, 0, 0, :8].tolist() == [0, 255, 254, 255, 0, 0, 255, 0]
    return x, want


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pack_rgb8(wm, tc, shape, pitch, dtype, F):
    """f32 in: clip and truncate, NaN -> 0; u8 in: the bytes; padding of the packed rows keeps its 0xA5; u8: unpack returns the planes"""
    eng = engine(wm, shape, F)
    R, Cc = shape
    x, want = pack_input(shape, F, dtype)
    lay = LY.make(PLANAR_OF[pitch], R, Cc, 3, F)
    _, xin = LY.place(tc, squeeze(x, F), lay, poison_of(dtype), 3)
    pbuf = tc.from_numpy(np.full(packed_strides(pitch, R, Cc, F)[3], POISON8, np.uint8)).cuda()
    pk = packed_desc(wm, pbuf.data_ptr(), pitch, R, Cc, F, wm.WM_MEM_DEVICE)
    tc.cuda.synchronize()
    eng.pack_rgb8_async(xin, pk, wm.WM_SLOT_SYNC)
    assert_bits(pbuf.cpu().numpy(), packed_expect(np.ascontiguousarray(want.transpose(0, 2, 3, 1)), pitch), f"pack {shape} {pitch} {dtype} F={F}")
    if dtype == "u8":  # the exact round trip
        back = tc.empty(squeeze(x, F).shape, dtype=tc.uint8, device="cuda")
        eng.unpack_rgb8_async(pk, back, None, wm.WM_SLOT_SYNC)
        assert_bits(back.cpu().numpy(), squeeze(x, F), f"pack / unpack round trip {shape} {pitch} F={F}")


@pytest.mark.parametrize("shape", SHAPES)
def test_pack_rgb8_host_planes(wm, tc, shape):
    """host planar input (odd layout) and host packed output (padded pitch), F = 3; then the synchronous method into a CPU tensor"""
    F = 3
    eng = engine(wm, shape, F)
    R, Cc = shape
    x, want = pack_input(shape, F, "f32")
    lay = LY.make("odd", R, Cc, 3, F)
    hin = LY.expect(x, lay, poison_of("f32"), 3)
    hout = np.full(packed_strides("padded", R, Cc, F)[3], POISON8, np.uint8)
    eng.pack_rgb8_async(host_plane(wm, hin, lay, R, Cc, 3, "f32", F), packed_desc(wm, hout.ctypes.data, "padded", R, Cc, F, wm.WM_MEM_HOST), 1)
    eng.sync(1)
    want_px = np.ascontiguousarray(want.transpose(0, 2, 3, 1))
    assert_bits(hout, packed_expect(want_px, "padded"), f"pack host planes {shape}")
    cpu = tc.full((F, R, Cc, 3), 7, dtype=tc.uint8)
    eng.packRgb8(tc.from_numpy(x).cuda(), out=cpu)
    assert_bits(cpu.numpy(), want_px, "Watermark.packRgb8 into a CPU tensor")


def test_pack_rgb8_host_output_from_slot_out(wm, tc):
    """WM_MEM_SLOT_OUT in, a host packed buffer (padded pitch) out: the bytes are the clipped, truncated pixels of the output the
    embed delivered, the padding keeps its 0xA5"""
    shape = (33, 258)
    R, Cc = shape
    eng = wm.Watermark(R, Cc, synth_watermark(R, Cc), 3, 40.0, nslots=2, max_frames=1)  # (its slot 1 is left naming `out`)
    rgb = rgb_frames(shape, 1, "f32")[0]
    gray_dev, rgb_dev = tc.from_numpy(np.array(gray_oracle(rgb, (shape, 1, "f32")))).cuda(), tc.from_numpy(np.array(rgb)).cuda()
    out = tc.empty((3, R, Cc), dtype=tc.float32, device="cuda")
    hout = np.full(packed_strides("padded", R, Cc, 1)[3], POISON8, np.uint8)
    a, st = (C.c_float * 1)(), (C.c_int * 1)()
    tc.cuda.synchronize()
    eng.embed_async(gray_dev, rgb_dev, out, wm.MASK_TYPE.NVF, 1, a, st)
    eng.pack_rgb8_async(slot_out_plane(wm, shape, wm.WM_F32), packed_desc(wm, hout.ctypes.data, "padded", R, Cc, 1, wm.WM_MEM_HOST), 1)
    eng.sync(1)
    y = out.cpu().numpy()
    assert st[0] == 0 and (y != rgb).any()
    want = np.clip(np.where(np.isnan(y), np.float32(0), y), 0, 255).astype(np.uint8)
    assert_bits(hout, packed_expect(np.ascontiguousarray(want.transpose(1, 2, 0))[None], "padded"), "pack of SLOT_OUT into a host buffer")
    eng.close()


# ---- the image protocol on the device ------------------------------------------------------------------------------------------------
def slot_out_plane(wm, shape, dtype_code):
    R, Cc = shape
    return wm.wm_plane(None, R, Cc, 3, dtype_code, wm.WM_MEM_SLOT_OUT, 1, Cc, R * Cc, 0)


@pytest.mark.parametrize("mask", ["ME", "NVF"])
@pytest.mark.parametrize("shape", [(64, 256), (130, 522)])
def test_image_protocol_on_the_device(wm, tc, shape, mask):
    """unpack -> embed on the planar f32 RGB base with the device grey as mask source -> grey of the output -> detect, all queued on one
    slot with one sync: strength and every output pixel are those of the same embed fed with the host-computed grey, the correlation is
    wm_detect's of the host-computed grey of the downloaded output.  Then once more with a host RGB output and WM_MEM_SLOT_OUT as
    wm_rgb2gray's (and wm_pack_rgb8's) input"""
    R, Cc = shape
    mt = wm.MASK_TYPE[mask]
    eng = engine(wm, shape, 1)
    rng = np.random.default_rng(R * 31 + Cc)
    px = rng.integers(0, 256, (R, Cc, 3), dtype=np.uint8)
    planar = np.ascontiguousarray(px.transpose(2, 0, 1)).astype(np.float32)
    gray_h = gray_oracle(planar)

    # the yardstick: the same embed with the host-computed grey, then detect of the host-computed grey of its output
    a_ref, st_ref, c_ref = (C.c_float * 1)(), (C.c_int * 1)(), (C.c_float * 1)()
    out_ref = tc.empty((3, R, Cc), dtype=tc.float32, device="cuda")
    tc.cuda.synchronize()
    gray_h_dev, planar_dev = tc.from_numpy(np.array(gray_h)).cuda(), tc.from_numpy(planar).cuda()
    eng.embed_async(gray_h_dev, planar_dev, out_ref, mt, 0, a_ref, st_ref)
    eng.sync(0)
    y_ref = out_ref.cpu().numpy()
    gray_y_h_dev = tc.from_numpy(np.array(gray_oracle(y_ref))).cuda()
    eng.detect_async(gray_y_h_dev, mt, 0, c_ref)
    eng.sync(0)
    assert st_ref[0] == 0 and np.isfinite(a_ref[0]) and np.isfinite(c_ref[0]) and c_ref[0] != 0.0

    pk = tc.from_numpy(px).cuda()
    rgb = tc.empty((3, R, Cc), dtype=tc.float32, device="cuda")
    gray, gray_y = tc.empty((R, Cc), dtype=tc.float32, device="cuda"), tc.empty((R, Cc), dtype=tc.float32, device="cuda")
    out = tc.empty((3, R, Cc), dtype=tc.float32, device="cuda")
    a, st, c = (C.c_float * 1)(), (C.c_int * 1)(), (C.c_float * 1)()
    tc.cuda.synchronize()
    eng.unpack_rgb8_async(pk, rgb, gray, 0)
    eng.embed_async(gray, rgb, out, mt, 0, a, st)
    eng.rgb2gray_async(out, gray_y, 0)
    eng.detect_async(gray_y, mt, 0, c)
    eng.sync(0)
    assert st[0] == 0
    assert_bits(np.float32(a[0]), np.float32(a_ref[0]), f"{mask} {shape}: strength")
    assert_bits(out.cpu().numpy(), y_ref, f"{mask} {shape}: output pixels")
    assert_bits(np.float32(c[0]), np.float32(c_ref[0]), f"{mask} {shape}: correlation")

    # a host RGB output; its device copy is what WM_MEM_SLOT_OUT names for the grey and for the packed bytes
    out_h = np.full((3, R, Cc), np.float32(-1e30), np.float32)
    pout = wm.wm_plane(out_h.ctypes.data, R, Cc, 3, wm.WM_F32, wm.WM_MEM_HOST, 1, Cc, R * Cc, 0)
    packed_y = tc.empty((R, Cc, 3), dtype=tc.uint8, device="cuda")
    a2, st2, c2 = (C.c_float * 1)(), (C.c_int * 1)(), (C.c_float * 1)()
    gray_y.fill_(-1.0)
    tc.cuda.synchronize()
    eng.unpack_rgb8_async(pk, rgb, gray, 0)
    eng.embed_async(gray, rgb, pout, mt, 0, a2, st2)
    eng.rgb2gray_async(slot_out_plane(wm, shape, wm.WM_F32), gray_y, 0)
    eng.pack_rgb8_async(slot_out_plane(wm, shape, wm.WM_F32), packed_y, 0)
    eng.detect_async(gray_y, mt, 0, c2)
    eng.sync(0)
    assert_bits(np.float32(a2[0]), np.float32(a_ref[0]), f"{mask} {shape}: strength (host out)")
    assert_bits(out_h, y_ref, f"{mask} {shape}: output pixels (host out)")
    assert_bits(np.float32(c2[0]), np.float32(c_ref[0]), f"{mask} {shape}: correlation (SLOT_OUT grey)")
    assert_bits(packed_y.cpu().numpy(), np.ascontiguousarray(y_ref.transpose(1, 2, 0)).astype(np.uint8), f"{mask} {shape}: packed bytes (SLOT_OUT)")


def test_rgb2gray_ends_a_handover(wm, tc):
    """a batched grey f32 ME embed leaves a checked hand-over of its output; wm_rgb2gray into that plane ends it: the detector of the
    pointer takes the ordinary path on the new pixels, and no frame is counted as trusted (or redone: nothing was checked)"""
    shape, F = (64, 256), 2
    R, Cc = shape
    W = synth_watermark(R, Cc)
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2, max_frames=F)
    plain = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2, max_frames=F)
    plain.set_checked_handover(False)
    rgb = rgb_frames(shape, F, "f32")
    new_pixels = gray_oracle(rgb, (shape, F, "f32"))
    x = tc.from_numpy(np.ascontiguousarray(rgb[:, 1])).cuda()  # (any grey batch: the green planes)
    y = tc.empty_like(x)
    c, c_plain = (C.c_float * F)(), (C.c_float * F)()
    tc.cuda.synchronize()
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    rgb_dev = tc.from_numpy(np.array(rgb)).cuda()
    eng.rgb2gray_async(rgb_dev, y, 0)
    eng.detect_async(y, wm.MASK_TYPE.ME, 0, c)
    eng.sync(0)
    assert_bits(y.cpu().numpy(), new_pixels, "the plane holds the grey")
    new_dev = tc.from_numpy(np.array(new_pixels)).cuda()
    plain.detect_async(new_dev, wm.MASK_TYPE.ME, 0, c_plain)
    plain.sync(0)
    assert_bits(np.array(c[:], np.float32), np.array(c_plain[:], np.float32), "score of the new pixels on the ordinary path")
    assert eng.checked_handover_counts() == (0, 0)
    # (the hand-over itself works on this engine: without the write in between the frames are trusted)
    eng.embed_async(x, x, y, wm.MASK_TYPE.ME, 0)
    eng.detect_async(y, wm.MASK_TYPE.ME, 0, c)
    eng.sync(0)
    assert eng.checked_handover_counts() == (F, 0)


# ---- error precedence: null pointers, shapes, channels / dtype (one plane's own rules), frames, overlap, slot, weights, SLOT_OUT -----
def test_error_precedence(wm, tc):
    shape, F = (5, 64), 3
    R, Cc = shape
    eng = engine(wm, shape, F)
    L = wm.lib()
    ctx = eng._ctx
    byref = C.byref

    def refused(rc, text, at=None):
        assert rc == wm.WM_ERR_BAD_ARG, (rc, text)
        msg = L.wm_last_error(ctx if at is None else at).decode()
        assert text in msg, (text, msg)

    rgb_t = tc.zeros((3, R, Cc), dtype=tc.float32, device="cuda")
    gray_t = tc.zeros((R, Cc), dtype=tc.float32, device="cuda")
    pk_t = tc.zeros((R, Cc, 3), dtype=tc.uint8, device="cuda")
    tc.cuda.synchronize()
    rgb, gray, pk = wm.plane_of(rgb_t, 3), wm.plane_of(gray_t, 1), wm.packed_of(pk_t)

    def plane(src, **kw):
        p = wm.wm_plane.from_buffer_copy(src)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def packed(**kw):
        p = wm.wm_packed.from_buffer_copy(pk)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    nan_w = (C.c_float * 3)(0.299, float("nan"), 0.114)
    inf_w = (C.c_float * 3)(float("inf"), 0.587, 0.114)
    BAD_SLOT = 2
    two = dict(frames=2, frame_stride=3 * R * Cc)
    wrong = dict(rows=R + 1)
    overlapping_gray = plane(gray, data=rgb.data + 4 * (2 * R * Cc))          # the blue plane of rgb
    slot_out = plane(rgb, data=None, mem=wm.WM_MEM_SLOT_OUT)                   # (no embed has run on this engine's slot 1)

    # the arguments these cases are built from are accepted as they stand
    assert L.wm_rgb2gray(ctx, byref(rgb), byref(gray), None, wm.WM_SLOT_SYNC) == wm.WM_OK
    assert L.wm_unpack_rgb8(ctx, byref(pk), byref(rgb), byref(gray), None, wm.WM_SLOT_SYNC) == wm.WM_OK
    assert L.wm_pack_rgb8(ctx, byref(rgb), byref(pk), wm.WM_SLOT_SYNC) == wm.WM_OK

    # wm_rgb2gray
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, **wrong)), None, None, 0), "null plane")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, data=None)), byref(plane(gray, **wrong)), None, 0), "null plane")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, channels=1)), byref(plane(gray, **wrong)), None, 0), "gray_out: plane is")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, **wrong)), byref(plane(gray, dtype=wm.WM_U8)), None, 0), "rgb: plane is")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, channels=1)), byref(plane(gray, **two)), None, 0), "rgb: channels must be 3")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(plane(gray, dtype=wm.WM_U8, **two)), None, 0), "gray_out: must be a 1-channel f32 plane")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(plane(gray, channels=3, channel_stride=R * Cc, **two)), None, 0), "gray_out: channels must be 1")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(plane(overlapping_gray, **two)), None, 0), "frame count mismatch")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(overlapping_gray), None, BAD_SLOT), "gray_out overlaps rgb")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(gray), nan_w, BAD_SLOT), "bad slot")
    refused(L.wm_rgb2gray(ctx, byref(slot_out), byref(gray), nan_w, 1), "weights: not finite")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(gray), inf_w, 1), "weights: not finite")
    refused(L.wm_rgb2gray(ctx, byref(slot_out), byref(gray), None, 1), "WM_MEM_SLOT_OUT: no matching 3-channel embed output")

    # wm_unpack_rgb8
    refused(L.wm_unpack_rgb8(ctx, None, byref(plane(rgb, **wrong)), byref(gray), None, 0), "null packed buffer")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(**wrong)), None, None, None, 0), "both null")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(**wrong)), byref(plane(rgb, data=None)), None, None, 0), "null plane")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(pitch_bytes=3 * Cc - 1, **wrong)), byref(rgb), byref(gray), None, 0), "packed: plane is")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(pitch_bytes=3 * Cc - 1)), byref(rgb), byref(plane(gray, **wrong)), None, 0), "gray_out: plane is")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(pitch_bytes=3 * Cc - 1)), byref(plane(rgb, **two)), byref(gray), None, 0), "packed: pitch_bytes < 3 * cols")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(plane(rgb, channels=1, **two)), byref(gray), None, 0), "rgb_out: channels must be 3")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(rgb), byref(plane(gray, dtype=wm.WM_U8, **two)), None, 0), "gray_out: must be a 1-channel f32 plane")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(rgb), byref(plane(overlapping_gray, **two)), None, 0), "gray_out: frame count mismatch")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(rgb), byref(overlapping_gray), None, BAD_SLOT), "must not overlap")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(plane(rgb, data=pk.data)), None, None, BAD_SLOT), "must not overlap")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(rgb), byref(gray), nan_w, BAD_SLOT), "bad slot")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(rgb), byref(gray), nan_w, 1), "weights: not finite")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(plane(rgb, mem=wm.WM_MEM_SLOT_OUT)), byref(gray), None, 1), "rgb_out: WM_MEM_SLOT_OUT is valid for")

    # wm_pack_rgb8
    refused(L.wm_pack_rgb8(ctx, byref(plane(rgb, **wrong)), None, 0), "null plane or packed buffer")
    refused(L.wm_pack_rgb8(ctx, byref(plane(rgb, channels=1)), byref(packed(**wrong)), 0), "packed_out: plane is")
    refused(L.wm_pack_rgb8(ctx, byref(plane(rgb, channels=1)), byref(packed(frames=2, frame_stride_bytes=3 * R * Cc)), 0), "rgb: channels must be 3")
    refused(L.wm_pack_rgb8(ctx, byref(rgb), byref(packed(pitch_bytes=3 * Cc - 1, frames=2, frame_stride_bytes=3 * R * Cc)), 0), "packed_out: pitch_bytes < 3 * cols")
    refused(L.wm_pack_rgb8(ctx, byref(rgb), byref(packed(data=rgb.data, frames=2, frame_stride_bytes=3 * R * Cc)), 0), "packed_out: frame count mismatch")
    refused(L.wm_pack_rgb8(ctx, byref(rgb), byref(packed(data=rgb.data)), BAD_SLOT), "packed_out overlaps rgb")
    refused(L.wm_pack_rgb8(ctx, byref(slot_out), byref(pk), BAD_SLOT), "bad slot")
    refused(L.wm_pack_rgb8(ctx, byref(slot_out), byref(pk), 1), "WM_MEM_SLOT_OUT: no matching 3-channel embed output")

    # the refusals no case above reaches.  One operand's own rules: check_plane's through rgb, check_packed's, the remaining shapes
    u8 = dict(dtype=wm.WM_U8)
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, dtype=7)), byref(plane(gray, **u8)), None, 0), "rgb: bad dtype")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, mem=9)), byref(plane(gray, **u8)), None, 0), "rgb: bad mem")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, pitch=Cc - 1)), byref(plane(gray, **u8)), None, 0), "rgb: pitch < cols")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, frames=F + 1, frame_stride=3 * R * Cc)), byref(plane(gray, **u8)), None, 0), "rgb: frames=4 exceeds wm_configure max_frames=3")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, channel_stride=R * Cc - 1)), byref(plane(gray, **u8)), None, 0), "rgb: channel_stride too small")
    refused(L.wm_rgb2gray(ctx, byref(plane(rgb, frames=2, frame_stride=3 * R * Cc - 1)), byref(plane(gray, **u8)), None, 0), "rgb: frame_stride too small")
    refused(L.wm_rgb2gray(ctx, byref(rgb), byref(plane(gray, pitch=Cc - 1, **two)), None, 0), "gray_out: pitch < cols")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(pitch_bytes=3 * Cc - 1)), byref(plane(rgb, **wrong)), byref(gray), None, 0), "rgb_out: plane is")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(mem=wm.WM_MEM_SLOT_OUT)), byref(plane(rgb, channels=1)), byref(gray), None, 0), "packed: bad mem (device or host)")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(frames=F + 1, frame_stride_bytes=3 * R * Cc)), byref(plane(rgb, channels=1)), byref(gray), None, 0),
            "packed: frames=4 exceeds wm_configure max_frames=3")
    refused(L.wm_unpack_rgb8(ctx, byref(packed(frames=2, frame_stride_bytes=3 * R * Cc - 1)), byref(plane(rgb, channels=1)), byref(gray), None, 0),
            "packed: frame_stride_bytes too small")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), byref(plane(rgb, **two)), byref(overlapping_gray), None, BAD_SLOT), "rgb_out: frame count mismatch")
    refused(L.wm_unpack_rgb8(ctx, byref(pk), None, byref(plane(gray, data=pk.data)), nan_w, BAD_SLOT), "must not overlap")
    refused(L.wm_pack_rgb8(ctx, byref(plane(rgb, **wrong)), byref(packed(pitch_bytes=3 * Cc - 1)), 0), "rgb: plane is")
    # (the launch grid's refusals cannot be reached: wm_create stops at 32768 rows and wm_configure at 4096 frames, the grid at 65535)

    # nothing above left work or results behind
    assert eng.sync(0) == wm.WM_OK and eng.sync(1) == wm.WM_OK

    # what needs an embed's output on the slot: a WM_MEM_SLOT_OUT input that does not match it, and an output laid over it
    shape2 = (33, 258)
    R2, C2 = shape2
    eng2 = wm.Watermark(R2, C2, synth_watermark(R2, C2), 3, 40.0, nslots=2, max_frames=2)
    ctx2 = eng2._ctx
    x = rgb_frames(shape2, 1, "f32")[0]
    gray_in, base = tc.from_numpy(np.array(gray_oracle(x, (shape2, 1, "f32")))).cuda(), tc.from_numpy(np.array(x)).cuda()
    y = tc.empty((2, 3, R2, C2), dtype=tc.float32, device="cuda")[0]  # (room for the two frames one case below asks for)
    gray2, free_pk = tc.zeros((2, R2, C2), dtype=tc.float32, device="cuda"), tc.zeros((R2, C2, 3), dtype=tc.uint8, device="cuda")
    free_gray = gray2[0]
    tc.cuda.synchronize()
    eng2.embed_async(gray_in, base, y, wm.MASK_TYPE.NVF, 1)
    assert eng2.sync(1) == wm.WM_OK
    named = slot_out_plane(wm, shape2, wm.WM_F32)
    gray_over_y = plane(wm.plane_of(free_gray, 1), data=y.data_ptr() + 4 * (2 * R2 * C2))  # the blue plane of y
    pk_over_y = wm.packed_of(free_pk)
    pk_over_y.data = y.data_ptr()
    assert L.wm_rgb2gray(ctx2, byref(named), byref(wm.plane_of(free_gray, 1)), None, 1) == wm.WM_OK
    assert L.wm_pack_rgb8(ctx2, byref(named), byref(wm.packed_of(free_pk)), 1) == wm.WM_OK
    no_match = "WM_MEM_SLOT_OUT: no matching 3-channel embed output"
    refused(L.wm_rgb2gray(ctx2, byref(slot_out_plane(wm, shape2, wm.WM_U8)), byref(gray_over_y), None, 1), no_match, ctx2)
    refused(L.wm_rgb2gray(ctx2, byref(plane(named, frames=2, frame_stride=3 * R2 * C2)), byref(wm.plane_of(gray2, 1)), None, 1), no_match, ctx2)
    refused(L.wm_pack_rgb8(ctx2, byref(slot_out_plane(wm, shape2, wm.WM_U8)), byref(pk_over_y), 1), no_match, ctx2)
    refused(L.wm_rgb2gray(ctx2, byref(named), byref(gray_over_y), nan_w, 1), "weights: not finite", ctx2)
    refused(L.wm_rgb2gray(ctx2, byref(named), byref(gray_over_y), None, 1), "wm_rgb2gray: gray_out overlaps rgb (the slot's last output)", ctx2)
    refused(L.wm_pack_rgb8(ctx2, byref(named), byref(pk_over_y), 1), "wm_pack_rgb8: packed_out overlaps rgb (the slot's last output)", ctx2)
    assert eng2.sync(1) == wm.WM_OK
    eng2.close()
