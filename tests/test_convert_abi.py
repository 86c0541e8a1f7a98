"""CPU tests of the pixel-format front (wm.h wm_rgb2gray, wm_unpack_rgb8, wm_pack_rgb8): the symbols are declared, exported and
bound, wm_packed has the header's layout, the Python and C++ surfaces exist, the list of profiling names is still the parent's (the
conversion kernels are launched outside any profiled scope), and calls without a context are refused whatever else they carry (no
GPU needed: nothing here reaches a device).  tests/test_gpu_convert.py checks the calls on a device."""
import ctypes as C
import os

import numpy as np
import pytest

from test_bits_abi import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_rgb2gray", "wm_unpack_rgb8", "wm_pack_rgb8")


@pytest.fixture(scope="module")
def L(wm):
    return wm.lib()


def test_symbols_declared_exported_and_bound(L, wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    bound = {name for name, _, _ in wm.ABI}
    for s in SYMBOLS:
        assert "int " + s + "(" in hdr, s
        assert hasattr(L, s), s
        assert s in bound, s
    assert "typedef struct wm_packed {" in hdr


def test_wm_packed_layout(wm):
    """the header's field order and sizes: a pointer, four int32, two int64 -- 40 bytes without padding"""
    names = [n for n, _ in wm.wm_packed._fields_]
    assert names == ["data", "rows", "cols", "mem", "frames", "pitch_bytes", "frame_stride_bytes"]
    assert C.sizeof(wm.wm_packed) == 40
    assert wm.wm_packed.pitch_bytes.offset == 24 and wm.wm_packed.frame_stride_bytes.offset == 32


def test_python_and_cpp_surfaces(wm):
    for name in ("rgb2gray", "unpackRgb8", "packRgb8", "rgb2gray_async", "unpack_rgb8_async", "pack_rgb8_async"):
        assert hasattr(wm.Watermark, name), name
    assert hasattr(wm, "packed_of")
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for text in ("wm::Image rgb2gray(const wm::Image& rgb, float r = 0.299f, float g = 0.587f, float b = 0.114f) const",
                 "std::pair<wm::Image, wm::Image> unpackRgb8(const uint8_t* interleavedHost, bool wantGray)",
                 "void packRgb8(const wm::Image& rgb, uint8_t* interleavedHost)", "wm_rgb2gray(", "wm_unpack_rgb8(", "wm_pack_rgb8("):
        assert text in hpp, text


def test_packed_of_describes_a_host_tensor(wm):
    import torch
    t = torch.zeros((2, 5, 8, 3), dtype=torch.uint8)[:, :, :7]  # rows padded by one pixel
    pk = wm.packed_of(t)
    assert (pk.rows, pk.cols, pk.frames, pk.mem) == (5, 7, 2, wm.WM_MEM_HOST)
    assert (pk.pitch_bytes, pk.frame_stride_bytes) == (24, 120) and pk.data == t.data_ptr()
    with pytest.raises(RuntimeError):
        wm.packed_of(torch.zeros((5, 7, 3), dtype=torch.float32))
    with pytest.raises(RuntimeError):
        wm.packed_of(torch.zeros((5, 7, 4), dtype=torch.uint8)[:, :, :3])


def test_profiling_names_unchanged(L):
    assert len(KERNELS) == 20
    assert [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())] == KERNELS


def test_refused_without_a_context(L, wm):
    """a null context, null planes and a packed row shorter than its pixels: WM_ERR_BAD_ARG, no device touched"""
    bad = wm.WM_ERR_BAD_ARG
    buf = np.zeros(64 * 64 * 3 * 4, np.uint8)
    data = buf.ctypes.data
    rgb = wm.wm_plane(data, 64, 64, 3, wm.WM_F32, wm.WM_MEM_HOST, 1, 64, 64 * 64, 0)
    gray = wm.wm_plane(data, 64, 64, 1, wm.WM_F32, wm.WM_MEM_HOST, 1, 64, 0, 0)
    pk = wm.wm_packed(data, 64, 64, wm.WM_MEM_HOST, 1, 3 * 64, 0)
    short = wm.wm_packed(data, 64, 64, wm.WM_MEM_HOST, 1, 3 * 64 - 1, 0)
    w = (C.c_float * 3)(0.299, 0.587, 0.114)
    r, g, p, s = C.byref(rgb), C.byref(gray), C.byref(pk), C.byref(short)
    for slot in (wm.WM_SLOT_SYNC, 0):
        assert L.wm_rgb2gray(None, r, g, w, slot) == bad
        assert L.wm_rgb2gray(None, None, None, None, slot) == bad
        assert L.wm_unpack_rgb8(None, p, r, g, None, slot) == bad
        assert L.wm_unpack_rgb8(None, None, None, None, None, slot) == bad
        assert L.wm_unpack_rgb8(None, s, r, g, None, slot) == bad
        assert L.wm_pack_rgb8(None, r, p, slot) == bad
        assert L.wm_pack_rgb8(None, None, None, slot) == bad
        assert L.wm_pack_rgb8(None, r, s, slot) == bad
