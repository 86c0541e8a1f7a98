"""CPU tests of the 9- to 16-bit front (wm.h wm_depth_scale, wm_unpack16, wm_pack16, wm_embed16, wm_detect16): the symbols are
declared, exported and bound, WM_U16 is 2, the Python and C++ surfaces exist, the list of profiling names is still the parent's (the
two kernels are launched outside any profiled scope), and calls without a context or planes are refused (no GPU needed: nothing here
reaches a device).  tests/test_gpu_convert16.py checks the calls on a device, tests/test_depth_model.py the arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

from test_bits_abi import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_depth_scale", "wm_unpack16", "wm_pack16", "wm_embed16", "wm_detect16")


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
    assert "WM_F32 = 0, WM_U8 = 1, WM_U16 = 2" in hdr
    assert (wm.WM_F32, wm.WM_U8, wm.WM_U16) == (0, 1, 2)


def test_python_and_cpp_surfaces(wm):
    for name in ("unpack16", "pack16", "makeWatermark16", "detectWatermark16", "unpack16_async", "pack16_async", "embed16_async", "detect16_async"):
        assert hasattr(wm.Watermark, name), name
    assert hasattr(wm, "plane_any") and hasattr(wm, "depth_scale")
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for text in ("wm::Image unpack16(const uint16_t* host, int channels, int bits, bool msbAligned = false) const",
                 "void pack16(const wm::Image& image, uint16_t* host, int bits, bool msbAligned = false) const",
                 "float makeWatermark16(uint16_t* hostY, int bits, MASK_TYPE maskType, bool msbAligned = false)",
                 "float detectWatermark16(const uint16_t* hostY, int bits, MASK_TYPE maskType, bool msbAligned = false)",
                 "wm_unpack16(", "wm_pack16(", "wm_embed16(", "wm_detect16("):
        assert text in hpp, text


def test_plane_any_describes_host_arrays(wm):
    import torch
    a = np.zeros((2, 5, 8), np.uint16)[:, :, :7]
    p = wm.plane_any(a)
    assert (p.rows, p.cols, p.channels, p.dtype, p.mem, p.frames, p.pitch, p.frame_stride) == (5, 7, 1, wm.WM_U16, wm.WM_MEM_HOST, 2, 8, 40)
    assert p.data == a.ctypes.data
    for dt in (torch.int16, torch.uint16):
        t = torch.zeros((3, 5, 8), dtype=dt)
        p = wm.plane_any(t, 3)
        assert (p.channels, p.dtype, p.mem, p.frames, p.channel_stride, p.data) == (3, wm.WM_U16, wm.WM_MEM_HOST, 1, 40, t.data_ptr())
    assert wm.plane_any(np.zeros((5, 8), np.float32)).dtype == wm.WM_F32
    with pytest.raises(RuntimeError):
        wm.plane_any(np.zeros((5, 8), np.uint8))
    with pytest.raises(RuntimeError):
        wm.plane_any(np.zeros((5, 8), np.uint16)[:, ::2])


def test_profiling_names_unchanged(L):
    assert len(KERNELS) == 20
    assert [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())] == KERNELS


def test_refused_without_a_context_or_planes(L, wm):
    """a null context, whatever else the call carries, and null planes: WM_ERR_BAD_ARG, no device touched"""
    bad = wm.WM_ERR_BAD_ARG
    buf = np.zeros(64 * 64 * 4, np.uint8)
    data = buf.ctypes.data
    p16 = wm.wm_plane(data, 64, 64, 1, wm.WM_U16, wm.WM_MEM_HOST, 1, 64, 0, 0)
    p32 = wm.wm_plane(data, 64, 64, 1, wm.WM_F32, wm.WM_MEM_HOST, 1, 64, 0, 0)
    a, st = (C.c_float * 1)(), (C.c_int * 1)()
    u, f = C.byref(p16), C.byref(p32)
    for slot in (wm.WM_SLOT_SYNC, 0):
        for bits in (10, 8):
            assert L.wm_unpack16(None, u, bits, 0, f, slot) == bad
            assert L.wm_pack16(None, f, u, bits, 0, slot) == bad
            assert L.wm_embed16(None, 0, u, u, bits, 0, a, st, slot) == bad
            assert L.wm_detect16(None, 0, u, bits, 0, a, st, slot) == bad
        assert L.wm_unpack16(None, None, 10, 0, None, slot) == bad
        assert L.wm_pack16(None, None, None, 10, 0, slot) == bad
        assert L.wm_embed16(None, 0, None, None, 10, 0, None, None, slot) == bad
        assert L.wm_detect16(None, 0, None, 10, 0, None, None, slot) == bad
