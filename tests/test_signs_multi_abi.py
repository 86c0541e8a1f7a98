"""CPU tests of the multi-copy payload surface (wm.h wm_embed_signs_group, wm_embed_signs_multi, wm_embed_bits_multi): the symbols
are declared, exported and bound, the Python and C++ surfaces exist, the list of profiling names is still the parent's (the new
kernel is launched outside any profiled scope), a null context is refused and the group size is a positive constant (no GPU
needed).  tests/test_gpu_signs_multi.py checks the calls on a device."""
import ctypes as C
import os

import numpy as np
import pytest

from test_bits_abi import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_embed_signs_group", "wm_embed_signs_multi", "wm_embed_bits_multi")


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


def test_python_and_cpp_surfaces(wm):
    for name in ("makeWatermarkSignsMulti", "makeWatermarkBitsMulti", "embed_signs_multi_async", "embed_bits_multi_async"):
        assert hasattr(wm.Watermark, name), name
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for text in ("std::vector<wm::Image> makeWatermarkSignsMulti(", "std::vector<wm::Image> makeWatermarkBitsMulti(", "wm_embed_signs_multi(",
                 "wm_embed_bits_multi("):
        assert text in hpp, text


def test_profiling_names_unchanged(L):
    assert len(KERNELS) == 20
    assert [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())] == KERNELS


def test_null_context(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    pp = C.byref(plane)
    signs = np.ones(8, np.int8)
    tb = np.zeros(4, np.int32)
    pay = np.zeros(2, np.uint8)
    assert L.wm_embed_signs_multi(None, 0, pp, pp, pp, 32, 32, 2, signs.ctypes.data_as(C.c_void_p), None, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_embed_bits_multi(None, 0, pp, pp, pp, 32, 32, tb.ctypes.data_as(C.c_void_p), 1, 2, pay.ctypes.data_as(C.c_void_p), None, None, 0) == bad
    assert L.wm_embed_signs_multi(None, 0, None, None, None, 32, 32, 1, None, None, None, 0) == bad
    assert L.wm_embed_bits_multi(None, 0, None, None, None, 32, 32, None, 1, 1, None, None, None, 0) == bad


def test_group_size(L):
    assert L.wm_embed_signs_group() >= 1
