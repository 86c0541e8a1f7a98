"""CPU tests of the clip-pooling surface (wm.h wm_clip_pool, wm_locate_pooled, wm_locate_bits_pooled, wm_locate_keys_pooled): the
symbols are declared, exported and bound, the Python and C++ surfaces exist, the profiling list is the parent's, and a null context
is refused by all four before anything else is looked at (no GPU needed; the refusals that need a context are held in order in
tests/test_gpu_locate_clip.py)."""
import ctypes as C
import os

import pytest

from test_locate_abi import PARENT_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_clip_pool", "wm_locate_pooled", "wm_locate_bits_pooled", "wm_locate_keys_pooled", "wm_clip_pool_bench")


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
    for name in ("poolClip", "locatePooled", "locateBitsPooled", "locateKeysPooled", "locateClip", "pool_clip_async", "locate_pooled_async",
                 "locate_bits_pooled_async", "locate_keys_pooled_async"):
        assert hasattr(wm.Watermark, name), name
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for sig, call in (("std::vector<int> poolClip(", "wm_clip_pool("), ("WmLocation locatePooled(", "wm_locate_pooled("),
                      ("WmLocation locateBitsPooled(", "wm_locate_bits_pooled("), ("std::vector<WmLocation> locateKeysPooled(", "wm_locate_keys_pooled(")):
        assert sig in hpp and call in hpp, sig


def test_profiling_list_is_the_parents(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names == PARENT_KERNELS


def test_null_context_is_refused_first(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    loc, soft, w = (C.c_float * 8)(), (C.c_float * 8)(), (C.c_float * 1)(1.0)
    tb = (C.c_int32 * 4)()
    assert L.wm_clip_pool(None, 0, C.byref(plane), w, None, 0, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_clip_pool(None, 7, None, None, None, 1, None, 99) == bad
    assert L.wm_locate_pooled(None, None, None, 0, loc, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_locate_bits_pooled(None, None, None, 0, 32, 32, tb, 2, loc, soft, None, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_locate_keys_pooled(None, None, None, 0, 2, loc, None, wm.WM_SLOT_SYNC) == bad


def test_bench_refusals(L, wm):
    """wm_clip_pool_bench: refused before a device is chosen"""
    us, eq = (C.c_double * 2)(), C.c_int()
    for args in ((64, 64, 1, 0, 3, 1, None, C.byref(eq)), (64, 64, 1, 0, 3, 1, us, None), (64, 64, 1, 0, 3, 0, us, C.byref(eq)),
                 (0, 64, 1, 0, 3, 1, us, C.byref(eq)), (64, 40000, 1, 0, 3, 1, us, C.byref(eq)), (64, 64, 0, 0, 3, 1, us, C.byref(eq)),
                 (64, 64, 1025, 0, 3, 1, us, C.byref(eq)), (64, 64, 1, 2, 3, 1, us, C.byref(eq)), (64, 64, 1, 0, 5, 1, us, C.byref(eq)),
                 (64, 64, 1, 1, 4, 1, us, C.byref(eq)), (64, 64, 1, 1, 11, 1, us, C.byref(eq))):
        assert L.wm_clip_pool_bench(0, *args) == wm.WM_ERR_BAD_ARG, args[:6]
    assert callable(wm.clip_pool_bench)
