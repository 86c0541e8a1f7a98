"""CPU tests of the wm_locate_keys surface (wm.h): the symbols are declared, exported and bound, the Python and C++ surfaces exist, the
profiling list is the parent's, a null context is refused, wm_locate_keys_bench refuses what it must before a device is chosen, and
wm_locate_keys_rank -- pure host arithmetic -- ranks as tests/locate_keys_model.py does: exhaustively over every arrangement of a few
z values (ties, NaN entries, all NaN, nk = 1), and refuses null pointers and nk < 1 (no GPU needed)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import locate_keys_model as LK
from test_locate_abi import PARENT_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_locate_keys", "wm_locate_keys_rank", "wm_locate_keys_bench")


@pytest.fixture(scope="module")
def L(wm):
    return wm.lib()


def test_symbols_declared_exported_and_bound(L, wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    bound = {name for name, _, _ in wm.ABI}
    for s in SYMBOLS:
        assert s + "(" in hdr, s
        assert hasattr(L, s), s
        assert s in bound, s
    assert re.search(r"#define\s+WM_LOCATE_KEYS_NVALS\s+4\b", hdr) and re.search(r"#define\s+WM_LOCATE_KEYS_BENCH_PASSES\s+2\b", hdr)
    assert wm.WM_LOCATE_KEYS_NVALS == 4 and len(wm.LOCATE_KEYS_BENCH_PASSES) == 2


def test_python_and_cpp_surfaces(wm):
    assert hasattr(wm.Watermark, "locateKeys") and hasattr(wm.Watermark, "locate_keys_async")
    assert callable(wm.locate_keys_rank) and callable(wm.locate_keys_bench)
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    assert "std::vector<WmLocation> locateKeys(" in hpp and "wm_locate_keys(" in hpp


def test_profiling_list_is_the_parents(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names == PARENT_KERNELS


def test_null_context_and_bench_refusals(L, wm):
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    loc = (C.c_float * 8)()
    assert L.wm_locate_keys(None, 0, C.byref(plane), None, 0, 2, loc, None, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert L.wm_locate_keys(None, 0, None, None, 0, 0, None, None, None, 0) == wm.WM_ERR_BAD_ARG
    # wm_locate_keys_bench: refused before a device is chosen
    us = (C.c_double * 2)()
    for args in ((128, 128, 1, 1, 1, None), (128, 128, 1, 1, 0, us), (64, 128, 1, 1, 1, us), (128, 100, 1, 1, 1, us), (128, 128, 129, 1, 1, us),
                 (128, 128, 1, 0, 1, us), (128, 128, 1, 129, 1, us), (16384, 128, 1, 1, 1, us)):
        assert L.wm_locate_keys_bench(0, *args) == wm.WM_ERR_BAD_ARG, args[:5]


def same(a, b):
    return a[0] == b[0] and all((np.isnan(x) and np.isnan(y)) or x == y for x, y in zip(a[1:], b[1:]))


def test_rank_exhaustively(wm):
    """every arrangement of nk = 1 .. 4 values out of {NaN, -2, 0, 3, +inf}, repeats included: ties, NaN entries and all NaN among them"""
    nan = float("nan")
    values = (nan, -2.0, 0.0, 3.0, float("inf"))
    count = 0
    for nk in (1, 2, 3, 4):
        for zs in itertools.product(values, repeat=nk):
            loc = np.array([[5, 6, 7, z] for z in zs], np.float32)
            got, want = wm.locate_keys_rank(loc), LK.rank(loc)
            assert same(got, want), (zs, got, want)
            count += 1
    assert count == 5 + 25 + 125 + 625
    assert same(wm.locate_keys_rank(np.array([[0, 0, 0, 7.0], [0, 0, 0, 7.0], [0, 0, 0, 3.0]])), (0, 7.0, 7.0))  # ties: the smallest index
    assert same(wm.locate_keys_rank(np.array([[0, 0, 0, nan], [0, 0, 0, 2.0], [0, 0, 0, nan]])), (1, 2.0, nan))
    assert same(wm.locate_keys_rank(np.array([[0, 0, 0, nan], [0, 0, 0, nan]])), (-1, nan, nan))
    assert same(wm.locate_keys_rank(np.array([[0, 0, 0, 4.0]])), (0, 4.0, nan))
    # the other three values of a record do not matter, NaN among them
    assert same(wm.locate_keys_rank(np.array([[nan, nan, nan, 1.0], [9, 9, 99.0, 2.0]])), (1, 2.0, 1.0))


def test_rank_refusals(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    loc = (C.c_float * 8)(0, 0, 0, 1, 0, 0, 0, 2)
    best, zb, zn = C.c_int(7), C.c_float(7), C.c_float(7)
    assert L.wm_locate_keys_rank(loc, 2, C.byref(best), C.byref(zb), C.byref(zn)) == wm.WM_OK and (best.value, zb.value, zn.value) == (1, 2.0, 1.0)
    assert L.wm_locate_keys_rank(None, 2, C.byref(best), C.byref(zb), C.byref(zn)) == bad
    assert L.wm_locate_keys_rank(loc, 2, None, C.byref(zb), C.byref(zn)) == bad
    assert L.wm_locate_keys_rank(loc, 2, C.byref(best), None, C.byref(zn)) == bad
    assert L.wm_locate_keys_rank(loc, 2, C.byref(best), C.byref(zb), None) == bad
    assert L.wm_locate_keys_rank(loc, 0, C.byref(best), C.byref(zb), C.byref(zn)) == bad
    assert L.wm_locate_keys_rank(loc, -1, C.byref(best), C.byref(zb), C.byref(zn)) == bad
    with pytest.raises(RuntimeError):
        wm.locate_keys_rank(np.zeros((2, 3), np.float32))
