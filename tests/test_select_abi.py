"""CPU tests of the key-per-frame surface (wm.h wm_key_schedule, wm_embed_select, wm_detect_select): the symbols are declared,
exported and bound with their prototypes, the Python and C++ surfaces exist with their signatures, the list of profiling names is
still the parent's (the new kernels are launched outside any profiled scope), a null context is refused and wm_key_schedule's errors
need no device.  tests/test_gpu_select.py checks the calls on a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_bits_abi import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_key_schedule", "wm_embed_select", "wm_detect_select")


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


def test_prototypes(wm):
    """the header's argument lists, and the bindings' argument counts and table types"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "wm.h")).read(), flags=re.S)
    flat = lambda s: " ".join(s.split())
    proto = {s: flat(re.search(r"int " + s + r"\((.*?)\);", hdr, re.S).group(1)) for s in SYMBOLS}
    assert proto["wm_key_schedule"] == "int nkeys, uint64_t seed, uint64_t first_frame, int frames, int32_t* key_of_frame"
    assert proto["wm_embed_select"] == ("wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, const wm_keys* keys, "
                                        "const int32_t* key_of_frame , float* a_out, int* status_out, int slot")
    assert proto["wm_detect_select"] == ("wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, const int32_t* key_of_frame , "
                                         "float* corr_out, int* status_out, int slot")
    abi = {name: (res, args) for name, res, args in wm.ABI}
    i32p, f32p, intp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert abi["wm_key_schedule"] == (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_int, i32p])
    res, args = abi["wm_embed_select"]
    assert res is C.c_int and len(args) == 10 and args[6] is i32p and args[7] is f32p and args[8] is intp and args[9] is C.c_int
    res, args = abi["wm_detect_select"]
    assert res is C.c_int and len(args) == 8 and args[4] is i32p and args[5] is f32p and args[6] is intp and args[7] is C.c_int


def test_python_signatures(wm):
    W = wm.Watermark
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(W.key_schedule) == ["nkeys", "seed", "first_frame", "frames"]
    assert isinstance(inspect.getattr_static(W, "key_schedule"), staticmethod)
    assert params(W.makeWatermarkSelect) == ["self", "inputImage", "outputImage", "keys", "key_of_frame", "maskType", "out"]
    assert params(W.detectSelect) == ["self", "image", "keys", "key_of_frame", "maskType"]
    assert params(W.embed_select_async) == ["self", "inputImage", "outputImage", "out", "keys", "key_of_frame", "maskType", "slot", "a_out", "status_out"]
    assert params(W.detect_select_async) == ["self", "image", "keys", "key_of_frame", "maskType", "slot", "corr_out", "status_out"]


def test_cpp_surface():
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for text in ("static std::vector<int32_t> keySchedule(", "std::vector<wm::Image> makeWatermarkSelect(", "std::vector<float> detectWatermarkSelect(",
                 "void makeWatermarkSelectAsync(", "void detectWatermarkSelectAsync(", "wm_key_schedule(", "wm_embed_select(", "wm_detect_select("):
        assert text in hpp, text
    selftest = open(os.path.join(ROOT, "watermarking-gpu_amd", "csrc", "app", "wm_selftest.cpp")).read()
    for text in ("keySchedule(", "makeWatermarkSelect(", "detectWatermarkSelectAsync(", "WM_MEM_SLOT_OUT"):
        assert text in selftest, text


def test_build_lists_the_new_file():
    mk = open(os.path.join(ROOT, "watermarking-gpu_amd", "csrc", "Makefile")).read()
    assert "wm_k_select.hip" in mk and "wm_stats_march.hpp" in mk
    assert '"wm_k_select.hip"' in open(os.path.join(ROOT, "tools", "resource_usage.py")).read()


def test_profiling_names_unchanged(L):
    assert len(KERNELS) == 20
    assert [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())] == KERNELS


def test_null_context(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    pp = C.byref(plane)
    kt = np.zeros(1, np.int32)
    pk = kt.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.wm_embed_select(None, 0, pp, pp, pp, None, pk, None, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_detect_select(None, 0, pp, None, pk, None, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_embed_select(None, 0, None, None, None, None, None, None, None, 0) == bad
    assert L.wm_detect_select(None, 0, None, None, None, None, None, 0) == bad


def test_key_schedule_errors_need_no_device(L, wm):
    out = np.full(3, -1, np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    bad = wm.WM_ERR_BAD_ARG
    for nkeys, frames, ptr in ((0, 3, p), (-1, 3, p), (4097, 3, p), (2, 0, p), (2, -1, p), (2, 3, None)):
        assert L.wm_key_schedule(nkeys, 5, 0, frames, ptr) == bad, (nkeys, frames)
    assert np.all(out == -1)
    assert L.wm_key_schedule(2, 5, 0, 3, p) == wm.WM_OK and set(out.tolist()) <= {0, 1}
