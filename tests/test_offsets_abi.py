"""CPU tests of the crop-search surface (wm.h wm_detect_offsets, wm_offsets_check): the symbols are exported and bound, the
Python and C++ surfaces exist, k_detect_offsets is a profiling name behind the existing ones, and every argument error comes
back before a device is touched (no GPU needed).  The rectangle test is wm_offsets_check, the function wm_detect_offsets
itself calls; tests/test_gpu_offsets.py checks the same refusals through wm_detect_offsets on a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_detect_offsets", "wm_offsets_check", "wm_detect_offsets_group")
# the profiling names the parent had, in their order: the new id goes behind them
EARLIER_KERNELS = ["k_gram", "k_me_stats", "k_nvf_stats", "k_embed", "k_detect", "k_mask", "k_fused_embed", "k_fused_detect", "k_gram_ho",
                   "k_fused_pair", "k_detect_keys", "k_gram_ho_checked", "k_gram_redo", "k_detect_redo", "k_stats_keys", "k_embed_keys_fold",
                   "k_embed_keys"]


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


def test_python_and_cpp_surfaces(wm):
    assert hasattr(wm.Watermark, "detectOffsets") and hasattr(wm.Watermark, "detect_offsets_async")
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    assert "std::vector<float> detectOffsets(" in hpp and "wm_detect_offsets(" in hpp


def test_profiling_name_appended(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names[:len(EARLIER_KERNELS)] == EARLIER_KERNELS  # existing ids keep their numbers
    assert "k_detect_offsets" in names[len(EARLIER_KERNELS):]
    assert 2 <= L.wm_detect_offsets_group() <= 4


def test_null_arguments(L, wm):
    plane = wm.wm_plane(None, 8, 8, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 8, 0, 0)
    corr = (C.c_float * 4)()
    # a null context is refused whatever else is passed (no context or bank exists without a device)
    assert L.wm_detect_offsets(None, 0, C.byref(plane), None, 0, 0, 0, 1, 1, corr, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert L.wm_detect_offsets(None, 0, None, None, 0, 0, 0, 1, 1, None, None, 0) == wm.WM_ERR_BAD_ARG


def test_rectangle_check(L, wm):
    """image 64x256 in a key plane of 80x300: row offsets 0..16, column offsets 0..44"""
    R, Cc, KR, KC = 64, 256, 80, 300
    ok, bad = wm.WM_OK, wm.WM_ERR_BAD_ARG
    chk = lambda oy0, ox0, ny, nx: L.wm_offsets_check(R, Cc, KR, KC, oy0, ox0, ny, nx)
    # the whole rectangle of admissible offsets, its corners, single offsets
    assert chk(0, 0, 17, 45) == ok
    assert chk(16, 44, 1, 1) == ok and chk(0, 44, 17, 1) == ok and chk(16, 0, 1, 45) == ok and chk(3, 5, 2, 7) == ok
    # every side violated by one
    assert chk(-1, 0, 1, 1) == bad
    assert chk(0, -1, 1, 1) == bad
    assert chk(0, 0, 18, 45) == bad and chk(17, 0, 1, 1) == bad and chk(1, 0, 17, 1) == bad
    assert chk(0, 0, 17, 46) == bad and chk(0, 45, 1, 1) == bad and chk(0, 1, 1, 45) == bad
    assert chk(0, 0, 0, 1) == bad and chk(0, 0, 1, 0) == bad and chk(0, 0, -2, 1) == bad and chk(0, 0, 1, -2) == bad
    # a key plane equal to the image admits the offset (0, 0) alone
    assert L.wm_offsets_check(R, Cc, R, Cc, 0, 0, 1, 1) == ok
    assert L.wm_offsets_check(R, Cc, R, Cc, 0, 0, 1, 2) == bad and L.wm_offsets_check(R, Cc, R, Cc, 1, 0, 1, 1) == bad
    # a key plane smaller than the image on either side
    assert L.wm_offsets_check(R, Cc, R - 1, KC, 0, 0, 1, 1) == bad and L.wm_offsets_check(R, Cc, KR, Cc - 1, 0, 0, 1, 1) == bad
    # sums that would overflow an int
    big = 2**31 - 1
    assert chk(big, 0, 1, 1) == bad and chk(0, big, 1, 1) == bad and chk(0, 0, big, 1) == bad and chk(1, 1, big, big) == bad
