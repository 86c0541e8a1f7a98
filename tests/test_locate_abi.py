"""CPU tests of the locate surface (wm.h wm_locate, wm_locate_shape, wm_fft2): the symbols are declared, exported and bound, the
Python and C++ surfaces exist, the profiling list is the parent's (the new kernels are not in it), null arguments are refused, and
wm_locate_shape -- pure host arithmetic, the function wm_locate itself calls -- gives the admissible offsets and the padded
transform and refuses what it must (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_locate", "wm_locate_shape", "wm_fft2", "wm_fft_bench")
PARENT_KERNELS = ["k_gram", "k_me_stats", "k_nvf_stats", "k_embed", "k_detect", "k_mask", "k_fused_embed", "k_fused_detect", "k_gram_ho",
                  "k_fused_pair", "k_detect_keys", "k_gram_ho_checked", "k_gram_redo", "k_detect_redo", "k_stats_keys", "k_embed_keys_fold",
                  "k_embed_keys", "k_detect_offsets", "k_detect_tiles", "k_tiles_fold"]


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
    assert re.search(r"#define\s+WM_LOCATE_NVALS\s+4\b", hdr)
    assert wm.WM_LOCATE_NVALS == 4


def test_python_and_cpp_surfaces(wm):
    assert hasattr(wm.Watermark, "locate") and hasattr(wm.Watermark, "locate_async")
    assert callable(wm.fft2) and callable(wm.locate_shape)
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    assert "std::vector<WmLocation> locate(" in hpp and "wm_locate(" in hpp and "struct WmLocation" in hpp


def test_profiling_list_is_the_parents(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names == PARENT_KERNELS


def test_null_arguments(L, wm):
    plane = wm.wm_plane(None, 8, 8, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 8, 0, 0)
    loc = (C.c_float * 4)()
    bad = wm.WM_ERR_BAD_ARG
    # a null context is refused whatever else is passed (no context or bank exists without a device)
    assert L.wm_locate(None, 0, C.byref(plane), None, 0, loc, None, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_locate(None, 0, None, None, 0, None, None, None, 0) == bad
    # wm_fft2: a null plane, and lengths that are no power of two in 64 .. 8192 (refused before a device is chosen)
    assert L.wm_fft2(0, None, 64, 64, 0) == bad
    one = C.c_void_p(16)
    for pr, pc in ((32, 64), (64, 32), (96, 64), (64, 100), (16384, 64), (64, 16384), (0, 64), (-64, 64)):
        assert L.wm_fft2(0, one, pr, pc, 0) == bad, (pr, pc)
    us = (C.c_double * 7)()
    assert L.wm_fft_bench(0, 64, 64, 1, None) == bad and L.wm_fft_bench(0, 64, 64, 0, us) == bad and L.wm_fft_bench(0, 64, 100, 1, us) == bad
    v = [C.c_int() for _ in range(4)]
    for hole in range(4):
        args = [C.byref(x) for x in v]
        args[hole] = None
        assert L.wm_locate_shape(64, 256, 80, 300, *args) == bad


def test_locate_shape(L, wm):
    ok, bad = wm.WM_OK, wm.WM_ERR_BAD_ARG

    def shape(r, c, kr, kc):
        v = [C.c_int(-7) for _ in range(4)]
        rc = L.wm_locate_shape(r, c, kr, kc, *[C.byref(x) for x in v])
        return rc, tuple(x.value for x in v)

    assert shape(64, 256, 80, 300) == (ok, (17, 45, 128, 512))
    assert wm.locate_shape(64, 256, 80, 300) == (17, 45, 128, 512)
    # a key equal to the image admits one offset; small keys are padded to 64
    assert shape(64, 256, 64, 256) == (ok, (1, 1, 64, 256))
    assert shape(8, 8, 8, 8) == (ok, (1, 1, 64, 64))
    assert shape(8, 8, 65, 64) == (ok, (58, 57, 128, 64))
    # the largest transform: 8192 per axis passes, 8193 needs 16384
    assert shape(64, 256, 80, 8192) == (ok, (17, 7937, 128, 8192))
    assert shape(64, 256, 8192, 300) == (ok, (8129, 45, 8192, 512))
    assert shape(64, 256, 80, 8193)[0] == bad and shape(64, 256, 8193, 300)[0] == bad
    # a key smaller than the image on either side, empty images
    assert shape(64, 256, 63, 300)[0] == bad and shape(64, 256, 80, 255)[0] == bad
    assert shape(0, 256, 80, 300)[0] == bad and shape(64, 0, 80, 300)[0] == bad and shape(-1, -1, 80, 300)[0] == bad
    # sizes whose sums or next power of two would overflow an int
    big = 2**31 - 1
    assert shape(64, 256, big, 300)[0] == bad and shape(64, 256, 80, big)[0] == bad and shape(big, big, big, big)[0] == bad
    with pytest.raises(RuntimeError):
        wm.locate_shape(64, 256, 63, 300)
