"""CPU tests of the tile-map surface (wm.h wm_detect_tiles, wm_tiles_shape): the symbols are declared, exported and bound, the
Python and C++ surfaces exist, k_detect_tiles and k_tiles_fold are profiling names behind the existing ones, wm_tiles_shape over a
table with every refusal off by one, and a null context is refused (no GPU needed).  tests/test_gpu_tiles.py checks the
refusals through wm_detect_tiles on a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_detect_tiles", "wm_tiles_shape")
# the profiling names the parent had, in their order: the new ids go behind them
EARLIER_KERNELS = ["k_gram", "k_me_stats", "k_nvf_stats", "k_embed", "k_detect", "k_mask", "k_fused_embed", "k_fused_detect", "k_gram_ho",
                   "k_fused_pair", "k_detect_keys", "k_gram_ho_checked", "k_gram_redo", "k_detect_redo", "k_stats_keys", "k_embed_keys_fold",
                   "k_embed_keys", "k_detect_offsets"]


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
    for name in ("tiles_shape", "detectTiles", "detect_tiles_async"):
        assert hasattr(wm.Watermark, name), name
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    assert "std::vector<float> detectTiles(" in hpp and "wm_detect_tiles(" in hpp and "wm_tiles_shape(" in hpp


def test_profiling_names_appended(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names[:len(EARLIER_KERNELS)] == EARLIER_KERNELS  # existing ids keep their numbers
    assert names[len(EARLIER_KERNELS):] == ["k_detect_tiles", "k_tiles_fold"]


def shape(L, rows, cols, th, tw):
    ny, nx = C.c_int(-7), C.c_int(-7)
    rc = L.wm_tiles_shape(rows, cols, th, tw, C.byref(ny), C.byref(nx))
    return rc, ny.value, nx.value


def test_tiles_shape_table(L, wm):
    ok = wm.WM_OK
    assert shape(L, 270, 480, 32, 64) == (ok, 8, 7)
    assert shape(L, 1080, 1920, 128, 128) == (ok, 8, 15)
    assert shape(L, 2160, 3840, 32, 32) == (ok, 67, 120)  # 8040 scores
    assert shape(L, 2160, 3840, 128, 128) == (ok, 16, 30)
    # a tile larger than the plane on either axis or both
    assert shape(L, 270, 480, 512, 512) == (ok, 1, 1)
    assert shape(L, 270, 480, 272, 64) == (ok, 1, 7)
    assert shape(L, 270, 480, 32, 484) == (ok, 8, 1)
    # exact fits and one pixel less
    assert shape(L, 64, 256, 32, 32) == (ok, 2, 8)
    assert shape(L, 63, 255, 32, 32) == (ok, 1, 7)
    # the smallest and the largest planes
    assert shape(L, 1, 1, 32, 32) == (ok, 1, 1)
    assert shape(L, 32768, 32768, 32, 32) == (ok, 1024, 1024)
    assert wm.Watermark.tiles_shape(1078, 1918, 64, 128) == (16, 14)


def test_tiles_shape_refusals(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    R, Cc = 270, 480
    # tile rows: a multiple of 8, >= 32; tile columns: a multiple of 4, >= 32 -- every rule off by one
    for th in (24, 36, 31, 33, 28, 0, -32, 8, 16):
        assert shape(L, R, Cc, th, 32)[0] == bad, th
    for tw in (28, 34, 31, 33, 30, 0, -32, 4, 16):
        assert shape(L, R, Cc, 32, tw)[0] == bad, tw
    assert shape(L, R, Cc, 40, 36)[0] == wm.WM_OK  # (the neighbours that are allowed)
    # plane sizes 1 .. 32768
    for rows, cols in ((0, Cc), (R, 0), (-1, Cc), (R, -1), (32769, Cc), (R, 32769)):
        assert shape(L, rows, cols, 32, 32)[0] == bad, (rows, cols)
    # null outputs
    n = C.c_int()
    assert L.wm_tiles_shape(R, Cc, 32, 32, None, C.byref(n)) == bad
    assert L.wm_tiles_shape(R, Cc, 32, 32, C.byref(n), None) == bad
    with pytest.raises(RuntimeError):
        wm.Watermark.tiles_shape(R, Cc, 24, 32)


def test_null_context(L, wm):
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    assert L.wm_detect_tiles(None, 0, C.byref(plane), 32, 32, None, None, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert L.wm_detect_tiles(None, 0, None, 32, 32, None, None, None, 0) == wm.WM_ERR_BAD_ARG
