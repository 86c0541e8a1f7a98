"""CPU tests of the per-key tile-map surface (wm.h wm_detect_keys_tiles): the symbol is declared, exported and bound, the Python
and C++ surfaces exist, the profiling names are exactly the earlier ones (the two new kernels are launched outside any profiling
scope), and a null context is refused (no GPU needed).  tests/test_gpu_keys_tiles.py checks the other refusals on a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_gram", "k_me_stats", "k_nvf_stats", "k_embed", "k_detect", "k_mask", "k_fused_embed", "k_fused_detect", "k_gram_ho",
           "k_fused_pair", "k_detect_keys", "k_gram_ho_checked", "k_gram_redo", "k_detect_redo", "k_stats_keys", "k_embed_keys_fold",
           "k_embed_keys", "k_detect_offsets", "k_detect_tiles", "k_tiles_fold"]


@pytest.fixture(scope="module")
def L(wm):
    return wm.lib()


def test_symbol_declared_exported_and_bound(L, wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert "int wm_detect_keys_tiles(" in hdr
    assert hasattr(L, "wm_detect_keys_tiles")
    entry = [e for e in wm.ABI if e[0] == "wm_detect_keys_tiles"]
    assert len(entry) == 1 and len(entry[0][2]) == 10  # ctx, mask, img, keys, tile_rows, tile_cols, map, sums, status, slot
    # wm.h states both notes the call inherits: the bank hazard of wm_detect_keys and the first-call reallocation of wm_detect_tiles
    doc = hdr[hdr.index("Tile map per key"):hdr.index("int wm_detect_keys_tiles(")]
    assert "HAZARD" in doc and "ALIVE and UNMODIFIED" in doc
    assert "reallocates" in doc and "waits for the whole" in doc and "WM_ERR_ALLOC" in doc


def test_python_and_cpp_surfaces(wm):
    for name in ("detectKeysTiles", "detect_keys_tiles_async"):
        assert hasattr(wm.Watermark, name), name
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    assert "std::vector<float> detectKeysTiles(" in hpp and "wm_detect_keys_tiles(" in hpp


def test_profiling_names_unchanged(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names == KERNELS


def test_kernel_file_is_built(wm):
    mk = open(os.path.join(ROOT, "watermarking-gpu_amd", "csrc", "Makefile")).read()
    assert "wm_k_detect_keys_tiles.hip" in mk and "wm_keys_march.hpp" in mk


def test_null_context(L, wm):
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    assert L.wm_detect_keys_tiles(None, 0, C.byref(plane), None, 32, 32, None, None, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert L.wm_detect_keys_tiles(None, 0, None, None, 32, 32, None, None, None, 0) == wm.WM_ERR_BAD_ARG
