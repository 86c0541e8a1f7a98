"""CPU tests of the payload surface (wm.h wm_bits_layout, wm_embed_signs, wm_embed_bits, wm_detect_bits): the symbols are
declared, exported and bound, the Python and C++ surfaces exist, the list of profiling names is the parent's, wm_bits_layout
against the plain-Python restatement (tests/bits_model.py) and three literal tables, its balance and its refusals, and a null
context is refused (no GPU needed).  tests/test_gpu_bits.py checks the calls on a device."""
import ctypes as C
import os

import numpy as np
import pytest

import bits_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_bits_layout", "wm_embed_signs", "wm_embed_bits", "wm_detect_bits")
# the profiling names of the parent, in their order: k_embed_signs and k_bits_fold are launched outside any profiled scope
KERNELS = ["k_gram", "k_me_stats", "k_nvf_stats", "k_embed", "k_detect", "k_mask", "k_fused_embed", "k_fused_detect", "k_gram_ho",
           "k_fused_pair", "k_detect_keys", "k_gram_ho_checked", "k_gram_redo", "k_detect_redo", "k_stats_keys", "k_embed_keys_fold",
           "k_embed_keys", "k_detect_offsets", "k_detect_tiles", "k_tiles_fold"]


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
    for name in ("bits_layout", "makeWatermarkSigns", "makeWatermarkBits", "detectBits", "embed_signs_async", "embed_bits_async",
                 "detect_bits_async"):
        assert hasattr(wm.Watermark, name), name
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for text in ("static std::vector<int32_t> bitsLayout(", "wm::Image makeWatermarkSigns(", "wm::Image makeWatermarkBits(",
                 "std::vector<float> detectBits(", "wm_bits_layout(", "wm_embed_signs(", "wm_embed_bits(", "wm_detect_bits("):
        assert text in hpp, text


def test_profiling_names_unchanged(L):
    assert [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())] == KERNELS


def layout(L, ny, nx, nbits, seed):
    tb = np.full(max(ny * nx, 1), -7, np.int32)
    rc = L.wm_bits_layout(ny, nx, nbits, seed, tb.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, tb


def test_generator_first_output():
    assert BM.splitmix64(0)[1] == 16294208416658607535


def test_layout_literal_tables(L, wm):
    assert list(layout(L, 2, 4, 3, 1)[1]) == [1, 0, 2, 1, 2, 0, 0, 1]
    assert list(layout(L, 2, 8, 16, 12345)[1]) == [1, 4, 8, 9, 11, 13, 15, 7, 14, 6, 10, 3, 2, 5, 12, 0]
    assert list(layout(L, 8, 15, 48, 12345)[1][:16]) == [16, 20, 41, 11, 42, 22, 27, 40, 19, 23, 37, 0, 9, 16, 10, 47]
    assert list(wm.Watermark.bits_layout(2, 4, 3, 1)) == [1, 0, 2, 1, 2, 0, 0, 1]


TABLE = [(1, 1, 1, 0), (2, 4, 3, 1), (2, 8, 16, 12345), (8, 15, 48, 12345), (8, 15, 24, 12345), (6, 13, 32, 12345), (16, 29, 64, 12345),
         (1, 7, 7, 2 ** 64 - 1), (7, 1, 2, 2 ** 63), (67, 120, 4096, 3), (67, 120, 1, 99), (64, 64, 4096, 0xDEADBEEFCAFEF00D)]


@pytest.mark.parametrize("ny,nx,nbits,seed", TABLE)
def test_layout_equals_restatement_and_is_balanced(L, ny, nx, nbits, seed):
    rc, tb = layout(L, ny, nx, nbits, seed)
    assert rc == 0
    assert np.array_equal(tb, BM.layout(ny, nx, nbits, seed))
    T = ny * nx
    counts = np.bincount(tb, minlength=nbits)
    assert len(counts) == nbits and counts.min() >= T // nbits and counts.max() <= -(-T // nbits)


def test_layout_refusals(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    ny, nx = 4, 6
    T = ny * nx
    assert layout(L, ny, nx, 0, 1)[0] == bad
    assert layout(L, ny, nx, T + 1, 1)[0] == bad
    assert layout(L, ny, nx, -1, 1)[0] == bad
    assert layout(L, 67, 120, 4097, 1)[0] == bad  # (T = 8040 tiles: the cap of 4096 bits, not T, refuses)
    assert layout(L, 0, nx, 1, 1)[0] == bad and layout(L, ny, 0, 1, 1)[0] == bad and layout(L, -1, nx, 1, 1)[0] == bad
    assert L.wm_bits_layout(ny, nx, 3, 1, None) == bad
    rc, tb = layout(L, ny, nx, T, 1)  # (the neighbour that is allowed: one tile per bit)
    assert rc == wm.WM_OK and sorted(tb) == list(range(T))
    with pytest.raises(RuntimeError):
        wm.Watermark.bits_layout(ny, nx, T + 1, 1)


def test_null_context(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    pp = C.byref(plane)
    signs = np.ones(4, np.int8)
    tb = np.zeros(4, np.int32)
    pay = np.zeros(1, np.uint8)
    soft = (C.c_float * 1)()
    assert L.wm_embed_signs(None, 0, pp, pp, pp, 32, 32, signs.ctypes.data_as(C.c_void_p), None, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_embed_bits(None, 0, pp, pp, pp, 32, 32, tb.ctypes.data_as(C.c_void_p), 1, pay.ctypes.data_as(C.c_void_p), None, None, 0) == bad
    assert L.wm_detect_bits(None, 0, pp, 32, 32, tb.ctypes.data_as(C.c_void_p), 1, soft, None, wm.WM_SLOT_SYNC) == bad
    assert L.wm_embed_signs(None, 0, None, None, None, 32, 32, None, None, None, 0) == bad
