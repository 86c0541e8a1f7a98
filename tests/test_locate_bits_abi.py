"""CPU tests of the wm_locate_bits surface (wm.h): the symbols are declared, exported and bound, the Python and C++ surfaces exist,
the profiling list is the parent's, a null context is refused, and wm_locate_bits_cover -- pure host arithmetic -- counts the window's
pixels per bit as tests/locate_bits_model.py does, on remainder tiles and -1 tiles, and refuses what it must (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bits_model as B
import locate_bits_model as LB
from test_locate_abi import PARENT_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_locate_bits", "wm_locate_bits_cover", "wm_locate_bits_bench")


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
    assert re.search(r"#define\s+WM_LOCATE_BITS_NVALS\s+4\b", hdr)
    assert wm.WM_LOCATE_BITS_NVALS == 4


def test_python_and_cpp_surfaces(wm):
    assert hasattr(wm.Watermark, "locate_bits") and hasattr(wm.Watermark, "locate_bits_async") and callable(wm.locate_bits_cover)
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    assert "std::vector<WmLocation> locateBits(" in hpp and "wm_locate_bits(" in hpp


def test_profiling_list_is_the_parents(L):
    names = [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())]
    assert names == PARENT_KERNELS


def test_null_context(L, wm):
    plane = wm.wm_plane(None, 64, 64, 1, wm.WM_F32, wm.WM_MEM_DEVICE, 1, 64, 0, 0)
    loc, soft = (C.c_float * 4)(), (C.c_float * 4)()
    tb = np.zeros(4, np.int32)
    assert L.wm_locate_bits(None, 0, C.byref(plane), None, 0, 32, 32, tb.ctypes.data_as(C.c_void_p), 4, loc, soft, None, None, None,
                            wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert L.wm_locate_bits(None, 0, None, None, 0, 0, 0, None, 0, None, None, None, None, None, 0) == wm.WM_ERR_BAD_ARG
    # wm_locate_bits_bench: refused before a device is chosen
    us = (C.c_double * 3)()
    for args in ((128, 128, 1, 1, 1, None), (128, 128, 1, 1, 0, us), (64, 128, 1, 1, 1, us), (128, 100, 1, 1, 1, us), (128, 128, 129, 1, 1, us),
                 (128, 128, 1, 0, 1, us), (16384, 128, 1, 1, 1, us)):
        assert L.wm_locate_bits_bench(0, *args) == wm.WM_ERR_BAD_ARG, args[:5]


# (crop shape, key shape, tile shape, bits, tiles set to -1)
COVER = [((64, 256), (120, 330), (32, 32), 8, ()), ((271, 483), (301, 523), (40, 36), 5, (3, 17)), ((64, 256), (70, 4100), (32, 32), 7, (0,)),
         ((10, 10), (70, 100), (32, 32), 3, (2,)), ((31, 33), (31, 33), (32, 32), 1, ())]


@pytest.mark.parametrize("shape,kshape,tile,nbits,holes", COVER)
def test_cover_against_numpy(wm, shape, kshape, tile, nbits, holes):
    ny, nx = LB.tiles_shape(kshape[0], kshape[1], *tile)
    assert (ny, nx) == wm.Watermark.tiles_shape(kshape[0], kshape[1], *tile)
    tb = B.layout(ny, nx, nbits, 5)
    for t in holes:
        tb[t] = -1
    offs = {(0, 0), (kshape[0] - shape[0], kshape[1] - shape[1]), ((kshape[0] - shape[0]) // 2, (kshape[1] - shape[1]) // 3)}
    for (oy, ox) in offs:
        got = wm.locate_bits_cover(shape[0], shape[1], kshape[0], kshape[1], tile[0], tile[1], tb, nbits, oy, ox)
        want = LB.cover(shape, kshape, tile[0], tile[1], tb, nbits, oy, ox)
        assert got.dtype == np.int64 and np.array_equal(got, want), (oy, ox)
        assert got.sum() == shape[0] * shape[1] - (LB.bit_plane(kshape, tile[0], tile[1], tb)[oy:oy + shape[0], ox:ox + shape[1]] < 0).sum()


def test_cover_refusals(L, wm):
    bad = wm.WM_ERR_BAD_ARG
    tb = np.array([0, 1, -1, 2, 0, 1], np.int32)  # a 70 x 100 key in 32 x 32 tiles: 2 x 3
    px = (C.c_int64 * 3)(7, 7, 7)

    def cover(rows=10, cols=10, kr=70, kc=100, th=32, tw=32, table=tb, nbits=3, oy=0, ox=0, out=px):
        return L.wm_locate_bits_cover(rows, cols, kr, kc, th, tw, table.ctypes.data_as(C.c_void_p) if table is not None else None, nbits, oy, ox, out)

    assert cover() == wm.WM_OK and list(px) == [100, 0, 0]
    assert cover(oy=60, ox=90) == wm.WM_OK and list(px) == [0, 100, 0]
    assert cover(table=None) == bad and cover(out=None) == bad
    assert cover(rows=71) == bad and cover(cols=0) == bad and cover(kc=8200) == bad          # wm_locate_shape's
    assert cover(th=30) == bad and cover(tw=34) == bad and cover(th=16) == bad                # wm_tiles_shape's
    assert cover(oy=61) == bad and cover(ox=91) == bad and cover(oy=-1) == bad and cover(ox=-1) == bad
    assert cover(nbits=0) == bad and cover(nbits=4097) == bad and cover(nbits=2) == bad       # (an entry 2 needs nbits >= 3)
    assert cover(table=np.array([0, 1, -2, 2, 0, 1], np.int32)) == bad
    with pytest.raises(RuntimeError):
        wm.locate_bits_cover(10, 10, 70, 100, 32, 32, tb[:5], 3, 0, 0)
