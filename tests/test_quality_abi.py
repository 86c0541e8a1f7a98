"""CPU tests of the quality call (wm.h wm_quality, wm_psnr_from_mse): the symbols are declared, exported and bound, the two constants
have their values, wm_psnr_from_mse is the documented host arithmetic, the Python and C++ surfaces exist, the list of profiling names
is still the parent's (the three kernels are launched outside any profiled scope), and a call without a context or planes is refused
(no GPU needed: nothing here reaches a device).  tests/test_gpu_quality.py checks the call on a device, tests/test_quality_model.py
the model that decides it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from test_bits_abi import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(wm):
    return wm.lib()


def test_symbols_declared_exported_and_bound(L, wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    bound = {name for name, _, _ in wm.ABI}
    assert "int wm_quality(wm_ctx* ctx, const wm_plane* ref, const wm_plane* test, int tile_rows, int tile_cols," in hdr
    assert "double wm_psnr_from_mse(double mse, double peak);" in hdr
    for s in ("wm_quality", "wm_psnr_from_mse"):
        assert hasattr(L, s), s
        assert s in bound, s


def test_constants(wm):
    hdr = open(os.path.join(ROOT, "include", "wm.h")).read()
    assert re.search(r"#define WM_QUALITY_NVALS 3\b", hdr) and re.search(r"#define WM_QUALITY_NSUMS 5\b", hdr)
    assert (wm.WM_QUALITY_NVALS, wm.WM_QUALITY_NSUMS) == (3, 5)


def test_psnr_from_mse(L, wm):
    assert L.wm_psnr_from_mse(100.0, 255.0) == pytest.approx(28.130803608679, abs=1e-11)
    assert L.wm_psnr_from_mse(100.0, 255.0) == 10.0 * math.log10(255.0 * 255.0 / 100.0)
    assert L.wm_psnr_from_mse(0.0, 255.0) == float("inf")
    for mse, peak in ((-1.0, 255.0), (float("nan"), 255.0), (1.0, 0.0), (1.0, -255.0), (1.0, float("nan")), (0.0, 0.0)):
        assert math.isnan(L.wm_psnr_from_mse(mse, peak)), (mse, peak)
    # a 10-bit plane: peak 1023 on the samples is peak 255 on the scaled plane
    assert L.wm_psnr_from_mse(16.0, 1023.0) == pytest.approx(L.wm_psnr_from_mse(16.0 * (255.0 / 1023.0) ** 2, 255.0), abs=1e-12)
    assert wm.psnr_from_mse(100.0) == L.wm_psnr_from_mse(100.0, 255.0) and wm.psnr_from_mse(4.0, 1023.0) == L.wm_psnr_from_mse(4.0, 1023.0)


def test_python_and_cpp_surfaces(wm):
    for name in ("quality", "quality_async"):
        assert hasattr(wm.Watermark, name), name
    assert hasattr(wm, "psnr_from_mse") and hasattr(wm, "plane_u8f32")
    hpp = open(os.path.join(ROOT, "include", "Watermark.hpp")).read()
    for text in ("struct Quality { float mse, psnr, ssim, maxAbs; };",
                 "std::vector<wm::Quality> quality(const wm::Image& ref, const wm::Image& test) const", "wm_quality(", "wm_psnr_from_mse("):
        assert text in hpp, text
    assert "wm1.quality(" in open(os.path.join(ROOT, "watermarking-gpu_amd", "csrc", "app", "wm_selftest.cpp")).read()
    assert "report_quality" in open(os.path.join(ROOT, "watermarking-gpu_amd", "csrc", "app", "wm_app.cpp")).read()
    # the kernels' file is built and is in the register check's list
    assert "wm_k_quality.hip" in open(os.path.join(ROOT, "watermarking-gpu_amd", "csrc", "Makefile")).read()
    assert '"wm_k_quality.hip"' in open(os.path.join(ROOT, "tools", "resource_usage.py")).read()


def test_plane_u8f32_describes_host_arrays(wm):
    import torch
    a = np.zeros((2, 5, 8), np.uint8)[:, :, :7]
    p = wm.plane_u8f32(a)
    assert (p.rows, p.cols, p.channels, p.dtype, p.mem, p.frames, p.pitch, p.frame_stride, p.data) == (5, 7, 1, wm.WM_U8, wm.WM_MEM_HOST, 2, 8, 40, a.ctypes.data)
    t = torch.zeros((3, 5, 8), dtype=torch.float32)
    p = wm.plane_u8f32(t, 3)
    assert (p.channels, p.dtype, p.mem, p.frames, p.channel_stride, p.data) == (3, wm.WM_F32, wm.WM_MEM_HOST, 1, 40, t.data_ptr())
    with pytest.raises(RuntimeError):
        wm.plane_u8f32(np.zeros((5, 8), np.uint16))
    with pytest.raises(RuntimeError):
        wm.plane_u8f32(np.zeros((5, 8), np.float32)[:, ::2])


def test_profiling_names_unchanged(L):
    assert len(KERNELS) == 20
    assert [L.wm_prof_kernel_name(i).decode() for i in range(L.wm_prof_kernel_count())] == KERNELS


def test_refused_without_a_context_or_planes(L, wm):
    """a null context, whatever else the call carries, and null planes: WM_ERR_BAD_ARG, no device touched"""
    bad = wm.WM_ERR_BAD_ARG
    buf = np.zeros(64 * 64 * 4, np.uint8)
    p8 = wm.wm_plane(buf.ctypes.data, 64, 64, 1, wm.WM_U8, wm.WM_MEM_HOST, 1, 64, 0, 0)
    p32 = wm.wm_plane(buf.ctypes.data, 64, 64, 1, wm.WM_F32, wm.WM_MEM_HOST, 1, 64, 0, 0)
    q = (C.c_float * 3)()
    for slot in (wm.WM_SLOT_SYNC, 0):
        for tile in (0, 32):
            assert L.wm_quality(None, C.byref(p8), C.byref(p32), tile, tile, q, None, slot) == bad
        assert L.wm_quality(None, None, None, 0, 0, q, None, slot) == bad
        assert L.wm_quality(None, None, None, 0, 0, None, None, slot) == bad
    assert list(q) == [0.0, 0.0, 0.0]
