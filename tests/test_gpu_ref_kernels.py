"""The HIP kernels against the reference's own kernel code, with no oracle in between: nvf.hpp, scaled_neighbors_p3.hpp
and me_p3.hpp built by oracle/build_ref.py with the reference's options (-cl-mad-enable) and run on the CPU
(tests/ref_lib.py).  Needs only oracle/_ref (never the reference tree); the last test needs neither and holds the HIP NVF
mask to the committed outputs of the same kernels (tests/golden/ref_kernels.npz).

  NVF mask      bit-exact against nvf.hpp, p = 3..9, f32 and u8, one-image (fused) and batched sweeps
  ME            e = x - scaled_neighbors_p3(x, the engine's coefficients) bit-exact, mask = |e| / max|e|
  Gram          wm_gram's 44 exact sums against the f64 fold of the me kernel's work-group sums, within the stated bound
  NVF embed     y = clamp(x + a * mask_ref * W) within 1e-3
"""
import os

import numpy as np
import pytest

import ref_lib as R
from conftest import GOLDEN
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

SMALL = [(7, 9), (16, 16), (17, 33), (31, 200), (64, 64)]
WIDE = [(70, 256), (70, 257), (70, 1918), (40, 3838)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture
def need_ref():
    if not R.available():
        pytest.skip("oracle/_ref is not built (python oracle/build_ref.py with a reference checkout)")


@pytest.fixture(params=["fused", "sweeps"])
def path(request, monkeypatch):
    """the one-image calls on the fused single-launch kernels and on the batched sweeps (WM_FUSED, read at engine creation)"""
    monkeypatch.setenv("WM_FUSED", "1" if request.param == "fused" else "0")
    return request.param


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frame(shape, dtype, k=0):
    return synth_frame(shape[0], shape[1], frame=k, dtype=np.uint8 if dtype == "u8" else np.float32)


def bits_equal(got, ref, what):
    bad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {ref.size} differ, max {np.nanmax(np.abs(got - ref)):.3g}"


@pytest.mark.parametrize("p", [3, 5, 7, 9])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_nvf_mask_vs_reference_kernel(need_ref, wm, torch_cuda, path, p, dtype):
    torch = torch_cuda
    for shape in SMALL + WIDE:
        x = frame(shape, dtype, k=p)
        eng = wm.Watermark(shape[0], shape[1], synth_watermark(*shape), p, 40.0)
        m, _, _, _ = eng.computeMask(dev(torch, x), wm.MASK_TYPE.NVF)
        bits_equal(m.cpu().numpy(), R.nvf(x.astype(np.float32), p, R.MAD), f"{path} {shape} {dtype} p={p}")


@pytest.mark.parametrize("p", [3, 9])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_nvf_mask_batched_vs_reference_kernel(need_ref, wm, torch_cuda, p, dtype):
    """three frames per call through the batched sweeps"""
    torch = torch_cuda
    F = 3
    for shape in [(31, 200), (70, 257), (70, 1918)]:
        xs = np.stack([frame(shape, dtype, k=f) for f in range(F)])
        eng = wm.Watermark(shape[0], shape[1], synth_watermark(*shape), p, 40.0, nslots=1, max_frames=F)
        m, _, _, _ = eng.computeMask(dev(torch, xs), wm.MASK_TYPE.NVF)
        m = m.cpu().numpy()
        for f in range(F):
            bits_equal(m[f], R.nvf(xs[f].astype(np.float32), p, R.MAD), f"batch {shape} {dtype} p={p} frame {f}")


def test_nvf_mask_1080p_vs_reference_kernel(need_ref, wm, torch_cuda):
    torch = torch_cuda
    shape = (1080, 1920)
    x = frame(shape, "u8", k=5)
    eng = wm.Watermark(shape[0], shape[1], synth_watermark(*shape), 3, 40.0)
    m, _, _, _ = eng.computeMask(dev(torch, x), wm.MASK_TYPE.NVF)
    bits_equal(m.cpu().numpy(), R.nvf(x.astype(np.float32), 3, R.MAD), "1080p")


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_me_error_sequence_vs_reference_kernel(need_ref, wm, torch_cuda, path, dtype):
    torch = torch_cuda
    for shape in [(16, 16), (31, 200), (64, 64)] + WIDE:
        x = frame(shape, dtype, k=2)
        xf = x.astype(np.float32)
        eng = wm.Watermark(shape[0], shape[1], synth_watermark(*shape), 3, 40.0)
        m, e, c, st = eng.computeMask(dev(torch, x), wm.MASK_TYPE.ME, want_error_sequence=True)
        assert st == 0, shape
        e_ref = xf - R.scaled_neighbors(xf, c, R.MAD)  # Watermark.cpp:210
        bits_equal(e.cpu().numpy(), e_ref, f"{path} e {shape} {dtype}")
        ae = np.abs(e_ref)
        bits_equal(m.cpu().numpy(), ae / ae.max(), f"{path} mask {shape} {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_gram_vs_reference_kernel(need_ref, wm, torch_cuda, dtype):
    """wm_gram sums exact products in f64; me_p3.hpp rounds every product to half (unit roundoff 2^-11) and sums 64 lanes
    in f32 (at most 63 additions: gamma_63 = 63 u / (1 - 63 u), u = 2^-24); the fold of its work-group sums is done here
    in f64 (exact to ~1e-16 relative).  Pixels are >= 0, so every product is, and the stated bound per sum is
    S * (2^-11 + gamma_63 * (1 + 2^-11)) + 1e-12 * S + n * 2^-25 with S = the exact sum and n products (2^-25: half's
    subnormal spacing / 2); anything more is a wrong tap, lane or sum"""
    torch = torch_cuda
    u = 2.0 ** -24
    g63 = 63 * u / (1 - 63 * u)
    for shape in [(7, 9), (17, 33), (64, 64), (5, 63), (5, 65), (70, 129), (70, 257), (70, 1918)]:
        x = frame(shape, dtype, k=4)
        eng = wm.Watermark(shape[0], shape[1], synth_watermark(*shape), 3, 40.0)
        got = eng.gram_totals(dev(torch, x))[:44]
        ref = R.gram_partials(x.astype(np.float32), R.MAD).astype(np.float64).sum(axis=0)
        bound = got * (2.0 ** -11 + g63 * (1 + 2.0 ** -11)) + 1e-12 * got + x.size * 2.0 ** -25
        assert np.all(np.abs(got - ref) <= bound), (shape, dtype, np.abs(got - ref) / np.maximum(got, 1e-30))
        assert np.all(got >= 0)


@pytest.mark.parametrize("p", [3, 5, 9])
def test_nvf_embed_vs_reference_kernel(need_ref, wm, torch_cuda, path, p):
    torch = torch_cuda
    for shape in [(31, 200), (70, 257), (70, 1918)]:
        x = frame(shape, "f32", k=1)
        W = synth_watermark(*shape)
        eng = wm.Watermark(shape[0], shape[1], W, p, 40.0)
        y, a = eng.makeWatermark(dev(torch, x), dev(torch, x), wm.MASK_TYPE.NVF)
        m = R.nvf(x, p, R.MAD).astype(np.float64)
        y_ref = np.clip(x + a * (m * W), 0, 255)
        np.testing.assert_allclose(y.cpu().numpy(), y_ref, rtol=0, atol=1e-3, err_msg=f"{path} {shape} p={p}")


def test_nvf_mask_vs_committed_reference_outputs(wm, torch_cuda, path):
    """without oracle/_ref: the HIP NVF mask against the nvf.hpp outputs recorded in tests/golden/ref_kernels.npz"""
    torch = torch_cuda
    fx = np.load(os.path.join(GOLDEN, "ref_kernels.npz"))
    n = 0
    for key in fx.files:
        if not key.startswith("nvf_"):
            continue
        _, name, ptag = key.split("_")
        x, p = fx["x_" + name], int(ptag[1:])
        if x.shape[0] < 4 or x.shape[1] < 5:
            continue
        eng = wm.Watermark(x.shape[0], x.shape[1], synth_watermark(*x.shape), p, 40.0)
        m, _, _, _ = eng.computeMask(dev(torch, x), wm.MASK_TYPE.NVF)
        bits_equal(m.cpu().numpy(), fx[key], f"{path} {key}")
        n += 1
    assert n >= 16
