"""wm_fft2 (k_fft_rows, k_fft_transpose) against numpy.fft.fft2 in complex128: every row length 2^6 .. 2^13 on either axis and one
shape with two long axes; forward and inverse; an impulse at a non-zero index, whose transform is an exact phase ramp (it catches
the direction and the sign of the turn factors); normal noise; and the round trip divided by pr pc.

Bound: relative L2 error <= 5e-6 = eps_f32 (6e-8) x log2 N (<= 26) as a worst-case linear growth, times three.  An indexing fault
gives O(1).  Measured on MI355X: DESIGN.md section 24."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND = 5e-6
SHAPES = [(64, 1 << k) for k in range(6, 14)] + [(1 << k, 64) for k in range(7, 14)] + [(512, 1024)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev_fft2(wm, torch, a, inverse):
    """a: complex64 [pr, pc] -> the device's transform as complex128"""
    t = torch.from_numpy(np.ascontiguousarray(np.stack([a.real, a.imag], -1), np.float32)).cuda()
    wm.fft2(t, inverse)
    r = t.cpu().numpy().astype(np.float64)
    return r[..., 0] + 1j * r[..., 1]


def rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


@pytest.mark.parametrize("shape", SHAPES)
def test_against_numpy(wm, torch_cuda, shape):
    pr, pc = shape
    rng = np.random.default_rng(pr * 31 + pc)
    x = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    x128 = x.astype(np.complex128)
    fwd = dev_fft2(wm, torch_cuda, x, False)
    inv = dev_fft2(wm, torch_cuda, x, True)
    e_f, e_i = rel(fwd, np.fft.fft2(x128)), rel(inv, np.fft.ifft2(x128) * (pr * pc))
    # the round trip: inverse(forward(x)) = pr pc x (neither direction is normalised)
    back = dev_fft2(wm, torch_cuda, fwd.astype(np.complex64), True) / (pr * pc)
    e_rt = rel(back, x128)
    # an impulse at (3, 5): forward exp(-2 pi i (3 u / pr + 5 v / pc)), inverse its conjugate
    imp = np.zeros(shape, np.complex64)
    imp[3, 5] = 1.0
    u, v = np.arange(pr)[:, None], np.arange(pc)[None, :]
    ramp = np.exp(-2j * np.pi * (3 * u / pr + 5 * v / pc))
    e_if, e_ii = rel(dev_fft2(wm, torch_cuda, imp, False), ramp), rel(dev_fft2(wm, torch_cuda, imp, True), np.conj(ramp))
    print(f"{pr}x{pc}: forward {e_f:.2e} inverse {e_i:.2e} round trip {e_rt:.2e} impulse {e_if:.2e} / {e_ii:.2e}")
    assert max(e_f, e_i, e_rt, e_if, e_ii) <= BOUND


def test_refusals(wm, torch_cuda):
    torch = torch_cuda
    bad = wm.WM_ERR_BAD_ARG
    t = torch.zeros((96, 64, 2), dtype=torch.float32, device="cuda")
    assert wm.lib().wm_fft2(0, t.data_ptr(), 96, 64, 0) == bad
    assert wm.lib().wm_fft2(0, t.data_ptr(), 32, 64, 0) == bad
    assert wm.lib().wm_fft2(0, None, 64, 64, 0) == bad
    with pytest.raises(RuntimeError):
        wm.fft2(t)


def test_pass_yardstick(wm, torch_cuda):
    """wm_fft_bench times the seven passes of one frame: seven positive figures, and the same refusals as wm_fft2"""
    us = wm.fft_bench(64, 128, 2)
    assert list(us) == list(wm.FFT_BENCH_PASSES) and len(us) == 7 and all(v > 0 for v in us.values())
    with pytest.raises(RuntimeError):
        wm.fft_bench(96, 128, 2)
    with pytest.raises(RuntimeError):
        wm.fft_bench(64, 128, 0)
