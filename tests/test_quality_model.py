"""CPU tests of tests/quality_model.py, the numpy restatement of wm_quality's definitions (include/wm.h) that decides the GPU tests:
its two evaluations agree, and it has the properties the definitions imply."""
import numpy as np
import pytest

import quality_model as Q
from synth import synth_frame


def noisy(x, seed, amp=3.0):
    rng = np.random.default_rng(seed)
    return np.clip(x + amp * rng.standard_normal(x.shape), 0, 255).astype(np.float32)


@pytest.fixture(scope="module")
def pair():
    x = synth_frame(70, 130, frame=1)
    return x, noisy(x, 7)


def test_weights():
    g = Q.weights()
    assert g.shape == (11,) and g.dtype == np.float64 and abs(g.sum() - 1.0) < 1e-15
    assert (g == g[::-1]).all() and g[5] == g.max()
    assert g[4] / g[5] == pytest.approx(np.exp(-1 / 4.5), rel=1e-15)


def test_separable_and_direct_agree_per_window(pair):
    x, y = pair
    a, b = Q.ssim_map(x, y), Q.ssim_map(x, y, direct=True)
    assert a.shape == (60, 120)
    assert np.abs(a - b).max() <= 1e-12
    # a bright flat patch, the worst case of the cancellation in E[x^2] - mx^2: the window sums are ~65025, an evaluation order adds
    # 11 taps at a time, each step within an ulp, so vx, vy and cxy may each move by 65025 * 2^-52 * 11 = 1.6e-10 against a
    # denominator of at least C2 = 58.5: 2.7e-12 per term, three terms -- 1e-11 (the GPU test's 1e-10 per window lies above it)
    xb = np.full((16, 16), 255, np.float32)
    yb = noisy(xb - 2, 3, 1.0)
    assert np.abs(Q.ssim_map(xb, yb) - Q.ssim_map(xb, yb, direct=True)).max() <= 1e-11


def test_identical_planes(pair):
    x, _ = pair
    s = Q.tile_sums(x, x)
    assert s[0, 0].tolist() == [0.0, 70 * 130, 60 * 120, 60 * 120, 0.0]
    assert (Q.ssim_map(x, x) == 1.0).all()
    mse, ssim, mx = Q.plane_values(s)
    assert mse == 0.0 and ssim == 1.0 and mx == 0.0 and Q.psnr_from_mse(mse) == float("inf")


@pytest.mark.parametrize("c1,c2", [(255, 0), (0, 255), (100, 101), (17, 17)])
def test_flat_against_flat(c1, c2):
    x, y = np.full((12, 13), c1, np.uint8), np.full((12, 13), c2, np.uint8)
    want = (2.0 * c1 * c2 + Q.C1) / (c1 * c1 + c2 * c2 + Q.C1)
    assert np.abs(Q.ssim_map(x, y) - want).max() <= 1e-12
    s = Q.tile_sums(x, y)[0, 0]
    assert s[0] == 12 * 13 * (c1 - c2) ** 2 and s[1] == 12 * 13 and s[3] == 2 * 3 and s[4] == abs(c1 - c2)
    if (c1, c2) == (255, 0):
        assert want == pytest.approx(6.5025 / 65031.5025, rel=1e-14)  # ((0.01 * 255)^2 is 6.5025 to an ulp)


def test_symmetric_in_its_arguments(pair):
    x, y = pair
    assert np.abs(Q.ssim_map(x, y) - Q.ssim_map(y, x)).max() <= 1e-15
    a, b = Q.tile_sums(x, y, 32, 32), Q.tile_sums(y, x, 32, 32)
    assert (a[..., [0, 1, 3, 4]] == b[..., [0, 1, 3, 4]]).all() and np.abs(a[..., 2] - b[..., 2]).max() <= 1e-12


@pytest.mark.parametrize("shape,tile", [((70, 130), (32, 32)), ((43, 67), (32, 32)), ((270, 480), (64, 128)), ((64, 300), (40, 36))])
def test_tile_sums_add_to_the_planes(shape, tile):
    x = synth_frame(*shape, frame=2)
    y = noisy(x, 11)
    whole = Q.tile_sums(x, y)[0, 0]
    t = Q.tile_sums(x, y, *tile)
    ny, nx = Q.tiles_shape(*shape, *tile)
    assert t.shape == (ny, nx, 5)
    assert t[..., 1].sum() == shape[0] * shape[1] and t[..., 3].sum() == (shape[0] - 10) * (shape[1] - 10) == whole[3]
    assert t[..., 0].sum() == pytest.approx(whole[0], rel=1e-13) and t[..., 2].sum() == pytest.approx(whole[2], rel=1e-13)
    assert t[..., 4].max() == whole[4]
    mse, ssim, mx = Q.plane_values(t)
    mse0, ssim0, mx0 = Q.plane_values(whole)
    assert mse == pytest.approx(mse0, rel=1e-13) and ssim == pytest.approx(ssim0, rel=1e-13) and mx == mx0


@pytest.mark.parametrize("shape", [(10, 40), (40, 10), (5, 5)])
def test_no_window(shape):
    x = synth_frame(64, 64, frame=3)[:shape[0], :shape[1]]
    y = noisy(x, 5)
    s = Q.tile_sums(x, y)[0, 0]
    assert s[3] == 0 and s[2] == 0 and s[1] == shape[0] * shape[1]
    mse, ssim, mx = Q.plane_values(s)
    assert np.isnan(ssim) and mse == pytest.approx(np.mean((x.astype(np.float64) - y) ** 2), rel=1e-13) and mx > 0


def test_one_changed_pixel():
    x = synth_frame(43, 67, frame=4)
    y = x.copy()
    y[20, 30] += 9.0
    s = Q.ssim_map(x, y)
    changed = s != 1.0
    assert changed.sum() == 121 and changed[10:21, 20:31].all()
    t = Q.tile_sums(x, y)[0, 0]
    assert t[4] == 9.0 and t[0] == 81.0


def test_psnr_from_mse():
    assert Q.psnr_from_mse(100.0) == pytest.approx(28.130803608679, abs=1e-11)
    assert Q.psnr_from_mse(0.0) == float("inf")
    assert np.isnan(Q.psnr_from_mse(-1.0)) and np.isnan(Q.psnr_from_mse(float("nan"))) and np.isnan(Q.psnr_from_mse(1.0, 0.0))
