"""The bracket the build states against the REFERENCE's own arithmetic (last row): coefficients <= 5e-3
(<= 720p) / 5e-2 (4K class), a <= 1 % rel, correlation <= 2e-3 abs, y RMS <= 0.25 grey levels.

The reference's host program cannot be run here (ArrayFire / OpenCL / MSVC) and ships no vectors, so "the reference's
arithmetic" is the oracle's ref_arith switch: products rounded to half, 64-lane f32 work-group sums in lane order, f32 fold
of the partials, f32 LU (me_p3.hpp:8-21,61-82; Watermark.cpp:148-149,203).  The per-work-group sums are pinned bit-exact
to the reference's own me kernel (tests/test_ref_kernels.py); what this file brackets is the rest: the order of af::sum
(a pairwise tree here) and af::solve (f32 LU here), which no reference source fixes.  CPU part: the oracle's exact policy against
its reference-arithmetic mode on the committed fixtures, and the records in golden.json (written by make_golden.py)."""
import numpy as np
import pytest

import oracle_lib as O

# (coefficients abs, a rel, corr abs, y rms): the stated bracket, and the one for the 96 x 200 crop -- a fragment whose
# Gram matrix (cond 2.4e5) is as ill-conditioned as a 4K frame's, so it takes the 4K-class coefficient bound and 2 % on a
BRACKET = {"512": (5e-3, 1e-2, 2e-3, 0.25), "480p": (5e-3, 1e-2, 2e-3, 0.25), "720p": (5e-3, 1e-2, 2e-3, 0.25),
           "720p_crop": (5e-2, 2e-2, 2e-3, 0.25)}


@pytest.mark.parametrize("tag", ["512", "720p_crop"])
def test_oracle_exact_vs_reference_arithmetic(golden, tag, pair512, pair_crop):
    rgb, W = pair512 if tag == "512" else pair_crop
    x = O.rgb2gray(rgb)
    tc, ta, tcorr, trms = BRACKET[tag]
    st, c, e, m, mx = O.me_mask(x)
    st, cr, er, mr, mxr = O.me_mask(x, ref_arith=True)
    assert np.abs(c - cr).max() <= tc
    st, y, a = O.embed(x, x, W)
    st, yr, ar = O.embed(x, x, W, ref_arith=True)
    assert abs(ar - a) <= ta * abs(a)
    assert np.sqrt(((yr.astype(np.float64) - y) ** 2).mean()) <= trms
    corr, corr_r = O.detect(y, W)[1], O.detect(y, W, ref_arith=True)[1]
    assert abs(corr - corr_r) <= tcorr
    # the committed record reproduces
    rec = golden[tag]["reference_arith"]
    np.testing.assert_allclose(cr, rec["coefficients"], rtol=0, atol=1e-6)
    assert ar == pytest.approx(rec["a_ME"], rel=1e-6) and corr_r == pytest.approx(rec["corr_ME_on_exact_y"], abs=1e-6)


@pytest.mark.parametrize("tag", ["512", "480p", "720p", "720p_crop"])
def test_golden_records_sit_inside_the_bracket(golden, tag):
    """480p / 720p: the reference's full sample pairs (their inputs stay in the reference tree; make_golden.py recorded
    the deviations between the two arithmetic policies)"""
    rec = golden[tag]["reference_arith"]
    tc, ta, tcorr, trms = BRACKET[tag]
    assert rec["max_abs_dcoef"] <= tc and rec["rel_da_ME"] <= ta and rec["abs_dcorr_ME"] <= tcorr and rec["y_rms_vs_exact"] <= trms
    assert abs(rec["psnr_exact_dB"] - rec["psnr_reference_arith_dB"]) <= 0.05 and rec["psnr_exact_dB"] >= 40.0 - 0.05


def test_f32_solve_matches_f64_solve_on_a_well_conditioned_system():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(8, 8))
    Rx = A @ A.T + 8 * np.eye(8)
    rx = rng.normal(size=8)
    c64 = np.zeros(8, np.float32)
    c32 = np.zeros(8, np.float32)
    L = O.lib()
    assert L.wmo_solve(O._d(np.ascontiguousarray(Rx)), O._d(rx), O._f(c64)) == 0
    assert L.wmo_solve_f32(O._d(np.ascontiguousarray(Rx)), O._d(rx), O._f(c32)) == 0
    np.testing.assert_allclose(c32, np.linalg.solve(Rx, rx), rtol=0, atol=2e-6)
    np.testing.assert_allclose(c64, np.linalg.solve(Rx, rx), rtol=0, atol=1e-7)
