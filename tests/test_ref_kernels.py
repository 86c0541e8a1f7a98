"""The oracle pinned to the reference's own kernel code: nvf.hpp, scaled_neighbors_p3.hpp and me_p3.hpp compiled from the
reference checkout as OpenCL C for the CPU and run by a work-item runtime (oracle/build_ref.py, oracle/clrt.c,
tests/ref_lib.py).  Two builds: MAD with the reference's options (-cl-mad-enable, main.cpp:106-108) and STRICT
(-ffp-contract=off).

(a) the harness checked without the oracle: STRICT against a float32 numpy restatement written here (and a wrong
    restatement must fail), so that a disagreement in (b) points at the oracle;
(b) the oracle against MAD, bit-exact: NVF for p = 3..9, the scaled neighbours, ref_arith's Gram partials and their fold;
(c) the oracle differs from STRICT on the crop, so a mix-up of the two builds cannot pass;
(d) the committed fixture tests/golden/ref_kernels.npz (MAD outputs, make_ref_fixture.py) holds the oracle even where
    oracle/_ref is absent, and the runtime reproduces it where it is present.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_lib as R
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "ref_kernels.npz")


def _need_ref():
    if R.available():
        return
    if R.reference_tree() is not None:
        pytest.fail("the reference tree is present but oracle/_ref is not built (python oracle/build_ref.py)")
    pytest.skip("neither oracle/_ref nor a reference tree")


SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (15, 17), (16, 16), (17, 33), (31, 200),
          (5, 63), (5, 64), (5, 65), (4, 127), (4, 128), (4, 129)]
DATA = ["u8", "const", "checker", "f32"]


def make(kind, shape, seed=0):
    rng = np.random.default_rng(seed + 7919 * shape[0] + shape[1])
    if kind == "u8":
        return rng.integers(0, 256, shape).astype(np.float32)
    if kind == "const":
        return np.full(shape, 173.0, np.float32)
    if kind == "checker":
        r, c = np.indices(shape)
        return (((r + c) & 1) * 255).astype(np.float32)
    return rng.uniform(0.0, 255.0, shape).astype(np.float32)


def crop_gray(pair_crop):
    return O.rgb2gray(pair_crop[0])


def gray512(pair512):
    return O.rgb2gray(pair512[0])


# ---- (a) float32 numpy restatements, sums in tap order ----------------------------------------------------------------
def np_window(x, pad, mode):
    xp = np.pad(x, pad, mode=mode)
    rows, cols = x.shape
    return [xp[pad + i:pad + i + rows, pad + j:pad + j + cols] for i in range(-pad, pad + 1) for j in range(-pad, pad + 1)]


def np_nvf(x, p, mode="edge"):
    f = np.float32
    s = np.zeros_like(x)
    sq = np.zeros_like(x)
    for v in np_window(x, p // 2, mode):
        s = s + v
        sq = sq + v * v
    mean = s / f(p * p)
    var = sq / f(p * p) - mean * mean
    return var / (f(1) + var)


def np_neighbors(x, c, mode="edge"):
    taps = np_window(x, 1, mode)
    taps = taps[:4] + taps[5:]  # the 8 neighbours, row-major, without the centre
    dot = np.zeros_like(x)
    for k in range(8):
        dot = dot + np.float32(c[k]) * taps[k]
    return dot


def np_me_partials(x, mode="edge"):
    """RxPartial / rxPartial as me_p3.hpp writes them: lane l of a 64-wide work-group sums, over the group's lanes in
    order, the half-rounded product of neighbours (l // 8, l % 8) (either order of the pair) and, for l < 8, of
    neighbour l with the centre; lanes beyond the width add 0"""
    rows, cols = x.shape
    pw = (cols + 63) // 64 * 64
    taps = np_window(x, 1, mode)
    n = np.stack(taps[:4] + taps[5:])  # [8, rows, cols]
    ctr = taps[4]
    h = lambda a: a.astype(np.float16).astype(np.float32)
    prod = np.zeros((8, 8, rows, pw), np.float32)
    prod[:, :, :, :cols] = h(n[:, None] * n[None, :])
    cprod = np.zeros((8, rows, pw), np.float32)
    cprod[:, :, :cols] = h(n * ctr[None])
    Rp = np.zeros((rows, pw), np.float32)
    rp = np.zeros((rows, pw // 8), np.float32)
    for g in range(pw // 64):
        accR = np.zeros((8, 8, rows), np.float32)
        accr = np.zeros((8, rows), np.float32)
        for lane in range(64):
            accR = accR + prod[:, :, :, 64 * g + lane]
            accr = accr + cprod[:, :, 64 * g + lane]
        Rp[:, 64 * g:64 * g + 64] = accR.reshape(64, rows).T
        rp[:, 8 * g:8 * g + 8] = accr.T
    return Rp, rp


@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (15, 17), (17, 33), (31, 200)])
@pytest.mark.parametrize("kind", DATA)
def test_harness_nvf_strict_vs_numpy(shape, kind):
    _need_ref()
    x = make(kind, shape)
    for p in (3, 5, 7, 9):
        np.testing.assert_array_equal(R.nvf(x, p, R.STRICT), np_nvf(x, p), err_msg=f"p={p}")


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (15, 17), (31, 200)])
@pytest.mark.parametrize("kind", DATA)
def test_harness_neighbors_strict_vs_numpy(shape, kind):
    _need_ref()
    x = make(kind, shape)
    c = np.random.default_rng(1).normal(size=8).astype(np.float32)
    np.testing.assert_array_equal(R.scaled_neighbors(x, c, R.STRICT), np_neighbors(x, c))


@pytest.mark.parametrize("kind", DATA)
def test_harness_me_partials_vs_numpy(kind):
    """one work-group pair along a row: a 3 x 70 plane (lanes 70..127 of the second group are padding)"""
    _need_ref()
    x = make(kind, (3, 70))
    Rp, rp = R.me_partials(x, R.STRICT)
    Rn, rn = np_me_partials(x)
    np.testing.assert_array_equal(Rp, Rn)
    np.testing.assert_array_equal(rp, rn)
    Rm, rm = R.me_partials(x, R.MAD)  # no product or sum in me_p3.hpp can contract: both builds agree
    np.testing.assert_array_equal(Rm, Rp)
    np.testing.assert_array_equal(rm, rp)


def test_harness_self_check_discriminates():
    """a restatement with the wrong border (zero padding instead of clamp-to-edge) must NOT match: the checks above
    can fail"""
    _need_ref()
    x = make("u8", (15, 17))
    c = np.random.default_rng(1).normal(size=8).astype(np.float32)
    assert not np.array_equal(R.nvf(x, 3, R.STRICT), np_nvf(x, 3, mode="constant"))
    assert not np.array_equal(R.scaled_neighbors(x, c, R.STRICT), np_neighbors(x, c, mode="constant"))
    assert not np.array_equal(R.me_partials(x, R.STRICT)[0], np_me_partials(x, mode="constant")[0])
    # and one tap out of order in the neighbour dot
    swapped = np.array(c)
    swapped[[3, 4]] = swapped[[4, 3]]
    assert not np.array_equal(R.scaled_neighbors(x, c, R.STRICT), np_neighbors(x, swapped))


# ---- (b) the oracle against the reference's build, bit-exact -----------------------------------------------------------
def _planes(pair512, pair_crop):
    for shape in SHAPES:
        for kind in DATA:
            yield f"{kind}{shape}", make(kind, shape)
    yield "crop", crop_gray(pair_crop)
    yield "512", gray512(pair512)


@pytest.mark.parametrize("p", [3, 5, 7, 9])
def test_oracle_nvf_bit_exact_vs_reference_kernel(p, pair512, pair_crop):
    _need_ref()
    for name, x in _planes(pair512, pair_crop):
        ref = R.nvf(x, p, R.MAD)
        got = O.nvf_mask(x, p)
        bad = int((ref.view(np.uint32) != got.view(np.uint32)).sum())
        assert bad == 0, f"{name} p={p}: {bad} of {x.size} differ, max {np.abs(ref - got).max():.3g}"


def _coefficient_sets(x):
    st, c, *_ = O.me_mask(x)
    sets = {"solved": c} if st == O.OK else {}
    sets.update({"negative": -np.abs(np.linspace(0.1, 3.7, 8, dtype=np.float32)),
                 "large": np.array([3e4, -1e5, 7e3, 2.5e5, -9e4, 1e6, -3e5, 4e4], np.float32),
                 "mixed": np.array([0.3333333, -1e-4, 12.5, -0.7071068, 1e-7, -255.0, 0.1, -3.14159], np.float32)})
    return sets


def test_oracle_neighbors_bit_exact_vs_reference_kernel(pair512, pair_crop):
    _need_ref()
    for name, x in _planes(pair512, pair_crop):
        for cname, c in _coefficient_sets(x).items():
            np.testing.assert_array_equal(O.scaled_neighbors(x, c), R.scaled_neighbors(x, c, R.MAD),
                                          err_msg=f"{name} {cname}")


def test_oracle_ref_arith_gram_partials_vs_reference_kernel(pair512, pair_crop):
    """ref_arith's per-work-group sums are the me kernel's, bit for bit, and the oracle's ref_arith Rx / rx are its f32
    fold of exactly those partials"""
    _need_ref()
    for name, x in _planes(pair512, pair_crop):
        part = R.gram_partials(x, R.MAD)
        np.testing.assert_array_equal(O.gram_ref_partials(x), part, err_msg=name)
        Rx, rx = O.gram(x, ref_arith=True)
        Rf, rf = O.gram_ref_fold(part)
        np.testing.assert_array_equal(Rf, Rx, err_msg=name)
        np.testing.assert_array_equal(rf, rx, err_msg=name)


# ---- (c) the two builds are told apart ---------------------------------------------------------------------------------
def test_oracle_differs_from_the_strict_build(pair_crop):
    _need_ref()
    x = crop_gray(pair_crop)
    for p in (3, 9):
        assert not np.array_equal(O.nvf_mask(x, p), R.nvf(x, p, R.STRICT)), p
    c = _coefficient_sets(x)["solved"]
    assert not np.array_equal(O.scaled_neighbors(x, c), R.scaled_neighbors(x, c, R.STRICT))


# ---- (d) the committed fixture ------------------------------------------------------------------------------------------
def _fixture():
    return np.load(FIXTURE)


def test_fixture_holds_the_oracle():
    """runs without oracle/_ref: the reference kernels' outputs recorded by make_ref_fixture.py"""
    fx = _fixture()
    for key in fx.files:
        if key.startswith("nvf_"):
            _, name, p = key.split("_")
            np.testing.assert_array_equal(O.nvf_mask(fx["x_" + name], int(p[1:])), fx[key], err_msg=key)
        elif key.startswith("sn_"):
            _, name, cname = key.split("_")
            np.testing.assert_array_equal(O.scaled_neighbors(fx["x_" + name], fx["c_" + cname]), fx[key], err_msg=key)
        elif key.startswith("part_"):
            np.testing.assert_array_equal(O.gram_ref_partials(fx["x_" + key[5:]]), fx[key], err_msg=key)


def test_fixture_reproduced_by_the_reference_kernels():
    _need_ref()
    fx = _fixture()
    assert str(fx["manifest_sources"]) == R.manifest_sources_text(), "the reference sources changed since the fixture"
    n = 0
    for key in fx.files:
        if key.startswith("nvf_"):
            _, name, p = key.split("_")
            np.testing.assert_array_equal(R.nvf(fx["x_" + name], int(p[1:]), R.MAD), fx[key], err_msg=key)
        elif key.startswith("sn_"):
            _, name, cname = key.split("_")
            np.testing.assert_array_equal(R.scaled_neighbors(fx["x_" + name], fx["c_" + cname], R.MAD), fx[key], err_msg=key)
        elif key.startswith("part_"):
            np.testing.assert_array_equal(R.gram_partials(fx["x_" + key[5:]], R.MAD), fx[key], err_msg=key)
        else:
            continue
        n += 1
    assert n >= 10


def test_runtime_respects_the_launch_contract():
    """wrong arguments are refused, not run"""
    _need_ref()
    x = np.zeros((4, 4), np.float32)
    out = np.empty_like(x)
    L = R.lib()
    assert L.wmref_nvf(0, 4, R._f(x), 4, 4, R._f(out)) == -1  # p must be 3, 5, 7 or 9 (Watermark.cpp:24-25)
    assert L.wmref_nvf(2, 3, R._f(x), 4, 4, R._f(out)) == -1
    assert L.wmref_nvf(0, 3, R._f(x), 0, 4, R._f(out)) == -1
    assert L.wmref_scaled_neighbors(0, R._f(x), 4, -1, R._f(np.zeros(8, np.float32)), R._f(out)) == -1
