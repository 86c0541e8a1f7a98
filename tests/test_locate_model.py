"""CPU tests of the identity behind wm_locate (tests/locate_model.py): with the exact adjoint of the replicate-border stencil,
sum_q h(q) W_window(q) IS the detector's <e_u, e_w> of tests/np_restatement.py at the true offset (<= 1e-8 relative: the two differ
by the f32 roundings of u and e_u, which do not add up coherently); with a zero-border adjoint it is not, which shows that the
border terms are tested; and the argmax of the model's map over every admissible offset is the true offset, far above the rest of the
map, while an unmarked crop's map has no such peak."""
import numpy as np
import pytest

import locate_model as M
import np_restatement as R
from synth import synth_frame, synth_watermark

# (key shape, crop shape, true offset, floored to 8 bits)
CASES = [((270, 480), (200, 384), (37, 53), False), ((270, 480), (200, 384), (37, 53), True),
         ((120, 330), (64, 256), (20, 31), False), ((300, 520), (96, 128), (150, 300), True)]
Z_MARKED, Z_UNMARKED = 15.0, 6.0
_marked = {}


def marked_and_plain(kshape, shape, at, floored, mask):
    """a frame marked at the key's shape (psnr 40, p = 3), cropped at `at`, and the same crop of the unmarked frame"""
    tag = (kshape, mask)
    if tag not in _marked:
        x = synth_frame(*kshape, frame=len(_marked))
        W = synth_watermark(*kshape, seed=4242 + kshape[0])
        y, _ = R.embed(x, x, W, 3, 40.0, "ME" if mask == 0 else "NVF")
        _marked[tag] = (x, y, W)
    x, y, W = _marked[tag]
    (r, c), (oy, ox) = shape, at
    crop, plain = y[oy:oy + r, ox:ox + c], x[oy:oy + r, ox:ox + c]
    if floored:
        crop, plain = np.floor(crop), np.floor(plain)
    return np.ascontiguousarray(crop, np.float32), np.ascontiguousarray(plain, np.float32), W


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at,floored", CASES)
def test_identity_at_the_true_offset(kshape, shape, at, floored, mask):
    crop, _, W = marked_and_plain(kshape, shape, at, floored, mask)
    win = W[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]]
    c = R.coefficients(crop)
    ew = R.error_sequence(crop, c)
    m = np.abs(ew) if mask == 0 else R.nvf_mask(crop, 3)
    eu = R.error_sequence((m * win).astype(np.float32), c)
    want = float(np.sum(eu.astype(np.float64) * ew.astype(np.float64)))
    got = float(np.sum(M.h_plane(crop, c, mask, e=ew) * win))
    off = float(np.sum(M.h_plane(crop, c, mask, e=ew, zero_border=True) * win))
    print(f"<e_u, e_w> {want:.9g}  sum h W {got:.9g} (rel {abs(got - want) / abs(want):.2e})  zero border: rel {abs(off - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-8 * abs(want)
    assert abs(off - want) > 1e-5 * abs(want)  # (measured 1e-3 .. 1e-2: five orders above the exact adjoint's residue)


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at,floored", CASES)
def test_argmax_is_the_true_offset(kshape, shape, at, floored, mask):
    crop, plain, W = marked_and_plain(kshape, shape, at, floored, mask)
    mp, (oy, ox, peak, z) = M.locate(crop, W, R.coefficients(crop), mask)
    assert mp.shape == (kshape[0] - shape[0] + 1, kshape[1] - shape[1] + 1)
    _, (_, _, _, zu) = M.locate(plain, W, R.coefficients(plain), mask)
    print(f"marked: ({oy}, {ox}) peak {peak:.6g} z {z:.1f}; unmarked: z {zu:.2f}")
    assert (oy, ox) == at
    assert z >= Z_MARKED and zu <= Z_UNMARKED
    # the map value at a few offsets against the direct sum
    h = M.h_plane(crop, R.coefficients(crop), mask)
    for (i, j) in ((0, 0), at, (mp.shape[0] - 1, mp.shape[1] - 1)):
        direct = float(np.sum(h * W[i:i + shape[0], j:j + shape[1]]))
        assert abs(mp[i, j] - direct) <= 1e-9 * np.sqrt(np.sum(h * h) * np.sum(W.astype(np.float64) ** 2))


def test_adjoint_is_the_transpose_of_the_stencil():
    """<F a, b> == <a, F^T b> on a plane with every kind of border pixel, one-pixel axes included"""
    rng = np.random.default_rng(3)
    c = rng.normal(size=8)
    for shape in ((5, 7), (1, 6), (6, 1), (2, 2), (1, 1)):
        a, b = rng.normal(size=shape), rng.normal(size=shape)
        lhs = float(np.sum(M.error_plane(a, c) * b))
        rhs = float(np.sum(a * M.adjoint(b, c)))
        assert abs(lhs - rhs) <= 1e-12 * (1 + abs(lhs)), shape


def test_fold_rules():
    m = np.zeros((4, 5))
    m[1, 2] = m[3, 4] = 2.0  # a tie: the smallest index wins
    assert M.fold(m)[:3] == (1, 2, 2.0)
    assert np.isnan(M.fold(np.zeros((4, 5)))[3])       # no variation
    assert np.isnan(M.fold(np.ones((1, 1)))[3])        # one offset
    assert np.isnan(M.fold(np.arange(4.0).reshape(2, 2))[3])  # every offset lies inside the block around the argmax
    m = np.arange(12.0).reshape(3, 4)                  # argmax (2, 3): the block covers rows 1-2, columns 2-3
    rest = np.array([0, 1, 2, 3, 4, 5, 8, 9.0])
    assert abs(M.fold(m)[3] - (11 - rest.mean()) / rest.std()) < 1e-12
