"""CPU tests of the identity behind wm_locate (tests/locate_model.py): with the exact adjoint of the replicate-border stencil,
sum_q h(q) W_window(q) IS the detector's <e_u, e_w> of tests/np_restatement.py at the true offset (<= 1e-8 relative: the two differ
by the f32 roundings of u and e_u, which do not add up coherently); with a zero-border adjoint it is not, which shows that the
border terms are tested; and the argmax of the model's map over every admissible offset is the true offset, far above the rest of the
map, while an unmarked crop's map has no such peak."""
import numpy as np
import pytest

import hard_frames as H
import locate_model as M
import np_restatement as R
import oracle_lib as O
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


U32 = 2.0 ** -24  # half an ulp of 1 in f32: the relative error of one rounding
RESTATED_MAP_BOUND = 8.3e-5  # of sigma_W: 1.5 x the largest measured figure (test_restated_h_against_the_f64_model)


def restated_h_bound(c, e, g, m, h, mask):
    """how far the f32 restatement of h may lie from the f64 model, from the roundings it makes (u = 2^-24 per rounding):
      e  eight fmaf whose partial results stay below 255 (1 + sum |c|):                    de <= 8 u 255 (1 + sum |c|)
      g  the model's g of the restated e is linear in e with gain A4 = 1 + 4 sum |c| (a corner's adjoint sets hold four pixels);
         the set sums (three additions of values below 4 max|e|) and eight fmaf whose partial results stay below A4 max|e|:
                                                                                             dg <= A4 de + 20 u A4 max|e|
      m  ME: |e|, dm = de; NVF: the two f32 restatements of the mask agree to 1e-6 (test_oracle.py)
      h  one product:                                                     dh <= max m dg + max|g| dm + u max|h| + dm dg"""
    a = float(np.abs(np.asarray(c, np.float64)).sum())
    de = 8 * U32 * 255.0 * (1 + a)
    a4 = 1 + 4 * a
    dg = a4 * de + 20 * U32 * a4 * float(np.abs(e).max())
    dm = de if mask == 0 else 1e-6
    return float(np.abs(m).max()) * dg + float(np.abs(g).max()) * dm + U32 * float(np.abs(h).max()) + dm * dg


def restated_case(x, key, mask, p):
    """(|dh| / max|h|, its bound / max|h|, map difference / sigma_W) of one crop: the oracle's f32 restatement of h with the device's
    operation sequence against locate_model.h_plane, both with np_restatement's coefficients"""
    x = np.asarray(x, np.float32)
    c = R.coefficients(x)
    e, g, m, h = O.locate_h(x, c, mask, p)
    want = M.h_plane(x, c, mask, p)
    hmax = float(np.abs(want).max())
    err = float(np.abs(h.astype(np.float64) - want).max())
    bound = restated_h_bound(c, e, g, m, h, mask)
    assert err <= bound, (err, bound)
    sw = M.sigma_w(x, key, c, mask, p)
    dmap = float(np.abs(M.correlate(h.astype(np.float64), key) - M.correlate(want, key)).max()) / sw
    return err / hmax, bound / hmax, dmap


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
@pytest.mark.parametrize("kshape,shape,at", H.LOCATE_GEOMS)
def test_restated_h_against_the_f64_model(kshape, shape, at, mask, p):
    """wmo_locate_h (f32, the device's operation sequence) against h_plane (f64) per pixel on every hard crop family: within the
    bound that follows from its roundings (restated_h_bound), and the maps of the two within RESTATED_MAP_BOUND.  Measured over
    the three geometries and four (mask, p), marked and unmarked, |dh| / max|h| and the map difference in sigma_W:
      texture 7.8e-7 / 2.6e-6, clipped 4.8e-7 / 1.9e-6, letterbox 6.9e-7 / 3.2e-6, pillar 8.1e-7 / 2.7e-6, binary 3.1e-7 / 1.4e-6,
      near_singular 1.8e-5 / 5.5e-5, low_contrast 3.2e-6 / 1.5e-5, impulse 7.1e-7 / 1.0e-5
    (hard_frames.RESTATEMENT_FIGURES holds them rounded up; no case may exceed its family's figure).  The near-singular map
    figure, 5.5e-5, lies above the 4.3e-5 of the numpy emulation the bound of 6e-5 was first drawn from (that one ran one geometry
    at p = 3), so the bound is 1.5 x the measured figure: 8.3e-5 sigma_W"""
    key = H.locate_key(kshape)
    worst = {}

    def take(family, x):
        rel, bnd, dmap = restated_case(x, key, mask, p)
        w = worst.setdefault(family, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], rel), max(w[1], bnd), max(w[2], dmap)

    for name, (marked, plain) in H.locate_crops(kshape, shape, at, mask, p).items():
        take(H.locate_family(name), marked)
        take(H.locate_family(name), plain)
    for x in H.locate_impulses(kshape, shape, at)[0]:
        take("impulse", x)
    for family, (rel, bnd, dmap) in worst.items():
        fig = H.RESTATEMENT_FIGURES[family]
        print(f"{kshape}->{shape}@{at} mask {mask} p {p} {family}: |dh| {rel:.2e} of max|h| (bound {bnd:.2e}, figure {fig[0]:.1e}); maps {dmap:.2e} sigma_W "
              f"(figure {fig[1]:.1e})")
        assert dmap <= RESTATED_MAP_BOUND and fig[1] <= RESTATED_MAP_BOUND
        assert rel <= fig[0] and dmap <= fig[1]


def test_restated_h_is_not_the_oracle_error_sequence():
    """wmo_locate_h's e (the chain from the centre pixel) and wmo_error_sequence (x - the chain from 0) differ in some pixels by a
    few ulp: the reason the restatement forms its own e"""
    kshape, shape, at = H.LOCATE_GEOMS[0]
    x = H.locate_crops(kshape, shape, at, 0, 3)["texture"][0]
    c = R.coefficients(x)
    e = O.locate_h(x, c, 0, 3)[0]
    d = np.abs(e - O.error_sequence(x, c))
    assert 0 < d.max() <= 8 * 2.0 ** -23 * 255.0 and (d > 0).mean() > 0.01


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
