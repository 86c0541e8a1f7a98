"""CPU tests of the identities behind wm_locate_keys (tests/locate_keys_model.py): one complex transform carries the maps of two
keys, the per-key model is wm_locate's, and on the finding table -- a bank of 5 keys, frame 0 marked with key 1, frame 1 with key 4,
frame 2 unmarked, each cropped, f32 and floored to 8 bits, ME and NVF -- the owner's key alone has a peak, at the true offset.

Thresholds are the project's (test_gpu_locate.py): z >= 15 for the owner, z <= 6 for every other (frame, key).  Seen with this
set-up (printed by the test): owners 21.6-82.1, every other pair 2.6-5.1."""
import numpy as np
import pytest

import locate_keys_model as LK
import locate_model as M
import np_restatement as R

Z_MARKED, Z_UNMARKED = 15.0, 6.0
PAIR_BOUND = 1e-12  # of sigma_W, f64


@pytest.mark.parametrize("kshape,shape,at", LK.CASES)
def test_one_complex_transform_carries_two_keys(kshape, shape, at):
    bank = LK.bank_of(kshape)
    x = LK.frames_of(kshape, shape, at, 1)[0]
    c = R.coefficients(x)
    h = M.h_plane(x, c, 1)
    for a, b in ((0, 1), (3, 4)):
        re, im = LK.pair_maps(h, bank[a], bank[b])
        sw = max(M.sigma_w(x, bank[a], c, 1), M.sigma_w(x, bank[b], c, 1))
        ea, eb = np.abs(re - M.correlate(h, bank[a])).max() / sw, np.abs(im - M.correlate(h, bank[b])).max() / sw
        print(f"{kshape}->{shape} keys ({a}, {b}): {ea:.2e} and {eb:.2e} sigma_W")
        assert ea <= PAIR_BOUND and eb <= PAIR_BOUND
    # the odd last key: a zero imaginary half gives a zero imaginary map, to the same bound
    re, im = LK.pair_maps(h, bank[4], np.zeros_like(bank[4]))
    sw = M.sigma_w(x, bank[4], c, 1)
    assert np.abs(re - M.correlate(h, bank[4])).max() <= PAIR_BOUND * sw and np.abs(im).max() <= PAIR_BOUND * sw


def test_per_key_model_is_wm_locates():
    kshape, shape, at = LK.CASES[1]
    bank = LK.bank_of(kshape).copy()
    bank[2] = 0.0
    x = LK.frames_of(kshape, shape, at, 0)[0]
    c = R.coefficients(x)
    maps, loc = LK.locate_keys(x, bank, c, 0)
    for k in range(LK.NKEYS):
        want_map, want_loc = M.locate(x, bank[k], c, 0)
        assert np.array_equal(maps[k], want_map) and np.array_equal(loc[k], np.array(want_loc), equal_nan=True)
    assert not maps[2].any() and list(loc[2][:3]) == [0, 0, 0] and np.isnan(loc[2][3])


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", LK.CASES)
def test_finding_table(kshape, shape, at, mask):
    bank = LK.bank_of(kshape)
    for dtype in ("f32", "u8"):
        xs = LK.frames_of(kshape, shape, at, mask, dtype)
        for f, owner in enumerate(LK.OWNER):
            x = xs[f].astype(np.float32)
            _, loc = LK.locate_keys(x, bank, R.coefficients(x), mask)
            best, z_best, z_next = LK.rank(loc)
            print(f"{kshape}->{shape}@{at} mask {mask} {dtype} frame {f}: z {np.round(loc[:, 3], 2)}; rank ({best}, {z_best:.2f}, {z_next:.2f})")
            for k in range(LK.NKEYS):
                if k == owner:
                    assert (int(loc[k][0]), int(loc[k][1])) == at and loc[k][3] >= Z_MARKED
                else:
                    assert loc[k][3] <= Z_UNMARKED
            if owner is not None:
                assert best == owner and z_best >= Z_MARKED and z_next <= Z_UNMARKED


def test_rank_rules():
    nan = float("nan")

    def rec(*zs):
        return np.array([[0, 0, 0, z] for z in zs], np.float64)

    def same(a, b):
        return a[0] == b[0] and all((np.isnan(x) and np.isnan(y)) or x == y for x, y in zip(a[1:], b[1:]))

    assert same(LK.rank(rec(1.0, 7.0, 3.0)), (1, 7.0, 3.0))
    assert same(LK.rank(rec(7.0, 7.0, 3.0)), (0, 7.0, 7.0))          # a tie goes to the smallest index, its twin is the next
    assert same(LK.rank(rec(nan, 2.0, nan, 5.0)), (3, 5.0, 2.0))     # NaN is ignored
    assert same(LK.rank(rec(nan, 2.0, nan)), (1, 2.0, nan))          # no other key with a z
    assert same(LK.rank(rec(4.0)), (0, 4.0, nan))
    assert same(LK.rank(rec(nan, nan)), (-1, nan, nan))
    assert same(LK.rank(rec(-3.0, -1.0)), (1, -1.0, -3.0))
