"""CPU tests of the clip-pooling model (tests/locate_clip_model.py; wm.h wm_clip_pool), f64 throughout.

Linearity: the map of the pooled plane is the weighted sum of the frames' maps, to 1e-12 sigma_W (f64 FFTs of a few hundred
thousand points sit three orders below that).  The finding table, as conditions on the inputs the GPU tests use too: on clips of 8
frames marked at PSNR 52 (ME) / 50 (NVF) no single frame reaches z = 15, the pooled clip does at the true offset, and the unmarked
clip and another key stay at or below 6.  The payload clip: frame 0 alone misreads a bit, the pooled clip reads all eight.  Weights:
unequal ones, and a weight of 0 equals leaving the frame out."""
import numpy as np
import pytest

import locate_clip_model as LC
import locate_keys_model as LK
import locate_model as M
import np_restatement as R

_h = {}


def planes(kshape, shape, at, mask, marked=True):
    """the clip's frames and their image-side planes with the model's own coefficients, computed once"""
    tag = (kshape, shape, at, mask, marked)
    if tag not in _h:
        xs = LC.clip_of(kshape, shape, at, mask, marked)
        _h[tag] = (xs, LC.clip_h(xs, [R.coefficients(x) for x in xs], mask))
    return _h[tag]


@pytest.mark.parametrize("mask", [0, 1])
def test_linearity(mask):
    kshape, shape, at = LC.CASES[1]
    key = LC.key_of(kshape)
    _, hs = planes(kshape, shape, at, mask)
    for w in (None, 1.0 / (1.0 + np.arange(len(hs))), np.array([1, -2, 0, 3, 0.5, 0, -1, 4.0])):
        hp = LC.pool(hs, w)
        ww = np.ones(len(hs)) if w is None else w
        want = sum(wf * M.correlate(h, key) for wf, h in zip(ww, hs))
        got, _ = LC.locate_pooled(hp, key)
        scale = sum(abs(wf) * LC.sigma_w(h, key) for wf, h in zip(ww, hs))
        err = float(np.abs(got - want).max()) / scale
        print(f"mask {mask} weights {None if w is None else list(np.round(w, 3))}: {err:.2e} sigma_W")
        assert err <= 1e-12
    # per payload bit and per key of a bank
    assert kshape == LC.P_KSHAPE
    tb = LC.payload_table()
    mp, _, _, _ = LC.locate_bits_pooled(LC.pool(hs), key, 32, 32, tb, 8)
    want = sum(LC.locate_bits_pooled(h, key, 32, 32, tb, 8)[0] for h in hs)
    assert np.abs(mp - want).max() <= 1e-12 * sum(LC.sigma_w(h, key) for h in hs)
    bank = LK.bank_of(kshape, 3)
    maps, _ = LC.locate_keys_pooled(LC.pool(hs), bank)
    want = sum(LC.locate_keys_pooled(h, bank)[0] for h in hs)
    assert np.abs(maps - want).max() <= 1e-12 * sum(LC.sigma_w(h, bank[0]) for h in hs)


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at", LC.CASES)
def test_pooled_clip_is_found_where_no_frame_is(kshape, shape, at, mask):
    key = LC.key_of(kshape)
    _, hs = planes(kshape, shape, at, mask)
    zs = [M.fold(M.correlate(h, key))[3] for h in hs]
    _, (oy, ox, _, z) = LC.locate_pooled(LC.pool(hs), key)
    _, hu = planes(kshape, shape, at, mask, marked=False)
    z_unmarked = LC.locate_pooled(LC.pool(hu), key)[1][3]
    z_other = LC.locate_pooled(LC.pool(hs), LC.key_of(kshape, other=True))[1][3]
    print(f"{kshape}->{shape}@{at} mask {mask}: per-frame z {min(zs):.1f}-{max(zs):.1f}; pooled ({oy}, {ox}) z {z:.1f}; unmarked clip {z_unmarked:.1f}; "
          f"other key {z_other:.1f}")
    assert max(zs) < LC.Z_MARKED
    assert (oy, ox) == at and z >= LC.Z_MARKED
    assert z_unmarked <= LC.Z_UNMARKED and z_other <= LC.Z_UNMARKED


@pytest.mark.parametrize("mask", [0, 1])
def test_payload_clip_is_read_where_frame_0_is_not(mask):
    key = LC.key_of(LC.P_KSHAPE)
    xs = LC.payload_clip(mask)
    hs = LC.clip_h(xs, [R.coefficients(x) for x in xs], mask)
    tb, bits = LC.payload_table(), LC.payload_bits()
    _, _, _, soft0 = LC.locate_bits_pooled(hs[0], key, *LC.P_TILE, tb, LC.P_NBITS)
    _, _, (oy, ox, _, z), soft = LC.locate_bits_pooled(LC.pool(hs), key, *LC.P_TILE, tb, LC.P_NBITS)
    wrong0 = int(((soft0 > 0) != (bits == 1)).sum())
    print(f"mask {mask}: frame 0 misreads {wrong0} bit(s); pooled E ({oy}, {ox}) z {z:.1f}, weakest |soft| {np.abs(soft).min():.2f}")
    assert wrong0 >= 1
    assert (oy, ox) == LC.P_AT and np.array_equal(soft > 0, bits == 1) and np.abs(soft).min() >= 3.0


def test_weights():
    kshape, shape, at = LC.CASES[0]
    key = LC.key_of(kshape)
    _, hs = planes(kshape, shape, at, 0)
    # a weight of 0 equals leaving the frame out
    w = np.ones(len(hs))
    w[2] = w[5] = 0.0
    kept = [h for f, h in enumerate(hs) if f not in (2, 5)]
    assert np.array_equal(LC.pool(hs, w), LC.pool(kept))
    # unequal weights: the pooled map is the weighted sum, and the clip is still found
    w = 1.0 / (1.0 + np.arange(len(hs)))
    m, (oy, ox, _, z) = LC.locate_pooled(LC.pool(hs, w), key)
    assert (oy, ox) == at and z > max(M.fold(M.correlate(h, key))[3] for h in hs)
    # 1 / ||h_f||_2 gives the plain sum's z to three digits (0.5 %; the eight clips differ by 0.006-0.23 %): the default is the plain sum
    wn = np.array([1.0 / np.sqrt(np.sum(h * h)) for h in hs])
    z_plain, z_norm = LC.locate_pooled(LC.pool(hs), key)[1][3], LC.locate_pooled(LC.pool(hs, wn), key)[1][3]
    print(f"z plain sum {z_plain:.3f}, weights 1/||h|| {z_norm:.3f}")
    assert abs(z_plain - z_norm) <= 5e-3 * z_plain
    with pytest.raises(AssertionError):
        LC.pool(hs, np.ones(3))
