"""CPU tests of the identities behind wm_locate_bits (tests/locate_bits_model.py): the per-bit maps add up to wm_locate's map, one
complex transform carries two of them, and on payload-marked crops the energy map names the true offset where wm_locate's own map
has no peak, an unmarked crop has none either, and every bit with enough pixels in the window is read.

Set-up: psnr 40, p = 3, 32 x 32 tiles on the key plane, wm_bits_layout's table with seed 5, frame 10 of synth_frame, a random
BALANCED payload (as many set bits as clear ones: a lopsided payload leaves a net mark, and the whole-key map of one drawn bit by
bit reached z 18-29 here).  Thresholds: z(E) >= 60 marked, <= 15 unmarked, wm_locate's own z <= 10 on the payload copy; they sit
between the values seen with this set-up (printed by the test): marked 149-694, unmarked 5.4-9.4, whole map on the payload copy
3.2-4.5; the weakest covered bit reads |soft| 4.2 at 672 px."""
import numpy as np
import pytest

import bits_model as B
import locate_bits_model as LB
import locate_model as M
import np_restatement as R
from synth import synth_frame, synth_watermark

TH = TW = 32
SEED = 5
Z_MARKED, Z_UNMARKED, Z_WHOLE = 60.0, 15.0, 10.0
MIN_COVER = 512
# (key shape, crop shape, true offset, bits, floored to 8 bits)
ROWS = [((120, 330), (64, 256), (20, 31), 8, False), ((270, 480), (200, 384), (37, 53), 16, False),
        ((270, 480), (200, 384), (37, 53), 16, True), ((300, 520), (96, 128), (150, 300), 8, False)]
_made = {}


def table(kshape, nbits):
    ny, nx = LB.tiles_shape(kshape[0], kshape[1], TH, TW)
    return B.layout(ny, nx, nbits, SEED)


def payload_copy(kshape, nbits, mask):
    """(x, y, W, bits): frame 10 marked at the key's shape with a random payload: +W where the tile's bit is set, -W where not"""
    tag = (kshape, nbits, mask)
    if tag not in _made:
        x = synth_frame(*kshape, frame=10)
        W = synth_watermark(*kshape, seed=9100 + 7 * kshape[0] + kshape[1])
        bits = LB.balanced_payload(nbits, 77 + nbits + kshape[0])
        name = "ME" if mask == 0 else "NVF"
        yp, _ = R.embed(x, x, W, 3, 40.0, name)
        ym, _ = R.embed(x, x, -W, 3, 40.0, name)
        s = LB.signs_plane(kshape, TH, TW, table(kshape, nbits), bits)
        _made[tag] = (x, np.where(s > 0, yp, np.where(s < 0, ym, x)).astype(np.float32), W, bits)
    return _made[tag]


def test_maps_add_up_to_the_whole_map():
    kshape, shape, at = (120, 330), (64, 256), (20, 31)
    _, y, W, _ = payload_copy(kshape, 8, 0)
    crop = y[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]]
    h = M.h_plane(crop, R.coefficients(crop), 0)
    mp = LB.maps(h, W, TH, TW, table(kshape, 8), 8)
    whole = M.correlate(h, W)
    assert np.abs(mp.sum(axis=0) - whole).max() <= 1e-9 * np.abs(whole).max()


def test_one_complex_transform_carries_two_maps():
    kshape, shape, at = (120, 330), (64, 256), (20, 31)
    _, y, W, _ = payload_copy(kshape, 8, 1)
    crop = y[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]]
    h = M.h_plane(crop, R.coefficients(crop), 1)
    tb = table(kshape, 8)
    ka, kb = LB.key_b(W, TH, TW, tb, 2), LB.key_b(W, TH, TW, tb, 3)
    re, im = LB.pair_maps(h, ka, kb)
    wa, wb = M.correlate(h, ka), M.correlate(h, kb)
    scale = max(np.abs(wa).max(), np.abs(wb).max())
    assert np.abs(re - wa).max() <= 1e-9 * scale and np.abs(im - wb).max() <= 1e-9 * scale
    # an odd last bit: a zero imaginary key gives a zero imaginary map
    _, im0 = LB.pair_maps(h, ka, np.zeros_like(ka))
    assert np.abs(im0).max() <= 1e-9 * scale


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("kshape,shape,at,nbits,floored", ROWS)
def test_payload_copy_is_found_and_read(kshape, shape, at, nbits, floored, mask):
    x, y, W, bits = payload_copy(kshape, nbits, mask)
    (r, c), (oy, ox) = shape, at
    crop, plain = y[oy:oy + r, ox:ox + c], x[oy:oy + r, ox:ox + c]
    if floored:
        crop, plain = np.floor(crop), np.floor(plain)
    crop, plain = np.ascontiguousarray(crop, np.float32), np.ascontiguousarray(plain, np.float32)
    tb = table(kshape, nbits)
    cc = R.coefficients(crop)
    _, _, (gy, gx, _, z), soft = LB.locate_bits(crop, W, cc, mask, TH, TW, tb, nbits)
    _, (_, _, _, z_whole) = M.locate(crop, W, cc, mask)
    _, _, (_, _, _, z_plain), _ = LB.locate_bits(plain, W, R.coefficients(plain), mask, TH, TW, tb, nbits)
    cov = LB.cover(shape, kshape, TH, TW, tb, nbits, oy, ox)
    read = cov >= MIN_COVER
    weakest = np.abs(soft[read]).min()
    print(f"{kshape}->{shape}@{at} mask {mask} floored {floored}: E ({gy}, {gx}) z {z:.1f}; whole map z {z_whole:.2f}; unmarked z(E) {z_plain:.2f}; "
          f"{int(read.sum())} of {nbits} bits covered, weakest |soft| {weakest:.2f}, least cover {int(cov[read].min())} px")
    assert (gy, gx) == at and z >= Z_MARKED
    assert z_whole <= Z_WHOLE and z_plain <= Z_UNMARKED
    assert np.array_equal((soft > 0)[read], bits[read] == 1)
    # a bit without a pixel in the window reads about zero (in standard deviations of its own map)
    assert np.all(np.abs(soft[cov == 0]) < 5.0)


def test_plainly_marked_copy_is_found_too():
    kshape, shape, at = (120, 330), (64, 256), (20, 31)
    x = synth_frame(*kshape, frame=10)
    W = synth_watermark(*kshape, seed=9100 + 7 * kshape[0] + kshape[1])
    y, _ = R.embed(x, x, W, 3, 40.0, "ME")
    crop = np.ascontiguousarray(y[at[0]:at[0] + shape[0], at[1]:at[1] + shape[1]])
    tb = table(kshape, 8)
    _, _, (gy, gx, _, z), soft = LB.locate_bits(crop, W, R.coefficients(crop), 0, TH, TW, tb, 8)
    cov = LB.cover(shape, kshape, TH, TW, tb, 8, *at)
    assert (gy, gx) == at and z >= Z_MARKED and np.all(soft[cov >= MIN_COVER] > 0)


def test_soft_and_cover_rules():
    rng = np.random.default_rng(1)
    mp = rng.normal(size=(3, 6, 7))
    mp[1] = 0.0  # a bit without a tile: no variation
    s = LB.soft(mp, 2, 3)
    out = np.ones((6, 7), bool)
    out[1:4, 2:5] = False
    assert np.isnan(s[1]) and abs(s[0] - (mp[0, 2, 3] - mp[0][out].mean()) / mp[0][out].std()) < 1e-12
    assert np.all(np.isnan(LB.soft(rng.normal(size=(2, 2, 2)), 0, 0)))  # every offset lies inside the block
    # remainder tiles and -1 tiles: 70 x 100 key, 32 x 32 tiles -> 2 x 3 tiles, the last row 38 and the last column 36 wide
    tb = np.array([0, 1, -1, 2, 0, 1], np.int32)
    cov = LB.cover((70, 100), (70, 100), 32, 32, tb, 3, 0, 0)
    assert list(cov) == [32 * 32 + 38 * 32, 32 * 32 + 38 * 36, 38 * 32]
    assert list(LB.cover((10, 10), (70, 100), 32, 32, tb, 3, 60, 90)) == [0, 100, 0]
