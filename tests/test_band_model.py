"""tests/band_model.py against the whole-image oracle, and the pure split rules of watermarking-gpu_amd/bands.py (no GPU).

(1) For any split of [0, R) into bands the band values add up to the whole image's: the 44 Gram sums to O.gram, the stats and the
    detector sums to the whole-image values (and through them to O.embed's strength and O.detect's score).
(2) bands.band_with_halo tiles [0, rows) and gives planes that wm_band_configure's halo rule accepts -- for every split that
    bands.check_split lets through; the splits it refuses (a rank with fewer rows than the halo) are exactly those in which
    exchange_halos would send halo rows, and among them are all the splits whose planes the halo rule refuses."""
import importlib

import numpy as np
import pytest

import band_model as BM
import oracle_lib as O
from synth import synth_frame, synth_watermark

R = 40
SHAPES = [(R, 131), (R, 272)]
WINDOWS = [("ME", 3), ("NVF", 3), ("NVF", 9)]


def splits(p):
    h = BM.halo_need(p)
    yield "whole", [(0, R)]
    yield "even3", [(0, 14), (14, 27), (27, R)]
    yield "ragged", [(0, h), (h, h + 1), (h + 1, R - 2), (R - 2, R)]      # the two-row bottom band
    yield "one-row-bottom", [(0, R - 1), (R - 1, R)]                      # band_model's rule for the border rows holds here too
    yield "rows", [(r, r + 1) for r in range(R)]


@pytest.fixture(scope="module")
def bands():
    return importlib.import_module("watermarking-gpu_amd.bands")


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gram_sums_of_the_bands_add_up_to_the_oracle(shape, dtype):
    x = synth_frame(*shape, frame=3, dtype=np.uint8 if dtype == "u8" else np.float32)
    whole = BM.oracle_gram_totals(x)
    # the position rows of a split tile -1 .. R with none twice
    for name, split in splits(9):
        rows = sorted(r for (r0, r1) in split for r in BM.position_rows(R, r0, r1))
        assert rows == list(range(-1, R + 1)), name
    for name, split in list(splits(3)) + list(splits(9)):
        tot = sum(BM.gram_sums(x, r0, r1) for (r0, r1) in split)
        if dtype == "u8":
            np.testing.assert_array_equal(tot, whole, err_msg=name)    # integers below 2^53: exact in any order
        else:
            np.testing.assert_allclose(tot, whole, rtol=1e-13, atol=0, err_msg=name)
    # a one-row bottom band takes the border rows R-2, R-1, R: it is not the sum over its own row's positions alone
    assert BM.position_rows(R, R - 1, R) == [R - 2, R - 1, R] and BM.position_rows(R, 0, R - 1)[-1] == R - 3


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: f"{w[0]}{w[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stats_and_detector_sums_of_the_bands_add_up(shape, win):
    mask, p = win
    omask = O.MASK_ME if mask == "ME" else O.MASK_NVF
    x = synth_frame(*shape, frame=3)
    W = synth_watermark(*shape)
    fr = BM.Frame(x, W, p, omask)
    mx_w, ss_w = fr.stats(0, R)
    so, yo, ao = O.embed(x, x, W, p=p, mask=omask)
    assert so == 0 and BM.strength(mx_w, ss_w, R * shape[1]) == pytest.approx(ao, rel=1e-6)   # (the oracle rounds to f32 on the way)
    fy = BM.Frame(yo, W, p, omask)
    sums_w = fy.detect_sums(0, R)
    assert BM.corr_of(sums_w) == pytest.approx(O.detect(yo, W, p=p, mask=omask)[1], abs=1e-6)
    for name, split in splits(p):
        st = [fr.stats(r0, r1) for (r0, r1) in split]
        assert max(s[0] for s in st) == mx_w, name                      # a maximum has no order: exact
        assert (mx_w == 1.0) == (mask == "NVF")
        assert sum(s[1] for s in st) == pytest.approx(ss_w, rel=1e-13), name
        sums = sum(fy.detect_sums(r0, r1) for (r0, r1) in split)
        # nu, nw are sums of squares; the dot has terms of both signs: its bound is on the scale of its terms, sqrt(nu nw)
        np.testing.assert_allclose(sums[1:], sums_w[1:], rtol=1e-13, err_msg=name)
        assert abs(sums[0] - sums_w[0]) <= 1e-13 * np.sqrt(sums_w[1] * sums_w[2]), name


def test_band_with_halo_tiles_the_image_and_keeps_the_halo_rule(bands):
    refused_by_rule = 0
    for rows in range(8, 65):
        for world in range(1, 9):
            own = [bands.band_rows(rows, r, world) for r in range(world)]
            assert own[0][0] == 0 and own[-1][1] == rows
            assert all(a[1] == b[0] for a, b in zip(own, own[1:])) and all(r0 < r1 for r0, r1 in own)   # no gap, no overlap, none empty
            for p in (3, 5, 7, 9):
                halo = bands.halo_rows(p)
                assert halo == BM.halo_need(p)
                planes = [bands.band_with_halo(rows, r, world, halo) for r in range(world)]
                for (g0, g1, lo, hi), (r0, r1) in zip(planes, own):
                    assert (g0 + lo, g0 + hi) == (r0, r1) and 0 <= g0 <= r0 and r1 <= g1 <= rows
                rule = all(BM.halo_rule(g1 - g0, lo, hi, p) for (g0, g1, lo, hi) in planes)
                thin = world > 1 and min(r1 - r0 for r0, r1 in own) < halo
                if thin:
                    with pytest.raises(ValueError, match=f"rows = {rows} .*world = {world} .*p = {p}"):
                        bands.check_split(rows, world, p)
                    refused_by_rule += not rule
                else:
                    bands.check_split(rows, world, p)
                    # every plane has 4 rows or more and the halo's rows on every interior side
                    assert rule, (rows, world, p, planes)
    assert refused_by_rule > 0   # (rows = 8 over 8 ranks: the band above the last row holds one row below its own)


def test_check_split_refuses_a_rank_thinner_than_the_halo(bands):
    with pytest.raises(ValueError, match="rows = 10 .*world = 4 .*p = 9"):
        bands.check_split(10, 4, 9)
    bands.check_split(203, 2, 3)
    bands.check_split(3, 1, 9)      # one rank: nothing is exchanged


def test_the_halo_rule_keeps_the_one_row_bottom_band_out():
    """the band above [R-1, R) holds one row below its own; an interior side needs two or more for every p"""
    for p in (3, 5, 7, 9):
        assert not BM.halo_rule(R, 0, R - 1, p)
        assert BM.halo_rule(R, 0, R - BM.halo_need(p), p)
        plane = max(4, BM.halo_need(p) + 1)
        assert BM.halo_rule(plane, plane - 1, plane, p)   # the one-row bottom band's own plane passes: the split is refused at the band above
