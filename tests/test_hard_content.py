"""The hard-content families (tests/hard_frames.py) on the CPU: every family's self-check (the property that makes it hard,
computed with the oracle), the oracle against the independent numpy restatement on every family (the tolerances of
test_oracle_vs_numpy_restatement_pinned_nvf), and the zero-energy rule of makeWatermark in the oracle: ||u|| = 0 gives
a = +inf with status OK and out == base bit for bit, f32 and u8."""
import numpy as np
import pytest

import hard_frames as H
import np_restatement as NP
import oracle_lib as O

R, C = 130, 516  # two full strips and a shifted last strip (516 = 2 * 256 + 4)
MASKS = ((O.MASK_ME, "ME"), (O.MASK_NVF, "NVF"))


def restatement_agrees(x, base, W, psnr=40.0, masks=MASKS, detect=True):
    """oracle vs np_restatement: Gram rtol 1e-12, coefficients 2e-6, strength rel 1e-5, y 2e-3, score 1e-5"""
    Rx, rx = O.gram(x)
    Rn, rn = NP.gram(x)
    np.testing.assert_allclose(Rx, Rn, rtol=1e-12)
    np.testing.assert_allclose(rx, rn, rtol=1e-12)
    for p in (3, 5, 7, 9):
        np.testing.assert_allclose(O.nvf_mask(x, p), NP.nvf_mask(x, p), rtol=0, atol=1e-6)
    for mask, name in masks:
        if mask == O.MASK_ME:
            st, c, e, m, mx = O.me_mask(x)
            assert st == O.OK
            np.testing.assert_allclose(c, NP.coefficients(x), atol=2e-6)
        st, y, a = O.embed(x, base, W, psnr=psnr, mask=mask)
        assert st == O.OK
        yn, an = NP.embed(x, base, W, psnr=psnr, mask=name)
        assert a == pytest.approx(an, rel=1e-5)
        np.testing.assert_allclose(y, yn, rtol=0, atol=2e-3)
        if detect:
            st, corr = O.detect(y, W, mask=mask)
            with np.errstate(invalid="ignore", divide="ignore"):
                cn = NP.detect(yn, W, mask=name)
            if np.isnan(corr):
                assert np.isnan(cn)
            else:
                assert corr == pytest.approx(cn, abs=1e-5)


# ---- clipped --------------------------------------------------------------------------------------------------------------
def test_clipped_self_check():
    x = H.clipped(R, C)
    W = H.watermark(R, C)
    assert 0.15 <= ((x == 0) | (x == 255)).mean() <= 0.3
    frac = {}
    for psnr in (10, 25, 40, 60):
        for mask, name in MASKS:
            st, y, a = O.embed(x, x, W, psnr=psnr, mask=mask)
            assert st == O.OK
            frac[psnr, name] = H.clamped_fraction(y, x)
    for _, name in MASKS:
        assert frac[10, name] >= 0.10, frac        # the clamp changes >= 10 % of the pixels at 10 dB
        assert frac[25, name] >= 0.01, frac
        assert frac[10, name] > frac[25, name] > frac[40, name] > frac[60, name] > 0, frac
    grey, rgb = H.clipped_rgb(R, C)
    st, y, a = O.embed(grey, rgb, W, psnr=25)
    assert st == O.OK
    assert (rgb[0] == 255).mean() >= 0.1 and (rgb[2] == 0).mean() >= 0.1
    assert H.clamped_fraction(y[0], rgb[0]) >= 0.1 and H.clamped_fraction(y[2], rgb[2]) >= 0.1
    np.testing.assert_array_equal(O.rgb2gray(rgb), grey)


@pytest.mark.parametrize("psnr", [10, 25, 40, 60])
def test_clipped_restatement(psnr):
    x = H.clipped(R, C, frame=1)
    restatement_agrees(x, x, H.watermark(R, C), psnr=psnr)


def test_clipped_rgb_restatement():
    grey, rgb = H.clipped_rgb(R, C)
    W = H.watermark(R, C)
    for mask, name in MASKS:
        st, y, a = O.embed(grey, rgb, W, psnr=25, mask=mask)
        yn, an = NP.embed(grey, rgb, W, psnr=25, mask=name)
        assert a == pytest.approx(an, rel=1e-5)
        np.testing.assert_allclose(y, yn, rtol=0, atol=2e-3)


# ---- letterbox ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 16])
@pytest.mark.parametrize("pillar", [False, True])
def test_letterbox_self_check(level, pillar):
    k = 12
    for dtype in (np.float32, np.uint8):
        x = H.letterbox(R, C, k, level, pillar=pillar, dtype=dtype)
        bars = np.zeros((R, C), bool)
        if pillar:
            bars[:, :k] = bars[:, C - k:] = True
        else:
            bars[:k] = bars[R - k:] = True
        assert (x[bars] == level).all() and (x[~bars] != level).mean() > 0.9
        xf = x.astype(np.float32)
        for p in (3, 5, 9):
            m = O.nvf_mask(xf, p)
            inner = H.bar_interior(R, C, k, pillar=pillar, halo=p // 2)
            assert inner.sum() > 0 and (m[inner] == 0).all()
            assert (m[~bars] > 0).mean() > 0.99
        st, c, e, m, mx = O.me_mask(xf)
        assert st == O.OK
        # deep inside a bar every neighbour equals the pixel: e = level (1 - sum c)
        inner = H.bar_interior(R, C, k, pillar=pillar, halo=1)
        assert np.unique(e[inner]).size == 1


@pytest.mark.parametrize("level", [0, 16])
def test_letterbox_restatement(level):
    W = H.watermark(R, C)
    for pillar in (False, True):
        x = H.letterbox(R, C, 12, level, pillar=pillar)
        restatement_agrees(x, x, W)


# ---- binary ---------------------------------------------------------------------------------------------------------------
def test_binary_self_check():
    x = H.binary(R, C)
    assert set(np.unique(x)) == {0.0, 255.0}
    Rx, rx = O.gram(x)
    tot = H.integer_gram(x)
    iu = np.triu_indices(8)
    np.testing.assert_array_equal(Rx[iu], tot[:36].astype(np.float64))
    np.testing.assert_array_equal(rx, tot[36:].astype(np.float64))
    assert H.pivot_ratio(Rx) >= 1e-3
    assert O.embed(x, x, H.watermark(R, C))[0] == O.OK


def test_binary_u8_reaches_the_lag_sum_bound():
    """4352 x 256 u8, nearly all 255: with 4096 rows per segment a lane's 4-column sum of one lag product over a segment comes
    close to the 4 * 255^2 * 4096 that k_gram's u32 accumulators are sized for (wm_k_gram.hip)"""
    x = H.binary(4352, 256, p255=0.98, dtype=np.uint8)
    xi = x.astype(np.int64)
    seg = xi[:4096]
    lane = (seg * seg).reshape(4096, 64, 4).sum(axis=(0, 2))  # the centre-times-centre term, per lane of 4 columns
    bound = 4 * 255 ** 2 * 4096
    assert lane.max() >= 0.9 * bound and lane.max() < 2 ** 32
    tot = H.integer_gram(x)
    Rx, rx = O.gram(x.astype(np.float32))
    np.testing.assert_array_equal(rx, tot[36:].astype(np.float64))
    assert H.pivot_ratio(Rx) >= 1e-6


def test_binary_restatement():
    restatement_agrees(H.binary(R, C, seed=1), H.binary(R, C, seed=1), H.watermark(R, C))


# ---- singular -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", H.SINGULAR_KINDS)
@pytest.mark.parametrize("shape", [(R, C), (64, 260), (1080, 1920)])
def test_singular_self_check(kind, shape):
    x = H.singular(kind, *shape)
    assert x.min() >= 0 and x.max() <= 255
    assert np.array_equal(x, np.floor(x * 16) / 16)  # multiples of 1/16: exact sums
    Rx, rx = O.gram(x)
    Rn, rn = NP.gram(x)
    np.testing.assert_array_equal(Rx, Rn)           # exact sums on both sides
    assert H.pivot_ratio(Rx) <= 1e-13               # >= 10x below the solve's 1e-12
    W = H.watermark(*shape)
    base = H.clipped(*shape)
    st, y, a = O.embed(x, base, W, mask=O.MASK_ME)  # (NVF embeds need no solve; their detector does)
    assert st == O.UNSOLVABLE and np.array_equal(y, base) and np.isnan(a)
    for mask in (O.MASK_ME, O.MASK_NVF):
        st, corr = O.detect(x, W, mask=mask)
        assert st == O.UNSOLVABLE and corr == 0.0


@pytest.mark.parametrize("shape", [(R, C), (64, 260), (1080, 1920)])
def test_near_singular_self_check(shape):
    x = H.near_singular(*shape)
    Rx, rx = O.gram(x)
    assert H.pivot_ratio(Rx) >= 1e-10 and np.linalg.cond(Rx) <= 1e7
    assert H.pivot_ratio(Rx) <= 1e-4                # ... and still far from an ordinary frame
    for mask in (O.MASK_ME, O.MASK_NVF):
        assert O.embed(x, x, H.watermark(*shape), mask=mask)[0] == O.OK
        assert O.detect(x, H.watermark(*shape), mask=mask)[0] == O.OK


def test_near_singular_restatement():
    x = H.near_singular(R, C)
    restatement_agrees(x, x, H.watermark(R, C))


# ---- impulse --------------------------------------------------------------------------------------------------------------
IMPULSE_GEOMS = [(R, C, 16, None, (43, 87)), (130, 512, 16, 64, ()), (257, 764, 32, 128, (86, 172))]


@pytest.mark.parametrize("geom", IMPULSE_GEOMS)
def test_impulse_self_check(geom):
    rows, cols, rps, tile, bands = geom
    spots = H.impulse_spots(rows, cols, rps=rps, tile_rows=tile, band_rows=bands)
    assert {"corner_tl", "corner_br", "row_1", "row_R-2", "col_1", "col_C-2", "strip_c255", "strip_c256"} <= set(spots)
    if cols % 256:
        assert "dup_first" in spots and "dup_last" in spots
    xs, items = H.impulse(rows, cols, spots)
    for x, (name, r, c) in zip(xs, items):
        st, cf, e, m, mx = O.me_mask(x)
        assert st == O.OK
        ae = np.abs(e)
        assert np.unravel_index(np.argmax(ae), ae.shape) == (r, c), name
        rest = ae.copy()
        rest[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = 0
        assert ae[r, c] >= 1.5 * rest.max(), (name, ae[r, c] / rest.max())
        assert mx == ae[r, c] and m[r, c] == 1.0


def test_impulse_restatement():
    spots = H.impulse_spots(R, C, rps=16, band_rows=(43, 87))
    xs, items = H.impulse(R, C, spots)
    W = H.watermark(R, C)
    for f in (0, 3, len(items) - 1):
        restatement_agrees(xs[f], xs[f], W)


# ---- zero-energy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,level", H.FLAT_LEVELS)
def test_zero_energy_flat_nvf(dtype, level):
    """an integer-flat frame under NVF: the mask is exactly 0, so ||u|| = 0, a = +inf, out == base, status OK"""
    x = H.flat(R, C, level, dtype)
    W = H.watermark(R, C)
    xf = x.astype(np.float32)
    for p in (3, 5, 9):
        m = O.nvf_mask(xf, p)
        assert (m == 0).all() and np.sum((m.astype(np.float64) * W) ** 2) == 0.0
        st, y, a = O.embed(xf, xf, W, p=p, mask=O.MASK_NVF)
        assert st == O.OK and a == np.inf and np.array_equal(y, xf)
    if dtype == np.uint8:
        st, y8, a = O.embed_u8(x, W, mask=O.MASK_NVF)
        assert st == O.OK and a == np.inf and np.array_equal(y8, x)
    # another base than the (flat) input: the base comes back bit for bit, values at 0 and 255 included
    base = H.clipped(R, C)
    st, y, a = O.embed(xf, base, W, mask=O.MASK_NVF)
    assert st == O.OK and a == np.inf and np.array_equal(y, base)
    yn, an = NP.embed(xf, base, W, mask="NVF")
    assert an == np.inf and np.array_equal(yn, base)
    # the detector's prediction system of a flat frame is singular
    assert O.detect(xf, W, mask=O.MASK_NVF) == (O.UNSOLVABLE, 0.0)


def test_zero_energy_zero_w():
    """an all-zero W: u = 0 under either mask; embed gives a = +inf and out == base, detect 0 / 0 = NaN with status OK"""
    x = H.clipped(R, C)
    Z = H.zero_w(R, C)
    x8 = H.clipped(R, C, dtype=np.uint8)
    for mask, name in MASKS:
        st, y, a = O.embed(x, x, Z, mask=mask)
        assert st == O.OK and a == np.inf and np.array_equal(y, x)
        grey, rgb = H.clipped_rgb(R, C)
        st, y, a = O.embed(grey, rgb, Z, mask=mask)
        assert st == O.OK and a == np.inf and np.array_equal(y, rgb)
        st, y8, a = O.embed_u8(x8, Z, mask=mask)
        assert st == O.OK and a == np.inf and np.array_equal(y8, x8)
        st, corr = O.detect(x, Z, mask=mask)
        assert st == O.OK and np.isnan(corr)
        st, corr = O.detect_u8(x8, Z, mask=mask)
        assert st == O.OK and np.isnan(corr)
        yn, an = NP.embed(x, x, Z, mask=name)
        assert an == np.inf and np.array_equal(yn, x)
        with np.errstate(invalid="ignore"):
            assert np.isnan(NP.detect(x, Z, mask=name))


def test_zero_energy_restatement():
    restatement_agrees(H.clipped(R, C), H.clipped(R, C), H.zero_w(R, C))


def test_non_integer_flat_frame_is_not_zero_energy():
    """77.3 everywhere: the NVF variance is a rounding residue, tiny but not 0 -- an ordinary (huge, finite) strength; the
    GPU tests hold the kernels to the oracle's result here whatever it is"""
    x = H.flat(R, C, 77.3)
    W = H.watermark(R, C)
    m = O.nvf_mask(x, 3)
    assert np.unique(m).size == 1 and m[0, 0] != 0 and abs(m[0, 0]) < 1e-2
    st, y, a = O.embed(x, x, W, mask=O.MASK_NVF)
    assert st == O.OK and np.isfinite(a) and a > 1e3
    yn, an = NP.embed(x, x, W, mask="NVF")
    assert a == pytest.approx(an, rel=1e-5)
    np.testing.assert_allclose(y, yn, rtol=0, atol=2e-3)


# ---- hard crops of the crop search ----------------------------------------------------------------------------------------
Z_FOUND, Z_NOISE = 10.0, 6.0


@pytest.mark.parametrize("mask,p", H.LOCATE_CONFIGS)
@pytest.mark.parametrize("kshape,shape,at", H.LOCATE_GEOMS)
def test_locate_crops_self_check(kshape, shape, at, mask, p):
    """the facts the GPU tests of the crop search lean on, with the f64 model and np_restatement's coefficients: every marked crop
    but `binary` has its argmax at the true offset with z >= 10, every unmarked crop z <= 6, and the marked `binary` crop z <= 6 --
    the clamp takes the mark away, which is why it is a parity-only family.  Measured over the three geometries, marked z (ME /
    NVF) and the largest unmarked z: texture 18-28 / 22-26, 4.7; clipped 11.5-14.5 / 10.6-13.6, 4.3; letterbox 13-33 / 17-34, 4.2;
    pillar 15-30 / 21-27, 4.4; near_singular 16-24 / 40-113, 4.3; low_contrast 25-59 / 40-91, 4.3; binary 3.4-4.0 / 3.5-3.7, 4.0"""
    import locate_model as M
    key = H.locate_key(kshape)
    crops = H.locate_crops(kshape, shape, at, mask, p)
    assert {H.locate_family(n) for n in crops} == set(H.LOCATE_FAMILIES)
    for name, (marked, plain) in crops.items():
        findable, has_u8 = H.LOCATE_FAMILIES[H.locate_family(name)]
        assert marked.shape == shape and plain.shape == shape and marked.dtype == plain.dtype
        assert marked.dtype == (np.uint8 if name.endswith("_u8") else np.float32) and (has_u8 or not name.endswith("_u8"))
        xm, xp = marked.astype(np.float32), plain.astype(np.float32)
        _, (oy, ox, _, z) = M.locate(xm, key, NP.coefficients(xm), mask, p)
        _, (_, _, _, zu) = M.locate(xp, key, NP.coefficients(xp), mask, p)
        print(f"{kshape}->{shape}@{at} mask {mask} p {p} {name}: marked ({oy}, {ox}) z {z:.1f}; unmarked z {zu:.2f}")
        if findable:
            assert (oy, ox) == at and z >= Z_FOUND, name
        else:
            assert z <= Z_NOISE, name
        assert zu <= Z_NOISE, name
        fam = H.locate_family(name)
        if fam == "clipped":
            assert ((xp == 0) | (xp == 255)).mean() >= 0.1 and ((xm == 0) | (xm == 255)).mean() >= 0.1
        if fam == "binary":
            assert set(np.unique(xp)) == {0.0, 255.0} and ((xm == 0) | (xm == 255)).mean() >= 0.4
        if fam in ("letterbox", "pillar"):
            bar = xp[:H.LOCATE_BAR] if fam == "letterbox" else xp[:, :H.LOCATE_BAR]
            rest = xp[H.LOCATE_BAR:] if fam == "letterbox" else xp[:, H.LOCATE_BAR:]
            level = 16.0 if fam == "letterbox" else 0.0
            assert (bar == level).all() and (rest != level).mean() > 0.9
            # under NVF the mask is exactly 0 where the GPU tests expect a pool of exactly 0 (an ME mark moves the whole bar)
            for mk, x in ((True, xm), (False, xp)) if mask == 1 else ((False, xp),):
                zero = H.locate_bar_zero(name, shape, p, mk)
                assert zero.sum() > 0 and (O.nvf_mask(x, p)[zero] == 0).all()
        if fam == "near_singular":
            ratio = H.pivot_ratio(O.gram(xp)[0])
            assert 1e-10 <= ratio <= 1e-4


@pytest.mark.parametrize("kshape,shape,at", H.LOCATE_GEOMS)
def test_locate_impulse_self_check(kshape, shape, at):
    """every impulse crop is solvable and, under every (mask, p), has its largest |h| within one pixel of the planted pixel; the
    spots cover the corners, the edges, k_clip_pool's tile seams and the last partial tile where the shape has them"""
    import locate_model as M
    spots = H.locate_impulse_spots(shape)
    assert {"corner_tl", "corner_tr", "corner_bl", "corner_br", "top", "bottom", "left", "right", "r1_c1"} <= set(spots)
    if shape[0] > 16 and shape[1] > 64:
        assert {"seam_r15_c63", "seam_r15_c64", "seam_r16_c63", "seam_r16_c64", "seam_r3_c64", "seam_r4_c63"} <= set(spots)
    if shape == (33, 66):
        assert spots["last_tile"] == (32, 64)
    assert len(set(spots.values())) == len(spots)
    for dtype in (np.float32, np.uint8):
        xs, items = H.locate_impulses(kshape, shape, at, dtype)
        assert xs.dtype == dtype and len(xs) == len(spots)
        for x, (name, r, c) in zip(xs, items):
            x = x.astype(np.float32)
            assert x[r, c] in (0.0, 255.0)
            cf = NP.coefficients(x)
            assert H.pivot_ratio(O.gram(x)[0]) >= 1e-6
            for mask, p in H.LOCATE_CONFIGS:
                h = np.abs(M.h_plane(x, cf, mask, p))
                rr, cc = np.unravel_index(int(np.argmax(h)), h.shape)
                assert max(abs(rr - r), abs(cc - c)) <= 1, (name, mask, p, (rr, cc))
