"""What ONE row band of a sharded image must return (include/wm.h wm_band_*), restated in numpy on the CPU oracle.

Every value is computed in f64 from the oracle's planes of the WHOLE image (tests/oracle_lib.py, tests/tiles_model.py) and then
restricted to the band's owned global rows [r0, r1): nothing here knows about halo rows, planes, strips or segments.

The 44 Gram sums.  tests/lag_gram_model.py writes term t as a sum over window positions q of the replicate-padded image X,

    T_t = sum over q in I + u_t of X(q) X(q + d_t),      q = (r, c),  -1 <= r <= R,  -1 <= c <= C,

and a band takes the positions of its rows.  Which band a row of positions belongs to:
  * the border rows go to the band that holds that image border: r = -1, 0 to the band with r0 == 0 and r = R-2, R-1, R to the band
    with r1 == R (k_gram's border frame: the rows that need the replicate padding, summed by one kernel as a whole);
  * every other row, 1 <= r <= R-3, goes to the band that owns it.
For any split of [0, R) every position is counted once, so the bands' sums add up to the whole image's.  A bottom band of ONE row
[R-1, R) takes row R-2 although the band above owns it: the band above must then stop at R-3.  wm_band_configure's halo rule
(halo_rule below) keeps that split out -- the band above would hold one row below its own where an interior side needs two.

{max|e|, sum (m W)^2} over the owned rows: under ME m = |e| BEFORE the division by max|e| (wm.h: "without the 1/max^2"), under NVF
the maximum is 1.  {<e_u,e_w>, |e_u|^2, |e_w|^2} over the owned rows: tiles_model.pixel_products(...)[:, r0:r1] summed -- under ME
with m = |e_w| there as well: a band cannot know the image's max|e_w| before the exchange, the factor cancels in the score, and
wm.h says so of these sums ("the 1 / max|e| cancels in every score and is not applied")."""
import numpy as np

import oracle_lib as O
import tiles_model as TM
from lag_gram_model import LAGS, terms

NGRAM = 44


def halo_need(p):
    """rows of image data wm_band_configure wants on every interior side (bands.halo_rows)"""
    return max(2, p // 2 + 1)


def halo_rule(plane_rows, own_lo, own_hi, p):
    """wm_band_configure's checks on [own_lo, own_hi) of a plane of plane_rows rows (own_lo == 0 / own_hi == plane_rows: image borders)"""
    need = halo_need(p)
    if own_lo < 0 or own_hi > plane_rows or own_lo >= own_hi or plane_rows < 4:
        return False
    return not ((0 < own_lo < need) or (own_hi < plane_rows and plane_rows - own_hi < need))


def position_rows(R, r0, r1):
    """rows r of the window positions q = (r, c) that the band [r0, r1) of an R-row image sums (see the module text)"""
    assert 0 <= r0 < r1 <= R and R >= 4
    rows = [r for r in range(max(r0, 1), min(r1, R - 2))]
    if r0 == 0:
        rows = [-1, 0] + rows
    if r1 == R:
        rows = rows + [R - 2, R - 1, R]
    return rows


def gram_sums(x, r0, r1):
    """the 44 sums (36 upper-triangle Rx entries, then the 8 rx entries) over the positions of band [r0, r1), f64.
    Products of u8 or f32 pixels are exact in f64; u8 sums stay below 2^53 and are exact too"""
    x = np.asarray(x).astype(np.float64)
    R, C = x.shape
    Xp = np.pad(x, 3, mode="edge")                      # Xp[r + 3, c + 3] = X(r, c)
    rows = np.array(position_rows(R, r0, r1), dtype=np.int64)   # (may be empty: the row R-2 alone belongs to the bottom band)
    cols = np.arange(-1, C + 1)
    xq = Xp[np.ix_(rows + 3, cols + 3)]
    prod = [xq * Xp[np.ix_(rows + 3 + a, cols + 3 + b)] for (a, b) in LAGS]
    out = np.zeros(NGRAM)
    for t, (ur, uc, lag) in enumerate(terms()):
        rin = (rows >= ur) & (rows <= R - 1 + ur)
        cin = (cols >= uc) & (cols <= C - 1 + uc)
        out[t] = prod[lag][np.ix_(rin, cin)].sum()
    return out


def oracle_gram_totals(x):
    """O.gram of the whole image in the order of wm_gram's 44 doubles"""
    Rx, rx = O.gram(np.asarray(x, np.float32))
    return np.concatenate([Rx[np.triu_indices(8)], rx])


class Frame:
    """the oracle's planes of one whole frame, computed once: e and the mask for the stats, the per-pixel detector products"""

    def __init__(self, x, W, p=3, mask=O.MASK_ME):
        self.x = np.ascontiguousarray(x, np.float32)
        self.W = np.ascontiguousarray(W, np.float32)
        self.p, self.mask = p, mask
        st, c, e, m, mx = O.me_mask(self.x)
        self.status, self.c, self.e = st, c, e
        if mask == O.MASK_ME:
            self.m = np.abs(e.astype(np.float64))       # |e|, not yet divided by its maximum
        else:
            self.m = O.nvf_mask(self.x, p).astype(np.float64)
        self.mw2 = (self.m * self.W.astype(np.float64)) ** 2
        self._prod = None

    def stats(self, r0, r1):
        """(max|e| over the owned rows (1 for NVF), sum (m W)^2 over the owned rows)"""
        mx = float(self.m[r0:r1].max()) if self.mask == O.MASK_ME else 1.0
        return mx, float(self.mw2[r0:r1].sum())

    def detect_sums(self, r0, r1):
        """[<e_u,e_w>, |e_u|^2, |e_w|^2] over the owned rows"""
        if self._prod is None:
            if self.mask == O.MASK_ME:
                # tiles_model.pixel_products with m = |e_w| in place of |e_w| / max|e_w|
                eu = O.error_sequence((np.abs(self.e) * self.W).astype(np.float32), self.c).astype(np.float64)
                ew = self.e.astype(np.float64)
                self._prod = np.stack([eu * ew, eu * eu, ew * ew])
            else:
                st, self._prod = TM.pixel_products(self.x, self.W, self.p, self.mask)
            assert self.status == 0
        return self._prod[:, r0:r1].sum(axis=(1, 2))


def strength(mx, ss, npix, psnr=40.0):
    """Watermark.cpp:170 from all-reduced stats: a = sF / (||m W|| / max / sqrt(N)), in f64"""
    return O.strength_factor(psnr) / (np.sqrt(ss) / mx / np.sqrt(npix))


def corr_of(sums):
    """the score from all-reduced detector sums {dot, nu, nw}: (float)dot / (float)(sqrt(nw) * sqrt(nu)) (wm.h)"""
    d, nu, nw = (float(v) for v in sums)
    return float(np.float32(d) / np.float32(np.sqrt(nw) * np.sqrt(nu)))
