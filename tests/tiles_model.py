"""The tile map of wm_detect_tiles restated on the CPU oracle (tests/oracle_lib.py).

The sums are taken exactly as wmo_detect composes them -- c, e_w and m from O.me_mask (m from O.nvf_mask under NVF),
u = (m W) in f32, e_u = O.error_sequence(u, c) -- and then kept per tile in f64 instead of over the whole plane:
pixel (r, c) belongs to tile (min(r // th, ny - 1), min(c // tw, nx - 1)), the last tile of each axis takes the remainder.
score = (float)dot / (float)(sqrt(nw) * sqrt(nu)) per tile."""
import numpy as np

import oracle_lib as O


def tiles_shape(rows, cols, th, tw):
    return max(1, rows // th), max(1, cols // tw)


def tile_edges(n, t):
    """first index of every tile along an axis of n pixels"""
    return np.arange(max(1, n // t)) * t


def pixel_products(img, W, p=3, mask=0):
    """(status, [<e_u,e_w>, e_u^2, e_w^2] per pixel as f64 [3, R, C]) -- None for an unsolvable frame"""
    x = np.ascontiguousarray(img, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    st, c, ew, m, _ = O.me_mask(x)
    if st != 0:
        return st, None
    if mask == 1:
        m = O.nvf_mask(x, p)
    eu = O.error_sequence((m * W).astype(np.float32), c)
    eu64, ew64 = eu.astype(np.float64), ew.astype(np.float64)
    return 0, np.stack([eu64 * ew64, eu64 * eu64, ew64 * ew64])


def sums_of(prod, th, tw):
    """f64 tile sums [ny, nx, 3] of per-pixel products [3, R, C]"""
    rb, cb = tile_edges(prod.shape[1], th), tile_edges(prod.shape[2], tw)
    s = np.add.reduceat(np.add.reduceat(prod, rb, axis=1), cb, axis=2)
    return np.ascontiguousarray(s.transpose(1, 2, 0))


def score_of(sums):
    """the score expression of wm_detect_tiles over sums [..., 3] = {dot, nu, nw}: f32, NaN where nu or nw is 0"""
    s = np.asarray(sums, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = (np.sqrt(s[..., 2]) * np.sqrt(s[..., 1])).astype(np.float32)
        return (s[..., 0].astype(np.float32) / den).astype(np.float32)


def tile_map(img, W, th, tw, p=3, mask=0):
    """(status, map f32 [ny, nx], sums f64 [ny, nx, 3]); an unsolvable frame: zeros"""
    st, prod = pixel_products(img, W, p, mask)
    ny, nx = tiles_shape(np.shape(img)[0], np.shape(img)[1], th, tw)
    if st != 0:
        return st, np.zeros((ny, nx), np.float32), np.zeros((ny, nx, 3))
    s = sums_of(prod, th, tw)
    return 0, score_of(s), s
