"""numpy model of wm_locate_bits (wm.h), f64 throughout, built on tests/locate_model.py.

Tile signs are a property of KEY coordinates.  With key_b = key * [tile_bit[tile(p)] == b] -- the key masked to the tiles of bit b,
tiles defined on the key plane by wm_tiles_shape's rule -- the numerator of a payload-marked crop at offset o is
sum_b s_b map_b(o), map_b(o) = sum_q h(q) key_b(q + o): locate_model.correlate with another key plane.  E = sum_b map_b^2 does not
see the signs; the sign of map_b at E's argmax is the bit.  h is real, so one complex transform carries two bits (pair_maps).
"""
import numpy as np

import locate_model as M


def tiles_shape(rows, cols, th, tw):
    return max(1, rows // th), max(1, cols // tw)


def tile_index(rows, cols, th, tw):
    """int [rows, cols]: the tile ty * nx + tx of every pixel (the last tile of each axis takes the remainder)"""
    ny, nx = tiles_shape(rows, cols, th, tw)
    ty = np.minimum(np.arange(rows) // th, ny - 1)
    tx = np.minimum(np.arange(cols) // tw, nx - 1)
    return ty[:, None] * nx + tx[None, :]


def bit_plane(kshape, th, tw, tile_bit):
    """int [key_rows, key_cols]: the bit every key pixel carries, -1 for none"""
    return np.asarray(tile_bit).reshape(-1)[tile_index(kshape[0], kshape[1], th, tw)]


def key_b(key, th, tw, tile_bit, b):
    key = np.asarray(key, np.float64)
    return np.where(bit_plane(key.shape, th, tw, tile_bit) == b, key, 0.0)


def signs_plane(kshape, th, tw, tile_bit, bits):
    """the sign +1 / -1 / 0 of every key pixel under the payload `bits` (an int array [nbits] of 0 / 1)"""
    bp = bit_plane(kshape, th, tw, tile_bit)
    return np.where(bp < 0, 0, np.where(np.asarray(bits)[np.maximum(bp, 0)] == 1, 1, -1))


def balanced_payload(nbits, seed):
    """a random payload with as many set bits as clear ones (one more clear for an odd nbits), an int array [nbits] of 0 / 1: the
    whole-key map of such a copy has no peak to speak of, while a lopsided payload leaves wm_locate a net mark to find"""
    return np.random.default_rng(seed).permutation(np.arange(nbits) % 2 == 1).astype(np.int64)


def maps(h, key, th, tw, tile_bit, nbits):
    """[nbits, ny, nx]: map_b = correlate(h, key_b)"""
    return np.stack([M.correlate(h, key_b(key, th, tw, tile_bit, b)) for b in range(nbits)])


def pair_maps(h, ka, kb):
    """the maps of two real key planes from ONE complex transform: correlate h with ka + i kb, take the real and imaginary parts"""
    ny, nx = ka.shape[0] - h.shape[0] + 1, ka.shape[1] - h.shape[1] + 1
    full = np.fft.ifft2(np.conj(np.fft.fft2(h, ka.shape)) * np.fft.fft2(np.asarray(ka, np.float64) + 1j * np.asarray(kb, np.float64)))
    return np.ascontiguousarray(full.real[:ny, :nx]), np.ascontiguousarray(full.imag[:ny, :nx])


def energy(mp):
    return np.sum(np.asarray(mp, np.float64) ** 2, axis=0)


def soft(mp, oy, ox):
    """[nbits]: (map_b(o*) - mu_b) / sigma_b over the offsets outside the 3 x 3 block around o* = (oy, ox); NaN where they do not vary
    or fewer than two lie outside"""
    mp = np.asarray(mp, np.float64)
    out = np.ones(mp.shape[1:], bool)
    out[max(oy - 1, 0):oy + 2, max(ox - 1, 0):ox + 2] = False
    res = np.full(len(mp), np.nan)
    for b, m in enumerate(mp):
        rest = m[out]
        if rest.size >= 2 and rest.std() > 0:
            res[b] = (m[oy, ox] - rest.mean()) / rest.std()
    return res


def locate_bits(x, key, c, mask, th, tw, tile_bit, nbits, p=3):
    """the model of one frame with the coefficients c: (maps, E, (oy, ox, peak, z) of E, soft)"""
    mp = maps(M.h_plane(x, c, mask, p), key, th, tw, tile_bit, nbits)
    E = energy(mp)
    loc = M.fold(E)
    return mp, E, loc, soft(mp, loc[0], loc[1])


def cover(shape, kshape, th, tw, tile_bit, nbits, oy, ox):
    """int64 [nbits]: the pixels of the window at (oy, ox) whose key tile carries bit b"""
    win = bit_plane(kshape, th, tw, tile_bit)[oy:oy + shape[0], ox:ox + shape[1]]
    return np.array([(win == b).sum() for b in range(nbits)], np.int64)
