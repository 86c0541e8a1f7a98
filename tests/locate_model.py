"""numpy model of wm_locate (wm.h), f64 throughout.

With the frame's coefficients c solved the detector's numerator is linear in W:

    <e_u, e_w>(oy, ox) = sum_q h(q) W(q + (oy, ox)),    h = m * F^T e_w

e_w: the frame's prediction error, m: its mask (ME: |e_w|, NVF: the mask of window p), F^T: the exact adjoint of the
replicate-border prediction-error stencil e = x - sum_k c_k x(clamp(. + d_k)).  The adjoint is written in scatter form with clamped
indices: pixel p sends -c_k e(p) to clamp(p + d_k); a border pixel so receives up to two terms per axis.  zero_border=True drops
what leaves the plane instead of folding it back: NOT the adjoint, kept so that the tests are seen to tell the two apart.
"""
import numpy as np

import np_restatement as R


def error_plane(x, c):
    """e = x - sum_k c_k x(clamp(p + d_k)) in f64"""
    x = np.asarray(x, np.float64)
    n = R.neighbours(x)
    return x - np.tensordot(np.asarray(c, np.float64), n, axes=1)


def mask_plane(x, e, mask, p=3):
    """m: |e| under ME (no 1 / max|e|: the scale of wm_detect_tiles' sums), the detector's NVF mask of window p under NVF"""
    if mask in (0, "ME"):
        return np.abs(np.asarray(e, np.float64))
    return R.nvf_mask(np.asarray(x, np.float32), p).astype(np.float64)


def adjoint(e, c, zero_border=False):
    """g(q) = e(q) - sum_k c_k sum_{p : clamp(p + d_k) = q} e(p)"""
    e = np.asarray(e, np.float64)
    rows, cols = e.shape
    g = e.copy()
    for ck, (dr, dc) in zip(np.asarray(c, np.float64), R.OFFS):
        t = np.zeros((rows + 2, cols + 2))
        t[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols] = e  # pixel p lands on p + d_k (the plane sits at [1, rows], [1, cols])
        if not zero_border:  # clamp: what left the plane falls on the border pixel
            t[1] += t[0]
            t[rows] += t[rows + 1]
            t[:, 1] += t[:, 0]
            t[:, cols] += t[:, cols + 1]
        g -= ck * t[1:rows + 1, 1:cols + 1]
    return g


def h_plane(x, c, mask, p=3, e=None, zero_border=False):
    """h = m * F^T e_w; e: the error plane to use in the place of error_plane(x, c)"""
    if e is None:
        e = error_plane(x, c)
    return mask_plane(x, e, mask, p) * adjoint(e, c, zero_border)


def correlate(h, key):
    """map[i][j] = sum_q h(q) key[q + (i, j)] for every admissible offset, by an f64 FFT of the key's size (no wrap-around
    reaches an admissible offset: q + o < key_rows)"""
    key = np.asarray(key, np.float64)
    ny, nx = key.shape[0] - h.shape[0] + 1, key.shape[1] - h.shape[1] + 1
    full = np.fft.irfft2(np.conj(np.fft.rfft2(h, key.shape)) * np.fft.rfft2(key), key.shape)
    return np.ascontiguousarray(full[:ny, :nx])


def fold(m):
    """(oy, ox, peak, z) of a map: the argmax (ties: the smallest i * nx + j), its value, and its distance from the mean of the
    offsets outside the 3 x 3 block around it in their population standard deviations; z is NaN when fewer than two offsets lie
    outside the block or they do not vary"""
    m = np.asarray(m, np.float64)
    ny, nx = m.shape
    oy, ox = np.unravel_index(int(np.argmax(m)), m.shape)
    out = np.ones(m.shape, bool)
    out[max(oy - 1, 0):oy + 2, max(ox - 1, 0):ox + 2] = False
    rest = m[out]
    z = float("nan")
    if rest.size >= 2 and rest.std() > 0:
        z = (m[oy, ox] - rest.mean()) / rest.std()
    return int(oy), int(ox), float(m[oy, ox]), float(z)


def locate(x, key, c, mask, p=3):
    """the model of one frame: (map, (oy, ox, peak, z)) with the coefficients c (the device's own in the parity tests)"""
    m = correlate(h_plane(x, c, mask, p), key)
    return m, fold(m)


def sigma_w(x, key, c, mask, p=3):
    """the scale the parity bounds are stated in: ||h||_2 rms(key), the standard deviation of the map of a white key"""
    h = h_plane(x, c, mask, p)
    return float(np.sqrt(np.sum(h * h)) * np.sqrt(np.mean(np.asarray(key, np.float64) ** 2)))
