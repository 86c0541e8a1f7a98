"""wm_quality's definitions (include/wm.h) restated in numpy float64, and nothing else.

d = ref - test per sample; per tile of wm_tiles_shape's grid {sse, npix, ssim_sum, nwin, max|d|}; SSIM is Wang et al.'s (2004) 11 x 11
Gaussian window, evaluated only where the window lies wholly inside the plane, a window belonging to the tile of its centre pixel.
Two evaluations of the window sums: a separable one (rows, then columns) and a direct one over the 121 terms."""
import numpy as np

C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
NVALS, NSUMS = 3, 5


def weights():
    g = np.exp(-(np.arange(11, dtype=np.float64) - 5.0) ** 2 / 4.5)
    return g / g.sum()


def _filter_separable(a):
    g = weights()
    R, C = a.shape
    h = np.zeros((R, C - 10))
    for k in range(11):
        h += g[k] * a[:, k:k + C - 10]
    v = np.zeros((R - 10, C - 10))
    for k in range(11):
        v += g[k] * h[k:k + R - 10]
    return v


def _filter_direct(a):
    g = weights()
    R, C = a.shape
    v = np.zeros((R - 10, C - 10))
    for i in range(11):
        for j in range(11):
            v += (g[i] * g[j]) * a[i:i + R - 10, j:j + C - 10]
    return v


def ssim_map(ref, test, direct=False):
    """s of every whole window, [rows - 10, cols - 10] (entry (i, j): the window centred at pixel (i + 5, j + 5)); empty below 11 x 11"""
    x, y = np.asarray(ref).astype(np.float64), np.asarray(test).astype(np.float64)
    R, C = x.shape
    if R < 11 or C < 11:
        return np.zeros((max(R - 10, 0), max(C - 10, 0)))
    f = _filter_direct if direct else _filter_separable
    mx, my = f(x), f(y)
    vx, vy, cxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def tiles_shape(rows, cols, tile_rows, tile_cols):
    """wm_tiles_shape; tile_rows == tile_cols == 0: one tile per plane"""
    if tile_rows == 0 and tile_cols == 0:
        return 1, 1
    assert tile_rows >= 32 and tile_rows % 8 == 0 and tile_cols >= 32 and tile_cols % 4 == 0
    return max(1, rows // tile_rows), max(1, cols // tile_cols)


def tile_bounds(n, tile, ntiles, t):
    return t * tile, (n if t == ntiles - 1 else (t + 1) * tile)


def tile_sums(ref, test, tile_rows=0, tile_cols=0, direct=False):
    """[ny, nx, 5] float64 = {sse, npix, ssim_sum, nwin, max|d|} of one plane pair"""
    x, y = np.asarray(ref).astype(np.float64), np.asarray(test).astype(np.float64)
    R, C = x.shape
    ny, nx = tiles_shape(R, C, tile_rows, tile_cols)
    d = x - y
    s = ssim_map(x, y, direct)
    out = np.zeros((ny, nx, NSUMS))
    for ty in range(ny):
        r0, r1 = tile_bounds(R, tile_rows, ny, ty)
        for tx in range(nx):
            c0, c1 = tile_bounds(C, tile_cols, nx, tx)
            dt = d[r0:r1, c0:c1]
            # the window centres among the tile's pixels: rows 5 .. R - 6, columns 5 .. C - 6
            wr0, wr1, wc0, wc1 = max(r0, 5), min(r1, R - 5), max(c0, 5), min(c1, C - 5)
            st = s[wr0 - 5:wr1 - 5, wc0 - 5:wc1 - 5] if wr1 > wr0 and wc1 > wc0 else np.zeros((0, 0))
            out[ty, tx] = (np.sum(dt * dt), dt.size, np.sum(st), st.size, np.max(np.abs(dt)))
    return out


def plane_values(sums):
    """(mse, ssim, max|d|) of a plane from its tile sums, added in ascending tile index; ssim is NaN when there is no window"""
    t = np.asarray(sums).reshape(-1, NSUMS)
    sse = npix = ssum = nwin = 0.0
    for k in range(t.shape[0]):
        sse += t[k, 0]; npix += t[k, 1]; ssum += t[k, 2]; nwin += t[k, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        return sse / npix, np.float64(ssum) / np.float64(nwin), float(t[:, 4].max())


def psnr_from_mse(mse, peak=255.0):
    if not (mse >= 0.0) or not (peak > 0.0):
        return float("nan")
    return float("inf") if mse == 0.0 else 10.0 * np.log10(peak * peak / mse)
