"""Hard content for the parity tests: the inputs synth_frame never produces.

synth_frame is mid-range texture centred on 128: it almost never reaches 0 or 255, has no flat regions, is never singular,
and its max|e| sits at a random interior pixel.  Each family here aims at one of those blind spots.  Every generator is plain
numpy, deterministic by its arguments, and returns the frames together with the facts the tests rely on; test_hard_content.py
asserts those facts against the oracle, so that a family cannot quietly become easy.

Families:
  clipped      contrast-stretched texture (about a fifth of the pixels at 0 / 255) and a planar-RGB base with one channel near
               255 and one near 0: the clamp of y = clamp(base + a u, 0, 255) fires on many pixels at low psnr
  letterbox    textured frames with bars (top/bottom, or left/right) at exactly 0 or 16: NVF variance, e and lag products are
               exactly 0 / constant inside them
  binary       random 0 / 255 pixels: the integer Gram at its largest products
  singular     ramp, plane, row-constant image, period-2 stripes: exactly singular Gram systems (WM_UNSOLVABLE everywhere),
               and near-singular solvable ramps
  impulse      a low-contrast frame with one pixel at 0 or 255 at a structural spot (corner, strip / segment / tile / band
               seam, shifted last strip): max|e| sits at that pixel, so a reduction that drops it changes the whole mask
  zero-energy  frames and W for which u = m W vanishes: ||u|| = 0, a = +inf
  hard crops   the families above as crops for the crop search (wm_locate, wm_clip_pool and their siblings): a frame of the key's
               shape marked at psnr 40, cropped at a known offset and paired with its unmarked twin, at three geometries that hold
               every tile edge of the pool kernel; impulse crops with the pixel on every corner, edge and tile seam

Only numpy and synth (the package's generator) are used, and np_restatement to mark the hard crops: these frames are built the
same way on every machine.
"""
import numpy as np

from synth import synth_frame, synth_watermark

STRIP = 256  # columns per strip of the batched sweeps


def _rng(*key):
    return np.random.default_rng([0x48415244] + [int(k) & 0xFFFFFFFF for k in key])


def _u8(x):
    return np.rint(np.clip(x, 0, 255)).astype(np.uint8)


# ---- clipped --------------------------------------------------------------------------------------------------------------
def clipped(rows, cols, frame=0, gain=2.2, dtype=np.float32):
    """synth frame stretched about 128: clip(gain (x - 128) + 128, 0, 255) -- about 21 % of the pixels at 0 or 255"""
    x = synth_frame(rows, cols, frame=frame).astype(np.float64)
    y = np.clip(gain * (x - 128.0) + 128.0, 0.0, 255.0)
    return _u8(y) if dtype == np.uint8 else y.astype(np.float32)


def clipped_rgb(rows, cols, frame=0):
    """(grey, planar RGB base [3, R, C]): R near 255 (often at it), G a stretched texture, B near 0 (often at it); grey is the
    base's luma, so the mask follows the picture the watermark is added to"""
    t = synth_frame(rows, cols, frame=frame).astype(np.float64) - 128.0
    r = np.clip(250.0 + 0.15 * t, 0.0, 255.0)
    g = np.clip(128.0 + 2.2 * t, 0.0, 255.0)
    b = np.clip(5.0 - 0.15 * t, 0.0, 255.0)
    rgb = np.stack([r, g, b]).astype(np.float32)
    grey = (0.299 * rgb[0] + 0.587 * rgb[1] + 0.114 * rgb[2]).astype(np.float32)
    return grey, rgb


def clamped_fraction(y, base):
    """fraction of output pixels at 0 or 255 where the base is not: the pixels the clamp changed"""
    y, base = np.asarray(y, np.float32), np.asarray(base, np.float32)
    hit = ((y == 0) & (base != 0)) | ((y == 255) & (base != 255))
    return float(hit.mean())


# ---- letterbox ------------------------------------------------------------------------------------------------------------
def letterbox(rows, cols, k, level, frame=0, pillar=False, dtype=np.float32):
    """synth frame with bars of k rows at the top and bottom (pillar: k columns at the left and right) at exactly `level`"""
    x = synth_frame(rows, cols, frame=frame).astype(np.float32)
    if pillar:
        x[:, :k] = level
        x[:, cols - k:] = level
    else:
        x[:k] = level
        x[rows - k:] = level
    return _u8(x) if dtype == np.uint8 else x


def bar_interior(rows, cols, k, pillar=False, halo=1):
    """boolean [R, C]: pixels inside the bars whose p x p window (p = 2 halo + 1) lies in the bar"""
    m = np.zeros((rows, cols), bool)
    if pillar:
        m[:, :max(k - halo, 0)] = True
        m[:, cols - k + halo:] = True
    else:
        m[:max(k - halo, 0)] = True
        m[rows - k + halo:] = True
    return m


# ---- binary ---------------------------------------------------------------------------------------------------------------
def binary(rows, cols, seed=0, p255=0.5, dtype=np.float32):
    """every pixel 0 or 255 (255 with probability p255)"""
    x = np.where(_rng(1, seed, rows, cols).random((rows, cols)) < p255, 255, 0).astype(np.uint8)
    return x if dtype == np.uint8 else x.astype(np.float32)


def integer_gram(x):
    """the 44 Gram sums (wm_gram's order: 36 upper-triangle Rx entries row-major, then the 8 rx) of an integer-valued frame,
    as exact int64 sums (replicate borders, the reference's neighbour order)"""
    x = np.asarray(x).astype(np.int64)
    xp = np.pad(x, 1, mode="edge")
    R, C = x.shape
    offs = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    n = [xp[1 + dr:1 + dr + R, 1 + dc:1 + dc + C] for dr, dc in offs]
    out = [int((n[i] * n[j]).sum()) for i in range(8) for j in range(i, 8)]
    out += [int((n[i] * x).sum()) for i in range(8)]
    return np.array(out, np.int64)


# ---- singular -------------------------------------------------------------------------------------------------------------
# every value below is a multiple of 1/16 in [0, 255]: exact in f32 and u8-free, so the Gram sums are exact in f64 too and
# the systems are exactly singular (not just ill-conditioned by rounding)
def singular(kind, rows, cols, seed=0):
    r = np.arange(rows, dtype=np.float64)[:, None]
    c = np.arange(cols, dtype=np.float64)[None, :]
    if kind == "ramp":       # horizontal ramp: every row alike, so up / mid / down neighbours are equal
        x = np.floor((16.0 + 200.0 * c / cols) * 16.0) / 16.0 + 0.0 * r
    elif kind == "plane":    # a r + b c + d: the 8 neighbours span {x, 1, 4 border indicators}
        a = max(np.floor(96.0 / rows * 16.0), 1.0) / 16.0
        b = max(np.floor(112.0 / cols * 16.0), 1.0) / 16.0
        x = 20.0 + a * r + b * c
    elif kind == "rows":     # row-constant image: the three neighbours of each row are equal
        v = np.floor(_rng(2, seed, rows).random(rows) * 255.0 * 16.0) / 16.0
        x = v[:, None] + 0.0 * c
    elif kind == "stripes":  # period-2 column stripes
        x = 100.0 + 50.0 * (c % 2) + 0.0 * r
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


SINGULAR_KINDS = ("ramp", "plane", "rows", "stripes")


def near_singular(rows, cols, density=0.03, seed=0):
    """a horizontal ramp plus sparse +-1 pixels: ill-conditioned, but solvable"""
    x = singular("ramp", rows, cols).astype(np.float64)
    g = _rng(3, seed, rows, cols)
    hit = g.random((rows, cols)) < density
    x = x + np.where(hit, np.where(g.random((rows, cols)) < 0.5, -1.0, 1.0), 0.0)
    return np.clip(x, 0, 255).astype(np.float32)


def pivot_ratio(Rx):
    """smallest pivot of an f64 LU with partial pivoting / max |Rx| (the solve declares the system unsolvable below 1e-12)"""
    A = np.array(Rx, np.float64)
    amax = np.abs(A).max()
    n = A.shape[0]
    pmin = np.inf
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        pmin = min(pmin, abs(A[p, k]))
        if A[p, k] == 0.0:
            break
        A[[k, p]] = A[[p, k]]
        A[k + 1:, k:] -= np.outer(A[k + 1:, k] / A[k, k], A[k, k:])
    return pmin / amax


# ---- impulse --------------------------------------------------------------------------------------------------------------
def low_contrast(rows, cols, frame=0, contrast=0.15):
    """synth texture squeezed about 128 (kept solvable, far from the clamp)"""
    x = synth_frame(rows, cols, frame=frame).astype(np.float64)
    return (128.0 + contrast * (x - 128.0)).astype(np.float32)


def impulse_spots(rows, cols, rps=None, tile_rows=None, band_rows=()):
    """named (r, c) positions where the reductions of max|e| meet: corners, the Gram core's edge rows / columns, strip seams,
    the shifted last strip's duplicate columns, segment seams (rows per segment `rps`), fused tile seams (`tile_rows`), band
    seams (`band_rows`: the first owned row of every band after the first).  Interior columns are picked mid-image"""
    R, C = rows, cols
    rm, cm = R // 2, C // 2
    s = {"corner_tl": (0, 0), "corner_tr": (0, C - 1), "corner_bl": (R - 1, 0), "corner_br": (R - 1, C - 1),
         "row_1": (1, cm + 1), "row_R-2": (R - 2, cm + 3), "col_1": (rm, 1), "col_2": (rm + 2, 2),
         "col_C-3": (rm - 2, C - 3), "col_C-2": (rm + 4, C - 2)}
    for sc in (STRIP - 1, STRIP, 2 * STRIP - 1, 2 * STRIP):
        if sc < C - 2:
            s[f"strip_c{sc}"] = (rm - 5 + sc % 7, sc)
    if C % STRIP and C > STRIP:  # shifted last strip: it starts at C - 256 and repeats the columns up to (C // 256) 256
        d0, d1 = C - STRIP, (C // STRIP) * STRIP - 1
        s["dup_first"] = (rm + 6, d0)
        s["dup_last"] = (rm - 6, d1)
    if rps:
        for r in (rps - 1, rps, 2 * rps - 1, 2 * rps):
            if 1 < r < R - 2:
                s[f"seg_r{r}"] = (r, cm - 7)
    if tile_rows:
        for r in (tile_rows - 1, tile_rows, 2 * tile_rows - 1, 2 * tile_rows):
            if 1 < r < R - 2:
                s[f"tile_r{r}"] = (r, cm + 9)
    for i, r0 in enumerate(band_rows):
        for r in (r0 - 1, r0):
            if 1 < r < R - 2:
                s[f"band{i}_r{r}"] = (r, cm - 11 + 3 * i)
    return s


def impulse(rows, cols, spots, frame=0, dtype=np.float32):
    """a batch [F, R, C]: frame f is a low-contrast frame with spots[f] set to 0 or 255 (alternating, chosen away from the
    local level); returns (frames, list of (name, r, c))"""
    items = list(spots.items()) if isinstance(spots, dict) else list(spots)
    base = low_contrast(rows, cols, frame=frame)
    xs = []
    for f, (_, (r, c)) in enumerate(items):
        x = base.copy()
        x[r, c] = 255.0 if f % 2 == 0 else 0.0
        xs.append(_u8(x) if dtype == np.uint8 else x)
    return np.stack(xs), [(n, r, c) for n, (r, c) in items]


# ---- zero-energy ----------------------------------------------------------------------------------------------------------
def flat(rows, cols, level, dtype=np.float32):
    """a constant frame: integer levels give an NVF mask of exactly 0 everywhere (u = 0); 77.3 gives a tiny non-zero
    variance from rounding"""
    return np.full((rows, cols), level, dtype=dtype)


FLAT_LEVELS = ((np.float32, 77.0), (np.uint8, 77), (np.uint8, 0), (np.uint8, 255))


def zero_w(rows, cols):
    return np.zeros((rows, cols), np.float32)


def watermark(rows, cols):
    return synth_watermark(rows, cols)


# ---- hard crops for the crop search (wm_locate, wm_clip_pool and their siblings) ------------------------------------------------
# (key shape, crop shape, true offset): between them every tile edge of k_clip_pool's 64 x 16 tiles occurs -- whole tiles, one
# column and one row past a tile edge, and a last tile of two columns and one row
LOCATE_GEOMS = (((120, 330), (64, 256), (20, 31)), ((140, 330), (65, 257), (75, 73)), ((100, 200), (33, 66), (5, 7)))
LOCATE_CONFIGS = ((0, 3), (1, 3), (1, 5), (1, 9))  # (mask, p): ME, and NVF at three windows (9: the gather path above window 3)
LOCATE_PSNR = 40.0  # ... of the marking; 30 for the 33 x 66 crop (locate_psnr)
LOCATE_BAR = 12  # rows / columns a bar reaches into the crop
# family -> (findable at psnr 40, has a u8 variant).  binary: the clamp takes the mark away (every pixel sits at 0 or 255), so a
# search cannot find it: parity only
LOCATE_FAMILIES = {"texture": (True, True), "clipped": (True, True), "letterbox": (True, True), "pillar": (True, True),
                   "binary": (False, True), "near_singular": (True, False), "low_contrast": (True, False)}
# the figures of the restatement of h (oracle wmo_locate_h) against the f64 model, measured by tests/test_locate_model.py, which
# asserts that no case exceeds them: (largest |dh| / max|h|, largest map difference in sigma_W) per family.  The GPU tests build
# their second map bound and the pool bound of test_gpu_locate_clip.py from them
RESTATEMENT_FIGURES = {"texture": (8e-7, 3e-6), "clipped": (5e-7, 2e-6), "letterbox": (7e-7, 4e-6), "pillar": (9e-7, 3e-6),
                       "binary": (4e-7, 2e-6), "near_singular": (1.9e-5, 5.6e-5), "low_contrast": (3.3e-6, 1.6e-5),
                       "impulse": (8e-7, 1.1e-5)}
_crops = {}


def locate_psnr(shape):
    """psnr 40; 30 for the crop of 33 x 66: z grows with the square root of the crop's area, and at psnr 40 its 2178 pixels leave
    even plain texture below z = 10 (9.6; clipped 5.1), so that no frame index or bar width could make its cases findable"""
    return LOCATE_PSNR if shape[0] * shape[1] >= 64 * 256 else 30.0


def locate_key(kshape):
    """the key of a shape (tests/locate_clip_model.py key_of)"""
    return synth_watermark(*kshape, seed=9100 + 7 * kshape[0] + kshape[1])


def locate_base(family, kshape, shape, at, frame=0):
    """the unmarked f32 frame of the key's shape of one family; the bars end LOCATE_BAR rows / columns inside the crop at `at`.
    near_singular on the 33 x 66 crop has +-1 pixels at a density of 0.1, not 0.03: under ME the mark itself is most of such a
    frame's prediction error, z does not grow with the strength, and at 0.03 the small crop stays at z = 8 (pivot ratio 1e-5; at
    0.1 z = 15.6, pivot ratio 3e-5: still three orders from an ordinary frame)"""
    kr, kc = kshape
    if family == "texture":
        return synth_frame(kr, kc, frame=10 + frame)
    if family == "clipped":
        return clipped(kr, kc, frame=frame)
    if family == "letterbox":
        x = synth_frame(kr, kc, frame=frame).astype(np.float32)
        x[:at[0] + LOCATE_BAR] = 16.0
        return x
    if family == "pillar":
        x = synth_frame(kr, kc, frame=frame).astype(np.float32)
        x[:, :at[1] + LOCATE_BAR] = 0.0
        return x
    if family == "binary":
        return binary(kr, kc, seed=frame)
    if family == "near_singular":
        return near_singular(kr, kc, density=0.03 if shape[0] * shape[1] >= 64 * 256 else 0.1, seed=frame)
    if family == "low_contrast":
        return low_contrast(kr, kc, frame=frame)
    raise ValueError(family)


def locate_crops(kshape, shape, at, mask, p):
    """{name: (marked crop, unmarked twin)}: every family's frame of the key's shape marked with np_restatement.embed (the shape's
    key, window p, locate_psnr) and cropped at `at`, beside the same crop of the unmarked frame.  name is the family (f32 crops) or
    family + '_u8' (both floored to uint8)"""
    import np_restatement as NP  # (the marking only; the frames themselves are numpy and synth)
    tag = (kshape, shape, at, mask, p)
    if tag not in _crops:
        (r, c), (oy, ox) = shape, at
        key = locate_key(kshape)
        out = {}
        for family, (_, has_u8) in LOCATE_FAMILIES.items():
            x = locate_base(family, kshape, shape, at)
            y = NP.embed(x, x, key, p, locate_psnr(shape), "ME" if mask == 0 else "NVF")[0]
            cy, cx = (np.ascontiguousarray(v[oy:oy + r, ox:ox + c], np.float32) for v in (y, x))
            out[family] = (cy, cx)
            if has_u8:
                out[family + "_u8"] = (np.floor(cy).astype(np.uint8), np.floor(cx).astype(np.uint8))
        if len(_crops) >= 4:
            _crops.clear()
        _crops[tag] = out
    return _crops[tag]


def locate_family(name):
    return name[:-3] if name.endswith("_u8") else name


def locate_bar_zero(name, shape, p, marked):
    """boolean [R, C]: the crop's pixels whose NVF window of p lies in bar pixels that the marking left alone (the marking moves
    the bar pixels whose own window reaches the picture), or None for a family without a bar"""
    pad = p // 2
    k = LOCATE_BAR - pad - (pad if marked else 0)
    z = np.zeros(shape, bool)
    if locate_family(name) == "letterbox":
        z[:max(k, 0)] = True
    elif locate_family(name) == "pillar":
        z[:, :max(k, 0)] = True
    else:
        return None
    return z


def locate_impulse_spots(shape):
    """named crop coordinates where the image side of the crop search can go wrong: the corners, the middle of every edge, (1, 1),
    the seams of k_clip_pool's 64 x 16 tiles and of k_locate_e's 64 x 4 blocks, the first pixel of the last partial tile -- each
    one that exists in the shape, each position once"""
    R, C = shape
    rm, cm = R // 2, C // 2
    cand = [("corner_tl", (0, 0)), ("corner_tr", (0, C - 1)), ("corner_bl", (R - 1, 0)), ("corner_br", (R - 1, C - 1)),
            ("top", (0, cm)), ("bottom", (R - 1, cm)), ("left", (rm, 0)), ("right", (rm, C - 1)), ("r1_c1", (1, 1))]
    cand += [(f"seam_r{a}_c{b}", (a, b)) for (a, b) in ((15, 63), (15, 64), (16, 63), (16, 64), (3, 64), (4, 63))]
    if R % 16 or C % 64:
        cand.append(("last_tile", ((R - 1) // 16 * 16, (C - 1) // 64 * 64)))
    out, seen = {}, set()
    for name, (a, b) in cand:
        if a < R and b < C and (a, b) not in seen:
            seen.add((a, b))
            out[name] = (a, b)
    return out


def locate_impulses(kshape, shape, at, dtype=np.float32):
    """(frames [F, R, C], [(name, r, c)]): the low-contrast crop with one pixel at 255 or 0 per frame (impulse)"""
    (r, c), (oy, ox) = shape, at
    base = low_contrast(*kshape)[oy:oy + r, ox:ox + c]
    xs, items = [], []
    for f, (name, (a, b)) in enumerate(locate_impulse_spots(shape).items()):
        x = base.copy()
        x[a, b] = 255.0 if f % 2 == 0 else 0.0
        xs.append(_u8(x) if dtype == np.uint8 else x)
        items.append((name, a, b))
    return np.stack(xs), items
