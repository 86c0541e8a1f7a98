"""numpy model of wm_clip_pool and the wm_locate_*_pooled calls (wm.h), f64 throughout, built on
tests/locate_model.py, tests/locate_bits_model.py and tests/locate_keys_model.py.

The map is linear in the image-side plane: map(o) = sum_q h(q) key(q + o), h = m * F^T e_w.  So the pooled map of a clip is the map
of the pooled h,

    sum_f w_f map_f = correlate(sum_f w_f h_f, key),

and the same holds per payload bit and per key of a bank: the three pooled models are the existing ones with the pooled plane in
the place of one frame's h.  The clips of the finding table are built here too, so that the CPU and the GPU tests stand on the same
inputs: 8 frames synth_frame(frame = 10 + f), key synth_watermark(seed = 9100 + 7 key_rows + key_cols), p = 3, floored to 8 bits.
"""
import numpy as np

import locate_bits_model as LB
import locate_model as M
import np_restatement as R
from synth import synth_frame, synth_watermark

Z_MARKED, Z_UNMARKED = 15.0, 6.0
F_CLIP = 8
PSNR = {0: 52.0, 1: 50.0}  # ME, NVF: marks so weak that no single frame of these crops reaches Z_MARKED
# (key shape, crop shape, true offset); 65 x 257 sits one past a tile edge of the pool kernel on both axes
CASES = [((80, 300), (64, 256), (16, 44)), ((120, 330), (64, 256), (20, 31)), ((300, 520), (96, 128), (150, 300)),
         ((140, 330), (65, 257), (75, 73))]
# the payload clip
P_KSHAPE, P_SHAPE, P_AT, P_TILE, P_NBITS, P_PSNR = (120, 330), (64, 256), (20, 31), (32, 32), 8, 52.0
_made = {}


def key_of(kshape, other=False):
    """the key of a shape; other: another key of that shape, which marked nothing"""
    return synth_watermark(*kshape, seed=9100 + 7 * kshape[0] + kshape[1] + (1 if other else 0))


def pool(hs, weights=None):
    """sum_f w_f h_f in f64; weights None: all 1"""
    hs = [np.asarray(h, np.float64) for h in hs]
    w = np.ones(len(hs)) if weights is None else np.asarray(weights, np.float64)
    assert len(w) == len(hs)
    out = np.zeros_like(hs[0])
    for wf, h in zip(w, hs):
        out += wf * h
    return out


def clip_h(xs, cs, mask, p=3):
    """the frames' image-side planes with the coefficients cs (the device's own in the parity tests)"""
    return [M.h_plane(x, c, mask, p) for x, c in zip(xs, cs)]


def sigma_w(h, key):
    """||h||_2 rms(key): the scale of the parity bounds (locate_model.sigma_w of a given plane)"""
    h = np.asarray(h, np.float64)
    return float(np.sqrt(np.sum(h * h)) * np.sqrt(np.mean(np.asarray(key, np.float64) ** 2)))


def locate_pooled(hp, key):
    """(map, (oy, ox, peak, z)) of a pooled plane: locate_model.locate with hp in the place of h"""
    m = M.correlate(hp, key)
    return m, M.fold(m)


def locate_bits_pooled(hp, key, th, tw, tile_bit, nbits):
    """(maps, E, (oy, ox, peak, z) of E, soft): locate_bits_model.locate_bits with hp in the place of h"""
    mp = LB.maps(hp, key, th, tw, tile_bit, nbits)
    E = LB.energy(mp)
    loc = M.fold(E)
    return mp, E, loc, LB.soft(mp, loc[0], loc[1])


def locate_keys_pooled(hp, bank):
    """(maps [nk, ny, nx], loc [nk, 4]): locate_keys_model.locate_keys with hp in the place of h"""
    maps = np.stack([M.correlate(hp, k) for k in bank])
    return maps, np.array([M.fold(m) for m in maps], np.float64)


def floored(x):
    return np.floor(np.asarray(x, np.float32)).astype(np.float32)


def clip_of(kshape, shape, at, mask, marked=True, frames=F_CLIP):
    """[frames, rows, cols] f32: frame f is synth_frame(frame = 10 + f), marked with the shape's key at PSNR[mask] (or left as it is),
    floored to 8 bits and cropped at `at`"""
    tag = ("clip", kshape, mask, marked, frames)
    if tag not in _made:
        key = key_of(kshape)
        out = []
        for f in range(frames):
            x = synth_frame(*kshape, frame=10 + f)
            out.append(floored(R.embed(x, x, key, 3, PSNR[mask], "ME" if mask == 0 else "NVF")[0] if marked else x))
        _made[tag] = np.stack(out)
    (r, c), (oy, ox) = shape, at
    return np.ascontiguousarray(_made[tag][:, oy:oy + r, ox:ox + c])


def payload_table():
    ny, nx = LB.tiles_shape(P_KSHAPE[0], P_KSHAPE[1], *P_TILE)
    return (np.arange(ny * nx) % P_NBITS).astype(np.int32)


def payload_bits():
    return LB.balanced_payload(P_NBITS, 5)


def payload_clip(mask, frames=F_CLIP, psnr=P_PSNR):
    """[frames, 64, 256] f32: the frames marked with +key where the tile's bit is set and -key where not (tile_bit[t] = t mod 8,
    balanced_payload(8, 5)), floored and cropped at (20, 31): 2048 pixels per bit in the window"""
    tag = ("payload", mask, frames, psnr)
    if tag not in _made:
        key = key_of(P_KSHAPE)
        s = LB.signs_plane(P_KSHAPE, P_TILE[0], P_TILE[1], payload_table(), payload_bits())
        name = "ME" if mask == 0 else "NVF"
        out = []
        for f in range(frames):
            x = synth_frame(*P_KSHAPE, frame=10 + f)
            yp, ym = R.embed(x, x, key, 3, psnr, name)[0], R.embed(x, x, -key, 3, psnr, name)[0]
            out.append(floored(np.where(s > 0, yp, np.where(s < 0, ym, x))))
        _made[tag] = np.stack(out)
    (r, c), (oy, ox) = P_SHAPE, P_AT
    return np.ascontiguousarray(_made[tag][:, oy:oy + r, ox:ox + c])
