"""numpy model of wm_locate_keys (wm.h), f64 throughout: wm_locate's model (tests/locate_model.py) per key of a
bank, the pairing identity that lets two keys ride in one complex transform, and the rank of a frame's records.

h and the keys are real, so with K = key_a + i key_b

    ifft2(conj(fft2(h)) fft2(K)) = map_a + i map_b

the two cross-correlations of locate_model.correlate.  The finding table of the issue is built here too (bank, marked and
unmarked frames, crops), so that the CPU and the GPU tests stand on the same inputs.
"""
import numpy as np

import locate_model as M
import np_restatement as R
from synth import synth_frame, synth_watermark

NKEYS = 5
OWNER = (1, 4, None)  # the key frame f is marked with; None: unmarked
# (key shape, crop shape, true offset)
CASES = [((80, 300), (64, 256), (16, 44)), ((120, 330), (64, 256), (20, 31)), ((300, 520), (96, 128), (150, 300)),
         ((301, 523), (271, 483), (30, 40))]
_banks, _marked = {}, {}


def bank_of(kshape, nkeys=NKEYS):
    """[nkeys, key_rows, key_cols] f32: key k is synth_watermark(seed = 9300 + 11 k + key_rows)"""
    tag = (kshape, nkeys)
    if tag not in _banks:
        _banks[tag] = np.stack([synth_watermark(*kshape, seed=9300 + 11 * k + kshape[0]) for k in range(nkeys)])
    return _banks[tag]


def frames_of(kshape, shape, at, mask, dtype="f32", owners=OWNER, bank=None):
    """[F, rows, cols]: frame f is synth_frame(frame = 10 + f) marked with key owners[f] of the bank at the key's shape (psnr 40,
    p = 3; None: left unmarked) and cropped at `at`; u8: floored to 8 bits"""
    bank = bank_of(kshape) if bank is None else bank
    tag = (kshape, mask, tuple(owners), id(bank))
    if tag not in _marked:
        out = []
        for f, k in enumerate(owners):
            x = synth_frame(*kshape, frame=10 + f)
            out.append(x if k is None else R.embed(x, x, bank[k], 3, 40.0, "ME" if mask == 0 else "NVF")[0].astype(np.float32))
        _marked[tag] = (np.stack(out), bank)  # (the bank is kept alive: its id is part of the tag)
    (r, c), (oy, ox) = shape, at
    x = np.ascontiguousarray(_marked[tag][0][:, oy:oy + r, ox:ox + c])
    return np.floor(x).astype(np.uint8) if dtype == "u8" else x


def pair_maps(h, ka, kb):
    """(map_a, map_b) out of ONE complex transform of ka + i kb, by an f64 FFT of the key's size"""
    ka, kb = np.asarray(ka, np.float64), np.asarray(kb, np.float64)
    ny, nx = ka.shape[0] - h.shape[0] + 1, ka.shape[1] - h.shape[1] + 1
    full = np.fft.ifft2(np.conj(np.fft.fft2(h, ka.shape)) * np.fft.fft2(ka + 1j * kb))
    return np.ascontiguousarray(full.real[:ny, :nx]), np.ascontiguousarray(full.imag[:ny, :nx])


def locate_keys(x, bank, c, mask, p=3):
    """the model of one frame against every key of `bank`: (maps [nk, ny, nx], loc [nk, 4]) -- locate_model.locate per key with the
    coefficients c; a key plane that is all zero gives a zero map and (0, 0, 0, NaN)"""
    h = M.h_plane(x, c, mask, p)
    maps = np.stack([M.correlate(h, k) for k in bank])
    return maps, np.array([M.fold(m) for m in maps], np.float64)


def rank(loc):
    """(best, z_best, z_next) of one frame's [nk, 4] records: the key with the largest z (NaN ignored, ties: the smallest index), that
    z and the largest z among the others (NaN: none); (-1, NaN, NaN) when every z is NaN"""
    z = np.asarray(loc, np.float64).reshape(-1, 4)[:, 3]
    ok = ~np.isnan(z)
    if not ok.any():
        return -1, float("nan"), float("nan")
    best = int(np.flatnonzero(ok & (z == z[ok].max()))[0])
    ok[best] = False
    return best, float(z[best]), float(z[ok].max()) if ok.any() else float("nan")
