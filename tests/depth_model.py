"""The meaning of a d-bit sample (wm.h, "Samples of 9 to 16 bits"), restated in numpy.  Nothing here reads the library.

bits = d in 9..16, maxv = 2^d - 1; k_in = (float)(255.0 / maxv) and k_out = (float)(maxv / 255.0), each the double quotient rounded
once to f32.
  unpack(v): s = v >> (16 - d) when msb-aligned, else min(v, maxv);  g = (float)s * k_in, one f32 multiply.
  pack(g):   t = g * k_out, one f32 multiply;  t = fmin(fmax(t, 0), maxv) with NaN -> 0;  q = rint(t), ties to even;
             v = q << (16 - d) when msb-aligned, else q."""
import numpy as np

BITS = tuple(range(9, 17))


def maxv(bits):
    assert 9 <= bits <= 16, bits
    return (1 << bits) - 1


def scale(bits):
    """(k_in, k_out) as numpy float32 scalars"""
    m = float(maxv(bits))
    return np.float32(255.0 / m), np.float32(m / 255.0)


def unpack(v, bits, msb_aligned=False):
    v = np.asarray(v)
    assert v.dtype == np.uint16, v.dtype
    s = (v >> np.uint16(16 - bits)) if msb_aligned else np.minimum(v, np.uint16(maxv(bits)))
    return (s.astype(np.float32) * scale(bits)[0]).astype(np.float32)


def pack(g, bits, msb_aligned=False):
    g = np.asarray(g)
    assert g.dtype == np.float32, g.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        t = (g * scale(bits)[1]).astype(np.float32)     # one f32 multiply (it may overflow to inf: clamped below)
        t = np.where(np.isnan(t), np.float32(0), t)     # fmax(NaN, 0) = 0
        t = np.minimum(np.maximum(t, np.float32(0)), np.float32(maxv(bits)))
        q = np.rint(t).astype(np.uint32)                # np.rint: ties to even
    return (q << np.uint32(16 - bits) if msb_aligned else q).astype(np.uint16)


def quantise(x, bits):
    """a [0, 255] f32 plane as d-bit samples (LSB-aligned): what a d-bit master of that picture holds"""
    return pack(np.asarray(x, np.float32), bits)


def tie_inputs(bits):
    """f32 values g whose t = g * k_out lands exactly on k + 0.5, for even and odd k: (g, k) arrays.  Searched among the floats around
    (k + 0.5) / k_out; only exact hits are kept (asserted non-empty for both parities by the tests that use them)"""
    k_out = scale(bits)[1]
    gs, ks = [], []
    m = maxv(bits)
    cand = sorted(set(list(range(0, 64)) + [m // 3, m // 3 + 1, m // 2, m // 2 + 1, m - 2, m - 1]))
    for k in cand:
        target = np.float32(k + 0.5)
        g0 = np.float32(float(target) / float(k_out))
        g = g0
        for _ in range(3):
            g = np.nextafter(g, np.float32(-np.inf))
        for _ in range(7):
            if np.float32(g * k_out) == target:
                gs.append(g)
                ks.append(k)
                break
            g = np.nextafter(g, np.float32(np.inf))
    return np.array(gs, np.float32), np.array(ks, np.int64)
