"""The payload of wm_embed_bits / wm_detect_bits restated in plain Python over the CPU oracle (tests/oracle_lib.py, tiles_model.py).

layout(ny, nx, nbits, seed): wm_bits_layout -- a Fisher-Yates shuffle of 0 .. T - 1 driven by splitmix64(seed), then mod nbits.
signs_of: tile signs +1 / -1 / 0 from a payload.  compose: the marked frame built from the oracle's embed with W and with -W,
selected per tile (the strength does not see the sign of W).  soft: the three f64 sums of every tile (tiles_model), added PER BIT
one after the other in ascending tile index (np.cumsum, not np.sum), then the score expression of every detector here."""
import numpy as np

import oracle_lib as O
import tiles_model as TM

M64 = (1 << 64) - 1


def splitmix64(state):
    """(next state, output)"""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def layout(ny, nx, nbits, seed):
    T = ny * nx
    perm = list(range(T))
    state = seed & M64
    for i in range(T - 1, 0, -1):
        state, z = splitmix64(state)
        j = z % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array([v % nbits for v in perm], np.int32)


def payload_bits(payload, nbits):
    """bit b = payload[b // 8] >> (b % 8) & 1 as an int array [nbits]"""
    raw = np.frombuffer(bytes(payload), np.uint8)
    return np.array([(int(raw[b // 8]) >> (b % 8)) & 1 for b in range(nbits)], np.int64)


def pack_bits(bits):
    return np.packbits(np.asarray(bits, bool), bitorder="little").tobytes()


def signs_of(tile_bit, payload, nbits):
    """int8 [T]: +1 where the tile's bit is set, -1 where it is not, 0 where the tile carries no bit"""
    bits = payload_bits(payload, nbits)
    tb = np.asarray(tile_bit)
    return np.where(tb < 0, 0, np.where(bits[np.maximum(tb, 0)] == 1, 1, -1)).astype(np.int8)


def tile_index(R, Cc, th, tw):
    """int [R, C]: the tile ty * nx + tx every pixel belongs to (the last tile of each axis takes the remainder)"""
    ny, nx = TM.tiles_shape(R, Cc, th, tw)
    ty = np.minimum(np.arange(R) // th, ny - 1)
    tx = np.minimum(np.arange(Cc) // tw, nx - 1)
    return ty[:, None] * nx + tx[None, :]


def select(signs, th, tw, plus, minus, zero):
    """per-tile selection of three planes [..., R, C] by the tile signs [T]"""
    R, Cc = plus.shape[-2:]
    s = np.asarray(signs).reshape(-1)[tile_index(R, Cc, th, tw)]
    return np.where(s > 0, plus, np.where(s < 0, minus, zero))


def compose(x, W, th, tw, signs, p=3, psnr=40.0, mask=0):
    """the frame wm_embed_signs writes, from the oracle: (status, y f32, a)"""
    st, yp, a = O.embed(x, x, W, p=p, psnr=psnr, mask=mask)
    st2, ym, a2 = O.embed(x, x, -W, p=p, psnr=psnr, mask=mask)
    assert st == st2 == 0 and a == a2
    return st, select(signs, th, tw, yp, ym, np.asarray(x, np.float32)).astype(np.float32), a


def pool(sums, tile_bit, nbits):
    """f64 [nbits, 3]: the tile sums [T, 3] of every bit added one after the other in ascending tile index (zeros for a bit without
    a tile: its score is 0 / 0)"""
    s = np.asarray(sums, np.float64).reshape(-1, 3)
    tb = np.asarray(tile_bit).reshape(-1)
    out = np.zeros((nbits, 3))
    for b in range(nbits):
        rows = s[tb == b]
        if len(rows):
            out[b] = np.cumsum(rows, axis=0)[-1]
    return out


def soft_of_sums(sums, tile_bit, nbits):
    return TM.score_of(pool(sums, tile_bit, nbits))


def soft(img, W, th, tw, tile_bit, nbits, p=3, mask=0):
    """(status, soft f32 [nbits]); an unsolvable frame: zeros"""
    st, prod = TM.pixel_products(img, W, p, mask)
    if st != 0:
        return st, np.zeros(nbits, np.float32)
    return 0, soft_of_sums(TM.sums_of(prod, th, tw), tile_bit, nbits)
