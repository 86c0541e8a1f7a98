"""wm_key_schedule restated in numpy: which key of a bank does frame n of a video take?

z(n) is the (n + 1)-th output of the splitmix64 that wm_bits_layout documents (bits_model.splitmix64), started at `seed`.  Its state
only ever grows by one constant, so the (n + 1)-th state is seed + (n + 1) * 0x9E3779B97F4A7C15 modulo 2^64 and z(n) needs no walk
from frame 0: schedule() forms every entry directly, in uint64 arithmetic that wraps as the C code's does.  schedule_walk() is the
same thing the slow way -- next() called first + i + 1 times -- for first frames small enough to walk."""
import numpy as np

from bits_model import splitmix64

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def z_of(seed, n):
    """the (n + 1)-th splitmix64 output from `seed`, in Python integers"""
    z = (seed + (n + 1) * GAMMA) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def schedule(nkeys, seed, first_frame, frames):
    """int32 [frames]: key_of_frame[i] = z(first_frame + i) mod nkeys"""
    with np.errstate(over="ignore"):
        n = np.uint64(first_frame & M64) + np.arange(frames, dtype=np.uint64) + np.uint64(1)
        z = np.uint64(seed & M64) + n * np.uint64(GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(nkeys)).astype(np.int32)


def round_trip_case(rows=270, cols=480, frames=8, nkeys=4, seed=0x5E1EC7, first_frame=1000):
    """the schedule round trip both test files run (the oracle alone on the CPU, the library on the GPU): `frames` synthetic frames
    of a clip that starts at `first_frame`, a bank of `nkeys` host-made keys, the clip's schedule and the schedule rotated by one key.
    Returns (xs f32 [F, R, C], Ws list of f32 [R, C], table int32 [F], rotated int32 [F])"""
    from synth import synth_frame, synth_watermark
    xs = np.stack([synth_frame(rows, cols, frame=first_frame + f) for f in range(frames)])
    Ws = [synth_watermark(rows, cols, seed=9100 + 17 * k) for k in range(nkeys)]
    table = schedule(nkeys, seed, first_frame, frames)
    return xs, Ws, table, ((table + 1) % nkeys).astype(np.int32)


def oracle_round_trip(xs, Ws, table, rotated, mask=0, p=3, psnr=40.0):
    """the oracle's marked frames, and its scores under the right and the rotated schedule: (ys [F, R, C], right [F], wrong [F])"""
    import oracle_lib as O
    ys, right, wrong = [], [], []
    for f, x in enumerate(xs):
        st, y, a = O.embed(x, x, Ws[table[f]], p=p, psnr=psnr, mask=mask)
        assert st == 0
        ys.append(y)
        right.append(O.detect(y, Ws[table[f]], p=p, mask=mask)[1])
        wrong.append(O.detect(y, Ws[rotated[f]], p=p, mask=mask)[1])
    return np.stack(ys), np.array(right), np.array(wrong)


def schedule_walk(nkeys, seed, first_frame, frames):
    """the same table from the generator itself: next() first_frame + frames times, the last `frames` outputs kept"""
    state = seed & M64
    out = []
    for n in range(first_frame + frames):
        state, z = splitmix64(state)
        if n >= first_frame:
            out.append(z % nkeys)
    return np.array(out, np.int32)
