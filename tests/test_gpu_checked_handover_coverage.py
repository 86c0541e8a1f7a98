"""Checked Gram hand-over (wm.h wm_detect), what test_gpu_checked_handover.py leaves open: the embed (embed_march, 256-column strips
with a shifted last one) and the checking detector (detect_march<DIG>, overlapped strips of 248 owned columns) each sum the digest under
an ownership rule of their own, and the sums are exact -- a pixel BOTH leave out (a last row of a segment, a seam column, a duplicate
column) keeps the digests equal and every score plausible.  Checked here, always against the ordinary path (an engine with the
checked hand-over off, on the same modified plane: a redone frame equals it in score bits and status, a trusted one to TOL_SWITCH)
and only after an unchanged pair of the same shape was seen to hand over (counts (F, 0), one k_gram, one k_gram_ho_checked):
  1. EVERY pixel of six small planes -- the smallest cases of each strip / segment layout under both block mappings of the detector
     (4 segments of a frame per block below 4 frames, 4 frames per block from 4 on) -- has its lowest mantissa bit flipped once;
  2. named structural positions (corners, border rows / columns, every segment seam, the strip seams of both kernels, the duplicate
     columns of the shifted embed strip), +3.0 and one bit, for 2, 3, 4 and 9 frames;
  3. redo patterns: every subset of 2 .. 5 frames, singles / all / all but one / alternating of 9, and a batch whose redo flips
     statuses both ways (a pass-through plane overwritten with texture, a textured one with a constant);
  4. what follows a redo on the slot: later pairs (8 and 2 frames), wm_detect, wm_detect_keys, wm_detect_tiles and an NVF embed are
     bit-equal to a fresh engine's; a redoing slot and a trusting slot in flight together."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

from synth import synth_frame
from test_gpu_checked_handover import TOL_SWITCH, embed_detect, engine, frames, ordinary_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def _u32(v):
    """scores as bit patterns (NaN compares equal to NaN)"""
    return np.array(v, np.float32).view(np.uint32)


def _prof(rep):
    return {k: v[0] for k, v in rep.items()}


def checked_pair(wm, torch, eng, off, x, y, change=None, changed=(), slot=0, what=""):
    """embed x into y and detect y on `slot` of `eng`, with change(y) from a side stream in between.  Asserts that the counts move by
    (F - |changed|, |changed|), that the statuses are the ordinary path's (`off`, on y as it is now), that every frame of `changed` has the
    ordinary path's score bit for bit and every other frame agrees to TOL_SWITCH.  Returns (score bits, detect statuses, strength bits,
    embed statuses)"""
    F = x.shape[0]
    changed = sorted(int(f) for f in changed)
    t0, r0 = eng.checked_handover_counts()
    _, a, st, corr, std = embed_detect(wm, torch, eng, x, out=y, slot=slot, between=change)
    t1, r1 = eng.checked_handover_counts()
    assert (t1 - t0, r1 - r0) == (F - len(changed), len(changed)), (what, changed)
    ref, ref_st = ordinary_scores(wm, off, y)
    assert std == ref_st, (what, changed, std, ref_st)
    got, want = _u32(corr), _u32(ref)
    redone = np.zeros(F, bool)
    redone[changed] = True
    bad = np.flatnonzero(redone & (got != want))
    assert bad.size == 0, (what, "redone frames differ from the ordinary path", [(int(f), corr[f], ref[f]) for f in bad])
    err = np.abs(np.array(corr, np.float64) - np.array(ref, np.float64))
    bad = np.flatnonzero(~redone & ~(err <= TOL_SWITCH))
    assert bad.size == 0, (what, "trusted frames off the ordinary path", [(int(f), corr[f], ref[f]) for f in bad])
    return got, std, _u32(a), st


class Pair:
    """an engine with the checked hand-over on, its ordinary reference, a batch x and the plane y every embed writes"""

    def __init__(self, wm, torch, R, Cc, F, rps, x=None):
        self.wm, self.torch, self.R, self.C, self.F = wm, torch, R, Cc, F
        self.eng, self.off = engine(wm, R, Cc, F, rps), engine(wm, R, Cc, F, rps, checked=False)
        self.x = torch.from_numpy(frames(R, Cc, F) if x is None else x).cuda()
        self.y = torch.empty_like(self.x)
        torch.cuda.synchronize()

    def call(self, change=None, changed=(), what=""):
        return checked_pair(self.wm, self.torch, self.eng, self.off, self.x, self.y, change, changed, what=what)

    def baseline(self):
        """the unchanged pair: this shape hands over (else every test below would pass without testing anything)"""
        self.eng.prof_enable(True)
        self.eng.prof_reset()
        out = self.call(what="unchanged pair")
        rep = _prof(self.eng.prof_report())
        self.eng.prof_enable(False)
        assert rep.get("k_gram") == 1 and rep.get("k_gram_ho_checked") == 1, rep
        return out

    def close(self):
        self.eng.close()
        self.off.close()


def flip_bit(f, r, c):
    def change(y):
        import torch
        y.view(torch.int32)[f, r, c] ^= 1
    return change


def add_three(f, r, c):
    def change(y):
        y[f, r, c] += 3.0
    return change


def all_of(*changes):
    def change(y):
        for ch in changes:
            ch(y)
    return change


# ---- 1. every pixel --------------------------------------------------------------------------------------------------------------
# (rows, cols, rows per segment, frames): what each is the smallest case of
EXHAUSTIVE = [
    (4, 256, 2, 3),    # the smallest plane that hands over; 4 segments of a frame per block; detector strips own 248 + 8 columns
    (4, 256, 2, 5),    # the same with 4 frames per block (one quad and a short one)
    (7, 260, 3, 33),   # embed: one full strip + a shifted last strip with 252 duplicate columns; the last segment is one row
    (5, 496, 5, 33),   # detector: exactly two full strips of 248 columns; one segment
    (6, 500, 4, 33),   # detector: three strips, the last owns 4 columns; a short last segment
    (11, 512, 2, 3),   # 4 segments per block with 6 segments (two blocks per strip and frame); embed seam 255 | 256, no shifted strip
]


@pytest.mark.parametrize("case", EXHAUSTIVE, ids=lambda c: "%dx%d_rps%d_F%d" % c)
def test_every_pixel_is_in_the_digest(wm, tc, case):
    """call i leaves frame i % F as the embed wrote it and flips the lowest mantissa bit of one pixel in each of the other F - 1 frames;
    the pixels are taken in row-major order, F - 1 per call (the last call wraps round to the first pixels), so every pixel is visited"""
    torch = tc
    R, Cc, rps, F = case
    p = Pair(wm, torch, R, Cc, F, rps)
    p.baseline()
    n, per = R * Cc, F - 1
    ncalls = -(-n // per)
    pix = (np.arange(ncalls * per, dtype=np.int64) % n).reshape(ncalls, per)
    fr = np.array([[f for f in range(F) if f != i % F] for i in range(ncalls)], np.int64)
    idx = torch.from_numpy(fr * n + pix).cuda()
    words = p.y.view(torch.int32).view(-1)
    torch.cuda.synchronize()
    seen = np.zeros(n, bool)
    t_start = time.perf_counter()
    for i in range(ncalls):
        k = idx[i]

        def change(y, k=k):
            words[k] ^= 1

        where = [(int(f), int(q // Cc), int(q % Cc)) for f, q in zip(fr[i], pix[i])] if F <= 5 else \
            "pixels %d .. %d (row-major), frame order %s" % (pix[i][0], pix[i][-1], fr[i].tolist())
        p.call(change, fr[i], what=("call", i, "(frame, row, col) flipped:", where))
        seen[pix[i]] = True
    dt = time.perf_counter() - t_start
    print("\nevery pixel %dx%d rps %d F %d: %d calls, %.2f s" % (R, Cc, rps, F, ncalls, dt))
    assert int(seen.sum()) == R * Cc
    p.close()


# ---- 2. structural positions ----------------------------------------------------------------------------------------------------
PLANE = (11, 500, 2)  # rows, cols, rows per segment: 6 segments, the last of one row; embed strips 0 .. 255 and 244 .. 499 (12 duplicate
                      # columns 244 .. 255); detector strips own 0 .. 247, 248 .. 495, 496 .. 499


def structural_spots(R, Cc, rps):
    """named (r, c): where the ownership rules of the two digests end (after hard_frames.impulse_spots, which names the places where
    the reductions of max|e| meet: here every segment seam, the detector's own strip seams and all four border rows / columns)"""
    rm, cm = R // 2, Cc // 2
    s = {"corner_tl": (0, 0), "corner_tr": (0, Cc - 1), "corner_bl": (R - 1, 0), "corner_br": (R - 1, Cc - 1),
         "row_0": (0, cm - 3), "row_1": (1, cm + 1), "row_R-2": (R - 2, cm + 3), "row_R-1": (R - 1, cm + 5),
         "col_0": (rm, 0), "col_1": (rm - 1, 1), "col_C-2": (rm + 1, Cc - 2), "col_C-1": (rm + 2, Cc - 1)}
    for seam in range(rps, R, rps):  # both sides of every segment seam
        s["seg_r%d" % (seam - 1)] = (seam - 1, cm - 7 - seam)
        s["seg_r%d" % seam] = (seam, cm - 7 - seam)
    for c in (247, 248, 495, 496):  # the detector's strips (248 owned columns each)
        if c < Cc:
            s["detect_c%d" % c] = (c % R, c)
    for c in (255, 256):  # the embed's strips
        if c < Cc:
            s["embed_c%d" % c] = ((c + 5) % R, c)
    if Cc % 256 and Cc > 256:  # the shifted last embed strip starts at C - 256 and repeats the columns up to the last full strip's end
        s["dup_first"] = (rm + 3, Cc - 256)
        s["dup_last"] = (rm - 3, (Cc // 256) * 256 - 1)
    return s


def test_structural_spots_name_what_they_should():
    """(no GPU work) the list holds the positions the layout of PLANE has"""
    R, Cc, rps = PLANE
    s = structural_spots(R, Cc, rps)
    assert len(set(s.values())) == len(s)
    rows, cols = {r for r, _ in s.values()}, {c for _, c in s.values()}
    assert rows == set(range(R))  # rps = 2: every row is one side of a seam
    assert {0, 1, Cc - 2, Cc - 1, 247, 248, 255, 256, 495, 496, Cc - 256} <= cols
    assert all(("seg_r%d" % r) in s for r in range(1, R))


@pytest.mark.parametrize("F", [2, 3, 4, 9])
def test_structural_positions_are_in_the_digest(wm, tc, F):
    """one position in one frame per call: +3.0 on even calls, the lowest mantissa bit on odd calls, every position both ways"""
    R, Cc, rps = PLANE
    p = Pair(wm, tc, R, Cc, F, rps)
    p.baseline()
    call = 0
    for name, (r, c) in structural_spots(R, Cc, rps).items():
        for kind in (add_three, flip_bit):
            f = (call + call // F) % F  # the changed frame cycles, and not in step with the kind of change
            p.call(kind(f, r, c), {f}, what=(name, kind.__name__, "frame", f, "row", r, "col", c))
            call += 1
    p.close()


# ---- 3. redo patterns ------------------------------------------------------------------------------------------------------------
def redo_sets(F):
    if F <= 5:
        return [set(s) for n in range(1, F + 1) for s in itertools.combinations(range(F), n)]
    every = set(range(F))
    return [{f} for f in range(F)] + [every] + [every - {f} for f in range(F)] + [set(range(0, F, 2)), set(range(1, F, 2))]


@pytest.mark.parametrize("F", [2, 3, 4, 5, 9])
def test_redo_patterns(wm, tc, F):
    R, Cc, rps = PLANE
    p = Pair(wm, tc, R, Cc, F, rps)
    p.baseline()
    rng = np.random.default_rng([0x5245444F, F])
    for S in redo_sets(F):
        spots = [(f, int(rng.integers(R)), int(rng.integers(Cc))) for f in sorted(S)]
        p.call(all_of(*[flip_bit(*s) for s in spots]), S, what=("changed (frame, row, col)", spots))
    p.close()


def test_a_redo_can_flip_a_frames_status(wm, tc):
    """frame 1 of the input is constant: unsolvable, its pass-through plane is handed over like the others.  Behind the embed frame 1 of
    y becomes texture (now solvable), frame 3 the constant 77 (now unsolvable), frame 4 is rewritten with its own values (unchanged)
    and one pixel of frame 0 becomes +inf"""
    torch = tc
    R, Cc, rps = PLANE
    F = 5
    xs = frames(R, Cc, F)
    xs[1] = 77.0
    p = Pair(wm, torch, R, Cc, F, rps, x=xs)
    _, std0, _, st0 = p.baseline()
    assert st0[1] == wm.WM_UNSOLVABLE and std0[1] == wm.WM_UNSOLVABLE and [st0[f] for f in (0, 2, 3, 4)] == [wm.WM_OK] * 4
    texture = torch.from_numpy(synth_frame(R, Cc, frame=50)).cuda()
    torch.cuda.synchronize()

    def change(y):
        y[1] = texture
        y[3] = 77.0
        y[4] = y[4].clone()
        y[0, 5, 123] = float("inf")

    got, std, _, st = p.call(change, {0, 1, 3}, what="status-flipping batch")  # (2 trusted, 3 redone; bits and statuses: the ordinary path's)
    assert st == st0
    assert std[1] == wm.WM_OK and got[1] != 0           # the embed's pass-through plane, now texture: scored
    assert std[3] == wm.WM_UNSOLVABLE and got[3] == 0   # 0.0f, not -0.0f or a stale score
    assert std[2] == wm.WM_OK and std[4] == wm.WM_OK
    # and the slot goes on handing over
    p.call(what="unchanged pair after the status flips")
    p.close()


# ---- 4. the slot after a redo ----------------------------------------------------------------------------------------------------
def test_the_slot_after_a_redo(wm, tc):
    """one engine, never re-created: every call after a redo gives what the same call gives on a fresh engine, bit for bit"""
    torch = tc
    ME, NVF = wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF
    R, Cc, rps = PLANE
    FM = 8
    eng, off = engine(wm, R, Cc, FM, rps), engine(wm, R, Cc, FM, rps, checked=False)

    def step(what, x, change, changed, e=eng, o=off, shape=(R, Cc, rps)):
        """the pair on the long-lived engine (checked against the ordinary path by checked_pair) and on a fresh one: the same bits"""
        y, y2 = torch.empty_like(x), torch.empty_like(x)
        got = checked_pair(wm, torch, e, o, x, y, change, changed, what=what)
        fresh = engine(wm, shape[0], shape[1], FM, shape[2])
        want = checked_pair(wm, torch, fresh, o, x, y2, change, changed, what=(what, "fresh engine"))
        fresh.close()
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), what
        for g, w in zip(got, want):
            assert list(g) == list(w), (what, list(g), list(w))

    x8 = torch.from_numpy(frames(R, Cc, FM)).cuda()
    x8b = torch.from_numpy(frames(R, Cc, FM, first=20)).cuda()
    x2 = torch.from_numpy(frames(R, Cc, 2, first=30)).cuda()
    x2b = torch.from_numpy(frames(R, Cc, 2, first=32)).cuda()
    two = all_of(flip_bit(1, 9, 250), add_three(6, 0, 499))
    step("1: frames 1 and 6 of 8 changed", x8, two, {1, 6})
    step("2: an unchanged pair of other frames", x8b, None, ())
    step("3: frame 1 of 2 changed (redo flags of frames 2 .. 7 left by step 1)", x2, flip_bit(1, 10, 3), {1})
    step("4: an unchanged pair of 2 frames", x2b, None, ())
    step("4b: all 8 changed", x8, all_of(*[flip_bit(f, f, 31 * f) for f in range(FM)]), set(range(FM)))
    step("4c: unchanged again", x8, None, ())

    # a slot on which a redo has run, then the other calls that share its tickets, partial records and solve scratch
    Rb, Cb = 40, 500
    engb, offb = engine(wm, Rb, Cb, FM), engine(wm, Rb, Cb, FM, checked=False)
    xb = torch.from_numpy(frames(Rb, Cb, FM)).cuda()
    z = torch.from_numpy(frames(Rb, Cb, FM, first=40)).cuda()
    keys = wm.KeySet.from_seeds(Rb, Cb, [11, 12, 13])
    ny, nx = wm.Watermark.tiles_shape(Rb, Cb, 32, 32)
    torch.cuda.synchronize()
    engb.prof_enable(True)
    checked_pair(wm, torch, engb, offb, xb, torch.empty_like(xb), None, (), what="40x500: unchanged pair")
    rep = _prof(engb.prof_report())
    engb.prof_enable(False)
    assert rep.get("k_gram") == 1 and rep.get("k_gram_ho_checked") == 1, rep
    step("40x500: frames 1 and 6 of 8 changed", xb, all_of(flip_bit(1, 39, 250), add_three(6, 0, 499)), {1, 6}, e=engb, o=offb, shape=(Rb, Cb, 0))

    def detect(e):
        corr, st = ordinary_scores(wm, e, z)
        return [_u32(corr), np.array(st)]

    def detect_keys(e):
        corr, st = np.zeros((FM, 3), np.float32), np.zeros(FM, np.int32)
        e.detect_keys_async(z, keys, ME, 0, corr, st)
        e.sync(0)
        return [corr.view(np.uint32), st]

    def detect_tiles(e):
        m = torch.empty((FM, ny, nx), dtype=torch.float32, device="cuda")
        sums = torch.empty((FM, ny, nx, 3), dtype=torch.float64, device="cuda")
        st = np.zeros(FM, np.int32)
        e.detect_tiles_async(z, 32, 32, ME, 0, m, sums, st)
        e.sync(0)
        return [m.cpu().numpy().view(np.uint32), sums.cpu().numpy().view(np.uint64), st]

    def embed_nvf(e):
        y = torch.empty_like(z)
        a, st = (C.c_float * FM)(), (C.c_int * FM)()
        e.embed_async(z, z, y, NVF, 0, a_out=a, status_out=st)
        e.sync(0)
        return [y.cpu().numpy().view(np.uint32), _u32(list(a)), np.array(list(st))]

    for name, call in (("5: wm_detect of another plane", detect), ("6: wm_detect_keys", detect_keys), ("7: wm_detect_tiles", detect_tiles),
                       ("8: wm_embed, NVF", embed_nvf)):
        t0, r0 = engb.checked_handover_counts()
        got = call(engb)
        assert engb.checked_handover_counts() == (t0, r0), name
        fresh = engine(wm, Rb, Cb, FM)
        want = call(fresh)
        fresh.close()
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, g, w)
    step("40x500: an unchanged pair after the other calls", xb, None, (), e=engb, o=offb, shape=(Rb, Cb, 0))
    keys.close()
    engb.close(); offb.close()

    # both slots in flight: slot 0 redoes k frames, slot 1 trusts all of its own.  Slot 0 runs on a torch stream, so that the change is
    # queued between its embed and its detect and nothing is synced before both pairs are enqueued
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        eng.set_stream_current(0)
    y0, y1 = torch.empty_like(x8), torch.empty_like(x8b)
    outs = [((C.c_float * FM)(), (C.c_int * FM)()) for _ in range(2)]
    rounds = [{1, 6}, set(range(FM)), {0}, set(range(1, FM)), {3, 4, 5, 7}]
    first1 = None
    for rnd, S in enumerate(rounds):
        change = all_of(*[flip_bit(f, (f + rnd) % R, 61 * f + rnd) for f in sorted(S)])
        t0, r0 = eng.checked_handover_counts()
        with torch.cuda.stream(s0):
            eng.embed_async(x8, x8, y0, ME, 0)
            change(y0)
            eng.detect_async(y0, ME, 0, corr_out=outs[0][0], status_out=outs[0][1])
        eng.embed_async(x8b, x8b, y1, ME, 1)
        eng.detect_async(y1, ME, 1, corr_out=outs[1][0], status_out=outs[1][1])
        eng.sync(0)
        eng.sync(1)
        t1, r1 = eng.checked_handover_counts()
        assert (t1 - t0, r1 - r0) == (2 * FM - len(S), len(S)), (rnd, S)
        got1 = (list(_u32(list(outs[1][0]))), list(outs[1][1]))
        first1 = first1 or got1
        assert got1 == first1, ("slot 1, round", rnd)
        ref, ref_st = ordinary_scores(wm, off, y0)
        corr = list(outs[0][0])
        assert list(outs[0][1]) == ref_st, (rnd, S)
        for f in range(FM):
            if f in S:
                assert _u32(corr)[f] == _u32(ref)[f], (rnd, f, corr[f], ref[f])
            else:
                assert abs(corr[f] - ref[f]) <= TOL_SWITCH, (rnd, f, corr[f], ref[f])
    ref1, ref1_st = ordinary_scores(wm, off, y1)
    assert first1[1] == ref1_st and max(abs(p - q) for p, q in zip(list(outs[1][0]), ref1)) <= TOL_SWITCH
    eng.close(); off.close()
