"""Every route of every launcher at the smallest shapes that take it.

The launchers choose a kernel instance from (mask, window, plane alignment, width) -- for_mask_pad, for_each_sweep_part, detect_plan
and for_each_detect_launch in csrc/wm_march.hpp.  The other suites cover wm_detect over many widths and the newer calls over some
windows per route; here every call runs every window on every route, so that a launcher which hands, say, the 5x5 instance to
the 7x7 case fails by name.

Planes (40 rows: tile_rows >= 32 forces at least 32, and 40 rows are two segments of a 32-row tile):
  40 x 272            detectors: overlapped strips (two of them);            embed family: one full strip + the shifted last strip
  40 x 267            detectors: overlapped strips + one generic strip;      embed family: one full strip + one generic strip
                      (u8 at pitch 268: a u8 plane takes the vector path only when its rows are dword-aligned; dense f32 rows do)
  40 x 131            generic strips only
  40 x 272 u8, pitch 273   the generic instance on a u8 plane whose rows are not dword-aligned
Windows: ME p = 3, NVF p = 3, 5, 7, 9.  f32 and u8.  One frame and five (the 4-frames-per-block mapping plus a remainder).

No new relation and no new bound: each call is held to what its own suite holds it to -- the CPU oracle (tests/oracle_lib.py,
tests/tiles_model.py) at test_gpu_parity.py's tolerances, and bit equality between calls where their suites claim it.  The embed
family runs twice: with the input itself as the base (taken from the stencil window) and with a base of its own.  Every setting
asserts that its plane lies on the side of the vector-path rule (wm.h: alignment of a plane) that its route needs."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import tiles_model as TM
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

TOL_A, TOL_Y, TOL_CORR = 1e-4, 1e-3, 1e-5   # test_gpu_parity.py's
TOL_REGROUP = 2e-7                           # test_gpu_tiles.py: the tile sums added up against wm_detect
R, TH, TW = 40, 32, 32
ROUTES = [("overlap", 272, "f32", 0), ("overlap", 272, "u8", 0), ("split", 267, "f32", 0), ("split", 267, "u8", 268),
          ("generic", 131, "f32", 0), ("generic", 131, "u8", 0), ("unaligned", 272, "u8", 273)]   # (name, cols, dtype, pitch or 0)
WINDOWS = [("ME", 3), ("NVF", 3), ("NVF", 5), ("NVF", 7), ("NVF", 9)]
FRAMES = [1, 5]
DETECT_CALLS = ["detect", "detect_keys", "detect_offsets", "detect_tiles", "detect_keys_tiles", "compute_mask"]
EMBED_CALLS = ["embed", "embed_signs", "embed_keys", "embed_signs_multi"]
BASES = ["in", "grey"]
NKEYS, NKEYS_EMBED = 3, 5   # one more than a key group of k_detect_keys (2) / k_embed_keys (4): a full group and a short one; W is the last
KEY_SEED = 8800

# cases that a call's own argument checks refuse: {case id: the reason}, skipped by name
REFUSED = {}

SETTINGS = [(rt, win, F) for rt in ROUTES for win in WINDOWS for F in FRAMES]
CASES = [(s, call, None) for s in SETTINGS for call in DETECT_CALLS] + [(s, call, b) for s in SETTINGS for call in EMBED_CALLS for b in BASES]
CASES.sort(key=lambda c: SETTINGS.index(c[0]))   # one setting after the other: they share an engine and the reference results


def case_id(case):
    ((name, cols, dtype, pitch), (mask, p), F), call, base = case
    return "-".join([call] + ([base] if base else []) + [name, dtype, f"{mask}{p}", f"F{F}"])


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def u8_rule(got, want):
    d = np.abs(np.asarray(got).astype(int) - np.asarray(want).astype(int))
    return d.max() <= 1 and (d != 0).mean() <= 1e-3


class Setting:
    """the engine, the planes and the reference results of one (route, window, frames): built once, left unchanged"""

    def __init__(self, wm, torch, setting):
        (self.route, self.cols, self.dtype, self.pitch), (self.mask, self.p), self.F = setting
        self.wm, self.torch = wm, torch
        Cc, F = self.cols, self.F
        self.mt = wm.MASK_TYPE[self.mask]
        self.omask = O.MASK_ME if self.mask == "ME" else O.MASK_NVF
        npdt = np.uint8 if self.dtype == "u8" else np.float32
        # the key plane is larger than the image; W is its window at (0, 0)
        self.G = wm.lib().wm_detect_offsets_group()
        self.KS = wm.lib().wm_embed_signs_group() + 1   # copies of wm_embed_signs_multi: a full copy group and a short one
        self.key = synth_watermark(R + 1, Cc + self.G + 4, KEY_SEED)
        self.W = np.ascontiguousarray(self.key[:R, :Cc])
        self.xs = np.stack([synth_frame(R, Cc, frame=3 + f, dtype=npdt) for f in range(F)])
        self.grey = np.stack([synth_frame(R, Cc, frame=40 + f, dtype=npdt) for f in range(F)])
        self.xv, self.gv = self.place(self.xs), self.place(self.grey)
        # the route this setting is named after is the one its planes take: the width rule of csrc/wm_march.hpp (overlapped strips
        # for multiples of 4, the split from 264 columns on) and, where the route is not generic anyway, the vector-path rule
        assert {"overlap": Cc % 4 == 0, "split": Cc % 4 != 0 and Cc >= 264, "generic": Cc % 4 != 0 and Cc < 264, "unaligned": True}[self.route]
        for t in (self.xv, self.gv, self.empty_like_plane(), self.empty_like_plane(F * NKEYS_EMBED), self.empty_like_plane(F * self.KS)):
            if self.route != "generic":
                assert self.vector_path(t) == (self.route != "unaligned"), (self.route, t.stride(), t.data_ptr())
        self.eng = wm.Watermark(R, Cc, self.W, self.p, 40.0, nslots=2, max_frames=F)
        self.eng.set_fused(False)             # the batched sweeps: the launchers under test
        self.eng.set_checked_handover(False)
        self.closers = [self.eng]
        self.memo = {}

    def place(self, a):
        """the batch on the device: dense, or at the route's pitch"""
        t = self.torch.from_numpy(np.array(a)).cuda()
        if not self.pitch:
            return t
        buf = self.torch.zeros(a.shape[:-1] + (self.pitch,), dtype=t.dtype, device="cuda")
        buf[..., :a.shape[-1]] = t
        return buf[..., :a.shape[-1]]

    def empty_like_plane(self, n=None):
        shape = ((n,) if n else (self.F,)) + (R, self.pitch or self.cols)
        buf = self.torch.zeros(shape, dtype=self.xv.dtype, device="cuda")
        return buf[..., :self.cols]

    def vector_path(self, t):
        """the library's rule for a grey plane: a 4-byte aligned base; u8 planes also a pitch and a frame stride that are multiples
        of 4 (a lane's 4 pixels are one dword)"""
        if t.data_ptr() % 4:
            return False
        return self.dtype == "f32" or (t.stride(-2) % 4 == 0 and (t.shape[0] == 1 or t.stride(0) % 4 == 0))

    def close(self):
        for c in self.closers:
            c.close()

    def once(self, what, make):
        if what not in self.memo:
            self.memo[what] = make()
        return self.memo[what]

    def frame_f32(self, f):
        return self.xs[f].astype(np.float32)

    # ---- the reference results that several calls are held against ----
    def detect(self):
        def run():
            corr = np.asarray(self.eng.detectWatermark(self.xv, self.mt), np.float32).reshape(self.F)
            corr.setflags(write=False)
            return corr
        return self.once("detect", run)

    def tiles(self):
        def run():
            m, s = self.eng.detectTiles(self.xv, TH, TW, self.mt, sums=True)
            return m, s
        return self.once("tiles", run)

    def embed(self, base):
        def run():
            bv = self.xv if base == "in" else self.gv
            ov = self.empty_like_plane()
            a, st = np.full(self.F, np.nan, np.float32), np.full(self.F, -5, np.int32)
            self.torch.cuda.synchronize()
            self.eng.embed_async(self.xv, bv, ov, self.mt, self.wm.WM_SLOT_SYNC, a.ctypes.data_as(C.POINTER(C.c_float)),
                                 st.ctypes.data_as(C.POINTER(C.c_int)))
            assert (st == 0).all()
            return ov.cpu().numpy(), a
        return self.once(("embed", base), run)


@pytest.fixture(scope="module")
def setting_of(wm, tc):
    """setting -> its Setting; the one of the previous setting is closed when the next is asked for, the last when the module ends"""
    current = {}

    def drop():
        if current:
            current.pop("obj").close()
            current.clear()

    def get(setting):
        if current.get("key") != setting:
            drop()
            current.update(key=setting, obj=Setting(wm, tc, setting))
        return current["obj"]

    yield get
    drop()


# ---- the calls ----------------------------------------------------------------------------------------------------------------

def check_detect(s):
    """wm_detect against the CPU oracle"""
    corr = s.detect()
    for f in range(s.F):
        ref = (O.detect_u8 if s.dtype == "u8" else O.detect)(s.xs[f], s.W, p=s.p, mask=s.omask)[1]
        print(f"frame {f}: {corr[f]:.7f} oracle {ref:.7f}")
        assert abs(float(corr[f]) - ref) <= TOL_CORR, (f, corr[f], ref)


def check_detect_keys(s):
    """the engine's W as the last key of a bank of NKEYS: that key's score is wm_detect's, bit for bit"""
    bank = s.wm.KeySet(R, s.cols, NKEYS)
    s.closers.append(bank)
    for k in range(NKEYS - 1):
        bank.set(k, synth_watermark(R, s.cols, KEY_SEED + 1 + k))
    bank.set(NKEYS - 1, s.W)
    got = np.asarray(s.eng.detectKeys(s.xv, bank, s.mt)).reshape(s.F, NKEYS)
    print(got[:, NKEYS - 1], s.detect())
    assert bits_equal(got[:, NKEYS - 1], s.detect()), (got, s.detect())
    assert not bits_equal(got[:, 0], s.detect())


def check_detect_offsets(s):
    """2 x (G + 1) offsets into the key plane (a full column group and the launch of the remainder): offset (0, 0) is W, so its
    score is wm_detect's bit for bit; the last offset against the oracle on the shifted window"""
    bank = s.wm.KeySet(s.key.shape[0], s.key.shape[1], 1)
    s.closers.append(bank)
    bank.set(0, s.key)
    ny, nx = 2, s.G + 1
    got = np.asarray(s.eng.detectOffsets(s.xv, bank, 0, 0, 0, ny, nx, s.mt)).reshape(s.F, ny, nx)
    assert bits_equal(got[:, 0, 0], s.detect()), (got[:, 0, 0], s.detect())
    win = np.ascontiguousarray(s.key[ny - 1:ny - 1 + R, nx - 1:nx - 1 + s.cols])
    for f in range(s.F):
        ref = O.detect(s.frame_f32(f), win, p=s.p, mask=s.omask)[1]
        print(f"frame {f}: offset ({ny - 1}, {nx - 1}) {got[f, -1, -1]:.7f} oracle {ref:.7f}")
        assert abs(float(got[f, -1, -1]) - ref) <= TOL_CORR, (f, got[f, -1, -1], ref)


def check_detect_tiles(s):
    """32 x 32 tiles: the tile sums added up give wm_detect's score; each tile agrees with tests/tiles_model.py"""
    m, sums = s.tiles()
    ny, nx = TM.tiles_shape(R, s.cols, TH, TW)
    assert m.shape == (s.F, ny, nx) and sums.shape == (s.F, ny, nx, 3)
    total = TM.score_of(sums.sum(axis=(1, 2)))
    assert np.all(np.abs(total.astype(np.float64) - s.detect().astype(np.float64)) <= TOL_REGROUP), (total, s.detect())
    for f in range(s.F):
        ref = TM.tile_map(s.xs[f], s.W, TH, TW, s.p, s.omask)[1]
        assert np.isfinite(m[f]).all() and np.isfinite(ref).all()
        print(f"frame {f}: worst tile {np.abs(m[f] - ref).max():.2e}")
        assert float(np.abs(m[f] - ref).max()) <= TOL_CORR, (f, m[f], ref)


def check_detect_keys_tiles(s):
    """W as the last key of a bank of NKEYS: that key's map and sums are wm_detect_tiles', bit for bit"""
    bank = s.wm.KeySet(R, s.cols, NKEYS)
    s.closers.append(bank)
    for k in range(NKEYS - 1):
        bank.set(k, synth_watermark(R, s.cols, KEY_SEED + 1 + k))
    bank.set(NKEYS - 1, s.W)
    m, sums = s.eng.detectKeysTiles(s.xv, bank, TH, TW, s.mt, sums=True)
    rm, rs = s.tiles()
    assert bits_equal(m[:, NKEYS - 1], rm) and bits_equal(sums[:, NKEYS - 1], rs)
    assert not bits_equal(m[:, 0], rm)


def check_compute_mask(s):
    """NVF: the mask equals the oracle's bit for bit; ME: the error sequence and the mask equal the oracle's on the GPU's own
    coefficients bit for bit (tests/test_gpu_parity.py)"""
    m, e, c, st = s.eng.computeMask(s.xv, s.mt, want_error_sequence=True)
    m, e = m.cpu().numpy(), e.cpu().numpy()
    assert list(st) == [0] * s.F
    for f in range(s.F):
        if s.mask == "NVF":
            assert bits_equal(m[f], O.nvf_mask(s.frame_f32(f), s.p)), f
        else:
            eo = O.error_sequence(s.frame_f32(f), c[f])
            assert bits_equal(e[f], eo), f
            assert bits_equal(m[f], np.abs(eo) / np.abs(eo).max()), f


def check_embed(s, base):
    """wm_embed against the CPU oracle.  A u8 base of its own: the oracle's embed on the planes as f32, clamped to [0, 255] and
    truncated as wmo_embed_u8 does (main.cpp:356,380,405), held to the u8 rule"""
    y, a = s.embed(base)
    for f in range(s.F):
        if s.dtype == "u8" and base == "in":
            so, yo, ao = O.embed_u8(s.xs[f], s.W, p=s.p, mask=s.omask)
            assert u8_rule(y[f], yo), f
        elif s.dtype == "u8":
            so, yo, ao = O.embed(s.frame_f32(f), s.grey[f].astype(np.float32), s.W, p=s.p, mask=s.omask)
            assert u8_rule(y[f], np.clip(yo, 0.0, 255.0).astype(np.uint8)), f
        else:
            so, yo, ao = O.embed(s.xs[f], s.xs[f] if base == "in" else s.grey[f], s.W, p=s.p, mask=s.omask)
            print(f"frame {f}: worst pixel {np.abs(y[f] - yo).max():.2e}")
            np.testing.assert_allclose(y[f], yo, rtol=0, atol=TOL_Y)
        assert so == 0 and a[f] == pytest.approx(ao, rel=TOL_A), (f, a[f], ao)
    assert not np.array_equal(y, s.xs if base == "in" else s.grey)


def check_embed_signs(s, base):
    """every tile +1: wm_embed's plane and strength, bit for bit"""
    ny, nx = TM.tiles_shape(R, s.cols, TH, TW)
    ov = s.empty_like_plane()
    a, st = np.full(s.F, np.nan, np.float32), np.full(s.F, -5, np.int32)
    s.torch.cuda.synchronize()
    s.eng.embed_signs_async(s.xv, s.xv if base == "in" else s.gv, ov, TH, TW, np.ones((s.F, ny, nx), np.int8), s.mt, s.wm.WM_SLOT_SYNC, a, st)
    y, ar = s.embed(base)
    assert (st == 0).all() and bits_equal(ov.cpu().numpy(), y) and bits_equal(a, ar)


def check_embed_keys(s, base):
    """W as the last key of a bank of NKEYS_EMBED: that key's copies and strengths are wm_embed's, bit for bit"""
    K = NKEYS_EMBED
    bank = s.wm.KeySet(R, s.cols, K)
    s.closers.append(bank)
    for k in range(K - 1):
        bank.set(k, synth_watermark(R, s.cols, KEY_SEED + 1 + k))
    bank.set(K - 1, s.W)
    ov = s.empty_like_plane(s.F * K)
    a, st = np.full((s.F, K), np.nan, np.float32), np.full(s.F, -5, np.int32)
    s.torch.cuda.synchronize()
    s.eng.embed_keys_async(s.xv, s.xv if base == "in" else s.gv, ov, bank, s.mt, s.wm.WM_SLOT_SYNC, a, st)
    y, ar = s.embed(base)
    copies = ov.cpu().numpy().reshape(s.F, K, R, s.cols)
    assert (st == 0).all() and bits_equal(copies[:, K - 1], y) and bits_equal(a[:, K - 1], ar)
    assert not bits_equal(copies[:, 0], y)


def check_embed_signs_multi(s, base):
    """one copy more than a copy group; the last copy's table is all +1: its planes and the call's strengths are wm_embed's, bit for
    bit (tests/test_gpu_signs_multi.py); the first copy's is all -1: its planes differ"""
    K = s.KS
    ny, nx = TM.tiles_shape(R, s.cols, TH, TW)
    signs = np.ones((s.F, K, ny, nx), np.int8)
    signs[:, 0] = -1
    ov = s.empty_like_plane(s.F * K)
    a, st = np.full(s.F, np.nan, np.float32), np.full(s.F, -5, np.int32)
    s.torch.cuda.synchronize()
    s.eng.embed_signs_multi_async(s.xv, s.xv if base == "in" else s.gv, ov, TH, TW, K, signs, s.mt, s.wm.WM_SLOT_SYNC, a, st)
    y, ar = s.embed(base)
    copies = ov.cpu().numpy().reshape(s.F, K, R, s.cols)
    assert (st == 0).all() and bits_equal(copies[:, K - 1], y) and bits_equal(a, ar)
    assert not bits_equal(copies[:, 0], y)


CHECKS = {"detect": check_detect, "detect_keys": check_detect_keys, "detect_offsets": check_detect_offsets, "detect_tiles": check_detect_tiles,
          "detect_keys_tiles": check_detect_keys_tiles, "compute_mask": check_compute_mask, "embed": check_embed, "embed_signs": check_embed_signs,
          "embed_keys": check_embed_keys, "embed_signs_multi": check_embed_signs_multi}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_route(setting_of, case):
    if case_id(case) in REFUSED:
        pytest.skip(REFUSED[case_id(case)])
    setting, call, base = case
    s = setting_of(setting)
    if base is None:
        CHECKS[call](s)
    else:
        CHECKS[call](s, base)


def test_the_case_list_is_complete():
    """every call x route x window x frame count is a case (the embed family with both bases), none twice, and REFUSED names
    cases of the list only"""
    ids = [case_id(c) for c in CASES]
    assert len(ids) == len(set(ids)) == len(SETTINGS) * (len(DETECT_CALLS) + len(EMBED_CALLS) * len(BASES)) == 980
    assert set(REFUSED) <= set(ids)
