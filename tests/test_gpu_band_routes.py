"""Row bands (include/wm.h wm_band_*, wm_band_*_dev) on every launch route, window, type and batch size, against a one-band run.

A band is not separate code: wm_band_configure sets the owned rows of the launch geometry, and every sweep clips to them on its own
route (make_job in wm_device.hpp, the core and border clips of k_gram, chunk_pos in wm_gram_common.hpp).  So a band goes through the
launch routes that tests/test_gpu_launch_routes.py walks for the whole-image calls; this file walks them for the bands, with the same
seven planes at 40 rows, the same windows (ME 3, NVF 3 / 5 / 7 / 9) and one frame or five.  A band's planes are ROW SLICES of the
batch buffer: pitch, base alignment and frame stride stay those of the route, and every setting asserts the side of the vector-path
rule its route needs.

Splits, in global rows, h = max(2, p // 2 + 1):
  even      band_rows(40, r, 3)
  ragged    [0, h) (a top band with exactly the halo below it), [h, h + 1) (a one-row interior band), [h + 1, 38) (the bulk, with 5 rows
            per segment -- 4 where 5 divide it -- so that its last segment is short), [38, 40) (a two-row bottom band).
            For p >= 5 wm_band_configure REFUSES the bulk band: it holds the 2 rows below row 38 where the halo rule wants h >= 3.
            Those settings are one case each that asserts the refusal, and the split runs as
  ragged-h  the same with the smallest bottom band the halo rule admits, [40 - h, 40) (p >= 5 only; for p = 3 it is `ragged`)
  one-row   [0, 39), [39, 40), on the overlap-f32 and generic-u8 routes: refused as well -- the band above the last row holds ONE
            row below its own, and an interior side needs two.  One case per setting asserts that refusal and holds the bottom band's
            own Gram sums to tests/band_model.py (it sums the border rows 38, 39, 40 of the positions; no accepted split has a band
            that sums row 38 too).

References: E1, a context over the whole plane in band mode (0, 40, 40) fed the same totals and scalars as the bands; a plain
context outside band mode; tests/band_model.py and the CPU oracle.  Bounds are those of the suites that hold the same quantities
(test_gpu_bands.py, test_gpu_parity.py, test_gpu_tiles.py) and bit equality where the arithmetic per pixel is the same: each is named
where it is used.  The band phases run with several frames through wm.lib() (the Python wrappers are for one)."""
import ctypes as C

import numpy as np
import pytest

import band_model as BM
import oracle_lib as O
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

TOL_A, TOL_Y, TOL_CORR = 1e-4, 1e-3, 1e-5   # test_gpu_parity.py's
TOL_EXACT_SUM = 1e-13                        # test_gpu_bands.py: f64 sums of exact products, added up in another order
TOL_ENGINES_SS, TOL_ENGINES_CORR = 1e-6, 2e-6   # test_gpu_bands.py: a band set against the whole-image engine
TOL_SQUARES = 1e-5                           # test_gpu_tiles.py: a tile's sums of squares against the model
R = 40
ROUTES = [("overlap", 272, "f32", 0), ("overlap", 272, "u8", 0), ("split", 267, "f32", 0), ("split", 267, "u8", 268),
          ("generic", 131, "f32", 0), ("generic", 131, "u8", 0), ("unaligned", 272, "u8", 273)]   # (name, cols, dtype, pitch or 0)
WINDOWS = [("ME", 3), ("NVF", 3), ("NVF", 5), ("NVF", 7), ("NVF", 9)]
FRAMES = [1, 5]
EVEN = [(0, 14), (14, 27), (27, 40)]         # bands.band_rows(40, r, 3)
ONE_ROW_ROUTES = [ROUTES[0], ROUTES[5]]
PHASES = ["gram", "solve", "stats", "embed-in", "embed-grey", "embed-rgb", "detect", "dev"]
FLAT_FRAME, FLAT_VALUE = 2, 77


def halo(p):
    return max(2, p // 2 + 1)


def split_rows(split, p):
    h = halo(p)
    return {"even": EVEN, "ragged": [(0, h), (h, h + 1), (h + 1, R - 2), (R - 2, R)],
            "ragged-h": [(0, h), (h, h + 1), (h + 1, R - h), (R - h, R)], "one-row": [(0, R - 1), (R - 1, R)]}[split]


def refused_band(split, p):
    """index of the band wm_band_configure refuses, or None"""
    if split == "one-row":
        return 0
    return 2 if split == "ragged" and p >= 5 else None


def splits_of(route, p):
    return ["even", "ragged"] + (["ragged-h"] if p >= 5 else []) + (["one-row"] if route in ONE_ROW_ROUTES else [])


SETTINGS = [(rt, win, F, sp) for rt in ROUTES for win in WINDOWS for F in FRAMES for sp in splits_of(rt, win[1])]


def phases_of(setting):
    rt, (mask, p), F, sp = setting
    if refused_band(sp, p) is not None:
        return ["refused"]
    ph = [x for x in PHASES if x != "embed-rgb" or rt == ROUTES[0]]
    return ph + (["flat"] if (mask, F, sp) == ("ME", 5, "even") else [])


CASES = [(s, ph) for s in SETTINGS for ph in phases_of(s)]   # one setting after the other: its cases share the engines and the results


def case_id(case):
    ((name, cols, dtype, pitch), (mask, p), F, sp), phase = case
    return "-".join([phase, name, dtype, f"{mask}{p}", f"F{F}", sp])


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


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Band:
    def __init__(self, eng, r0, r1, g0, g1):
        self.eng, self.r0, self.r1, self.g0, self.g1 = eng, r0, r1, g0, g1

    def view(self, t):
        """the band's plane of a batch [F, (3,) 40, cols]: a row slice, not a copy"""
        return t[..., self.g0:self.g1, :]


class Setting:
    """the planes, the band engines, E1, the plain engine and the results of one (route, window, frames, split): built once, each
    phase run once (`once`) and left unchanged"""

    def __init__(self, wm, torch, setting, flat=False):
        (self.route, self.cols, self.dtype, self.pitch), (self.mask, self.p), self.F, self.split = setting
        self.wm, self.torch, self.L = wm, torch, wm.lib()
        Cc, F = self.cols, self.F
        self.mt = wm.MASK_TYPE[self.mask]
        self.omask = O.MASK_ME if self.mask == "ME" else O.MASK_NVF
        npdt = np.uint8 if self.dtype == "u8" else np.float32
        self.W = synth_watermark(R, Cc, 8800)
        self.xs = np.stack([synth_frame(R, Cc, frame=3 + f, dtype=npdt) for f in range(F)])
        if flat:
            self.xs[FLAT_FRAME] = FLAT_VALUE
        self.grey = np.stack([synth_frame(R, Cc, frame=40 + f, dtype=npdt) for f in range(F)])
        self.xv, self.gv = self.place(self.xs), self.place(self.grey)
        assert {"overlap": Cc % 4 == 0, "split": Cc % 4 != 0 and Cc >= 264, "generic": Cc % 4 != 0 and Cc < 264, "unaligned": True}[self.route]
        self.closers = []
        self.memo = {}
        h = halo(self.p)
        self.bands = []
        self.refusals = []
        for k, (r0, r1) in enumerate(split_rows(self.split, self.p)):
            g0, g1 = max(0, r0 - h), min(R, r1 + h)
            g0 = min(g0, max(0, g1 - 4))       # as many halo rows as it takes to reach 4 plane rows
            g1 = max(g1, min(R, g0 + 4))
            e = self.engine(g1 - g0, np.ascontiguousarray(self.W[g0:g1]))
            b = Band(e, r0, r1, g0, g1)
            try:
                e.band_configure(r0 - g0, r1 - g0, R)
            except RuntimeError as err:
                self.refusals.append((k, str(err)))
                continue
            if self.split.startswith("ragged") and k == 2:
                rps = 5 if (r1 - r0) % 5 else 4
                assert (r1 - r0) % rps and r1 - r0 > rps     # more than one segment, the last one short
                e.set_rows_per_segment(rps)
            self.bands.append(b)
            for t in (self.xv, self.gv, self.sentinel_like(self.xv)[0]):
                # the route this setting is named after is the one the band's planes take (wm.h: alignment of a plane)
                if self.route != "generic":
                    assert self.vector_path(b.view(t)) == (self.route != "unaligned"), (self.route, b.view(t).stride(), b.view(t).data_ptr())
        want = refused_band(self.split, self.p)
        assert [k for k, _ in self.refusals] == ([] if want is None else [want]), self.refusals
        self.e1 = Band(self.engine(R, self.W), 0, R, 0, R)
        self.e1.eng.band_configure(0, R, R)
        self.plain = self.engine(R, self.W)

    def engine(self, rows, W):
        e = self.wm.Watermark(rows, self.cols, W, self.p, 40.0, nslots=2, max_frames=self.F)
        e.set_fused(False)               # the batched sweeps: the launchers under test
        e.set_checked_handover(False)
        self.closers.append(e)
        return e

    def place(self, a):
        """the batch on the device: dense, or at the route's pitch"""
        t = self.torch.from_numpy(np.array(a)).cuda()
        if not self.pitch:
            return t
        buf = self.torch.zeros(a.shape[:-1] + (self.pitch,), dtype=t.dtype, device="cuda")
        buf[..., :a.shape[-1]] = t
        return buf[..., :a.shape[-1]]

    def whole(self, v):
        """the whole buffer under a plane view: the pitch padding included"""
        if not self.pitch or v.stride(-2) == v.shape[-1]:
            return v
        return self.torch.as_strided(v, v.shape[:-1] + (self.pitch,), v.stride(), v.storage_offset())

    def sentinel_like(self, base_view):
        """(a view like base_view, its whole buffer) filled with what no store of an embed leaves: NaN for f32; for u8 a checkerboard
        that differs from the base at every pixel (base + 1 or base - 1 mod 256), so that a stray store of the base shows as well"""
        torch = self.torch
        wb = self.whole(base_view)
        if wb.dtype == torch.float32:
            buf = torch.full(wb.shape, float("nan"), dtype=torch.float32, device="cuda")
        else:
            rr = torch.arange(wb.shape[-2], device="cuda")[:, None]
            cc = torch.arange(wb.shape[-1], device="cuda")[None, :]
            step = torch.where((rr + cc) % 2 == 0, 1, 255)
            buf = ((wb.to(torch.int32) + step) % 256).to(torch.uint8).contiguous()
        return buf[..., :self.cols], buf

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

    def f32(self, a):
        return np.asarray(a).astype(np.float32)

    def everyone(self):
        return self.bands + [self.e1]

    # ---- the band calls with F frames, through the C ABI ----
    def c_gram(self, b, batch):
        pl = self.wm.plane_of(b.view(batch), 1)
        out = np.full(44 * self.F, np.nan)
        self.torch.cuda.synchronize()
        b.eng._chk(self.L.wm_gram(b.eng._ctx, C.byref(pl), dp(out), 0))
        return out.reshape(self.F, 44)

    def c_solve(self, b, totals):
        st = np.full(self.F, -5, np.int32)
        t = np.ascontiguousarray(totals, np.float64)
        b.eng._chk(self.L.wm_band_solve(b.eng._ctx, dp(t), self.F, st.ctypes.data_as(C.POINTER(C.c_int)), 0))
        return st

    def c_stats(self, b, batch):
        pl = self.wm.plane_of(b.view(batch), 1)
        out = np.full(2 * self.F, np.nan)
        self.torch.cuda.synchronize()
        b.eng._chk(self.L.wm_band_stats(b.eng._ctx, int(self.mt), C.byref(pl), dp(out), 0))
        return out.reshape(self.F, 2)

    def planes3(self, b, xv, bv, ov):
        ch = 3 if bv.dim() - xv.dim() == 1 else 1
        return self.wm.plane_of(b.view(xv), 1), self.wm.plane_of(b.view(bv), ch), self.wm.plane_of(b.view(ov), ch)

    def c_embed(self, b, xv, bv, ov, ms):
        pin, pb, po = self.planes3(b, xv, bv, ov)
        a = np.full(self.F, np.nan, np.float32)
        m = np.ascontiguousarray(ms, np.float64)
        self.torch.cuda.synchronize()
        b.eng._chk(self.L.wm_band_embed(b.eng._ctx, int(self.mt), C.byref(pin), C.byref(pb), C.byref(po), dp(m), a.ctypes.data_as(C.POINTER(C.c_float)), 0))
        return a

    def c_detect(self, b, batch):
        pl = self.wm.plane_of(b.view(batch), 1)
        out = np.full(3 * self.F, np.nan)
        self.torch.cuda.synchronize()
        b.eng._chk(self.L.wm_band_detect_sums(b.eng._ctx, int(self.mt), C.byref(pl), dp(out), 0))
        return out.reshape(self.F, 3)

    # ---- the phases through the host-exchange calls ----
    def gram(self):
        def run():
            tb = [self.c_gram(b, self.xv) for b in self.bands]
            t1 = self.c_gram(self.e1, self.xv)
            tp = np.asarray(self.plain.gram_totals(self.xv)).reshape(self.F, 44)
            return tb, t1, tp
        return self.once("gram", run)

    def solve(self, of="x"):
        """E1's totals (of the input, or of the stitched y) to every context; not kept: each phase loads the coefficients it needs"""
        t1 = self.gram()[1] if of == "x" else self.detect()["t1"]
        return [self.c_solve(b, t1) for b in self.everyone()]

    def stats(self):
        def run():
            self.solve()
            return [self.c_stats(b, self.xv) for b in self.bands], self.c_stats(self.e1, self.xv)
        return self.once("stats", run)

    def max_sum(self):
        sb, s1 = self.stats()
        ms = np.empty((self.F, 2))
        for f in range(self.F):
            ms[f] = max(s[f, 0] for s in sb), sum(float(s[f, 1]) for s in sb)
        return ms

    def base_of(self, base):
        if base == "in":
            return self.xv
        if base == "grey":
            return self.gv
        def run():
            rgb = np.stack([np.stack([np.clip(self.f32(g) + 12.0 * (k - 1), 0, 255).astype(g.dtype) for k in range(3)]) for g in self.grey])
            return self.place(rgb)
        return self.once("rgb", run)

    def embed(self, base):
        """every band and E1 into a buffer of its own that is pre-filled with the sentinel; the same {mx, ss} to every context"""
        def run():
            bv = self.base_of(base)
            ms = self.max_sum()
            self.solve()
            outs, strengths = [], []
            for b in self.everyone():
                ov, whole = self.sentinel_like(bv)
                strengths.append(self.c_embed(b, self.xv, bv, ov, ms))
                self.torch.cuda.synchronize()
                outs.append(whole.cpu().numpy())
            sent = self.sentinel_like(bv)[1].cpu().numpy()
            y = np.empty_like(outs[-1])
            for b, o in zip(self.bands, outs):
                y[..., b.r0:b.r1, :] = o[..., b.r0:b.r1, :]
            return dict(outs=outs, a=strengths, sent=sent, y=np.ascontiguousarray(y[..., :self.cols]), base=bv.cpu().numpy())
        return self.once(("embed", base), run)

    def detect(self):
        """on the stitched y of the embed with the input as its base; a band's halo rows are its neighbours' owned rows"""
        def run():
            y = self.embed("in")["y"]
            yv = self.place(y)
            tb = [self.c_gram(b, yv) for b in self.bands]
            t1 = self.c_gram(self.e1, yv)
            res = dict(yv=yv, tb=tb, t1=t1)
            self.memo["detect"] = res          # (solve("y") reads it)
            res["status"] = self.solve("y")
            res["sums"] = [self.c_detect(b, yv) for b in self.bands]
            res["sums1"] = self.c_detect(self.e1, yv)
            res["plain"] = np.asarray(self.plain.detectWatermark(yv, self.mt), np.float32).reshape(self.F)
            total = sum(res["sums"])
            res["score"] = np.array([0.0 if res["status"][-1][f] != 0 else BM.corr_of(total[f]) for f in range(self.F)], np.float32)
            return res
        return self.once("detect", run)

    # ---- the same phases through wm_band_*_dev, the collectives emulated by tensor sums and concatenation ----
    def dev(self):
        def run():
            torch, L, F, mt = self.torch, self.L, self.F, int(self.mt)
            f64 = dict(dtype=torch.float64, device="cuda")
            vp = lambda t: C.c_void_p(t.data_ptr())
            ev = self.everyone()
            for b in ev:
                b.eng.set_stream_current()

            def gram_solve(batch):
                tots = []
                for b in self.bands:
                    t = torch.zeros(F * 44, **f64)
                    pl = self.wm.plane_of(b.view(batch), 1)
                    b.eng._chk(L.wm_band_gram_dev(b.eng._ctx, C.byref(pl), vp(t), 0))
                    tots.append(t)
                tot = torch.stack(tots).sum(0)                   # what the all-reduce leaves on every rank
                t1 = torch.zeros(F * 44, **f64)
                pl = self.wm.plane_of(self.e1.view(batch), 1)
                self.e1.eng._chk(L.wm_band_gram_dev(self.e1.eng._ctx, C.byref(pl), vp(t1), 0))
                # E1's totals to every context, as in the host-exchange phases: f32 sums added up in another order differ in the last
                # bits of f64, and the bits of y are compared
                for b in ev:
                    b.eng._chk(L.wm_band_solve_dev(b.eng._ctx, vp(t1), F, 0))
                return tot, t1

            tot, t1 = gram_solve(self.xv)
            parts = []
            for b in self.bands:
                ms = torch.zeros(F * 2, **f64)
                pl = self.wm.plane_of(b.view(self.xv), 1)
                b.eng._chk(L.wm_band_stats_dev(b.eng._ctx, mt, C.byref(pl), vp(ms), 0))
                parts.append(ms)
            gathered = torch.stack(parts).contiguous()           # what the all-gather leaves: [part][frame][2]
            assert gathered.shape == (len(self.bands), F * 2)
            y = torch.zeros((F, R, self.cols), dtype=self.xv.dtype, device="cuda")
            a = []
            for b in self.bands:
                ov, whole = self.sentinel_like(self.xv)
                ad = torch.zeros(F, dtype=torch.float32, device="cuda")
                pin, pb, po = self.planes3(b, self.xv, self.xv, ov)
                b.eng._chk(L.wm_band_embed_dev(b.eng._ctx, mt, C.byref(pin), C.byref(pb), C.byref(po), vp(gathered), len(self.bands), vp(ad), 0))
                y[:, b.r0:b.r1] = ov[:, b.r0:b.r1]
                a.append(ad)
            torch.cuda.synchronize()
            res = dict(tot=tot.cpu().numpy().reshape(F, 44), t1=t1.cpu().numpy().reshape(F, 44), y=y.cpu().numpy(), a=[t.cpu().numpy() for t in a])
            yv = self.place(res["y"])
            gram_solve(yv)
            sums = []
            for b in self.bands:
                sm = torch.zeros(F * 3, **f64)
                pl = self.wm.plane_of(b.view(yv), 1)
                b.eng._chk(L.wm_band_detect_sums_dev(b.eng._ctx, mt, C.byref(pl), vp(sm), 0))
                sums.append(sm)
            total = torch.stack(sums).sum(0)
            corr = []
            for b in self.bands:
                cd = torch.full((F,), float("nan"), dtype=torch.float32, device="cuda")
                b.eng._chk(L.wm_band_corr_dev(b.eng._ctx, vp(total), F, vp(cd), 0))
                corr.append(cd)
            torch.cuda.synchronize()
            res.update(sums=[t.cpu().numpy().reshape(F, 3) for t in sums], corr=[t.cpu().numpy() for t in corr])
            return res
        return self.once("dev", run)

    # ---- the CPU references ----
    def model_x(self, f):
        return self.once(("mx", f), lambda: BM.Frame(self.f32(self.xs[f]), self.W, self.p, self.omask))

    def model_y(self, f):
        return self.once(("my", f), lambda: BM.Frame(self.f32(self.embed("in")["y"][f]), self.W, self.p, self.omask))


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


# ---- the phases -----------------------------------------------------------------------------------------------------------------

def assert_sums(s, got, want, what):
    """Gram sums: u8 as integers, exactly; f32 at test_gpu_bands.py's bound"""
    if s.dtype == "u8":
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_allclose(got, want, rtol=TOL_EXACT_SUM, atol=0, err_msg=what)


def check_gram(s):
    tb, t1, tp = s.gram()
    assert_sums(s, sum(tb), t1, "the bands' totals summed against E1's")
    assert_sums(s, t1, tp, "E1's totals against the plain context's wm_gram")
    for b, t in zip(s.bands, tb):
        for f in range(s.F):
            assert_sums(s, t[f], BM.gram_sums(s.xs[f], b.r0, b.r1), f"band [{b.r0}, {b.r1}) frame {f} against band_model")


def check_solve(s):
    for st in s.solve():
        assert (st == 0).all(), st


def check_stats(s):
    sb, s1 = s.stats()
    for f in range(s.F):
        mx = max(t[f, 0] for t in sb)
        if s.mask == "ME":
            assert bits_equal(np.float64(mx), np.float64(s1[f, 0])), (f, mx, s1[f, 0])   # a maximum has no order
        else:
            assert all(t[f, 0] == 1.0 for t in sb) and s1[f, 0] == 1.0
        ss = sum(float(t[f, 1]) for t in sb)
        print(f"frame {f}: sum of the band sums {ss:.9e} E1 {s1[f, 1]:.9e}")
        assert ss == pytest.approx(s1[f, 1], rel=TOL_ENGINES_SS)
        for b, t in zip(s.bands, sb):
            mxo, sso = s.model_x(f).stats(b.r0, b.r1)
            got, want = t[f, 1] / t[f, 0] ** 2, sso / mxo ** 2
            print(f"  band [{b.r0}, {b.r1}): ss / mx^2 {got:.7e} model {want:.7e}")
            assert got == pytest.approx(want, rel=TOL_A), (f, b.r0, b.r1)


def check_embed(s, base):
    e = s.embed(base)
    outs, a, sent, bn = e["outs"], e["a"], e["sent"], e["base"]
    o1 = outs[-1]
    if s.dtype == "u8":
        assert (sent[..., :s.cols] != bn).all()                      # a stray store of the base would show at any pixel
    else:
        assert np.isnan(sent).all()
    assert all(bits_equal(x, a[-1]) for x in a), a                   # the strength: the same bits on every band and on E1
    assert np.isfinite(a[-1]).all()
    # E1 wrote every pixel and nothing of the pitch padding
    assert bits_equal(o1[..., s.cols:], sent[..., s.cols:]) and not np.isnan(s.f32(o1[..., :s.cols])).any()
    for b, o in zip(s.bands, outs):
        want = sent.copy()
        want[..., b.r0:b.r1, :s.cols] = o1[..., b.r0:b.r1, :s.cols]
        # the owned rows are E1's rows, every channel and frame; every other row and the pitch padding is still the sentinel
        assert bits_equal(o[..., b.r0:b.r1, :s.cols], o1[..., b.r0:b.r1, :s.cols]), (b.r0, b.r1)
        assert bits_equal(o, want), (b.r0, b.r1)
    y = e["y"]
    for f in range(s.F):
        x = s.xs[f]
        if s.dtype == "u8" and base == "in":
            so, yo, ao = O.embed_u8(x, s.W, p=s.p, mask=s.omask)
            assert u8_rule(y[f], yo), f
        elif s.dtype == "u8":
            so, yo, ao = O.embed(s.f32(x), s.f32(bn[f]), s.W, p=s.p, mask=s.omask)
            assert u8_rule(y[f], np.clip(yo, 0.0, 255.0).astype(np.uint8)), f
        else:
            so, yo, ao = O.embed(x, bn[f], s.W, p=s.p, mask=s.omask)
            print(f"frame {f}: worst pixel {np.abs(y[f] - yo).max():.2e}")
            np.testing.assert_allclose(y[f], yo, rtol=0, atol=TOL_Y)
        assert so == 0 and a[-1][f] == pytest.approx(ao, rel=TOL_A), (f, a[-1][f], ao)
    assert not np.array_equal(y, bn)


def check_detect(s):
    d = s.detect()
    for st in d["status"]:
        assert (st == 0).all(), st
    assert_sums(s, sum(d["tb"]), d["t1"], "the bands' totals of y summed against E1's")
    y = s.embed("in")["y"]
    for f in range(s.F):
        for b, sm in zip(s.bands, d["sums"]):
            dot, nu, nw = s.model_y(f).detect_sums(b.r0, b.r1)
            print(f"frame {f} band [{b.r0}, {b.r1}): {sm[f]} model {dot, nu, nw}")
            assert sm[f, 1] == pytest.approx(nu, rel=TOL_SQUARES) and sm[f, 2] == pytest.approx(nw, rel=TOL_SQUARES), (f, b.r0, b.r1)
            assert abs(sm[f, 0] - dot) <= TOL_CORR * np.sqrt(nu * nw), (f, b.r0, b.r1)
        ref = (O.detect_u8 if s.dtype == "u8" else O.detect)(y[f], s.W, p=s.p, mask=s.omask)[1]
        print(f"frame {f}: score {d['score'][f]:.7f} plain {d['plain'][f]:.7f} oracle {ref:.7f}")
        assert abs(float(d["score"][f]) - float(d["plain"][f])) <= TOL_ENGINES_CORR
        assert abs(float(d["score"][f]) - ref) <= TOL_CORR


def check_dev(s):
    """wm_band_*_dev: y and a as the host-exchange phases give them, bit for bit; a and corr the same on every band"""
    v = s.dev()
    h = s.embed("in")
    tb, t1, tp = s.gram()
    assert_sums(s, v["tot"], t1, "the device totals summed against E1's host totals")
    assert bits_equal(v["t1"], t1)
    assert bits_equal(v["y"], h["y"])
    assert all(bits_equal(a, h["a"][-1]) for a in v["a"]), (v["a"], h["a"][-1])
    assert all(bits_equal(c, v["corr"][0]) for c in v["corr"]), v["corr"]
    d = s.detect()
    for b, sd, sh in zip(s.bands, v["sums"], d["sums"]):
        assert bits_equal(sd, sh), (b.r0, b.r1, sd, sh)                # the same sweep on the same planes
    print(v["corr"][0], d["score"])
    assert np.abs(v["corr"][0].astype(np.float64) - d["score"].astype(np.float64)).max() <= TOL_ENGINES_CORR


def check_flat(s):
    """frame FLAT_FRAME of five constant: its status alone is non-zero, its owned rows are the base, its strength on the device
    path alone is NaN, its score alone is 0.0; the other four frames are those of the run without the flat frame, bit for bit"""
    setting = ((s.route, s.cols, s.dtype, s.pitch), (s.mask, s.p), s.F, s.split)
    t = Setting(s.wm, s.torch, setting, flat=True)
    try:
        others = [f for f in range(s.F) if f != FLAT_FRAME]
        for st in t.solve():
            assert st[FLAT_FRAME] != 0 and (st[others] == 0).all(), st
        for base in ("in", "grey"):
            e, n = t.embed(base), s.embed(base)
            print("strengths of wm_band_embed:", e["a"][-1])
            assert bits_equal(e["a"][-1][others], n["a"][-1][others])
            assert all(bits_equal(a, e["a"][-1]) for a in e["a"])
            assert bits_equal(e["y"][others], n["y"][others])
            assert bits_equal(e["y"][FLAT_FRAME], e["base"][FLAT_FRAME][..., :s.cols])
            for b, o in zip(t.everyone(), e["outs"]):
                want = e["sent"].copy()
                want[..., b.r0:b.r1, :s.cols] = e["outs"][-1][..., b.r0:b.r1, :s.cols]
                assert bits_equal(o, want), (b.r0, b.r1)
        d, dn = t.detect(), s.detect()
        for st in d["status"]:
            assert st[FLAT_FRAME] != 0 and (st[others] == 0).all(), st
        assert d["score"][FLAT_FRAME] == 0.0 and (d["score"][others] != 0.0).all()
        assert bits_equal(d["score"][others], dn["score"][others])
        v, vn = t.dev(), s.dev()
        for a in v["a"]:
            assert np.isnan(a[FLAT_FRAME]) and bits_equal(a[others], vn["a"][0][others]), a
        assert bits_equal(v["y"], t.embed("in")["y"])
        for c in v["corr"]:
            assert c[FLAT_FRAME] == 0.0 and bits_equal(c[others], vn["corr"][0][others]) and (c[others] != 0.0).all(), c
    finally:
        t.close()


def check_refused(s):
    """wm_band_configure refuses one band of the split, by the halo rule; the others it takes"""
    k = refused_band(s.split, s.p)
    need = halo(s.p)
    assert [r[0] for r in s.refusals] == [k], s.refusals
    assert f"an interior side needs {need} halo rows" in s.refusals[0][1], s.refusals
    r0, r1 = split_rows(s.split, s.p)[k]
    assert 0 < R - r1 < need                       # the rows below the band's own, down to the image's last: fewer than the rule wants
    assert not BM.halo_rule(R - max(0, r0 - need), r0 - max(0, r0 - need), r1 - max(0, r0 - need), s.p)
    if s.split == "one-row":
        # the bottom band alone: the border rows 38, 39, 40 of the window positions, as band_model has them
        b = s.bands[-1]
        assert (b.r0, b.r1) == (R - 1, R) and b.g1 - b.g0 >= 4
        tot = s.c_gram(b, s.xv)
        for f in range(s.F):
            assert_sums(s, tot[f], BM.gram_sums(s.xs[f], b.r0, b.r1), f"frame {f}")


CHECKS = {"gram": check_gram, "solve": check_solve, "stats": check_stats, "embed-in": lambda s: check_embed(s, "in"),
          "embed-grey": lambda s: check_embed(s, "grey"), "embed-rgb": lambda s: check_embed(s, "rgb"), "detect": check_detect,
          "dev": check_dev, "flat": check_flat, "refused": check_refused}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_band_route(setting_of, case):
    setting, phase = case
    CHECKS[phase](setting_of(setting))


def test_the_case_list_is_complete():
    """every route x window x frame count with the even and the ragged split (the ragged-h one where ragged is refused), the one-row
    split on its two routes; every phase of a split that wm_band_configure takes, one refusal case of one that it does not, the
    3-channel base on the overlap-f32 route, one flat-frame case per route; none twice"""
    import importlib
    bands = importlib.import_module("watermarking-gpu_amd.bands")
    assert EVEN == [bands.band_rows(R, r, 3) for r in range(3)] and all(halo(p) == bands.halo_rows(p) for _, p in WINDOWS)
    ids = [case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    nrw = len(ROUTES) * len(WINDOWS) * len(FRAMES)
    full = [s for s in SETTINGS if refused_band(s[3], s[1][1]) is None]
    refused = [s for s in SETTINGS if refused_band(s[3], s[1][1]) is not None]
    assert len(full) == 2 * nrw == 140                                  # even + (ragged or ragged-h)
    assert len(refused) == len(ROUTES) * 3 * len(FRAMES) + 2 * len(WINDOWS) * len(FRAMES) == 62
    for rt in ROUTES:
        for win in WINDOWS:
            for F in FRAMES:
                have = {ph for (s, ph) in CASES if s[:3] == (rt, win, F) and s[3] == "even"}
                assert have == set(PHASES) - ({"embed-rgb"} if rt != ROUTES[0] else set()) | ({"flat"} if (win[0], F) == ("ME", 5) else set())
                rag = "ragged" if win[1] == 3 else "ragged-h"
                assert {ph for (s, ph) in CASES if s == (rt, win, F, rag)} == have - {"flat"}
    assert len([c for c in CASES if c[1] == "flat"]) == len(ROUTES)
    assert len(ids) == 140 * 7 + 2 * len(WINDOWS) * len(FRAMES) + 62 + len(ROUTES) == 1069
