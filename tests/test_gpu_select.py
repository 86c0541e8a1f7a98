"""wm_embed_select / wm_detect_select: frame f of a batch marked, or scored, with key key_of_frame[f] of a bank (k_me_stats_sel,
k_nvf_stats_sel, k_embed_sel, k_detect_sel).

The contract is bit equality with the per-key contexts: for every distinct key of the table a context whose W is that key
(Watermark.generated, fused kernels off, max_frames = F) runs wm_embed / wm_detect on the WHOLE batch -- the same planes, so the same
strips, segments and frame quads -- and frame f is taken from the run of key table[f].  Output bytes, strengths and scores are
compared as integers.  Then parity with the CPU oracle, every input kind, the schedule round trip, special frames, the lifetime of
the table, hand-over hygiene, the refusals and determinism.

Shapes: (5, 7) generic tiny; (64, 256) one aligned strip; (270, 480) overlapped strips; (271, 483) overlapped strips + one generic
strip.  F = 1, 3: no frame quad; F = 5: the quad mapping with a short last quad."""
import ctypes as C

import numpy as np
import pytest

import hard_frames as HF
import layouts as LY
import oracle_lib as O
import select_model as SM
from synth import synth_frame

pytestmark = pytest.mark.gpu

ME, NVF = 0, 1
TOL_Y, TOL_A, TOL_CORR = 1e-3, 1e-4, 1e-5
SEEDS = [2000, 2031, 2062]
TABLE = [2, 0, 2, 1, 0]  # repeats keys, not monotone
SHAPES = [(5, 7), (64, 256), (270, 480), (271, 483)]
MASKS = [(ME, 3), (NVF, 3), (NVF, 5), (NVF, 9)]
F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def frames_of(R, Cc, F, dtype, first=1):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def u32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    """two arrays / tensors hold the same bytes"""
    return np.array_equal(LY.raw(a), LY.raw(b))


def make_base(torch, xs, kind):
    """xs: [F, R, C] device tensor.  'in' the input itself, 'grey' another grey plane, 'rgb' [F, 3, R, C]"""
    if kind == "in":
        return xs
    if kind == "grey":
        return (xs.flip(-1) if xs.dtype == torch.uint8 else xs.flip(-1) * 0.5 + 20.0).contiguous()
    return torch.stack([xs, xs.flip(-2), xs.flip(-1)], 1).contiguous()


def host_plane(wm, a, channels=1):
    F, R, Cc = a.shape[0], a.shape[-2], a.shape[-1]
    return wm.wm_plane(a.ctypes.data, R, Cc, channels, wm.WM_U8 if a.dtype == np.uint8 else wm.WM_F32, wm.WM_MEM_HOST, F, Cc, R * Cc, channels * R * Cc)


def slot_out_plane(wm, R, Cc, F, u8):
    return wm.wm_plane(None, R, Cc, 1, wm.WM_U8 if u8 else wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)


def key_engines(wm, R, Cc, p, F, table, seeds=SEEDS):
    """{key: a context whose W is that key, on the batched sweeps} for the distinct keys of the table"""
    out = {}
    for k in sorted(set(int(t) for t in table)):
        e = wm.Watermark.generated(R, Cc, seeds[k], p, 40.0, max_frames=F)
        e.set_fused(False)
        out[k] = e
    return out


def reference_embed(wm, torch, engines, xs, base, outs, mask, table):
    """wm_embed of the whole batch on every key's context into outs[k] (tensors or planes shaped like the caller's output), frame f of
    the result taken from the run of key table[f]: (a float32 [F], status int32 [F]); the caller picks the frames of outs"""
    F = len(table)
    a, st = np.full(F, np.nan, np.float32), np.zeros(F, np.int32)
    torch.cuda.synchronize()
    for k, e in engines.items():
        ak, sk = np.full(F, np.nan, np.float32), np.zeros(F, np.int32)
        e.embed_async(xs, base, outs[k], wm.MASK_TYPE(mask), wm.WM_SLOT_SYNC, ak.ctypes.data_as(F32P), sk.ctypes.data_as(I32P))
        for f in range(F):
            if table[f] == k:
                a[f], st[f] = ak[f], sk[f]
    return a, st


def reference_detect(wm, torch, engines, ys, mask, table):
    """wm_detect of the whole batch on every key's context, frame f from the run of key table[f]: float32 [F]"""
    F = len(table)
    c = np.zeros(F, np.float32)
    torch.cuda.synchronize()
    for k, e in engines.items():
        ck = np.zeros(F, np.float32)
        e.detect_async(ys, wm.MASK_TYPE(mask), wm.WM_SLOT_SYNC, ck.ctypes.data_as(F32P))
        for f in range(F):
            if table[f] == k:
                c[f] = ck[f]
    return c


def reference(wm, torch, R, Cc, p, mask, xs, base, table, seeds=SEEDS):
    """case 1's reference for dense device planes: (y like base, a [F], status [F], corr [F] of y)"""
    F = len(table)
    engines = key_engines(wm, R, Cc, p, F, table, seeds)
    outs = {k: torch.empty_like(base) for k in engines}
    a, st = reference_embed(wm, torch, engines, xs, base, outs, mask, table)
    y = torch.stack([outs[int(table[f])][f] for f in range(F)])
    grey = y if y.dim() == 3 else None
    corr = reference_detect(wm, torch, engines, grey, mask, table) if grey is not None else None
    for e in engines.values():
        e.close()
    return y, a, st, corr


def select_engine(wm, R, Cc, p, F, nslots=2):
    """the engine of the calls under test: its own W is all zero, so a result that used it would be base / NaN"""
    return wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0, nslots=nslots, max_frames=F)


def run_select(wm, torch, eng, keys, xs, base, mask, table, out=None):
    """wm_embed_select, then wm_detect_select of its output: (y, a float32 [F] NaN where untouched, status, corr float32 [F])"""
    F = len(table)
    y = torch.empty_like(base) if out is None else out
    a, st = np.full(F, np.nan, np.float32), np.full(F, -5, np.int32)
    torch.cuda.synchronize()
    eng.embed_select_async(xs, base, y, keys, table, wm.MASK_TYPE(mask), 0, a, st)
    eng.sync(0)
    corr = None
    if y.dim() == 3:
        corr = np.full(F, 9.0, np.float32)
        eng.detect_select_async(y, keys, table, wm.MASK_TYPE(mask), 0, corr)
        eng.sync(0)
    return y, a, st, corr


# ---- 1. bit equality with the per-key contexts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 5])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("mask,p", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_equal_to_per_key_contexts(wm, torch_cuda, shape, mask, p, dtype, F):
    torch = torch_cuda
    R, Cc = shape
    table = TABLE[:F]
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype)).cuda()
    yr, ar, sr, cr = reference(wm, torch, R, Cc, p, mask, xs, xs, table)
    eng = select_engine(wm, R, Cc, p, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xs, xs, mask, table)
    assert np.array_equal(st, sr) and np.all(st == 0)
    assert same_bits(y, yr), (shape, mask, p, dtype, F)
    assert np.array_equal(u32(a), u32(ar)), (a, ar)
    assert np.array_equal(u32(c), u32(cr)), (c, cr)
    # the synchronous Python surface gives the same
    y2, a2 = eng.makeWatermarkSelect(xs, xs, keys, table, wm.MASK_TYPE(mask))
    c2 = eng.detectSelect(y2, keys, table, wm.MASK_TYPE(mask))
    assert same_bits(y2, yr) and np.array_equal(u32(a2), u32(ar)) and np.array_equal(u32(c2), u32(cr))
    eng.close()
    keys.close()


def test_bit_equal_1080p(wm, torch_cuda):
    """1078 x 1918, F = 5, ME f32: aligned strips with a generic remainder in the stats and embed sweeps, overlapped strips and one
    generic strip in the detector, several segments per strip, two frame quads"""
    torch = torch_cuda
    R, Cc, F = 1078, 1918, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    yr, ar, sr, cr = reference(wm, torch, R, Cc, 3, ME, xs, xs, TABLE)
    eng = select_engine(wm, R, Cc, 3, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xs, xs, ME, TABLE)
    assert np.all(st == 0) and same_bits(y, yr) and np.array_equal(u32(a), u32(ar)) and np.array_equal(u32(c), u32(cr))
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask,p,dtype", [(ME, 3, "f32"), (NVF, 5, "u8")])
def test_all_equal_table_is_wm_embed_and_wm_detect(wm, torch_cuda, mask, p, dtype):
    torch = torch_cuda
    R, Cc, F = 270, 480, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype)).cuda()
    one = wm.Watermark.generated(R, Cc, SEEDS[1], p, 40.0, max_frames=F)
    one.set_fused(False)
    yr, ar = one.makeWatermark(xs, xs, wm.MASK_TYPE(mask))
    cr = one.detectWatermark(yr, wm.MASK_TYPE(mask))
    eng = select_engine(wm, R, Cc, p, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xs, xs, mask, [1] * F)
    assert same_bits(y, yr) and np.array_equal(u32(a), u32(ar)) and np.array_equal(u32(c), u32(cr))
    for obj in (one, eng, keys):
        obj.close()


# ---- 2. oracle parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("mask", [ME, NVF])
@pytest.mark.parametrize("shape", [(64, 256), (270, 480)])
def test_oracle_parity(wm, torch_cuda, shape, mask, dtype):
    """the project's bounds: y <= 1e-3 abs, a <= 1e-4 rel, score <= 1e-5.  A u8 output is y truncated to 8 bits: a deviation of 1e-3
    in front of the truncation moves a code by at most one level and only where y lies within 1e-3 of an integer -- the project's u8
    rule, at most one level on at most 1e-3 of the pixels (tests/test_gpu_launch_routes.py u8_rule)"""
    torch = torch_cuda
    R, Cc = shape
    F = 3
    table = TABLE[:F]
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    Ws = [keys.plane(k) for k in range(len(SEEDS))]
    x = frames_of(R, Cc, F, dtype, first=4)
    xs = torch.from_numpy(x).cuda()
    eng = select_engine(wm, R, Cc, 3, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xs, xs, mask, table)
    yh = y.cpu().numpy()
    for f in range(F):
        W = Ws[table[f]]
        if dtype == "u8":
            so, yo, ao = O.embed_u8(x[f], W, mask=mask)
            d = np.abs(yh[f].astype(int) - yo.astype(int))
            print(f"frame {f}: u8 levels off {int(d.max())}, share {(d != 0).mean():.2e}")
            assert d.max() <= 1 and (d != 0).mean() <= 1e-3
            co = O.detect_u8(yh[f], W, mask=mask)[1]
        else:
            so, yo, ao = O.embed(x[f], x[f], W, mask=mask)
            print(f"frame {f}: max |y - oracle| {float(np.abs(yh[f] - yo).max()):.2e}")
            assert float(np.abs(yh[f] - yo).max()) <= TOL_Y
            co = O.detect(yh[f], W, mask=mask)[1]
        print(f"frame {f}: a {a[f]:.6f} oracle {ao:.6f}  score {c[f]:.7f} oracle {co:.7f}")
        assert so == 0 and st[f] == 0 and abs(float(a[f]) - ao) <= TOL_A * abs(ao)
        assert abs(float(c[f]) - co) <= TOL_CORR
    eng.close()
    keys.close()


# ---- 3. inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,p,dtype", [(ME, 3, "f32"), (NVF, 3, "u8")])
@pytest.mark.parametrize("base_kind", ["rgb", "grey"])
def test_rgb_and_grey_bases(wm, torch_cuda, base_kind, mask, p, dtype):
    torch = torch_cuda
    R, Cc, F = 271, 483, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype)).cuda()
    base = make_base(torch, xs, base_kind)
    yr, ar, sr, cr = reference(wm, torch, R, Cc, p, mask, xs, base, TABLE)
    eng = select_engine(wm, R, Cc, p, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xs, base, mask, TABLE)
    assert tuple(y.shape) == tuple(base.shape) and same_bits(y, yr) and np.array_equal(u32(a), u32(ar))
    if base_kind == "grey":
        assert np.array_equal(u32(c), u32(cr))
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask,p,dtype", [(ME, 3, "f32"), (NVF, 5, "u8")])
def test_in_place(wm, torch_cuda, mask, p, dtype):
    """input, base and output are one plane: the stencil reads the snapshot"""
    torch = torch_cuda
    R, Cc, F = 270, 480, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype)).cuda()
    yr, ar, sr, cr = reference(wm, torch, R, Cc, p, mask, xs, xs, TABLE)
    eng = select_engine(wm, R, Cc, p, F)
    buf = xs.clone()
    y, a, st, c = run_select(wm, torch, eng, keys, buf, buf, mask, TABLE, out=buf)
    assert same_bits(buf, yr) and np.array_equal(u32(a), u32(ar)) and np.array_equal(u32(c), u32(cr))
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask,p,dtype", [(ME, 3, "f32"), (NVF, 3, "u8")])
def test_host_planes_and_slot_output(wm, torch_cuda, mask, p, dtype):
    """WM_MEM_HOST in and out, then wm_detect_select on WM_MEM_SLOT_OUT: the reference runs on the same host planes and slot output"""
    torch = torch_cuda
    R, Cc, F = 271, 483, 5
    u8 = dtype == "u8"
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    hx = frames_of(R, Cc, F, dtype)
    pin = host_plane(wm, hx)
    ps = slot_out_plane(wm, R, Cc, F, u8)
    engines = key_engines(wm, R, Cc, p, F, TABLE)
    houts = {k: np.zeros_like(hx) for k in engines}
    ar, sr = reference_embed(wm, torch, engines, pin, pin, {k: host_plane(wm, v) for k, v in houts.items()}, mask, TABLE)
    cr = reference_detect(wm, torch, engines, ps, mask, TABLE)  # (every context's own slot output: its whole batch with its key)
    yr = np.stack([houts[TABLE[f]][f] for f in range(F)])
    eng = select_engine(wm, R, Cc, p, F)
    hy = np.zeros_like(hx)
    a, st, c = np.full(F, np.nan, np.float32), np.zeros(F, np.int32), np.zeros(F, np.float32)
    eng.embed_select_async(pin, pin, host_plane(wm, hy), keys, TABLE, wm.MASK_TYPE(mask), 0, a, st)
    eng.detect_select_async(ps, keys, TABLE, wm.MASK_TYPE(mask), 0, c)
    assert eng.sync(0) == wm.WM_OK
    assert same_bits(hy, yr) and np.array_equal(u32(a), u32(ar))
    # frame f of the slot output holds the same pixels in both runs, the batch around it differs only in the other frames
    assert np.array_equal(u32(c), u32(cr)), (c, cr)
    for e in engines.values():
        e.close()
    eng.close()
    keys.close()


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("lin,lout", [("pitched", "gapped"), ("odd", "odd"), ("every_other", "odd_frames_only")])
def test_pitched_and_offset_planes(wm, torch_cuda, lin, lout, dtype):
    """planes whose offset, pitch and frame stride differ (tests/layouts.py): the right pixels in the right place, not one byte
    outside the plane, and the bits of the per-key contexts on the same planes"""
    torch = torch_cuda
    R, Cc, F = 270, 480, 5
    mask, p = (ME, 3) if dtype == "f32" else (NVF, 3)
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    x = frames_of(R, Cc, F, dtype)
    poison = LY.POISON[dtype][0]
    li, lo = LY.make(lin, R, Cc, 1, F), LY.make(lout, R, Cc, 1, F)
    _, xin = LY.place(torch, x, li, poison)
    engines = key_engines(wm, R, Cc, p, F, TABLE)
    routs = {k: LY.place(torch, np.zeros_like(x), lo, poison) for k in engines}
    ar, sr = reference_embed(wm, torch, engines, xin, xin, {k: v[1] for k, v in routs.items()}, mask, TABLE)
    yr = np.stack([routs[TABLE[f]][1][f].cpu().numpy() for f in range(F)])
    obuf, oview = LY.place(torch, np.zeros_like(x), lo, poison)
    cr = None
    eng = select_engine(wm, R, Cc, p, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xin, xin, mask, TABLE, out=oview)
    assert np.array_equal(LY.raw(obuf), LY.raw(LY.expect(yr, lo, poison))), (lin, lout, dtype)
    assert np.array_equal(u32(a), u32(ar))
    # the detector on the pitched output against the per-key contexts on the same plane
    cr = reference_detect(wm, torch, engines, oview, mask, TABLE)
    assert np.array_equal(u32(c), u32(cr)), (c, cr)
    for e in engines.values():
        e.close()
    eng.close()
    keys.close()


# ---- 4. schedule round trip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [ME, NVF])
def test_schedule_round_trip(wm, torch_cuda, mask):
    """270 x 480, psnr 40, F = 8, K = 4, the table from key_schedule: every score under the right schedule and under the schedule
    rotated by one key agrees with the oracle's to 1e-5, and the weakest right score is more than 4 times the largest |wrong| one
    (test_select_model.py shows the oracle alone has about 30 between them, under ME and under NVF)"""
    torch = torch_cuda
    xs, Ws, table, rotated = SM.round_trip_case()
    F, R, Cc = xs.shape
    K = len(Ws)
    assert np.array_equal(wm.Watermark.key_schedule(K, 0x5E1EC7, 1000, F), table)
    keys = wm.KeySet(R, Cc, K)
    for k in range(K):
        keys.set(k, Ws[k])
    eng = select_engine(wm, R, Cc, 3, F)
    xt = torch.from_numpy(xs).cuda()
    y, a = eng.makeWatermarkSelect(xt, xt, keys, table, wm.MASK_TYPE(mask))
    right = np.array(eng.detectSelect(y, keys, table, wm.MASK_TYPE(mask)))
    wrong = np.array(eng.detectSelect(y, keys, rotated, wm.MASK_TYPE(mask)))
    yh = y.cpu().numpy()
    for f in range(F):
        ro = O.detect(yh[f], Ws[table[f]], mask=mask)[1]
        wo = O.detect(yh[f], Ws[rotated[f]], mask=mask)[1]
        print(f"frame {f} key {table[f]}: {right[f]:.7f} oracle {ro:.7f}; key {rotated[f]}: {wrong[f]:.7f} oracle {wo:.7f}")
        assert abs(right[f] - ro) <= TOL_CORR and abs(abs(wrong[f]) - abs(wo)) <= TOL_CORR
    assert right.min() > 4 * np.abs(wrong).max(), (right, wrong)
    eng.close()
    keys.close()


# ---- 5. special frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramp", "stripes"])
def test_unsolvable_frame_in_the_middle(wm, torch_cuda, kind):
    torch = torch_cuda
    R, Cc, F = 270, 480, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    x = frames_of(R, Cc, F, "f32")
    x[2] = HF.singular(kind, R, Cc)
    xs = torch.from_numpy(x).cuda()
    base = make_base(torch, xs, "grey")
    yr, ar, sr, cr = reference(wm, torch, R, Cc, 3, ME, xs, base, TABLE)
    assert list(sr) == [0, 0, 1, 0, 0]
    eng = select_engine(wm, R, Cc, 3, F)
    out = torch.full_like(base, -1.0)
    a, st = np.full(F, 7.0, np.float32), np.full(F, -5, np.int32)
    torch.cuda.synchronize()
    eng.embed_select_async(xs, base, out, keys, TABLE, wm.MASK_TYPE.ME, 0, a, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    assert list(st) == [0, 0, 1, 0, 0]
    assert same_bits(out[2], base[2]) and a[2] == 7.0  # out == base, `a` untouched
    assert same_bits(out, yr)
    ok = [0, 1, 3, 4]
    assert np.array_equal(u32(a[ok]), u32(ar[ok]))
    # the detector on the batch with the singular frame in it
    c, sc = np.full(F, 9.0, np.float32), np.full(F, -5, np.int32)
    eng.detect_select_async(xs, keys, TABLE, wm.MASK_TYPE.ME, 0, c, sc)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    engines = key_engines(wm, R, Cc, 3, F, TABLE)
    cx = reference_detect(wm, torch, engines, xs, ME, TABLE)
    assert list(sc) == [0, 0, 1, 0, 0] and c[2] == 0.0 and np.array_equal(u32(c), u32(cx))
    for e in engines.values():
        e.close()
    eng.close()
    keys.close()


@pytest.mark.parametrize("mask", [ME, NVF])
def test_zero_key(wm, torch_cuda, mask):
    """key 1 of the bank is left all zero: its frame has a = +inf and out == base, the detector scores it NaN with status OK, and
    the other frames are those of the per-key contexts"""
    torch = torch_cuda
    R, Cc, F = 270, 480, 5
    keys = wm.KeySet(R, Cc, 3)
    for k in (0, 2):
        keys.set(k, wm.Watermark.generated(R, Cc, SEEDS[k], 3, 40.0).watermark())
    assert not keys.plane(1).any()
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    base = make_base(torch, xs, "grey")
    table = TABLE  # frame 3 takes key 1
    others = [0, 1, 2, 4]
    engines = key_engines(wm, R, Cc, 3, F, [TABLE[f] for f in others])
    outs = {k: torch.empty_like(base) for k in engines}
    tab_ref = [t if t != 1 else -1 for t in table]
    ar, sr = reference_embed(wm, torch, engines, xs, base, outs, mask, tab_ref)
    eng = select_engine(wm, R, Cc, 3, F)
    y, a, st, c = run_select(wm, torch, eng, keys, xs, base, mask, table)
    assert np.all(st == 0) and np.isposinf(a[3]) and same_bits(y[3], base[3])
    for f in others:
        assert same_bits(y[f], outs[table[f]][f]) and u32(a[f]) == u32(ar[f]), f
    assert np.isnan(c[3]) and not np.isnan(c[others]).any()
    # (the other frames' scores: the per-key contexts on the same batch)
    cr = reference_detect(wm, torch, engines, y, mask, tab_ref)
    assert np.array_equal(u32(c[others]), u32(cr[others]))
    for e in engines.values():
        e.close()
    eng.close()
    keys.close()


# ---- 6. table lifetime -----------------------------------------------------------------------------------------------------------
def test_table_is_copied_at_call_time(wm, torch_cuda):
    """the table is overwritten after the async call and before sync; two un-synced calls with different tables share a slot: the
    results are those of the tables as they were at call time"""
    torch = torch_cuda
    R, Cc, F = 270, 480, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    t1, t2 = list(TABLE), [1, 1, 0, 2, 2]
    y1r, a1r, _, c1r = reference(wm, torch, R, Cc, 3, ME, xs, xs, t1)
    y2r, a2r, _, c2r = reference(wm, torch, R, Cc, 3, ME, xs, xs, t2)
    eng = select_engine(wm, R, Cc, 3, F)
    L = wm.lib()
    tab = np.array(t1, np.int32)
    ptab = tab.ctypes.data_as(C.POINTER(C.c_int32))
    y1, y2 = torch.empty_like(xs), torch.empty_like(xs)
    a1, a2 = np.zeros(F, np.float32), np.zeros(F, np.float32)
    c1, c2 = np.zeros(F, np.float32), np.zeros(F, np.float32)
    px, p1, p2 = wm.plane_of(xs, 1), wm.plane_of(y1, 1), wm.plane_of(y2, 1)
    mt = int(wm.MASK_TYPE.ME)
    torch.cuda.synchronize()
    assert L.wm_embed_select(eng._ctx, mt, C.byref(px), C.byref(px), C.byref(p1), keys.handle, ptab, a1.ctypes.data_as(F32P), None, 0) == wm.WM_OK
    assert L.wm_detect_select(eng._ctx, mt, C.byref(p1), keys.handle, ptab, c1.ctypes.data_as(F32P), None, 0) == wm.WM_OK
    tab[:] = t2  # the caller's array changes while both calls are queued
    assert L.wm_embed_select(eng._ctx, mt, C.byref(px), C.byref(px), C.byref(p2), keys.handle, ptab, a2.ctypes.data_as(F32P), None, 0) == wm.WM_OK
    assert L.wm_detect_select(eng._ctx, mt, C.byref(p2), keys.handle, ptab, c2.ctypes.data_as(F32P), None, 0) == wm.WM_OK
    tab[:] = 0
    assert eng.sync(0) == wm.WM_OK
    assert same_bits(y1, y1r) and np.array_equal(u32(a1), u32(a1r)) and np.array_equal(u32(c1), u32(c1r))
    assert same_bits(y2, y2r) and np.array_equal(u32(a2), u32(a2r)) and np.array_equal(u32(c2), u32(c2r))
    eng.close()
    keys.close()


# ---- 7. hand-over hygiene --------------------------------------------------------------------------------------------------------
def test_no_handover_out_of_embed_select(wm, torch_cuda):
    """wm_embed (F = 4, ME f32) into plane P leaves its sums for a checked hand-over; wm_embed_select then overwrites P; wm_detect(P)
    must score the plane as it now is -- the per-key reference's bits -- and must not trust the old sums"""
    torch = torch_cuda
    R, Cc, F = 270, 480, 4
    table = TABLE[:F]
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    yr, ar, sr, _ = reference(wm, torch, R, Cc, 3, ME, xs, xs, table)
    eng = wm.Watermark.generated(R, Cc, SEEDS[0], 3, 40.0, nslots=1, max_frames=F)
    eng.set_fused(False)
    eng.set_checked_handover(True)
    plain = wm.Watermark.generated(R, Cc, SEEDS[0], 3, 40.0, nslots=1, max_frames=F)
    plain.set_fused(False)
    plain.set_checked_handover(False)
    want = np.array(plain.detectWatermark(yr, wm.MASK_TYPE.ME), np.float32)  # the engine's own W against the select output
    P = torch.empty_like(xs)
    a0, a1, c = np.zeros(F, np.float32), np.zeros(F, np.float32), np.zeros(F, np.float32)
    torch.cuda.synchronize()
    trusted0 = eng.checked_handover_counts()[0]
    eng.embed_async(xs, xs, P, wm.MASK_TYPE.ME, 0, a0.ctypes.data_as(F32P), None)
    eng.embed_select_async(xs, xs, P, keys, table, wm.MASK_TYPE.ME, 0, a1)
    eng.detect_async(P, wm.MASK_TYPE.ME, 0, c.ctypes.data_as(F32P))
    assert eng.sync(0) == wm.WM_OK
    assert same_bits(P, yr) and np.array_equal(u32(a1), u32(ar))
    assert np.array_equal(u32(c), u32(want)), (c, want)
    assert eng.checked_handover_counts()[0] == trusted0
    # ... and WM_MEM_SLOT_OUT names the select output
    c2 = np.zeros(F, np.float32)
    eng.detect_async(slot_out_plane(wm, R, Cc, F, False), wm.MASK_TYPE.ME, 0, c2.ctypes.data_as(F32P))
    assert eng.sync(0) == wm.WM_OK and np.array_equal(u32(c2), u32(want))
    for obj in (plain, eng, keys):
        obj.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_refusals(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc, F = 64, 256, 3
    bad = wm.WM_ERR_BAD_ARG
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    other = wm.KeySet(R, Cc + 4, 3)
    eng = select_engine(wm, R, Cc, 3, F)
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    big = torch.from_numpy(frames_of(R, Cc, F + 1, "f32")).cuda()
    y = torch.empty_like(xs)
    px, py, pbig = wm.plane_of(xs, 1), wm.plane_of(y, 1), wm.plane_of(big, 1)
    a, c = np.zeros(F + 1, np.float32), np.zeros(F + 1, np.float32)
    pa, pc = a.ctypes.data_as(F32P), c.ctypes.data_as(F32P)
    mt = int(wm.MASK_TYPE.ME)
    tab = lambda t: np.array(t, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    good = np.array(TABLE[:F], np.int32)
    pg = good.ctypes.data_as(C.POINTER(C.c_int32))
    torch.cuda.synchronize()

    def embed(ctx=eng._ctx, pin=px, pout=py, k=keys.handle, t=pg, slot=0, mask=mt):
        return L.wm_embed_select(ctx, mask, C.byref(pin) if pin else None, C.byref(pin) if pin else None, C.byref(pout) if pout else None, k, t, pa, None, slot)

    def detect(ctx=eng._ctx, pimg=px, k=keys.handle, t=pg, slot=0, mask=mt, out=pc):
        return L.wm_detect_select(ctx, mask, C.byref(pimg) if pimg else None, k, t, out, None, slot)

    for call in (embed, detect):
        assert call(t=tab([0, -1, 1])) == bad
        assert "frame 1" in L.wm_last_error(eng._ctx).decode()
        assert call(t=tab([0, 1, 3])) == bad  # index = nkeys
        msg = L.wm_last_error(eng._ctx).decode()
        assert "frame 2" in msg and "3" in msg, msg
        assert call(t=None) == bad
        assert call(k=None) == bad
        assert call(k=other.handle) == bad  # a bank of another shape
        assert call(mask=2) == bad and call(slot=9) == bad and call(slot=-3) == bad
    assert embed(pin=None) == bad and embed(pout=None) == bad and detect(pimg=None) == bad and detect(out=None) == bad
    assert embed(pin=pbig, pout=pbig, t=tab([0, 1, 2, 0])) == bad and detect(pimg=pbig, t=tab([0, 1, 2, 0])) == bad  # frames > max_frames
    e5 = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 5, 40.0, max_frames=F)
    assert embed(ctx=e5._ctx) == wm.WM_ERR_BAD_P and detect(ctx=e5._ctx) == wm.WM_ERR_BAD_P
    assert embed(ctx=e5._ctx, mask=NVF) == wm.WM_OK and detect(ctx=e5._ctx, mask=NVF) == wm.WM_OK and e5.sync(0) == wm.WM_OK
    eb = select_engine(wm, R, Cc, 3, F)
    assert L.wm_band_configure(eb._ctx, 8, 40, 128) == wm.WM_OK
    assert embed(ctx=eb._ctx) == bad and detect(ctx=eb._ctx) == bad  # band mode refuses the calls
    assert "band" in L.wm_last_error(eb._ctx).decode()
    # the Python surface: a table of the wrong length, an index the int32 table cannot hold
    with pytest.raises(RuntimeError, match="key_of_frame"):
        eng.embed_select_async(xs, xs, y, keys, [0, 1], wm.MASK_TYPE.ME, 0)
    with pytest.raises(RuntimeError):
        eng.detect_select_async(xs, keys, [0, 1, 2 ** 40], wm.MASK_TYPE.ME, 0, c)
    # nothing was queued, and a valid call works
    assert eng.sync(0) == wm.WM_OK
    yr, ar, sr, cr = reference(wm, torch, R, Cc, 3, ME, xs, xs, TABLE[:F])
    assert embed() == wm.WM_OK and detect(pimg=py) == wm.WM_OK and eng.sync(0) == wm.WM_OK
    assert same_bits(y, yr) and np.array_equal(u32(a[:F]), u32(ar)) and np.array_equal(u32(c[:F]), u32(cr))
    for obj in (eb, e5, eng, other, keys):
        obj.close()


def test_record_limit(wm, torch_cuda):
    """`frames` results per call count against the slot's 4096; a refused call consumes none: after the refusals two calls of 2048
    frames fill the slot exactly, the next one is WM_ERR_BUSY, and after a sync the slot takes calls again"""
    torch = torch_cuda
    L = wm.lib()
    R, Cc, F = 16, 16, 2048
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS[:2])
    eng = select_engine(wm, R, Cc, 3, F, nslots=1)
    xs = torch.from_numpy(np.tile(frames_of(R, Cc, 8, "f32"), (F // 8, 1, 1))).cuda()
    y = torch.empty_like(xs)
    table = np.arange(F, dtype=np.int32) % 2
    a, c = np.zeros(F, np.float32), np.zeros(F, np.float32)
    worse = table.copy()
    worse[F - 1] = 2
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=f"frame {F - 1}"):
        eng.embed_select_async(xs, xs, y, keys, worse, wm.MASK_TYPE.ME, 0, a)
    with pytest.raises(RuntimeError, match=f"frame {F - 1}"):
        eng.detect_select_async(xs, keys, worse, wm.MASK_TYPE.ME, 0, c)
    eng.embed_select_async(xs, xs, y, keys, table, wm.MASK_TYPE.ME, 0, a)
    eng.detect_select_async(y, keys, table, wm.MASK_TYPE.ME, 0, c)
    px = wm.plane_of(xs, 1)
    tp = table.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.wm_detect_select(eng._ctx, 0, C.byref(px), keys.handle, tp, c.ctypes.data_as(F32P), None, 0) == wm.WM_ERR_BUSY
    assert L.wm_embed_select(eng._ctx, 0, C.byref(px), C.byref(px), C.byref(wm.plane_of(y, 1)), keys.handle, tp, a.ctypes.data_as(F32P), None, 0) == wm.WM_ERR_BUSY
    assert eng.sync(0) == wm.WM_OK
    assert np.all(np.isfinite(a)) and np.all(a > 0) and np.all(c > 0.1)
    # frames 0 .. 7 repeat through the batch with alternating keys: equal frames with equal keys give equal bits
    assert np.array_equal(u32(a[:8]), u32(a[8:16])) and np.array_equal(u32(c[:8]), u32(c[8:16]))
    eng.detect_select_async(y, keys, table, wm.MASK_TYPE.ME, 0, c)
    assert eng.sync(0) == wm.WM_OK
    eng.close()
    keys.close()


# ---- 9. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,p,dtype", [(ME, 3, "f32"), (NVF, 5, "u8")])
def test_repeats_are_bit_equal(wm, torch_cuda, mask, p, dtype):
    torch = torch_cuda
    R, Cc, F = 271, 483, 5
    keys = wm.KeySet.from_seeds(R, Cc, SEEDS)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype)).cuda()
    eng = select_engine(wm, R, Cc, p, F)
    y0, a0, st0, c0 = run_select(wm, torch, eng, keys, xs, xs, mask, TABLE)
    for _ in range(2):
        y, a, st, c = run_select(wm, torch, eng, keys, xs, xs, mask, TABLE)
        assert same_bits(y, y0) and np.array_equal(u32(a), u32(a0)) and np.array_equal(u32(c), u32(c0))
    eng.close()
    keys.close()
