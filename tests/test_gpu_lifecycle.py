"""The life cycle of a context: wm_reinit, wm_reinit_from_file, wm_configure, wm_set_rows_per_segment and wm_clone around every call.

(a) path independence, bit for bit: an engine that REACHED a configuration X = (shape, W, p, psnr, slots, max_frames, rps, fused mode,
    hand-over settings, band) by reconfiguration gives the battery dict (tests/lifecycle_battery.py: every call family once) of an
    engine CREATED in X.  The battery also runs before every transition, so the scratch that grows on demand exists at the old size.
(b) an oracle leg: the created engine's dict against lifecycle_battery.expectations(), once per X.
(c) the contract of include/wm.h: what a reconfiguring call refuses afterwards, keeps, clears and delivers.

A fused fallback would change bits legitimately: every test asserts there was none."""
import ctypes as C

import numpy as np
import pytest

import hard_frames as H
import lifecycle_battery as LB
import oracle_lib as O
from lifecycle_battery import fp, ip
from sequence_model import GRAM_KERNELS
from synth import synth_frame

pytestmark = pytest.mark.gpu

S_SEQ, S_STRIP, S_SPLIT, S_TILES, S_TINY = LB.S_SEQ, LB.S_STRIP, LB.S_SPLIT, LB.S_TILES, LB.S_TINY


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_BANKS, _PLANES, _WANT, _FRESH = {}, {}, {}, {}


def banks_of(wm, shape):
    if shape not in _BANKS:
        _BANKS[shape] = LB.banks(wm, shape)
        _PLANES[shape] = tuple([b.plane(k) for k in range(LB.K)] for b in _BANKS[shape])
    return _BANKS[shape]


def create(wm, shape, p, cfg, w_seed=None):
    """an engine created directly in X.  rps comes from one wm_set_rows_per_segment made before any other call: the only way to give an
    engine an rps, and the rebuild it causes comes before any queued work or grown scratch"""
    eng = wm.Watermark(shape[0], shape[1], LB.watermark_of(shape, w_seed), p, 40.0)
    if cfg["rps"]:
        eng.set_rows_per_segment(cfg["rps"])
    if (cfg["nslots"], cfg["max_frames"]) != (2, 1):
        eng.configure(cfg["nslots"], cfg["max_frames"])
    eng.set_fused(cfg["fused"])
    eng.set_checked_handover(cfg["checked"])
    eng.set_handover(cfg["handover"])
    return eng


def run(wm, torch, eng, shape, p, cfg, w_seed=None):
    keys, big = banks_of(wm, shape)
    return LB.battery(wm, torch, eng, shape, p=p, F=cfg["max_frames"], slot=cfg["nslots"] - 1, keys=keys, keys_big=big, w_seed=w_seed)


def no_fallback(wm, eng):
    assert eng.fused_info()[3] == 0 and wm.lib().wm_fused_lock_skips(eng._ctx) == 0


def assert_same(got, want, what):
    bad = LB.same_bits(got, want)
    assert not bad, f"{what}: {len(bad)} of {len(want)} results differ in bits: {bad[:12]}"


def fresh(wm, torch, shape, p, cfg, w_seed=None):
    """the battery of an engine created in X, held to the oracle (leg b); computed once per X and left unchanged"""
    key = (shape, p, w_seed, tuple(sorted(cfg.items())))
    if key not in _FRESH:
        eng = create(wm, shape, p, cfg, w_seed)
        got = run(wm, torch, eng, shape, p, cfg, w_seed)
        no_fallback(wm, eng)
        eng.close()
        wkey = (shape, p, cfg["max_frames"], w_seed)
        if wkey not in _WANT:
            banks_of(wm, shape)
            _WANT[wkey] = LB.expectations(shape, p=p, F=cfg["max_frames"], key_planes=_PLANES[shape][0], key_planes_big=_PLANES[shape][1], w_seed=w_seed)
        bad = LB.check(got, _WANT[wkey])
        assert not bad, f"created engine against the oracle, {shape} p={p} {cfg}: {bad[:12]}"
        for v in got.values():
            v.setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def plane1(wm, t):
    return wm.plane_of(t, 1)


def refused(wm, torch, eng, old, new, cfg):
    """after a reinit from shape `old` to `new`: planes and banks of the old shape, and the slot's WM_MEM_SLOT_OUT, are WM_ERR_BAD_ARG"""
    L, mk, slot = wm.lib(), int(wm.MASK_TYPE.NVF), cfg["nslots"] - 1
    corr = (C.c_float * (LB.K * cfg["max_frames"]))()
    xn = torch.zeros(new, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    so = LB.slot_out_plane(wm, new, cfg["max_frames"])   # (the battery's last embed on this slot wrote max_frames frames)
    assert L.wm_detect(eng._ctx, mk, C.byref(so), corr, None, slot) == wm.WM_ERR_BAD_ARG
    if old != new:
        xo = torch.zeros(old, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        po, pn = plane1(wm, xo), plane1(wm, xn)
        assert L.wm_embed(eng._ctx, mk, C.byref(po), C.byref(po), C.byref(po), None, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
        assert L.wm_detect(eng._ctx, mk, C.byref(po), corr, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
        assert L.wm_detect_keys(eng._ctx, mk, C.byref(pn), banks_of(wm, old)[0].handle, corr, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    assert eng.sync(slot) == 0


def one_frame_kernels(wm, torch, eng, shape):
    """the kernels a synchronous one-frame embed + detect launches (prof_report, as test_fused_calls_in_vector_layouts reads it)"""
    x = torch.from_numpy(np.array(LB.inputs(shape)["xf32"][0])).cuda()
    eng.prof_enable(True)
    eng.prof_reset()
    y, a = eng.makeWatermark(x, x, wm.MASK_TYPE.ME)
    eng.detectWatermark(y, wm.MASK_TYPE.ME)
    rep = eng.prof_report()
    eng.prof_enable(False)
    return set(rep)


# ---- 1. wm_reinit / wm_reinit_from_file ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("settings", ["default", "custom"])
@pytest.mark.parametrize("case", LB.REINIT_CASES, ids=lambda c: c[0].replace(" ", "_"))
def test_reinit(wm, tc, case, settings, tmp_path):
    """the battery at the old shape, the reinit, the battery at the new shape: the bits of an engine created there.  The settings
    (fused off, rps 5, 3 slots, 3 frames) survive; planes and banks of the old shape and the slot's WM_MEM_SLOT_OUT are refused; a band
    is cleared; after fusable -> not fusable -> fusable the one-frame calls take the fused kernels again"""
    torch = tc
    kind, shapes, how = case
    cfg = LB.DEFAULTS if settings == "default" else LB.CUSTOM
    same = kind == "reinit same shape"
    eng = create(wm, shapes[0], 3, cfg)
    assert_same(run(wm, torch, eng, shapes[0], 3, cfg), fresh(wm, torch, shapes[0], 3, cfg), f"before the reinit, {shapes[0]}")
    follows = kind == "reinit fusable switch"   # (40 x 272 and 70 x 300 take the fused kernels, 5 x 7 does not)
    assert not follows or eng.fused_info()[0] == cfg["fused"]
    prev = shapes[0]
    for s in shapes[1:]:
        w_seed = LB.W2_SEED if same else None
        W = LB.watermark_of(s, w_seed)
        if same:
            eng.band_configure(2, prev[0] - 2, prev[0])   # belongs to the old W's planes: a reinit clears it
        if how == "file":
            path = tmp_path / "w.dat"
            W.tofile(path)
            eng.reinitialize(str(path), s[0], s[1])
        else:
            eng.reinitialize(W, s[0], s[1])
        assert (eng.rows, eng.cols) == s
        refused(wm, torch, eng, prev, s, cfg)
        assert not follows or eng.fused_info()[0] == (cfg["fused"] and s != S_TINY)
        assert_same(run(wm, torch, eng, s, 3, cfg, w_seed), fresh(wm, torch, s, 3, cfg, w_seed), f"{kind}: {prev} -> {s}, {settings} settings")
        no_fallback(wm, eng)
        prev = s
    if same:
        # the old W's marks now score like unmarked frames: the oracle's figure for the NEW W, far below a marked frame's
        old = LB.inputs(s)["markedf32"][0]
        c = eng.detectWatermark(torch.from_numpy(np.array(old)).cuda(), wm.MASK_TYPE.ME)
        assert abs(c - O.detect(old, W)[1]) <= LB.TOLERANCES["score"][0]
        marked = float(fresh(wm, torch, s, 3, cfg)["detect/ME/f32/F1.corr"][0])
        print(f"old W's mark under the new W: {c:.4f}; under its own W: {marked:.4f}")
        assert abs(c) < 0.1 < marked
    if kind == "reinit fusable switch":
        names = one_frame_kernels(wm, torch, eng, prev)
        if cfg["fused"]:
            assert {"k_fused_embed", "k_fused_detect"} <= names and not {"k_gram", "k_embed", "k_detect"} & names, names
        else:
            assert {"k_gram", "k_embed", "k_detect"} <= names and not {"k_fused_embed", "k_fused_detect"} & names, names
        no_fallback(wm, eng)
    eng.close()


# ---- 2. wm_configure -----------------------------------------------------------------------------------------------------------------

def test_configure_walk(wm, tc):
    """(2, 1) -> (3, 3) -> (1, 2) with the battery at every stop; after the shrink F = 3 and slots 1 and 2 are WM_ERR_BAD_ARG"""
    torch = tc
    shape, cfg = S_SEQ, dict(LB.DEFAULTS)
    eng = create(wm, shape, 3, cfg)
    for ns, mf in LB.CONFIGURE_STOPS:
        if (ns, mf) != (cfg["nslots"], cfg["max_frames"]):
            eng.configure(ns, mf)
            cfg = dict(cfg, nslots=ns, max_frames=mf)
        assert_same(run(wm, torch, eng, shape, 3, cfg), fresh(wm, torch, shape, 3, cfg), f"configured to ({ns}, {mf})")
        no_fallback(wm, eng)
    L, mk = wm.lib(), int(wm.MASK_TYPE.NVF)
    x3 = torch.zeros((3,) + shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p3, p2, p1 = plane1(wm, x3), plane1(wm, x3[:2]), plane1(wm, x3[0])
    corr = (C.c_float * 3)()
    assert L.wm_embed(eng._ctx, mk, C.byref(p3), C.byref(p3), C.byref(p3), None, None, 0) == wm.WM_ERR_BAD_ARG
    assert L.wm_detect(eng._ctx, mk, C.byref(p3), corr, None, 0) == wm.WM_ERR_BAD_ARG
    for slot in (1, 2):
        assert L.wm_embed(eng._ctx, mk, C.byref(p1), C.byref(p1), C.byref(p1), None, None, slot) == wm.WM_ERR_BAD_ARG
        assert L.wm_sync(eng._ctx, slot) == wm.WM_ERR_BAD_ARG
    assert L.wm_detect(eng._ctx, mk, C.byref(p2), corr, None, 0) == 0 and eng.sync(0) in (0, 1)   # (F = 2 on slot 0 is what is left)
    eng.close()


def test_configure_keeps_the_band(wm, tc):
    """a band set before wm_configure is in force after it: wm_band_stats / wm_band_embed on two bands (test_gpu_bands.py's construction)
    give the bits of a banded pair created at (3, 3)"""
    torch = tc
    shape = S_STRIP
    W = LB.watermark_of(shape)
    engs = LB.banded_engines(wm, shape, W, lambda r, c, Wb: wm.Watermark(r, c, Wb, 3, 40.0))
    LB.band_battery(wm, torch, engs, shape)   # (the scratch exists at the old size)
    for e in engs:
        e.configure(3, 3)
    got = LB.band_battery(wm, torch, engs, shape)
    ref_engs = LB.banded_engines(wm, shape, W, lambda r, c, Wb: wm.Watermark(r, c, Wb, 3, 40.0, nslots=3, max_frames=3))
    assert_same(got, LB.band_battery(wm, torch, ref_engs, shape), "banded pair behind wm_configure")
    # ... and the pair is a banded pair: its strength is the whole image's (oracle), and whole-image calls are still refused
    x = LB.inputs(shape)["xf32"][0]
    for m, omk in (("ME", O.MASK_ME), ("NVF", O.MASK_NVF)):
        assert abs(got[f"band0/{m}.a"][0] - O.embed(x, x, W, mask=omk)[2]) <= LB.TOLERANCES["a"][0] * abs(got[f"band0/{m}.a"][0])
        assert np.array_equal(got[f"band0/{m}.a"], got[f"band1/{m}.a"])
    xt = torch.zeros((engs[0].rows, engs[0].cols), dtype=torch.float32, device="cuda")
    mt = torch.zeros((1, 1, engs[0].cols // 32), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pl = plane1(wm, xt)
    assert wm.lib().wm_detect_tiles(engs[0]._ctx, 1, C.byref(pl), 32, 32, C.c_void_p(mt.data_ptr()), None, None, wm.WM_SLOT_SYNC) == wm.WM_ERR_BAD_ARG
    for e in engs + ref_engs:
        e.close()


# ---- 3. wm_set_rows_per_segment: every family at rps 1, one segment, a ragged last segment and the automatic value ---------------------

@pytest.mark.parametrize("p", [3, 7])
@pytest.mark.parametrize("shape", LB.RPS_SHAPES, ids=lambda s: "%dx%d" % s)
def test_rows_per_segment_walk(wm, tc, shape, p):
    """0 -> 1 -> 4096 -> 5 -> 0 on one engine, the full battery at each stop: the bits of an engine created at that rps, which is held
    to the oracle.  The key-bank, offsets, select, tiles and 16-bit families have no other test at a segment length but the automatic"""
    torch = tc
    cfg = dict(LB.DEFAULTS, max_frames=LB.MAX_F)
    eng = create(wm, shape, p, cfg)
    for i, rps in enumerate(LB.RPS_STOPS):
        if i:
            eng.set_rows_per_segment(rps)
            cfg = dict(cfg, rps=rps)
        assert_same(run(wm, torch, eng, shape, p, cfg), fresh(wm, torch, shape, p, cfg), f"stop {i}: rps {rps}")
        no_fallback(wm, eng)
    eng.close()


# ---- 4. wm_clone ---------------------------------------------------------------------------------------------------------------------

def gram_kernels(eng):
    return {k for k in eng.prof_report() if k in GRAM_KERNELS}


@pytest.mark.parametrize("variant", LB.CLONE_VARIANTS)
def test_clone_takes_every_setting(wm, tc, variant):
    """a source with every setting away from its default: the clone's battery equals the source's bit for bit, its checked hand-over
    counts move alike and its profile names the same Gram kernels.  Source and clone do not see each other's reinit, and the clone
    outlives the source (W is shared)"""
    torch = tc
    if variant == "band":
        shape = S_STRIP
        W = LB.watermark_of(shape)

        def make(r, c, Wb):
            e = wm.Watermark(r, c, Wb, 3, 40.0, nslots=3, max_frames=3)
            e.set_rows_per_segment(5)
            e.set_fused(False)
            return e
        engs = LB.banded_engines(wm, shape, W, make)
        clones = [e.copy() for e in engs]
        want = LB.band_battery(wm, torch, engs, shape)
        assert_same(LB.band_battery(wm, torch, clones, shape), want, "clones of a banded pair")
        for e in engs:
            e.close()
        assert_same(LB.band_battery(wm, torch, clones, shape), want, "clones of a banded pair, sources destroyed")
        for e in clones:
            e.close()
        return
    shape, other = S_SEQ, S_SPLIT
    cfg = dict(LB.CUSTOM, checked=variant != "checked_off", handover=variant == "handover_on")
    src = create(wm, shape, 3, cfg)
    clone, clone2 = src.copy(), src.copy()
    assert clone.fused_info()[0] == src.fused_info()[0] == False  # noqa: E712
    for e in (src, clone):
        e.prof_enable(True)
        e.prof_reset()
    before = src.checked_handover_counts(), clone.checked_handover_counts()
    got_src = run(wm, torch, src, shape, 3, cfg)
    got_clone = run(wm, torch, clone, shape, 3, cfg)
    moved = [tuple(b - a for a, b in zip(c0, e.checked_handover_counts())) for c0, e in zip(before, (src, clone))]
    ks, kc = gram_kernels(src), gram_kernels(clone)
    print(f"{variant}: counts moved by {moved}, Gram kernels {sorted(ks)} / {sorted(kc)}")
    assert moved[0] == moved[1], moved
    assert ks == kc, (ks, kc)   # k_gram_ho on both, or on neither
    if variant == "handover_on":
        assert "k_gram_ho" in ks, ks
    else:
        assert "k_gram_ho_checked" not in ks and moved[0] == (0, 0), (ks, moved)
    assert_same(got_clone, got_src, "the clone's battery against the source's")
    assert_same(got_src, fresh(wm, torch, shape, 3, cfg), "the source against an engine created in its configuration")
    for e in (src, clone):
        e.prof_enable(False)
    # reinit the clone: the source is unchanged, and the clone kept its settings
    clone.reinitialize(LB.watermark_of(other), other[0], other[1])
    assert_same(run(wm, torch, src, shape, 3, cfg), got_src, "the source behind the clone's reinit")
    assert_same(run(wm, torch, clone, other, 3, cfg), fresh(wm, torch, other, 3, cfg), "the reinitialised clone")
    # reinit the source: the second clone is unchanged; destroy the source: it still works
    src.reinitialize(LB.watermark_of(other), other[0], other[1])
    assert_same(run(wm, torch, clone2, shape, 3, cfg), got_src, "a clone behind the source's reinit")
    src.close()
    assert_same(run(wm, torch, clone2, shape, 3, cfg), got_src, "a clone behind the source's destruction")
    for e in (clone, clone2):
        no_fallback(wm, e)
        e.close()


# ---- 5. queued results at a reconfiguration ------------------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.0)


def queue_three(wm, torch, eng, xs, keys, T):
    """an embed of F = 3, a wm_detect_keys and a wm_embed_bits queued on slot 0, caller arrays pre-filled: (host arrays, planes)"""
    F, mk = xs.shape[0], wm.MASK_TYPE.ME
    xt = torch.from_numpy(xs).cuda()
    planes = {"y": torch.zeros_like(xt), "yb": torch.zeros_like(xt), "x": xt}
    r = {"a": np.full(F, SENTINEL), "a_st": np.full(F, -5, np.int32), "ck": np.full((F, LB.K), SENTINEL), "ck_st": np.full(F, -5, np.int32),
         "ab": np.full(F, SENTINEL), "ab_st": np.full(F, -5, np.int32)}
    torch.cuda.synchronize()
    eng.embed_async(xt, xt, planes["y"], mk, 0, fp(r["a"]), ip(r["a_st"]))
    eng.detect_keys_async(xt, keys, mk, 0, r["ck"], r["ck_st"])
    eng.embed_bits_async(xt, xt, planes["yb"], LB.TH, LB.TW, T["tile_bit"], T["nbits"], T["payload"], mk, 0, r["ab"], r["ab_st"])
    return r, planes


@pytest.mark.parametrize("how", ["configure", "rows_per_segment", "reinit"])
def test_queued_results_are_delivered_by_a_reconfiguration(wm, tc, how):
    """no wm_sync in front of the reconfiguring call: it delivers every strength, score and status as wm_sync does on a twin engine (the
    singular frame keeps its sentinel strength, status 1), returns WM_OK, and a wm_sync afterwards has nothing left to deliver"""
    torch = tc
    shape, F = S_SEQ, 3
    R, Cc = shape
    W = LB.watermark_of(shape)
    xs = np.stack([synth_frame(R, Cc, frame=0), H.singular("ramp", R, Cc), synth_frame(R, Cc, frame=2)])
    keys, T, L = banks_of(wm, shape)[0], LB.tables(shape, F), wm.lib()
    twin = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2, max_frames=F)
    want, want_planes = queue_three(wm, torch, twin, xs, keys, T)
    assert list(want["a_st"]) == [-5] * F and want["ck"][0, 0] == SENTINEL   # (nothing is delivered before the sync)
    assert twin.sync(0) == wm.WM_UNSOLVABLE
    assert list(want["a_st"]) == [0, 1, 0] == list(want["ab_st"]) == list(want["ck_st"]) and want["a"][1] == SENTINEL == want["ab"][1]
    assert want["a"][0] != SENTINEL and (want["ck"][1] == 0.0).all() and (want["ck"][0] != SENTINEL).all()
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=2, max_frames=F)
    got, got_planes = queue_three(wm, torch, eng, xs, keys, T)
    if how == "configure":
        rc = L.wm_configure(eng._ctx, 2, F)
    elif how == "rows_per_segment":
        rc = L.wm_set_rows_per_segment(eng._ctx, 7)
    else:
        rc = L.wm_reinit(eng._ctx, R, Cc, W.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == wm.WM_OK   # (the unsolvable frame is in the statuses, as with wm_set_stream)
    torch.cuda.synchronize()
    for n in want:
        assert np.array_equal(LB.raw(got[n]), LB.raw(want[n])), (how, n, got[n], want[n])
    for n in ("y", "yb", "x"):
        assert torch.equal(got_planes[n], want_planes[n]), n
    assert torch.equal(got_planes["y"][1], got_planes["x"][1])   # the unsolvable frame: out == base
    snapshot = {n: v.copy() for n, v in got.items()}
    assert L.wm_sync(eng._ctx, 0) == wm.WM_OK
    for n in got:
        assert np.array_equal(LB.raw(got[n]), LB.raw(snapshot[n])), n
    eng.close()
    twin.close()


# ---- 6. the caller's stream ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["configure", "rows_per_segment", "reinit", "reinit_from_file"])
def test_caller_stream_survives_a_reconfiguration(wm, tc, how, tmp_path):
    """a slot that was given the caller's stream still runs on it after each of the four calls, ordered with the caller's own work
    (test_gpu_api.py test_caller_stream's check); NULL restores the slot's own stream; a slot that no longer exists is WM_ERR_BAD_ARG"""
    torch = tc
    shape = S_SEQ
    R, Cc = shape
    W, W2 = LB.watermark_of(shape), LB.watermark_of(shape, LB.W2_SEED)
    x = np.array(LB.inputs(shape)["xf32"][0])
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=3, max_frames=1)
    L = wm.lib()
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    own0 = L.wm_get_stream(eng._ctx, 0)
    assert L.wm_set_stream(eng._ctx, 0, C.c_void_p(s.cuda_stream)) == 0 and L.wm_set_stream(eng._ctx, 2, C.c_void_p(s2.cuda_stream)) == 0
    xd0 = torch.from_numpy(x).cuda()
    eng.makeWatermark(xd0, xd0, wm.MASK_TYPE.NVF)   # (the slot has run on the stream before the reconfiguration)
    if how == "configure":
        eng.configure(2, 2)
    elif how == "rows_per_segment":
        eng.set_rows_per_segment(5)
    elif how == "reinit":
        eng.reinitialize(W2, R, Cc)
        W = W2
    else:
        W2.tofile(tmp_path / "w.dat")
        eng.reinitialize(str(tmp_path / "w.dat"), R, Cc)
        W = W2
    assert L.wm_get_stream(eng._ctx, 0) == s.cuda_stream
    if how == "configure":   # slot 2 is gone, and its stream with it
        assert L.wm_get_stream(eng._ctx, 2) is None and L.wm_set_stream(eng._ctx, 2, None) == wm.WM_ERR_BAD_ARG
        assert L.wm_get_stream(eng._ctx, 1) not in (None, s.cuda_stream, s2.cuda_stream)
    else:
        assert L.wm_get_stream(eng._ctx, 2) == s2.cuda_stream
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).cuda(non_blocking=True) * 1.0   # produced on the same stream, no host sync in between
        out = torch.empty_like(xd)
        a = (C.c_float * 1)()
        eng.embed_async(xd, xd, out, wm.MASK_TYPE.NVF, 0, a_out=a)
        doubled = out * 2.0                                      # consumer on the same stream
    assert eng.sync(0) == 0
    s.synchronize()
    so, yo, ao = O.embed(x, x, W, mask=O.MASK_NVF)
    assert a[0] == pytest.approx(ao, rel=1e-4)
    np.testing.assert_allclose(doubled.cpu().numpy(), 2 * yo, rtol=0, atol=2e-3)
    assert L.wm_set_stream(eng._ctx, 0, None) == 0
    restored = L.wm_get_stream(eng._ctx, 0)
    assert restored not in (None, s.cuda_stream, s2.cuda_stream)
    y, a2 = eng.makeWatermark(xd0, xd0, wm.MASK_TYPE.NVF)       # the slot's own stream works
    assert a2 == pytest.approx(ao, rel=1e-4)
    assert own0 is not None
    eng.close()


# ---- 7. state that must not survive --------------------------------------------------------------------------------------------------

def test_handover_state_does_not_survive_a_configure(wm, tc):
    """an ME embed of F = 3 leaves a checked hand-over behind; wm_configure with the same numbers drops it and restarts the counters:
    the detector of the embed's output then takes the ordinary path, bit for bit.  The same with a promised hand-over: the
    WM_MEM_SLOT_OUT plane is refused"""
    torch = tc
    shape, F = S_SEQ, 3
    W = LB.watermark_of(shape)
    xt = torch.from_numpy(np.array(LB.inputs(shape)["xf32"])).cuda()
    mk = wm.MASK_TYPE.ME

    def embed_then(eng, between):
        o = torch.zeros_like(xt)
        c, st = np.full(F, np.nan, np.float32), np.full(F, -7, np.int32)
        torch.cuda.synchronize()
        eng.embed_async(xt, xt, o, mk, 0)
        assert eng.sync(0) == 0
        between(eng)
        counts = eng.checked_handover_counts()
        eng.detect_async(o, mk, 0, fp(c), ip(st))
        assert eng.sync(0) == 0 and list(st) == [0] * F
        return c, counts, eng.checked_handover_counts()

    # the control: without a configure in between the detector does take the checked hand-over
    eng = wm.Watermark(shape[0], shape[1], W, 3, 40.0, nslots=2, max_frames=F)
    c_ho, c0, c1 = embed_then(eng, lambda e: None)
    assert c0 == (0, 0) and c1 == (F, 0), (c0, c1)
    # behind a configure: counters at zero, no hand-over, the ordinary path's bits
    c_cfg, c0, c1 = embed_then(eng, lambda e: e.configure(2, F))
    assert c0 == (0, 0) and c1 == (0, 0), (c0, c1)
    plain = wm.Watermark(shape[0], shape[1], W, 3, 40.0, nslots=2, max_frames=F)
    plain.set_checked_handover(False)
    c_plain, _, _ = embed_then(plain, lambda e: None)
    assert np.array_equal(LB.raw(c_cfg), LB.raw(c_plain)), (c_cfg, c_plain)
    assert np.abs(c_ho - c_plain).max() <= 1.2e-7   # (wm.h wm_detect: the checked hand-over against the ordinary path)
    # a promised hand-over: WM_MEM_SLOT_OUT is refused behind the configure
    eng.set_handover(True)
    o = torch.zeros_like(xt)
    torch.cuda.synchronize()
    eng.embed_async(xt, xt, o, mk, 0)
    assert eng.sync(0) == 0
    so = LB.slot_out_plane(wm, shape, F)
    corr = (C.c_float * F)()
    assert wm.lib().wm_detect(eng._ctx, int(mk), C.byref(so), corr, None, 0) == 0 and eng.sync(0) == 0   # (valid before)
    eng.configure(2, F)
    assert wm.lib().wm_detect(eng._ctx, int(mk), C.byref(so), corr, None, 0) == wm.WM_ERR_BAD_ARG
    eng.close()
    plain.close()


# ---- 8. profiling across a reconfiguration -------------------------------------------------------------------------------------------

def test_profile_counts_across_reconfigurations(wm, tc):
    """prof_enable, a call, a reconfiguration, a call: prof_report returns and counts both calls (events recorded on the old slots'
    streams are still read)"""
    torch = tc
    shape = S_SEQ
    W = LB.watermark_of(shape)
    eng = wm.Watermark(shape[0], shape[1], W, 3, 40.0)
    eng.set_fused(False)
    x = torch.from_numpy(np.array(LB.inputs(shape)["xf32"][0])).cuda()
    eng.prof_enable(True)
    eng.prof_reset()
    calls = 0
    for step in (None, lambda: eng.configure(3, 2), lambda: eng.set_rows_per_segment(5), lambda: eng.reinitialize(W, shape[0], shape[1])):
        if step:
            step()
        eng.makeWatermark(x, x, wm.MASK_TYPE.NVF)
        calls += 1
    rep = eng.prof_report()
    assert rep["k_embed"][0] == calls and rep["k_nvf_stats"][0] == calls, rep
    eng.close()
