"""The host layer's state from call to call (wm_api.hip: result queue, table arenas, grow-on-demand scratch, WM_MEM_SLOT_OUT, the
hand-over flags, the in-place snapshot, the one-call pair), held to what include/wm.h promises about it.

A. Seeded random call sequences on three slots that share a pool of output planes (tests/sequence_model.py draws them and states
   wm.h's slot rules as a model).  The engine under test runs a sequence as drawn -- asynchronous slots, WM_SLOT_SYNC calls, hand-over
   switches as the seed sets them --, a reference engine with the fused kernels and both hand-overs off replays every call alone and
   synchronously on the inputs the model says the call saw.  Ordinary results are the replay's bit for bit; a score whose Gram matrix
   came from a hand-over may differ by wm.h's bound; the path the model predicts is held to the checked hand-over's counters and the
   launch counts of the four Gram kernels, so the tolerance cannot hide a wrong path.  One exception to "fused off": the fused kernels
   and the sweeps agree to rounding only (wm.h wm_set_fused), so for a call the model classes as fused (synchronous, one frame, fused
   on) the replay switches its fused kernels on for that one call.  Such a call is therefore held to the same fused kernel, run alone
   on a fresh queue; what it leaves in the pool and on the slot is held to the sweeps by every call behind it.  The first wm_embed and
   the first wm_detect of every sequence are also held to the CPU oracle.
B. Table arenas, record scratch and staging buffers that are replaced while calls are queued.
C. A synchronous call with asynchronous work still queued on slot 0."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sequence_model as M
from synth import synth_frame, synth_watermark
from test_gpu_parity import TOL_A, TOL_CORR, TOL_Y

pytestmark = pytest.mark.gpu

R, Cc = M.R, M.C
SENT_F, SENT_I = -777.0, -99
TOL_DETECT, TOL_PAIR = 1.2e-7, 2e-7   # wm.h: wm_detect's checked hand-over; the pair, and with it every promised hand-over
# per-tile sums behind a handed-over Gram matrix (wm.h wm_detect_tiles states this bound): the coefficients are f32 and may move by
# one ulp (6e-8 relative), which moves a prediction error of a few grey levels by ~1e-5 of a level and a sum of 1024 squared errors
# by < 1e-5 relative.  The maps keep 2e-7; everything else of a handed-over call stays bitwise
RTOL_SUMS = 1e-5


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def fl(n, v=SENT_F):
    return (C.c_float * n)(*([v] * n))


def il(n):
    return (C.c_int * n)(*([SENT_I] * n))


def u32(a):
    """the bits of a ctypes float / int array"""
    return np.frombuffer(a, dtype=np.uint32).copy()


def f32(a):
    return np.frombuffer(a, dtype=np.float32).copy()


def same_bits(torch, a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((np.abs(a - b) <= tol) | (np.isnan(a) & np.isnan(b))))


def host_plane(wm, ptr, F, dtype):
    return wm.wm_plane(ptr, R, Cc, 1, dtype, wm.WM_MEM_HOST, F, Cc, 0, R * Cc)


def slot_plane(wm, F, dtype=None, rows=R, cols=Cc):
    return wm.wm_plane(None, rows, cols, 1, wm.WM_F32 if dtype is None else dtype, wm.WM_MEM_SLOT_OUT, F, cols, 0, rows * cols)


# ---- A. random sequences ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(wm, tc):
    """what every sequence shares and leaves unchanged: input frames, the pool's first contents, W and the key banks"""
    torch = tc
    W = synth_watermark(R, Cc)
    X = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=f) for f in range(M.NFRESH)])).cuda()
    BX = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=40 + f) for f in range(M.NFRESH)])).cuda()
    P0 = torch.from_numpy(np.stack([synth_frame(R, Cc, frame=80 + f) for f in range(M.POOL_FRAMES)])).cuda()
    keys = wm.KeySet.from_seeds(R, Cc, [11, 12, 13])
    keys.set(M.KEY_W, W)
    okeys = wm.KeySet.from_seeds(M.OFF_ROWS, M.OFF_COLS, [21])
    torch.cuda.synchronize()
    yield dict(W=W, X=X, BX=BX, P0=P0, keys=keys, okeys=okeys)
    keys.close(); okeys.close()


def own_outputs(torch, step):
    """the device tensors a step writes that are not pool frames, filled with a sentinel"""
    kind, F = step["kind"], step.get("F", 0)
    full = lambda shape, dt=torch.float32: torch.full(shape, SENT_F, dtype=dt, device="cuda")
    if kind == "detect_tiles":
        return dict(map=full((F, M.NY, M.NX)), sums=full((F, M.NY, M.NX, 3), torch.float64))
    if kind == "detect_keys_tiles":
        return dict(map=full((F, M.NKEYS, M.NY, M.NX)), sums=full((F, M.NKEYS, M.NY, M.NX, 3), torch.float64))
    if kind in M.COPIES and step["out"] is None:
        return dict(copies=full((F * (M.NKEYS if kind == "embed_keys" else M.NCOPIES), R, Cc)))
    if kind == "compute_mask":
        d = dict()
        if step["out"] is None:
            d["mask"] = full((F, R, Cc))
        if step["e_out"]:
            d["e"] = full((F, R, Cc))
        return d
    return {}


def issue(wm, torch, world, eng, P, step, ann, slot, dev, as_ref):
    """makes one call of a sequence on `eng` with the pool P; returns (host outputs, pool frames written).  as_ref: the isolated
    replay -- WM_MEM_SLOT_OUT is the plane the model says it names, the pair is wm_embed then wm_detect"""
    L, ctx = wm.lib(), eng._ctx
    kind, F, mask = step["kind"], step["F"], step["mask"]
    rng = np.random.default_rng(step["dseed"])
    pl = lambda t: wm.plane_of(t, 1)
    host, writes = {}, []

    def source():
        src = step["src"]
        if src[0] == "fresh":
            return pl(world["X"][src[1]:src[1] + F])
        if src[0] == "pool" or as_ref:
            r0 = ann["src_range"][0]
            return pl(P[r0:r0 + F])
        return slot_plane(wm, F)

    if kind in M.EMBEDS:
        o = P[step["out"]:step["out"] + F]
        x = world["X"][step["x0"]:step["x0"] + F]
        pin, pbase = {"base_is_in": (x, x), "grey_base": (x, world["BX"][step["b0"]:step["b0"] + F]), "in_place": (o, o), "base_is_out": (x, o)}[step["variant"]]
        pin, pbase, pout = pl(pin), pl(pbase), pl(o)
        writes.append((step["out"], F))
        host["a"], host["st"] = fl(F), il(F)
        if kind == "embed":
            rc = L.wm_embed(ctx, mask, C.byref(pin), C.byref(pbase), C.byref(pout), host["a"], host["st"], slot)
        elif kind == "embed_detect":
            host["corr"] = fl(F)
            if as_ref:
                rc = L.wm_embed(ctx, mask, C.byref(pin), C.byref(pbase), C.byref(pout), host["a"], host["st"], slot)
                assert rc >= 0
                rc = L.wm_detect(ctx, mask, C.byref(pout), host["corr"], None, slot)
            else:
                rc = L.wm_embed_detect(ctx, mask, C.byref(pin), C.byref(pbase), C.byref(pout), host["a"], host["corr"], host["st"], slot)
        elif kind == "embed_signs":
            eng.embed_signs_async(pin, pbase, pout, M.TILE, M.TILE, rng.integers(-1, 2, F * M.T).astype(np.int8), mask, slot, host["a"], host["st"])
            rc = 0
        else:
            tile_bit = rng.integers(-1, M.NBITS, M.T).astype(np.int32)
            eng.embed_bits_async(pin, pbase, pout, M.TILE, M.TILE, tile_bit, M.NBITS, rng.integers(0, 256, F).astype(np.uint8), mask, slot, host["a"], host["st"])
            rc = 0
    elif kind in M.COPIES:
        n = F * (M.NKEYS if kind == "embed_keys" else M.NCOPIES)
        pin = source()
        base_is_in = step["src"][0] == "fresh" and step["dseed"] % 2 == 0
        pbase = pin if base_is_in else pl(world["BX"][step["b0"]:step["b0"] + F])
        if step["out"] is None:
            pout = pl(dev["copies"])
        else:
            pout = pl(P[step["out"]:step["out"] + n])
            writes.append((step["out"], n))
        host["st"] = il(F)
        if kind == "embed_keys":
            host["a"] = fl(n)
            eng.embed_keys_async(pin, pbase, pout, world["keys"], mask, slot, host["a"], host["st"])
        else:
            host["a"] = fl(F)
            eng.embed_signs_multi_async(pin, pbase, pout, M.TILE, M.TILE, M.NCOPIES, rng.integers(-1, 2, n * M.T).astype(np.int8), mask, slot,
                                        host["a"], host["st"])
        rc = 0
    elif kind == "compute_mask":
        pin = source()
        if step["out"] is None:
            pm = pl(dev["mask"])
        else:
            pm = pl(P[step["out"]:step["out"] + F])
            writes.append((step["out"], F))
        pe = pl(dev["e"]) if step["e_out"] else None
        host["coef"], host["st"] = fl(8 * F), il(F)
        rc = L.wm_compute_mask(ctx, mask, C.byref(pin), C.byref(pm), C.byref(pe) if pe is not None else None, host["coef"], host["st"], slot)
    else:
        pimg = source()
        host["st"] = il(F)
        rc = 0
        if kind == "detect":
            host["corr"] = fl(F)
            rc = L.wm_detect(ctx, mask, C.byref(pimg), host["corr"], host["st"], slot)
        elif kind == "detect_keys":
            host["corr"] = fl(F * M.NKEYS)
            eng.detect_keys_async(pimg, world["keys"], mask, slot, host["corr"], host["st"])
        elif kind == "detect_offsets":
            host["corr"] = fl(F * M.OFF_N * M.OFF_N)
            eng.detect_offsets_async(pimg, world["okeys"], 0, step["oy0"], step["ox0"], M.OFF_N, M.OFF_N, mask, slot, host["corr"], host["st"])
        elif kind == "detect_tiles":
            eng.detect_tiles_async(pimg, M.TILE, M.TILE, mask, slot, dev["map"], dev["sums"], host["st"])
        elif kind == "detect_keys_tiles":
            eng.detect_keys_tiles_async(pimg, world["keys"], M.TILE, M.TILE, mask, slot, dev["map"], dev["sums"], host["st"])
        else:
            tile_bit = rng.integers(-1, M.NBITS, M.T).astype(np.int32)
            host["soft"] = fl(F * M.NBITS)
            eng.detect_bits_async(pimg, M.TILE, M.TILE, tile_bit, M.NBITS, mask, slot, host["soft"], host["st"])
    assert rc >= 0, (step, rc, L.wm_last_error(ctx))
    return host, writes


def undelivered(host):
    return all(np.all(f32(v) == SENT_F) if k != "st" else np.all(np.frombuffer(v, np.int32) == SENT_I) for k, v in host.items())


def compare(torch, step, ann, got, ref, what):
    """one delivered call against its isolated replay"""
    kind, F = step["kind"], step["F"]
    handed = ann["path"] in ("promised", "checked")
    tol = TOL_DETECT if kind == "detect" else TOL_PAIR
    for name, g in got["host"].items():
        r = ref["host"][name]
        if handed and name in ("corr", "soft"):
            gv, rv = f32(g).reshape(F, -1), f32(r).reshape(F, -1)
            for f in range(F):
                if ann["frame_paths"][f] == "redone":   # wm.h: a redone frame's result "is then the ordinary path's"
                    assert np.array_equal(gv[f].view(np.uint32), rv[f].view(np.uint32)), (what, name, f, gv[f], rv[f])
                else:
                    assert close(gv[f], rv[f], tol), (what, name, f, gv[f], rv[f], ann["path"])
        else:
            assert np.array_equal(u32(g), u32(r)), (what, name, f32(g), f32(r), ann["path"])
    for name, g in got["dev"].items():
        r = ref["dev"][name]
        if handed and name == "map":
            assert close(g.cpu().numpy(), r.cpu().numpy(), tol), (what, name)
        elif handed and name == "sums":
            gs, rs = g.cpu().numpy(), r.cpu().numpy()
            assert np.all(np.abs(gs - rs) <= RTOL_SUMS * np.abs(rs)), (what, name)
        else:
            assert same_bits(torch, g, r), (what, name, ann["path"])


@pytest.mark.parametrize("seed", M.SEEDS)
def test_a_random_sequence_is_its_isolated_replay(wm, tc, world, seed):
    torch = tc
    seq = M.generate(seed)
    W = world["W"]
    eng = wm.Watermark(R, Cc, W, 3, 40.0, nslots=M.NSLOTS, max_frames=M.MAX_F)
    ref = wm.Watermark(R, Cc, W, 3, 40.0, nslots=M.NSLOTS, max_frames=M.MAX_F)
    eng.set_fused(seq.fused); eng.set_handover(seq.handover); eng.set_checked_handover(seq.checked)
    ref.set_fused(False); ref.set_handover(False); ref.set_checked_handover(False)
    if seq.fused:
        assert eng.fused_info()[0], "40 x 272 should take the fused kernels"
    eng.prof_enable(True)
    t0, r0 = eng.checked_handover_counts()
    Pe, Pr = world["P0"].clone(), world["P0"].clone()
    devs = [(own_outputs(torch, st), own_outputs(torch, st)) for st in seq.steps]
    torch.cuda.synchronize()
    results = {}                                   # step index -> the engine's and the replay's outputs
    pending = [[] for _ in range(M.NSLOTS)]         # per slot: the steps queued and not delivered
    anchored = set()

    def deliver(si):
        batch, pending[si] = pending[si], []
        for n, i in enumerate(batch):
            got, rf = results.pop(i)
            what = (seed, i, seq.steps[i]["kind"])
            assert not undelivered(got["host"]) or not got["host"], ("wm_sync delivered nothing", what)
            compare(torch, seq.steps[i], seq.annotations[i], got, rf, what)
            later = [w for j in batch[n + 1:] for w in seq.annotations[j]["writes"]]
            for (start, cnt), snap in rf["snaps"]:
                if not any(M.overlap((start, cnt), w) for w in later):
                    assert same_bits(torch, Pe[start:start + cnt], snap), ("plane", what, seq.annotations[i]["path"])

    for i, (st, ann) in enumerate(zip(seq.steps, seq.annotations)):
        kind = st["kind"]
        for q in pending:  # nothing is delivered before its slot is synced
            for j in q:
                assert undelivered(results[j][0]["host"]), ("delivered before wm_sync", seed, j, seq.steps[j])
        if kind == "sync":
            assert eng.sync(st["slot"]) in (wm.WM_OK, wm.WM_UNSOLVABLE)
            deliver(st["slot"])
            continue
        if kind == "caller_write":
            # the write the library cannot see: one pixel of an output plane, from torch's stream, with every slot that uses it synced
            for P in (Pe, Pr):
                P[st["frame"], st["row"], st["col"]] += 3.0
            torch.cuda.synchronize()
            continue
        slot = wm.WM_SLOT_SYNC if st["slot"] == M.SLOT_SYNC else st["slot"]
        # the replay first (its own pool, its own engine, alone and synchronous), then the engine under test
        before = None
        if kind in ("embed", "detect") and kind not in anchored:
            anchored.add(kind)
            before = Pr.cpu().numpy()
        ref.set_fused(ann["path"] == "fused")
        rhost, rwrites = issue(wm, torch, world, ref, Pr, st, ann, wm.WM_SLOT_SYNC, devs[i][1], True)
        ref.set_fused(False)
        snaps = [((s0, n), Pr[s0:s0 + n].clone()) for s0, n in rwrites]
        torch.cuda.current_stream().synchronize()
        if before is not None:
            anchor_to_the_oracle(world, st, ann["src_range"], before, rhost, Pr)
        ghost, gwrites = issue(wm, torch, world, eng, Pe, st, ann, slot, devs[i][0], False)
        assert gwrites == rwrites == ann["writes"]
        results[i] = (dict(host=ghost, dev=devs[i][0]), dict(host=rhost, dev=devs[i][1], snaps=snaps))
        si = M.Model.slot_index(st["slot"])
        pending[si].append(i)
        if st["slot"] == M.SLOT_SYNC:
            deliver(0)   # wm.h: "runs on slot 0 and synchronises before returning"
    assert not any(pending) and not results
    torch.cuda.synchronize()
    assert same_bits(torch, Pe, Pr), "the pools differ at the end of the sequence"
    # the paths the model predicted are the paths the engine took
    t1, r1 = eng.checked_handover_counts()
    assert (t1 - t0, r1 - r0) == (seq.model.trusted, seq.model.redone), (seed, seq.model.transitions)
    rep = eng.prof_report()
    took = {k: rep.get(k, (0, 0.0))[0] for k in M.GRAM_KERNELS}
    assert took == {k: seq.model.gram[k] for k in M.GRAM_KERNELS}, (seed, took, dict(seq.model.gram))
    n_fused = sum(1 for st, a in zip(seq.steps, seq.annotations) if a["path"] == "fused" for _ in range(2 if st["kind"] == "embed_detect" else 1))
    assert sum(rep.get(k, (0, 0.0))[0] for k in ("k_fused_embed", "k_fused_detect", "k_fused_pair")) == n_fused, (seed, rep)
    for e in (eng, ref):
        assert e.fused_info()[3] == 0 and wm.lib().wm_fused_lock_skips(e._ctx) == 0, "a fused launch fell back to the sweeps"
    eng.close(); ref.close()


def anchor_to_the_oracle(world, st, src_range, pool_before, rhost, Pr):
    """the first embed and the first detect of a sequence against the CPU oracle: an anchor outside the engine, for the replay
    the engine under test is held to"""
    F, W, omask = st["F"], world["W"], O.MASK_ME if st["mask"] == M.ME else O.MASK_NVF
    if st["kind"] == "embed":
        o0 = st["out"]
        x = world["X"][st["x0"]:st["x0"] + F].cpu().numpy()
        xin, base = {"base_is_in": (x, x), "grey_base": (x, world["BX"][st["b0"]:st["b0"] + F].cpu().numpy()),
                     "in_place": (pool_before[o0:o0 + F],) * 2, "base_is_out": (x, pool_before[o0:o0 + F])}[st["variant"]]
        y = Pr[o0:o0 + F].cpu().numpy()
        for f in range(F):
            so, yo, ao = O.embed(xin[f], base[f], W, mask=omask)
            assert so == rhost["st"][f]
            if so == 0:
                assert rhost["a"][f] == pytest.approx(ao, rel=TOL_A)
            np.testing.assert_allclose(y[f], yo, rtol=0, atol=TOL_Y)
    else:
        # (a pool plane or WM_MEM_SLOT_OUT: the plane as the replay's pool held it before the call)
        src = st["src"]
        img = world["X"][src[1]:src[1] + F].cpu().numpy() if src[0] == "fresh" else pool_before[src_range[0]:src_range[0] + F]
        for f in range(F):
            so, co = O.detect(img[f], W, mask=omask)
            assert so == rhost["st"][f] and rhost["corr"][f] == pytest.approx(co, abs=TOL_CORR)


@pytest.mark.parametrize("checked", [True, False])
def test_the_pairs_promise_ends_with_the_pair(wm, tc, world, checked):
    """wm_embed_detect hands the embed's sums to its own detector whether or not wm_set_handover is on.  Without wm_set_handover
    the caller has promised nothing about the plane afterwards: one pixel changed behind the pair, then detectors of the slot's
    WM_MEM_SLOT_OUT -- they score the plane as it is, bit for bit as an engine without hand-overs does, and launch no k_gram_ho
    beyond the pair's (the sums used to stay promised: old Gram matrix, new pixels, no error)"""
    torch = tc
    F, ME = 2, wm.MASK_TYPE.ME
    eng = wm.Watermark(R, Cc, world["W"], 3, 40.0, nslots=2, max_frames=F)
    plain = wm.Watermark(R, Cc, world["W"], 3, 40.0, nslots=2, max_frames=F)
    eng.set_checked_handover(checked)
    plain.set_checked_handover(False)
    eng.prof_enable(True)
    x, y = world["X"][0:F], torch.empty((F, R, Cc), device="cuda")
    torch.cuda.synchronize()
    px, py = wm.plane_of(x), wm.plane_of(y)
    a, corr, st = fl(F), fl(F), il(F)
    assert wm.lib().wm_embed_detect(eng._ctx, int(ME), C.byref(px), C.byref(px), C.byref(py), a, corr, st, 1) == 0
    eng.sync(1)
    assert eng.prof_report()["k_gram_ho"][0] == 1
    y[1, 20, 100] += 3.0
    torch.cuda.synchronize()
    got, ref, keys_got, keys_ref = fl(F), fl(F), fl(F * M.NKEYS), fl(F * M.NKEYS)
    eng.detect_async(slot_plane(wm, F), ME, 1, got)
    eng.detect_keys_async(slot_plane(wm, F), world["keys"], ME, 1, keys_got)
    eng.sync(1)
    plain.detect_async(y, ME, 0, ref)
    plain.detect_keys_async(y, world["keys"], ME, 0, keys_ref)
    plain.sync(0)
    assert eng.prof_report()["k_gram_ho"][0] == 1, "a detector behind the pair took the pair's sums"
    assert np.array_equal(u32(got), u32(ref)) and np.array_equal(u32(keys_got), u32(keys_ref)), (f32(got), f32(ref))
    assert f32(got)[1] != f32(corr)[1]
    eng.close(); plain.close()


# ---- B. scratch and arenas that grow while calls are queued -------------------------------------------------------------------------

def test_table_arenas_are_replaced_with_calls_still_queued(wm, tc):
    """800 un-synced wm_embed_signs + wm_detect_bits pairs on one slot, every call with a table of its own.  Each table takes 256 bytes
    of the slot's arenas (table_room in wm_api.hip rounds to 256), two tables per pair, 400 KiB in all.  wm.h does not state the
    arenas' first size: it is 65536 bytes in table_room (`need = max(2 * tab_bytes, bytes, 65536)`), doubled on every growth, and a
    replaced arena starts empty (the queued calls have run by then).  So the arenas are replaced twice with earlier calls still
    queued and undelivered: at pair 128 (64 KiB of tables; to 128 KiB) and at pair 384 (256 pairs more; to 256 KiB); the next
    replacement would fall at pair 896.  If that constant reaches 400 KiB this test no longer makes them grow and has to queue more.
    Every plane, strength and soft vector is the synchronous result for its pattern on a fresh engine, bit for bit."""
    torch = tc
    Rr, Cw, N, NB = 64, 256, 800, 4
    W = synth_watermark(Rr, Cw)
    ny, nx = wm.Watermark.tiles_shape(Rr, Cw, 32, 32)
    T = ny * nx
    assert T == 16
    prng = np.random.default_rng(7)
    signs = [prng.integers(-1, 2, T).astype(np.int8) for _ in range(4)]
    signs[0][:] = 1
    tbits = [prng.integers(-1, NB, T).astype(np.int32) for _ in range(4)]
    x = torch.from_numpy(synth_frame(Rr, Cw, frame=3, dtype=np.uint8)).cuda()
    # the synchronous results, one fresh engine
    fresh = wm.Watermark(Rr, Cw, W, 3, 40.0, nslots=1, max_frames=1)
    want = []
    for p in range(4):
        y, a = fresh.makeWatermarkSigns(x, x, 32, 32, signs[p].reshape(ny, nx), wm.MASK_TYPE.ME)
        _, soft = fresh.detectBits(y, 32, 32, tbits[p], NB, wm.MASK_TYPE.ME)
        want.append((y, np.float32(a), soft.copy()))
    fresh.close()
    eng = wm.Watermark(Rr, Cw, W, 3, 40.0, nslots=1, max_frames=1)
    out = torch.zeros((N, Rr, Cw), dtype=torch.uint8, device="cuda")   # 13 MB
    torch.cuda.synchronize()
    a = np.full(N, SENT_F, np.float32)
    st = np.full(N, SENT_I, np.int32)
    soft = np.full((N, NB), SENT_F, np.float32)
    st2 = np.full(N, SENT_I, np.int32)
    for i in range(N):
        p = i % 4
        eng.embed_signs_async(x, x, out[i], 32, 32, signs[p].copy(), wm.MASK_TYPE.ME, 0, a[i:i + 1], st[i:i + 1])
        eng.detect_bits_async(out[i], 32, 32, tbits[p].copy(), NB, wm.MASK_TYPE.ME, 0, soft[i], st2[i:i + 1])
    assert np.all(a == SENT_F) and np.all(st == SENT_I) and np.all(soft == SENT_F), "delivered before wm_sync"
    assert eng.sync(0) == wm.WM_OK
    assert not st.any() and not st2.any()
    for p in range(4):
        y, ap, sp = want[p]
        assert bool((out[p::4] == y[None]).all()), f"pattern {p}: a plane differs"
        assert np.array_equal(a[p::4].view(np.uint32), np.full(N // 4, ap, np.float32).view(np.uint32)), p
        assert np.array_equal(soft[p::4].view(np.uint32), np.broadcast_to(sp, (N // 4, NB)).copy().view(np.uint32)), p
    eng.close()


GROW_R, GROW_C = 96, 264
SMALL, LARGE = dict(F=1, th=48, K=2), dict(F=3, th=424, K=5)   # two 48-row segments; twelve 8-row segments (424 = 8 * 53)


@pytest.fixture(scope="module")
def grow_world(wm, tc):
    torch = tc
    x = torch.from_numpy(np.stack([synth_frame(GROW_R, GROW_C, frame=f) for f in range(3)])).cuda()
    banks = {2: wm.KeySet.from_seeds(GROW_R, GROW_C, [5, 6]), 5: wm.KeySet.from_seeds(GROW_R, GROW_C, [5, 6, 7, 8, 9])}
    torch.cuda.synchronize()
    yield dict(x=x, banks=banks, W=synth_watermark(GROW_R, GROW_C))
    for b in banks.values():
        b.close()


def grow_outputs(wm, torch, family, shape):
    """what one call of a family writes at the small or the large shape: host arrays and device tensors, holding sentinels"""
    F, th, K = shape["F"], shape["th"], shape["K"]
    ny, nx = wm.Watermark.tiles_shape(GROW_R, GROW_C, th, 32)
    full = lambda sh, dt=torch.float32: torch.full(sh, SENT_F, dtype=dt, device="cuda")
    out = dict(st=il(F))
    if family == "wm_detect_tiles":
        out.update(map=full((F, ny, nx)), sums=full((F, ny, nx, 3), torch.float64))
    elif family == "wm_detect_bits":
        out.update(soft=fl(F * 3))
    elif family == "wm_detect_keys_tiles":
        out.update(map=full((F, K, ny, nx)), sums=full((F, K, ny, nx, 3), torch.float64))
    elif family == "wm_detect_keys":
        out.update(corr=fl(F * K))
    else:
        out.update(a=fl(F * K), copies=full((F * K, GROW_R, GROW_C)))
    return out


def grow_call(wm, g, eng, family, shape, slot, out):
    """one call of a family at the small or the large shape into `out` (grow_outputs); enqueues only, nothing here waits"""
    F, th, K = shape["F"], shape["th"], shape["K"]
    x = g["x"][:F]
    ny, nx = wm.Watermark.tiles_shape(GROW_R, GROW_C, th, 32)
    ME = wm.MASK_TYPE.ME
    if family == "wm_detect_tiles":
        eng.detect_tiles_async(x, th, 32, ME, slot, out["map"], out["sums"], out["st"])
    elif family == "wm_detect_bits":
        eng.detect_bits_async(x, th, 32, (np.arange(ny * nx) % 3).astype(np.int32), 3, ME, slot, out["soft"], out["st"])
    elif family == "wm_detect_keys_tiles":
        eng.detect_keys_tiles_async(x, g["banks"][K], th, 32, ME, slot, out["map"], out["sums"], out["st"])
    elif family == "wm_detect_keys":
        eng.detect_keys_async(x, g["banks"][K], ME, slot, out["corr"], out["st"])
    else:
        eng.embed_keys_async(x, x, out["copies"], g["banks"][K], ME, slot, out["a"], out["st"])


@pytest.mark.parametrize("family", ["wm_detect_tiles", "wm_detect_bits", "wm_detect_keys_tiles", "wm_detect_keys", "wm_embed_keys"])
def test_record_scratch_grows_between_queued_calls(wm, tc, grow_world, family):
    """a call with a small need, one with a larger need, the small one again, on one slot with nothing between them that waits (every
    output is allocated and filled before the first call is queued): the second call replaces the slot's record / partial scratch
    with the first still queued, the third runs in the larger buffer.  All three are the isolated results (each call alone,
    synchronous, on an engine of its own), bit for bit"""
    torch = tc
    make = lambda: wm.Watermark(GROW_R, GROW_C, grow_world["W"], 3, 40.0, nslots=1, max_frames=3)
    shapes = (SMALL, LARGE, SMALL)
    eng = make()
    got = [grow_outputs(wm, torch, family, shape) for shape in shapes]
    want = [grow_outputs(wm, torch, family, shape) for shape in shapes]
    torch.cuda.synchronize()
    for o, shape in zip(got, shapes):
        grow_call(wm, grow_world, eng, family, shape, 0, o)
    for o in got:
        assert np.all(np.frombuffer(o["st"], np.int32) == SENT_I), "delivered before wm_sync"
    assert eng.sync(0) == wm.WM_OK
    eng.close()
    for o, w, shape in zip(got, want, shapes):
        iso = make()
        grow_call(wm, grow_world, iso, family, shape, wm.WM_SLOT_SYNC, w)
        for name, v in w.items():
            if isinstance(v, torch.Tensor):
                assert same_bits(torch, o[name], v), (family, shape, name)
            else:
                assert np.array_equal(u32(o[name]), u32(v)), (family, shape, name, list(o[name]), list(v))
        assert not np.frombuffer(w["st"], np.int32).any()
        iso.close()


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_staging_buffers_are_replaced_between_queued_calls(wm, tc, dtype):
    """host planes on one slot, no sync until the end: a one-frame embed and the detector of its WM_MEM_SLOT_OUT, then a three-frame
    embed (the staging buffers are replaced, and WM_MEM_SLOT_OUT moves with them), its detector, and an embed whose input is
    WM_MEM_SLOT_OUT and whose output lands in the same staging buffer (in place on the resolved planes: the snapshot).  Everything
    equals the same calls made one by one with syncs on a fresh engine, bit for bit; the last plane also equals the same embed run
    out of place on device planes"""
    torch = tc
    L = wm.lib()
    npdt, wdt, es = (np.float32, wm.WM_F32, 4) if dtype == "f32" else (np.uint8, wm.WM_U8, 1)
    W = synth_watermark(R, Cc)
    xs = np.stack([synth_frame(R, Cc, frame=f, dtype=npdt) for f in range(4)])
    n = R * Cc
    ctype = C.c_float if dtype == "f32" else C.c_uint8

    def pinned(frames):
        p = L.wm_host_alloc(frames * n * es)
        assert p
        return p, np.ctypeslib.as_array((ctype * (frames * n)).from_address(p)).reshape(frames, R, Cc)

    def run(eng, sync_each):
        bufs = dict(x1=pinned(1), y1=pinned(1), x3=pinned(3), y3=pinned(3), y5=pinned(3))
        bufs["x1"][1][:] = xs[:1]
        bufs["x3"][1][:] = xs[1:4]
        for k in ("y1", "y3", "y5"):
            bufs[k][1][:] = 0
        hp = lambda k, F: host_plane(wm, bufs[k][0], F, wdt)
        res = dict(a1=fl(1), c1=fl(1), a3=fl(3), c3=fl(3), a5=fl(3))
        calls = [
            lambda: L.wm_embed(eng._ctx, 0, C.byref(hp("x1", 1)), C.byref(hp("x1", 1)), C.byref(hp("y1", 1)), res["a1"], None, 0),
            lambda: L.wm_detect(eng._ctx, 0, C.byref(slot_plane(wm, 1, wdt)), res["c1"], None, 0),
            lambda: L.wm_embed(eng._ctx, 0, C.byref(hp("x3", 3)), C.byref(hp("x3", 3)), C.byref(hp("y3", 3)), res["a3"], None, 0),
            lambda: L.wm_detect(eng._ctx, 0, C.byref(slot_plane(wm, 3, wdt)), res["c3"], None, 0),
            lambda: L.wm_embed(eng._ctx, 0, C.byref(slot_plane(wm, 3, wdt)), C.byref(hp("x3", 3)), C.byref(hp("y5", 3)), res["a5"], None, 0),
        ]
        for call in calls:
            assert call() == 0, L.wm_last_error(eng._ctx)
            if sync_each:
                assert L.wm_sync(eng._ctx, 0) == 0
            else:
                assert all(np.all(f32(v) == SENT_F) for v in res.values()), "delivered before wm_sync"
        assert L.wm_sync(eng._ctx, 0) == 0
        out = {k: f32(v) for k, v in res.items()}
        for k in ("y1", "y3", "y5"):
            out[k] = bufs[k][1].copy()
        for p, _ in bufs.values():
            L.wm_host_free(p)
        return out

    make = lambda: wm.Watermark(R, Cc, W, 3, 40.0, nslots=1, max_frames=3)
    eng, fresh = make(), make()
    eng.set_fused(False); fresh.set_fused(False)
    got, want = run(eng, False), run(fresh, True)
    for k in want:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (dtype, k)
    assert not np.array_equal(got["y3"], xs[1:4]) and not np.array_equal(got["y5"], got["y3"])
    # the in-place embed through the slot, out of place on device planes
    y3 = torch.from_numpy(got["y3"]).cuda()
    x3 = torch.from_numpy(xs[1:4]).cuda()
    y5 = torch.empty_like(y3)
    a5 = fl(3)
    torch.cuda.synchronize()
    fresh.embed_async(y3, x3, y5, wm.MASK_TYPE.ME, 0, a5, None)
    fresh.sync(0)
    assert np.array_equal(y5.cpu().numpy(), got["y5"]) and np.array_equal(f32(a5).view(np.uint32), got["a5"].view(np.uint32))
    eng.close(); fresh.close()


# ---- C. a synchronous call with work still queued on slot 0 -------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("call", ["wm_embed", "wm_detect", "wm_embed_detect"])
def test_a_synchronous_call_delivers_what_is_queued_on_slot_0(wm, tc, world, call, fused):
    """three asynchronous calls of different kinds queued on slot 0, then a one-frame WM_SLOT_SYNC call: it "runs on slot 0 and
    synchronises before returning" (wm.h), so the queued calls' results are delivered when it returns and are the isolated ones; its
    own result is the same call's on a fresh engine with the same fused setting; a following wm_sync(0) is WM_OK and changes nothing"""
    torch = tc
    L = wm.lib()
    ME = wm.MASK_TYPE.ME
    X = world["X"]

    def run(eng, queued):
        y2 = torch.full((2, R, Cc), SENT_F, device="cuda")
        tmap = torch.full((1, M.NY, M.NX), SENT_F, device="cuda")
        ys = torch.full((1, R, Cc), SENT_F, device="cuda")
        torch.cuda.synchronize()
        h = dict(a2=fl(2), st2=il(2), ck=fl(2 * M.NKEYS), stt=il(1), a=fl(1), corr=fl(1), st=il(1))
        slot = 0 if queued else wm.WM_SLOT_SYNC
        eng.embed_async(X[0:2], X[0:2], y2, ME, slot, h["a2"], h["st2"])
        eng.detect_keys_async(X[2:4], world["keys"], ME, slot, h["ck"], None)
        eng.detect_tiles_async(X[4:5], M.TILE, M.TILE, wm.MASK_TYPE.NVF, slot, tmap, None, h["stt"])
        if queued:
            assert all(undelivered({k: h[k]}) for k in ("a2", "ck")) and undelivered(dict(st=h["st2"])) and undelivered(dict(st=h["stt"]))
        px, py = wm.plane_of(X[5:6]), wm.plane_of(ys)
        if call == "wm_embed":
            rc = L.wm_embed(eng._ctx, 0, C.byref(px), C.byref(px), C.byref(py), h["a"], h["st"], wm.WM_SLOT_SYNC)
        elif call == "wm_detect":
            rc = L.wm_detect(eng._ctx, 0, C.byref(px), h["corr"], h["st"], wm.WM_SLOT_SYNC)
        else:
            rc = L.wm_embed_detect(eng._ctx, 0, C.byref(px), C.byref(px), C.byref(py), h["a"], h["corr"], h["st"], wm.WM_SLOT_SYNC)
        assert rc == 0, L.wm_last_error(eng._ctx)
        # delivered now, not at the wm_sync below
        snap = {k: u32(v) for k, v in h.items()}
        planes = [t.clone() for t in (y2, tmap, ys)]
        torch.cuda.synchronize()
        assert L.wm_sync(eng._ctx, 0) == wm.WM_OK
        torch.cuda.synchronize()
        assert all(np.array_equal(snap[k], u32(v)) for k, v in h.items()), "wm_sync after a synchronous call changed a result"
        assert all(same_bits(torch, p, t) for p, t in zip(planes, (y2, tmap, ys)))
        return snap, planes

    def engine():
        e = wm.Watermark(R, Cc, world["W"], 3, 40.0, nslots=1, max_frames=2)
        e.set_fused(fused)
        assert e.fused_info()[0] == fused
        return e

    eng, iso = engine(), engine()
    got, got_planes = run(eng, True)
    want, want_planes = run(iso, False)
    delivered = ("a2", "st2", "ck", "stt") + {"wm_embed": ("a", "st"), "wm_detect": ("corr", "st"), "wm_embed_detect": ("a", "corr", "st")}[call]
    for k in delivered:
        assert not np.array_equal(got[k], u32(fl(len(got[k]))) if k not in ("st", "st2", "stt") else u32(il(len(got[k])))), ("not delivered", k)
        assert np.array_equal(got[k], want[k]), (call, fused, k, got[k].view(np.float32), want[k].view(np.float32))
    for p, q in zip(got_planes, want_planes):
        assert same_bits(torch, p, q)
    for e in (eng, iso):
        assert e.fused_info()[3] == 0 and L.wm_fused_lock_skips(e._ctx) == 0
    eng.close(); iso.close()
