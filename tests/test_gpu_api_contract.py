"""What the host layer of the C ABI (wm_api.hip) promises around its kernels, recorded so that a change to how the entry points
share their front halves cannot move it: which of two simultaneous argument faults a call reports, and that one wm_sync
delivers the records of every kind of queued call exactly as the synchronous calls return them."""
import ctypes as C

import numpy as np
import pytest

import hard_frames as H
import oracle_lib as O
from synth import synth_frame, synth_watermark

pytestmark = pytest.mark.gpu

R, CC, F, K = 40, 264, 2, 3
KEY_R, KEY_C = 42, 268  # the larger key plane of wm_detect_offsets
W_SEED = 9300


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- which of two faults is reported --------------------------------------------------------------------------------------
# fault -> (return code, a piece of wm_last_error no other fault of the same call produces)
def _faults(wm):
    bad = wm.WM_ERR_BAD_ARG
    return {"mask": (bad, b"bad mask type"), "me_p": (wm.WM_ERR_BAD_P, b"ME mask needs p == 3"), "slot": (bad, b"bad slot"),
            "shape": (bad, b"engine was initialised for"), "dtype_pair": (bad, b"same dtype"), "dtype": (bad, b"bad dtype"),
            "mask_out": (bad, b"mask_out must be"), "bank": (bad, b"the key bank is"), "tile": (bad, b"tile shape"),
            "key": (bad, b"of a bank of"), "window": (bad, b"leave the"), "band": (bad, b"not in band mode")}


# the order in which each entry point looks at its arguments: of the faults present, the first one listed is reported
# ("me_p": the ME mask on an engine with p != 3; "dtype_pair": in_gray f32 with a u8 base and out; "dtype": a plane whose dtype
# is no dtype; "mask_out": a u8 mask plane; "band": the engine in band mode (wm_band_configure), which these calls refuse)
ORDER = {
    "wm_embed": ["mask", "me_p", "slot", "shape", "dtype_pair"],
    "wm_detect": ["mask", "me_p", "slot", "shape", "dtype"],
    "wm_detect_keys": ["mask", "me_p", "bank", "band", "slot", "shape", "dtype"],
    "wm_detect_offsets": ["mask", "me_p", "key", "bank", "window", "band", "slot", "shape", "dtype"],
    "wm_detect_tiles": ["tile", "mask", "me_p", "band", "slot", "shape", "dtype"],
    "wm_detect_keys_tiles": ["tile", "mask", "me_p", "bank", "band", "slot", "shape", "dtype"],
    "wm_embed_signs": ["tile", "mask", "me_p", "band", "slot", "shape", "dtype_pair"],
    "wm_embed_bits": ["tile", "mask", "me_p", "band", "slot", "shape", "dtype_pair"],
    "wm_detect_bits": ["tile", "mask", "me_p", "band", "slot", "shape", "dtype"],
    "wm_embed_keys": ["mask", "me_p", "bank", "band", "slot", "shape", "dtype_pair"],
    "wm_compute_mask": ["mask", "me_p", "slot", "shape", "mask_out"],
    "wm_band_stats": ["slot", "mask", "me_p", "shape", "dtype"],
    "wm_band_detect_sums": ["slot", "mask", "me_p", "shape", "dtype"],
}
COMMON = [{"mask", "slot"}, {"slot", "shape"}]
BAND = [{"mask", "band"}, {"band", "slot"}]  # (with p = 5 the first also sets "me_p" against "band")
PAIRS = {
    "wm_embed": COMMON + [{"shape", "dtype_pair"}],
    "wm_detect": COMMON + [{"shape", "dtype"}],
    "wm_detect_keys": COMMON + [{"shape", "dtype"}, {"bank", "slot"}] + BAND + [{"bank", "band"}],
    "wm_detect_offsets": COMMON + [{"shape", "dtype"}, {"bank", "slot"}, {"key", "window"}] + BAND + [{"window", "band"}],
    "wm_detect_tiles": COMMON + [{"shape", "dtype"}, {"tile", "mask"}] + BAND,
    "wm_detect_keys_tiles": COMMON + [{"shape", "dtype"}, {"tile", "mask"}, {"bank", "slot"}] + BAND + [{"bank", "band"}],
    "wm_embed_signs": COMMON + [{"shape", "dtype_pair"}, {"tile", "mask"}] + BAND,
    "wm_embed_bits": COMMON + [{"shape", "dtype_pair"}, {"tile", "mask"}] + BAND,
    "wm_detect_bits": COMMON + [{"shape", "dtype"}, {"tile", "mask"}] + BAND,
    "wm_embed_keys": COMMON + [{"shape", "dtype_pair"}, {"bank", "slot"}] + BAND + [{"bank", "band"}],
    "wm_compute_mask": COMMON + [{"shape", "mask_out"}],
    "wm_band_stats": COMMON + [{"shape", "dtype"}],
    "wm_band_detect_sums": COMMON + [{"shape", "dtype"}],
}


def _copy(wm, pl, **changes):
    q = wm.wm_plane.from_buffer_copy(pl)
    for k, v in changes.items():
        setattr(q, k, v)
    return q


def test_error_precedence(wm, tc):
    torch = tc
    L = wm.lib()
    W = synth_watermark(R, CC, W_SEED)
    x = synth_frame(R, CC, frame=1)
    xt = torch.from_numpy(x).cuda()
    x8 = xt.to(torch.uint8)
    yt, y8 = torch.empty_like(xt), torch.empty_like(x8)
    yk = torch.empty((K, R, CC), dtype=torch.float32, device="cuda")
    yk8 = torch.empty((K, R, CC), dtype=torch.uint8, device="cuda")
    mp = torch.zeros((1, CC // 32), dtype=torch.float32, device="cuda")
    mkp = torch.zeros((K, 1, CC // 32), dtype=torch.float32, device="cuda")
    NBITS = 2
    signs = np.ones(CC // 32, np.int8)  # one frame of 1 x 8 tiles
    tile_bit = wm.Watermark.bits_layout(1, CC // 32, NBITS, 5)
    payload = np.array([2], np.uint8)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)
    bank = wm.KeySet(R, CC, K)
    bank_other = wm.KeySet(R, CC - 4, K)      # not the engine's shape, and smaller than it
    bank_large = wm.KeySet(KEY_R, KEY_C, K)
    torch.cuda.synchronize()
    good, good8 = wm.plane_of(xt, 1), wm.plane_of(x8, 1)
    pout, pout8 = wm.plane_of(yt, 1), wm.plane_of(y8, 1)
    pk, pk8 = wm.plane_of(yk, 1), wm.plane_of(yk8, 1)
    dbuf = (C.c_double * 8)()
    fbuf = (C.c_float * (F * K * 4))()
    faults = _faults(wm)

    def call(ctx, name, mask, present):
        m = 7 if "mask" in present else mask
        slot = 9 if "slot" in present else 0
        pin = _copy(wm, good, cols=CC - 1) if "shape" in present else _copy(wm, good)
        if "dtype" in present:
            pin.dtype = 7
        pair8 = "dtype_pair" in present
        ref = C.byref
        tr = 36 if "tile" in present else 32
        if "band" in present:  # the whole plane as one band: band mode with no halo to ask for
            assert L.wm_band_configure(ctx, 0, R, R) == wm.WM_OK
            try:
                return call(ctx, name, mask, present - {"band"})
            finally:
                assert L.wm_band_configure(ctx, 0, 0, 0) == wm.WM_OK
        if name == "wm_embed":
            return L.wm_embed(ctx, m, ref(pin), ref(good8 if pair8 else good), ref(pout8 if pair8 else pout), fbuf, None, slot)
        if name == "wm_detect":
            return L.wm_detect(ctx, m, ref(pin), fbuf, None, slot)
        if name == "wm_detect_keys":
            return L.wm_detect_keys(ctx, m, ref(pin), (bank_other if "bank" in present else bank).handle, fbuf, None, slot)
        if name == "wm_detect_offsets":
            kb = bank_other if "bank" in present else bank_large
            return L.wm_detect_offsets(ctx, m, ref(pin), kb.handle, K + 2 if "key" in present else 1, 3 if "window" in present else 0, 0, 2, 2,
                                       fbuf, None, slot)
        if name == "wm_detect_tiles":
            return L.wm_detect_tiles(ctx, m, ref(pin), tr, 32, C.c_void_p(mp.data_ptr()), None, None, slot)
        if name == "wm_detect_keys_tiles":
            return L.wm_detect_keys_tiles(ctx, m, ref(pin), (bank_other if "bank" in present else bank).handle, tr, 32, C.c_void_p(mkp.data_ptr()), None,
                                          None, slot)
        if name == "wm_embed_signs":
            return L.wm_embed_signs(ctx, m, ref(pin), ref(good8 if pair8 else good), ref(pout8 if pair8 else pout), tr, 32, vp(signs), fbuf, None, slot)
        if name == "wm_embed_bits":
            return L.wm_embed_bits(ctx, m, ref(pin), ref(good8 if pair8 else good), ref(pout8 if pair8 else pout), tr, 32, vp(tile_bit), NBITS,
                                   vp(payload), fbuf, None, slot)
        if name == "wm_detect_bits":
            return L.wm_detect_bits(ctx, m, ref(pin), tr, 32, vp(tile_bit), NBITS, fbuf, None, slot)
        if name == "wm_embed_keys":
            return L.wm_embed_keys(ctx, m, ref(pin), ref(good8 if pair8 else good), (bank_other if "bank" in present else bank).handle,
                                   ref(pk8 if pair8 else pk), fbuf, None, slot)
        if name == "wm_compute_mask":
            return L.wm_compute_mask(ctx, m, ref(pin), ref(pout8 if "mask_out" in present else pout), None, fbuf, None, slot)
        if name == "wm_band_stats":
            return L.wm_band_stats(ctx, m, ref(pin), dbuf, slot)
        if name == "wm_band_detect_sums":
            return L.wm_band_detect_sums(ctx, m, ref(pin), dbuf, slot)
        raise AssertionError(name)

    checked = 0
    for p in (3, 5):
        eng = wm.Watermark(R, CC, W, p, 40.0, nslots=2, max_frames=2)
        for name, pairs in PAIRS.items():
            for pair in pairs:
                for mask in (0, 1):
                    present = set(pair)
                    if p != 3 and mask == 0 and "mask" not in present:
                        present.add("me_p")
                    first = next(f for f in ORDER[name] if f in present)
                    want_rc, want_text = faults[first]
                    rc = call(eng._ctx, name, mask, set(pair))
                    text = L.wm_last_error(eng._ctx)
                    assert rc == want_rc, (p, name, sorted(pair), mask, first, rc, text)
                    assert want_text in text, (p, name, sorted(pair), mask, first, text)
                    for other in present - {first}:
                        assert faults[other][1] not in text, (p, name, sorted(pair), mask, first, other, text)
                    checked += 1
        # nothing was queued, and the context still works
        assert eng.sync(0) == wm.WM_OK and eng.sync(1) == wm.WM_OK
        mt = wm.MASK_TYPE.ME if p == 3 else wm.MASK_TYPE.NVF
        y, a = eng.makeWatermark(xt, xt, mt)
        corr = eng.detectWatermark(y, mt)
        st, yo, ao = O.embed(x, x, W, p=p, mask=int(mt))
        assert st == 0 and abs(a - ao) <= 1e-4 * abs(ao) and float(np.abs(y.cpu().numpy() - yo).max()) <= 1e-3
        assert abs(corr - O.detect(y.cpu().numpy(), W, p=p, mask=int(mt))[1]) <= 1e-5
        eng.close()
    assert checked == 2 * 2 * sum(len(v) for v in PAIRS.values())
    for b in (bank, bank_other, bank_large):
        b.close()


# ---- one wm_sync behind every kind of queued call --------------------------------------------------------------------------
SENTINEL = -7.5
NBITS = 2


def _run_all(wm, torch, eng, mask, slot, inputs):
    """embed, detect of WM_MEM_SLOT_OUT, detect_keys, embed_keys, detect_offsets, detect_tiles, wm_compute_mask, detect_keys_tiles,
    detect_bits and embed_signs on `slot`; returns every buffer the calls deliver into (the caller syncs a real slot; WM_SLOT_SYNC
    has delivered on return)"""
    L = wm.lib()
    xt, bank, bank_large = inputs
    mt = wm.MASK_TYPE(mask)
    ny, nx = wm.Watermark.tiles_shape(R, CC, 32, 32)
    d = {
        "y": torch.zeros_like(xt), "a": (C.c_float * F)(*([SENTINEL] * F)), "a_st": (C.c_int * F)(*([-5] * F)),
        "corr": (C.c_float * F)(*([SENTINEL] * F)), "corr_st": (C.c_int * F)(*([-5] * F)),
        "ck": np.full((F, K), SENTINEL, np.float32), "ck_st": np.full(F, -5, np.int32),
        "yk": torch.zeros((F * K, R, CC), dtype=torch.float32, device="cuda"),
        "ak": np.full((F, K), SENTINEL, np.float32), "ak_st": np.full(F, -5, np.int32),
        "co": np.full((F, 2, 2), SENTINEL, np.float32), "co_st": np.full(F, -5, np.int32),
        "map": torch.zeros((F, ny, nx), dtype=torch.float32, device="cuda"),
        "sums": torch.zeros((F, ny, nx, 3), dtype=torch.float64, device="cuda"), "map_st": np.full(F, -5, np.int32),
        "m": torch.zeros_like(xt), "e": torch.zeros_like(xt),
        "coef": (C.c_float * (8 * F))(*([SENTINEL] * (8 * F))), "coef_st": (C.c_int * F)(*([-5] * F)),
        "kmap": torch.zeros((F, K, ny, nx), dtype=torch.float32, device="cuda"),
        "ksums": torch.zeros((F, K, ny, nx, 3), dtype=torch.float64, device="cuda"), "kmap_st": np.full(F, -5, np.int32),
        "soft": np.full((F, NBITS), SENTINEL, np.float32), "soft_st": np.full(F, -5, np.int32),
        "ys": torch.zeros_like(xt), "as": np.full(F, SENTINEL, np.float32), "as_st": np.full(F, -5, np.int32),
    }
    tile_bit = wm.Watermark.bits_layout(ny, nx, NBITS, 5)
    signs = np.where(np.arange(F * ny * nx) % 3 == 0, -1, 1).astype(np.int8)
    torch.cuda.synchronize()
    slot_plane = wm.wm_plane(None, R, CC, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, CC, 0, R * CC)
    eng.embed_async(xt, xt, d["y"], mt, slot, d["a"], d["a_st"])
    eng.detect_async(slot_plane, mt, slot, d["corr"], d["corr_st"])
    eng.detect_keys_async(d["y"], bank, mt, slot, d["ck"], d["ck_st"])
    eng.embed_keys_async(xt, xt, d["yk"], bank, mt, slot, d["ak"], d["ak_st"])
    eng.detect_offsets_async(d["y"], bank_large, 1, 0, 0, 2, 2, mt, slot, d["co"], d["co_st"])
    eng.detect_tiles_async(d["y"], 32, 32, mt, slot, d["map"], d["sums"], d["map_st"])
    pin, pm, pe = wm.plane_of(xt, 1), wm.plane_of(d["m"], 1), wm.plane_of(d["e"], 1)
    rc = L.wm_compute_mask(eng._ctx, mask, C.byref(pin), C.byref(pm), C.byref(pe), d["coef"], d["coef_st"], slot)
    assert rc >= 0, L.wm_last_error(eng._ctx)
    eng.detect_keys_tiles_async(d["y"], bank, 32, 32, mt, slot, d["kmap"], d["ksums"], d["kmap_st"])
    eng.detect_bits_async(d["y"], 32, 32, tile_bit, NBITS, mt, slot, d["soft"], d["soft_st"])
    eng.embed_signs_async(xt, xt, d["ys"], 32, 32, signs, mt, slot, d["as"], d["as_st"])
    return d


def _bits(v):
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    return np.ascontiguousarray(np.asarray(v)).view(np.uint8).ravel()


@pytest.mark.parametrize("mask", [0, 1])
def test_mixed_queue_delivers_like_sync(wm, tc, mask):
    """Ten calls of ten kinds queued on one slot, frame 1 a flat frame, then ONE wm_sync: every value, status, coefficient and
    plane equals, bit for bit, what the same calls deliver when each is made with WM_SLOT_SYNC on a fresh engine.  Under ME the
    flat frame is unsolvable for every call and its strengths (single and all K) keep their sentinel; under NVF it is solvable
    for the embed-side calls and unsolvable for the detectors, which solve the prediction system under either mask"""
    torch = tc
    W = synth_watermark(R, CC, W_SEED + 1)
    xs = np.stack([synth_frame(R, CC, frame=3), H.flat(R, CC, 77.0)])
    xt = torch.from_numpy(xs).cuda()
    bank = wm.KeySet(R, CC, K)
    bank_large = wm.KeySet(KEY_R, KEY_C, K)
    for k in range(K):
        bank.set(k, W if k == 1 else synth_watermark(R, CC, W_SEED + 10 + k))
        big = synth_watermark(KEY_R, KEY_C, W_SEED + 20 + k)
        if k == 1:
            big[1:1 + R, 1:1 + CC] = W  # the engine's W at offset (1, 1)
        bank_large.set(k, big)
    inputs = (xt, bank, bank_large)
    queued_eng = wm.Watermark(R, CC, W, 3, 40.0, nslots=2, max_frames=F)
    got = _run_all(wm, torch, queued_eng, mask, 0, inputs)
    assert list(got["a_st"]) == [-5] * F and list(got["coef"])[:2] == [SENTINEL] * 2  # nothing is delivered before the sync
    rc = queued_eng.sync(0)
    sync_eng = wm.Watermark(R, CC, W, 3, 40.0, nslots=2, max_frames=F)
    want = _run_all(wm, torch, sync_eng, mask, wm.WM_SLOT_SYNC, inputs)
    torch.cuda.synchronize()
    for name in want:
        assert np.array_equal(_bits(got[name]), _bits(want[name])), (name, got[name], want[name])
    # the statuses come from the CPU oracle.  The embed-side calls solve the prediction system under ME only, so the flat frame is
    # unsolvable there under ME and fine under NVF (strength +inf, output = base).  Every detector solves it whatever the mask
    # (Watermark.cpp:234-250), so the flat frame of the embed's output is unsolvable for the four detectors under NVF as well:
    # wm_sync reports WM_UNSOLVABLE under both masks
    y = got["y"].cpu().numpy()
    embed_st = [O.embed(xs[f], xs[f], W, mask=mask)[0] for f in range(F)]
    detect_st = [O.detect(y[f], W, mask=mask)[0] for f in range(F)]
    assert embed_st == ([0, 1] if mask == 0 else [0, 0]) and detect_st == [0, 1]
    for name in ("a_st", "ak_st", "coef_st"):
        assert list(got[name]) == embed_st, (name, list(got[name]))
    for name in ("corr_st", "ck_st", "co_st", "map_st"):
        assert list(got[name]) == detect_st, (name, list(got[name]))
    assert list(got["as_st"]) == embed_st and list(got["kmap_st"]) == detect_st and list(got["soft_st"]) == detect_st
    assert rc == wm.WM_UNSOLVABLE
    assert got["corr"][1] == 0.0 and np.all(got["ck"][1] == 0.0) and np.all(got["co"][1] == 0.0)  # detectors deliver 0
    if mask == 0:
        assert got["a"][1] == SENTINEL and np.all(got["ak"][1] == SENTINEL)  # embeds keep the caller's value
        assert got["as"][1] == SENTINEL
    else:
        assert np.isinf(got["a"][1]) and np.all(np.isinf(got["ak"][1]))  # solvable, no energy: the oracle's +inf is delivered
    assert got["a"][0] != SENTINEL and np.all(got["ak"][0] != SENTINEL) and np.all(got["ck"][0] != SENTINEL)
    assert got["as"][0] != SENTINEL and np.all(got["soft"][0] != SENTINEL) and np.all(got["soft"][1] == 0.0)
    # the marked frame answers to key 1, the engine's W (an unmarked frame of this size scores about 1 / sqrt(R CC) = 0.01)
    print("mask", mask, "a", got["a"][0], "corr", got["corr"][0], "keys", got["ck"][0], "offsets", got["co"][0].ravel())
    assert float(got["corr"][0]) > 0.1 and float(got["ck"][0, 1]) > 0.1 and float(got["co"][0, 1, 1]) > 0.1
    queued_eng.close()
    sync_eng.close()
    bank.close()
    bank_large.close()
