"""One run of every call family on one engine, and the oracle's answer to it (no tests in here).

battery(wm, torch, eng, shape, ...) calls every family of include/wm.h once on the engine it is handed, at small fixed inputs, and
returns {name: numpy array} of everything the calls return: output planes, strengths and statuses of the writing calls; scores, maps,
sums and soft values of the detectors; masks and coefficients.  It reads nothing from the engine but what it is told (shape, p, the
largest batch F, the slot to queue on), so two engines in the same configuration X = (shape, W, p, psnr, slots, max_frames, rps, fused
mode, hand-over settings) give the same dict BIT FOR BIT however they got there: the geometry and the reduction order follow from X
alone (tests/test_gpu_lifecycle.py compares a reconfigured engine with one created in X).

expectations(shape, ...) is the CPU oracle's answer for the same names, each with the KIND of comparison the suite already uses for it
(TOLERANCES names where each number is taken from; none is new).  check(got, want) applies them.

The transition lists at the end are data; coverage() counts transition kind x family as test_gpu_layouts.coverage() counts layouts."""
import ctypes as C

import numpy as np

import bits_model as BM
import depth_model as D
import oracle_lib as O
import select_model as SM
import tiles_model as TM
from synth import synth_frame, synth_watermark

TH = TW = 32                      # tiles
K = 3
SEEDS = [7001, 7032, 7063]        # the key banks of tests/test_gpu_layouts.py
TABLE_SEED = 4242                 # ... and the seed of its tile tables
NBITS, LAYOUT_SEED = 5, 99
NCOPIES = 3
BITS16 = 10
OFFSETS = (1, 0, 0, 2, 3)         # wm_detect_offsets: key k, oy0, ox0, ny, nx
KEY_PAD = (1, 2)                  # the offsets bank is that much larger than the frame
SCHEDULE_SEED = 0x5E1EC7
MAX_F = 3
W2_SEED = 9100                    # "same shape, new W"

# kind of comparison -> (number, where the suite takes it from)
TOLERANCES = {
    "a": (1e-4, "relative; test_gpu_parity.py TOL_A"),
    "y": (1e-3, "absolute; test_gpu_parity.py TOL_Y"),
    "u8": (1e-3, "within 1 LSB on at most this share of the pixels; test_gpu_layouts.py u8_rule"),
    "score": (1e-5, "absolute, NaN in the same places; test_gpu_parity.py TOL_CORR, test_gpu_tiles.py / test_gpu_bits.py TOL"),
    "gram": (1e-13, "relative; test_gpu_parity.py test_gram_exact"),
    "coef": (1e-4, "absolute; test_gpu_parity.py TOL_C"),
    "mask_me": (1e-4, "absolute; test_gpu_parity.py test_coefficients_and_me_mask"),
    "sumsq": (1e-5, "relative, the two sums of squares of a tile; test_gpu_tiles.py"),
    "exact": (0, "raw bytes: u8 Gram sums, the 16-bit conversions against depth_model, grey, NVF masks, statuses"),
    "none": (None, "no oracle figure in the suite for it: held by the bit-for-bit comparison between engines only"),
}

FAMILIES = ("wm_embed", "wm_detect", "wm_embed_detect", "wm_compute_mask", "wm_gram", "wm_detect_keys", "wm_embed_keys", "wm_detect_offsets",
            "wm_detect_tiles", "wm_detect_keys_tiles", "wm_embed_signs", "wm_embed_bits", "wm_detect_bits", "wm_embed_signs_multi",
            "wm_embed_select", "wm_detect_select", "wm_rgb2gray", "wm_unpack_rgb8", "wm_pack_rgb8", "wm_unpack16", "wm_pack16", "wm_embed16",
            "wm_detect16", "host planes", "WM_MEM_SLOT_OUT")


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def masks_of(p):
    return ("ME", "NVF") if p == 3 else ("NVF",)


# ---- the fixed inputs (computed once per shape and left unchanged) -----------------------------------------------------------------

_INPUTS = {}


def watermark_of(shape, seed=None):
    return synth_watermark(*shape) if seed is None else synth_watermark(shape[0], shape[1], seed=seed)


def inputs(shape, w_seed=None):
    """synthetic frames of tests/synth.py: x / xu [3, R, C] f32 and u8, rgb / rgbu [3 channels, R, C], marked / markedu: frames that
    carry the engine's W (the oracle's ME embed, so the detectors see a real score), x16 / m16: 10-bit samples of x and of marked"""
    key = (shape, w_seed)
    if key not in _INPUTS:
        R, Cc = shape
        W = watermark_of(shape, w_seed)
        I = {"W": W}
        for dt, npdt in (("f32", np.float32), ("u8", np.uint8)):
            I["x" + dt] = np.stack([synth_frame(R, Cc, frame=f, dtype=npdt) for f in range(MAX_F)])
            I["rgb" + dt] = np.stack([synth_frame(R, Cc, frame=60 + 10 * ch, dtype=npdt) for ch in range(3)])
        I["markedf32"] = np.stack([O.embed(x, x, W)[1] for x in (synth_frame(R, Cc, frame=20 + f) for f in range(MAX_F))])
        I["markedu8"] = np.stack([O.embed_u8(x, W)[1] for x in (synth_frame(R, Cc, frame=20 + f, dtype=np.uint8) for f in range(MAX_F))])
        I["x16"] = D.quantise(I["xf32"], BITS16)
        I["m16"] = D.quantise(I["markedf32"], BITS16)
        I["packed"] = np.ascontiguousarray(I["rgbu8"].transpose(1, 2, 0))
        for v in I.values():
            v.setflags(write=False)
        _INPUTS[key] = I
    return _INPUTS[key]


def tables(shape, F, seed=TABLE_SEED):
    """the tile tables, seeded as in tests/test_gpu_layouts.py tables_for: signs [F, ny, nx], copies' signs [F, NCOPIES, ny, nx],
    tile_bit [T] with one unmarked tile where there are more than three, payload [F, 1], and the key schedule [F]"""
    ny, nx = TM.tiles_shape(shape[0], shape[1], TH, TW)
    T = ny * nx
    rng = np.random.default_rng(seed)
    nbits = min(NBITS, T)
    tb = BM.layout(ny, nx, nbits, LAYOUT_SEED).astype(np.int32)
    if T > 3:
        tb[3] = -1
    return {"signs": rng.integers(-1, 2, size=(F, ny, nx)).astype(np.int8),
            "multi": rng.integers(-1, 2, size=(F, NCOPIES, ny, nx)).astype(np.int8),
            "tile_bit": tb, "nbits": nbits, "payload": rng.integers(0, 256, size=(F, 1)).astype(np.uint8),
            "schedule": SM.schedule(K, SCHEDULE_SEED, 0, F)}


def banks(wm, shape):
    """(bank of the frame's shape, the larger bank of wm_detect_offsets): three keys from seeds"""
    R, Cc = shape
    return wm.KeySet.from_seeds(R, Cc, SEEDS), wm.KeySet.from_seeds(R + KEY_PAD[0], Cc + KEY_PAD[1], SEEDS)


def host_plane(wm, arr, channels=1):
    """a dense host array [R, C], [F, R, C] or [3, R, C] as a WM_MEM_HOST plane"""
    dt = wm.WM_F32 if arr.dtype == np.float32 else wm.WM_U8
    R, Cc = arr.shape[-2:]
    frames = arr.shape[0] if channels == 1 and arr.ndim == 3 else 1
    return wm.wm_plane(arr.ctypes.data, R, Cc, channels, dt, wm.WM_MEM_HOST, frames, Cc, R * Cc if channels > 1 else 0, R * Cc if frames > 1 else 0)


def slot_out_plane(wm, shape, F):
    return wm.wm_plane(None, shape[0], shape[1], 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, shape[1], 0, shape[0] * shape[1])


# ---- the battery -------------------------------------------------------------------------------------------------------------------

def battery(wm, torch, eng, shape, p=3, F=1, slot=0, keys=None, keys_big=None, w_seed=None):
    """every family once.  F: the engine's max_frames (the batched and queued calls carry F frames); slot: the slot the queued calls
    use.  keys / keys_big: banks(wm, shape), made here (and closed again) when not given"""
    R, Cc = shape
    I, T = inputs(shape, w_seed), tables(shape, F)
    own_banks = keys is None
    if own_banks:
        keys, keys_big = banks(wm, shape)
    SYNC = wm.WM_SLOT_SYNC
    out = {}

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def scal(n, per=1):
        return np.full((n, per) if per > 1 else n, np.nan, np.float32), np.full(n, -7, np.int32)

    def go(s, call, *args):
        """one library call on slot s (WM_SLOT_SYNC: it waits itself; else wm_sync of the slot delivers)"""
        torch.cuda.synchronize()
        call(*args)
        if s != SYNC:
            eng.sync(s)

    X = {dt: dev(I["x" + dt]) for dt in ("f32", "u8")}
    RGB = {dt: dev(I["rgb" + dt]) for dt in ("f32", "u8")}
    M = {dt: dev(I["marked" + dt]) for dt in ("f32", "u8")}

    def embed(name, mk, x, b, s):
        n = x.shape[0] if x.dim() == 3 else 1
        o = torch.zeros_like(b)
        a, st = scal(n)
        go(s, eng.embed_async, x, b, o, mk, s, fp(a), ip(st))
        out[name + ".y"], out[name + ".a"], out[name + ".st"] = host(o), a, st
        return o

    def detect(name, mk, img, s):
        n = img.shape[0] if img.dim() == 3 else 1
        c, st = scal(n)
        go(s, eng.detect_async, img, mk, s, fp(c), ip(st))
        out[name + ".corr"], out[name + ".st"] = c, st

    for m in masks_of(p):
        mk = wm.MASK_TYPE[m]
        # wm_embed: one frame synchronously (the fused kernels where the engine takes them), F frames queued on a slot
        for dt in ("f32", "u8"):
            embed(f"embed/{m}/{dt}/grey/F1", mk, X[dt][0], X[dt][0], SYNC)
            embed(f"embed/{m}/{dt}/rgb/F1", mk, X[dt][0], RGB[dt], SYNC)
        embed(f"embed/{m}/f32/grey/Fq", mk, X["f32"][:F], X["f32"][:F], slot)
        embed(f"embed/{m}/u8/rgb/Fq", mk, X["u8"][:F], torch.stack([RGB["u8"]] * F), slot)
        # wm_detect
        for dt in ("f32", "u8"):
            detect(f"detect/{m}/{dt}/F1", mk, M[dt][0], SYNC)
        detect(f"detect/{m}/f32/Fq", mk, M["f32"][:F], slot)
        detect(f"detect/{m}/u8/Fq", mk, M["u8"][:F], slot)
        # wm_embed_detect
        y, a, c = eng.makeAndDetect(X["f32"][1], X["f32"][1], mk)
        out[f"embed_detect/{m}.y"], out[f"embed_detect/{m}.a"], out[f"embed_detect/{m}.corr"] = host(y), np.float32([a]), np.float32([c])
        # wm_compute_mask
        mm, e, coef, st = eng.computeMask(X["f32"][:F], mk, want_error_sequence=(m == "ME"))
        out[f"compute_mask/{m}.m"], out[f"compute_mask/{m}.coef"], out[f"compute_mask/{m}.st"] = host(mm), coef, np.int32(st)
        if m == "ME":
            out[f"compute_mask/{m}.e"] = host(e)
        # the key banks
        for dt in ("f32", "u8"):
            out[f"detect_keys/{m}/{dt}.corr"] = eng.detectKeys(M[dt][:F], keys, mk)
        copies, ak = eng.makeWatermarkKeys(X["f32"][:F], X["f32"][:F], keys, mk)
        out[f"embed_keys/{m}.y"], out[f"embed_keys/{m}.a"] = host(copies), ak
        k, oy0, ox0, ny, nx = OFFSETS
        out[f"detect_offsets/{m}.corr"] = eng.detectOffsets(M["f32"][:F], keys_big, k, oy0, ox0, ny, nx, mk)
        # the tile maps
        for dt in ("f32", "u8"):
            tm, ts = eng.detectTiles(M[dt][:F], TH, TW, mk, sums=True)
            out[f"detect_tiles/{m}/{dt}.map"], out[f"detect_tiles/{m}/{dt}.sums"] = tm, ts
        tm, ts = eng.detectKeysTiles(M["f32"][:F], keys, TH, TW, mk, sums=True)
        out[f"detect_keys_tiles/{m}.map"], out[f"detect_keys_tiles/{m}.sums"] = tm, ts
        # the payload calls
        o = torch.zeros_like(X["f32"][:F])
        a, st = scal(F)
        go(slot, eng.embed_signs_async, X["f32"][:F], X["f32"][:F], o, TH, TW, T["signs"], mk, slot, a, st)
        out[f"embed_signs/{m}.y"], out[f"embed_signs/{m}.a"], out[f"embed_signs/{m}.st"] = host(o), a, st
        o = torch.zeros_like(X["u8"][:F])
        a, st = scal(F)
        go(SYNC, eng.embed_bits_async, X["u8"][:F], X["u8"][:F], o, TH, TW, T["tile_bit"], T["nbits"], T["payload"], mk, SYNC, a, st)
        out[f"embed_bits/{m}.y"], out[f"embed_bits/{m}.a"], out[f"embed_bits/{m}.st"] = host(o), a, st
        soft, st = np.full((F, T["nbits"]), np.nan, np.float32), np.full(F, -7, np.int32)
        go(slot, eng.detect_bits_async, M["f32"][:F], TH, TW, T["tile_bit"], T["nbits"], mk, slot, soft, st)
        out[f"detect_bits/{m}.soft"], out[f"detect_bits/{m}.st"] = soft, st
        copies, a = eng.makeWatermarkSignsMulti(X["f32"][:F], X["f32"][:F], TH, TW, T["multi"], mk)
        out[f"embed_signs_multi/{m}.y"], out[f"embed_signs_multi/{m}.a"] = host(copies), a
        # a key per frame
        o = torch.zeros_like(X["f32"][:F])
        a, st = scal(F)
        go(slot, eng.embed_select_async, X["f32"][:F], X["f32"][:F], o, keys, T["schedule"], mk, slot, a, st)
        out[f"embed_select/{m}.y"], out[f"embed_select/{m}.a"], out[f"embed_select/{m}.st"] = host(o), a, st
        c, st = scal(F)
        go(SYNC, eng.detect_select_async, M["f32"][:F], keys, T["schedule"], mk, SYNC, c, st)
        out[f"detect_select/{m}.corr"], out[f"detect_select/{m}.st"] = c, st
        # 16-bit samples
        y16, a = eng.makeWatermark16(np.array(I["x16"][:F]), BITS16, mk)
        out[f"embed16/{m}.y"], out[f"embed16/{m}.a"] = y16, np.float32([np.nan if v is None else v for v in a])
        out[f"detect16/{m}.corr"] = np.float32(eng.detectWatermark16(np.array(I["m16"][:F]), BITS16, mk))
        # all three planes in host memory: the staging buffers
        hx, hb, ho = np.array(I["xf32"][2]), np.array(I["rgbf32"]), np.zeros((3, R, Cc), np.float32)
        px, pb, po = host_plane(wm, hx), host_plane(wm, hb, 3), host_plane(wm, ho, 3)
        a, st = scal(1)
        go(slot, eng.embed_async, px, pb, po, mk, slot, fp(a), ip(st))
        out[f"host/{m}.y"], out[f"host/{m}.a"], out[f"host/{m}.st"] = ho, a, st
        # an embed, then the detector of its output: by the slot's WM_MEM_SLOT_OUT, and by the output's pointer
        o = torch.zeros_like(X["f32"][:F])
        a, st = scal(F)
        c, cst = scal(F)
        c2, cst2 = scal(F)
        torch.cuda.synchronize()
        eng.embed_async(X["f32"][:F], X["f32"][:F], o, mk, slot, fp(a), ip(st))
        eng.detect_async(slot_out_plane(wm, shape, F), mk, slot, fp(c), ip(cst))
        eng.sync(slot)
        eng.embed_async(X["f32"][:F], X["f32"][:F], o, mk, slot, fp(a), ip(st))
        eng.detect_async(o, mk, slot, fp(c2), ip(cst2))
        eng.sync(slot)
        out[f"slot_out/{m}.corr"], out[f"slot_out/{m}.st"], out[f"slot_out/{m}.corr_ptr"], out[f"slot_out/{m}.st_ptr"] = c, cst, c2, cst2

    # the calls without a mask
    for dt in ("f32", "u8"):
        out[f"gram/{dt}.tot"] = eng.gram_totals(X[dt][:F])
        out[f"rgb2gray/{dt}.gray"] = host(eng.rgb2gray(RGB[dt]))
    rgb, g = eng.unpackRgb8(dev(I["packed"]), torch.float32)
    out["unpack_rgb8.rgb"], out["unpack_rgb8.gray"] = host(rgb), host(g)
    out["pack_rgb8.packed"] = host(eng.packRgb8(RGB["f32"]))
    out["unpack16.x"] = host(eng.unpack16(np.array(I["x16"][:F]), BITS16))
    out["pack16.v"] = eng.pack16(X["f32"][:F], BITS16)
    torch.cuda.synchronize()
    if own_banks:
        keys.close()
        keys_big.close()
    return {k: np.array(v) for k, v in out.items()}


def band_battery(wm, torch, engs, shape, world=2):
    """the two-band construction of tests/test_gpu_bands.py test_band_building_blocks on banded engines the caller made (engs: one per
    band, created on the band's rows with their halo and band_configure'd): Gram totals, wm_band_stats, wm_band_embed and
    wm_band_detect_sums of both bands under both masks"""
    import importlib
    bands = importlib.import_module("watermarking-gpu_amd.bands")
    R, Cc = shape
    xd = torch.from_numpy(np.array(inputs(shape)["xf32"][0])).cuda()
    out = {}
    spans = [bands.band_with_halo(R, r, world) for r in range(world)]
    views = [xd[g0:g1].contiguous() for g0, g1, lo, hi in spans]
    tots = [e.gram_totals(v) for e, v in zip(engs, views)]
    tot = sum(tots)
    for m in ("ME", "NVF"):
        mk = wm.MASK_TYPE[m]
        for r, (e, v) in enumerate(zip(engs, views)):
            out[f"band{r}/gram"] = tots[r]
            out[f"band{r}/{m}.solve"] = np.int32([e.band_solve(tot)])
        st = [e.band_stats(v, mk) for e, v in zip(engs, views)]
        mx, ss = max(s[0] for s in st), sum(s[1] for s in st)
        for r, (e, v) in enumerate(zip(engs, views)):
            o = v.clone()
            a = e.band_embed(v, v, o, mk, mx, ss)
            torch.cuda.synchronize()
            out[f"band{r}/{m}.stats"], out[f"band{r}/{m}.y"], out[f"band{r}/{m}.a"] = np.float64(st[r]), o.cpu().numpy(), np.float32([a])
            out[f"band{r}/{m}.sums"] = np.float64(e.band_detect_sums(v, mk))
    return {k: np.array(v) for k, v in out.items()}


def banded_engines(wm, shape, W, make, world=2):
    """world engines on the row bands of `shape` with their halo rows: make(rows, cols, W_band) creates one, band_configure is applied"""
    import importlib
    bands = importlib.import_module("watermarking-gpu_amd.bands")
    engs = []
    for r in range(world):
        g0, g1, lo, hi = bands.band_with_halo(shape[0], r, world)
        e = make(g1 - g0, shape[1], np.ascontiguousarray(W[g0:g1]))
        e.band_configure(lo, hi, shape[0])
        engs.append(e)
    return engs


# ---- the oracle's answer -----------------------------------------------------------------------------------------------------------

def expectations(shape, p=3, F=1, key_planes=None, key_planes_big=None, w_seed=None):
    """{name: (kind, array)} for every name battery() returns.  key_planes / key_planes_big: the banks' planes as numpy arrays (a bank
    from seeds is generated on the device: download them with KeySet.plane); default host-made stand-ins, for the CPU tests"""
    R, Cc = shape
    I, T = inputs(shape, w_seed), tables(shape, F)
    W = I["W"]
    if key_planes is None:
        key_planes = [synth_watermark(R, Cc, seed=s) for s in SEEDS]
        key_planes_big = [synth_watermark(R + KEY_PAD[0], Cc + KEY_PAD[1], seed=s) for s in SEEDS]
    want = {}
    x, xu, m32, mu = I["xf32"], I["xu8"], I["markedf32"], I["markedu8"]

    def emb(name, omk, gray, base, Wk=W, u8=False, st_name=True):
        """the oracle's embed of a batch: gray [n, R, C], base [n, R, C] or [n, 3, R, C]"""
        ys, as_, sts = [], [], []
        for f in range(len(gray)):
            st, y, a = O.embed(gray[f].astype(np.float32), base[f].astype(np.float32), Wk, p=p, mask=omk)
            ys.append(y.astype(np.uint8) if u8 else y)
            as_.append(a)
            sts.append(st)
        want[name + ".y"] = ("u8" if u8 else "y", np.stack(ys))
        want[name + ".a"] = ("a", np.float32(as_))
        if st_name:
            want[name + ".st"] = ("exact", np.int32(sts))
        return np.stack(ys)

    def det(img, Wk, omk):
        return np.float32([O.detect(np.asarray(v, np.float32), Wk, p=p, mask=omk)[1] for v in img])

    for m in masks_of(p):
        omk = O.MASK_ME if m == "ME" else O.MASK_NVF
        zeros = np.zeros(F, np.int32)
        for dt, xs in (("f32", x), ("u8", xu)):
            u8 = dt == "u8"
            emb(f"embed/{m}/{dt}/grey/F1", omk, xs[:1], xs[:1], u8=u8)
            emb(f"embed/{m}/{dt}/rgb/F1", omk, xs[:1], I["rgb" + dt][None], u8=u8)
            want[f"embed/{m}/{dt}/grey/F1.y"] = (want[f"embed/{m}/{dt}/grey/F1.y"][0], want[f"embed/{m}/{dt}/grey/F1.y"][1][0])
            want[f"embed/{m}/{dt}/rgb/F1.y"] = (want[f"embed/{m}/{dt}/rgb/F1.y"][0], want[f"embed/{m}/{dt}/rgb/F1.y"][1][0])
        emb(f"embed/{m}/f32/grey/Fq", omk, x[:F], x[:F])
        emb(f"embed/{m}/u8/rgb/Fq", omk, xu[:F], np.stack([I["rgbu8"]] * F), u8=True)
        for dt, ms in (("f32", m32), ("u8", mu)):
            want[f"detect/{m}/{dt}/F1.corr"], want[f"detect/{m}/{dt}/F1.st"] = ("score", det(ms[:1], W, omk)), ("exact", zeros[:1])
            want[f"detect/{m}/{dt}/Fq.corr"], want[f"detect/{m}/{dt}/Fq.st"] = ("score", det(ms[:F], W, omk)), ("exact", zeros)
        yo = emb(f"embed_detect/{m}", omk, x[1:2], x[1:2], st_name=False)
        want[f"embed_detect/{m}.y"] = ("y", yo[0])
        want[f"embed_detect/{m}.corr"] = ("score", det(yo, W, omk))
        # masks and coefficients
        me = [O.me_mask(v) for v in x[:F]]
        want[f"compute_mask/{m}.coef"] = ("coef" if m == "ME" else "none", np.stack([r[1] for r in me]))
        want[f"compute_mask/{m}.st"] = ("exact" if m == "ME" else "none", np.int32([r[0] for r in me]))
        if m == "ME":
            want[f"compute_mask/{m}.m"] = ("mask_me", np.stack([r[3] for r in me]))
            want[f"compute_mask/{m}.e"] = ("none", np.stack([r[2] for r in me]))
        else:
            want[f"compute_mask/{m}.m"] = ("exact", np.stack([O.nvf_mask(v, p) for v in x[:F]]))
        # key banks
        for dt, ms in (("f32", m32), ("u8", mu)):
            want[f"detect_keys/{m}/{dt}.corr"] = ("score", np.stack([det(ms[:F], Wk, omk) for Wk in key_planes], axis=1))
        ys, as_ = [], []
        for k in range(K):
            ys.append(emb("tmp", omk, x[:F], x[:F], Wk=key_planes[k]))
            as_.append(want["tmp.a"][1])
        for n in ("tmp.y", "tmp.a", "tmp.st"):
            del want[n]
        want[f"embed_keys/{m}.y"], want[f"embed_keys/{m}.a"] = ("y", np.stack(ys, axis=1)), ("a", np.stack(as_, axis=1))
        k, oy0, ox0, ny, nx = OFFSETS
        big = key_planes_big[k]
        want[f"detect_offsets/{m}.corr"] = ("score", np.stack([np.stack([det(m32[:F], np.ascontiguousarray(big[oy0 + i:oy0 + i + R, ox0 + j:ox0 + j + Cc]), omk)
                                                                         for j in range(nx)], axis=1) for i in range(ny)], axis=1))
        # tile maps.  Under ME the library takes the sums with m = |e_w|: the oracle's mask is |e_w| / max|e_w|, so its <e_u,e_w> is
        # scaled by max|e_w| and its ||e_u||^2 by the square (wm.h wm_detect_tiles: the factor cancels in every score)
        def unscaled(v, sums):
            mx = float(O.me_mask(v.astype(np.float32))[4]) if m == "ME" else 1.0
            return sums * np.array([mx, mx * mx, 1.0])

        for dt, ms in (("f32", m32), ("u8", mu)):
            tm = [TM.tile_map(v.astype(np.float32), W, TH, TW, p=p, mask=omk) for v in ms[:F]]
            want[f"detect_tiles/{m}/{dt}.map"] = ("score", np.stack([r[1] for r in tm]))
            want[f"detect_tiles/{m}/{dt}.sums"] = ("sumsq", np.stack([unscaled(v, r[2]) for v, r in zip(ms[:F], tm)]))
        tm = [[TM.tile_map(v, Wk, TH, TW, p=p, mask=omk) for Wk in key_planes] for v in m32[:F]]
        want[f"detect_keys_tiles/{m}.map"] = ("score", np.stack([np.stack([r[1] for r in row]) for row in tm]))
        want[f"detect_keys_tiles/{m}.sums"] = ("sumsq", np.stack([np.stack([unscaled(v, r[2]) for r in row]) for v, row in zip(m32[:F], tm)]))
        # payload
        yp, ym = emb("tmp", omk, x[:F], x[:F]), emb("tmp2", omk, x[:F], x[:F], Wk=-W)
        a_w = want["tmp.a"][1]
        want[f"embed_signs/{m}.y"] = ("y", np.stack([BM.select(T["signs"][f], TH, TW, yp[f], ym[f], x[f]) for f in range(F)]).astype(np.float32))
        want[f"embed_signs/{m}.a"], want[f"embed_signs/{m}.st"] = ("a", a_w), ("exact", zeros)
        want[f"embed_signs_multi/{m}.y"] = ("y", np.stack([np.stack([BM.select(T["multi"][f, c], TH, TW, yp[f], ym[f], x[f]) for c in range(NCOPIES)])
                                                           for f in range(F)]).astype(np.float32))
        want[f"embed_signs_multi/{m}.a"] = ("a", a_w)
        ypu, ymu = emb("tmp", omk, xu[:F], xu[:F], u8=True), emb("tmp2", omk, xu[:F], xu[:F], Wk=-W, u8=True)
        want[f"embed_bits/{m}.y"] = ("u8", np.stack([BM.select(BM.signs_of(T["tile_bit"], T["payload"][f], T["nbits"]), TH, TW, ypu[f], ymu[f], xu[f])
                                                     for f in range(F)]).astype(np.uint8))
        want[f"embed_bits/{m}.a"], want[f"embed_bits/{m}.st"] = ("a", want["tmp.a"][1]), ("exact", zeros)
        for n in ("tmp.y", "tmp.a", "tmp.st", "tmp2.y", "tmp2.a", "tmp2.st"):
            del want[n]
        want[f"detect_bits/{m}.soft"] = ("score", np.stack([BM.soft(v, W, TH, TW, T["tile_bit"], T["nbits"], p=p, mask=omk)[1] for v in m32[:F]]))
        want[f"detect_bits/{m}.st"] = ("exact", zeros)
        # a key per frame
        ys, as_ = [], []
        for f in range(F):
            st, y, a = O.embed(x[f], x[f], key_planes[T["schedule"][f]], p=p, mask=omk)
            ys.append(y)
            as_.append(a)
        want[f"embed_select/{m}.y"], want[f"embed_select/{m}.a"], want[f"embed_select/{m}.st"] = ("y", np.stack(ys)), ("a", np.float32(as_)), ("exact", zeros)
        want[f"detect_select/{m}.corr"] = ("score", np.float32([det(m32[f:f + 1], key_planes[T["schedule"][f]], omk)[0] for f in range(F)]))
        want[f"detect_select/{m}.st"] = ("exact", zeros)
        # 16-bit samples: the strength is the embed's of the unpacked plane; the samples themselves are held between engines only
        x16 = D.unpack(I["x16"][:F], BITS16)
        emb("tmp", omk, x16, x16)
        want[f"embed16/{m}.y"], want[f"embed16/{m}.a"] = ("none", D.pack(want["tmp.y"][1], BITS16)), ("a", want["tmp.a"][1])
        for n in ("tmp.y", "tmp.a", "tmp.st"):
            del want[n]
        want[f"detect16/{m}.corr"] = ("score", det(D.unpack(I["m16"][:F], BITS16), W, omk))
        # host planes
        emb(f"host/{m}", omk, x[2:3], I["rgbf32"][None])
        want[f"host/{m}.y"] = ("y", want[f"host/{m}.y"][1][0])
        # the detector of an embed's output
        yo = emb("tmp", omk, x[:F], x[:F])
        for n in ("tmp.y", "tmp.a", "tmp.st"):
            del want[n]
        c = det(yo, W, omk)
        want[f"slot_out/{m}.corr"], want[f"slot_out/{m}.st"] = ("score", c), ("exact", zeros)
        want[f"slot_out/{m}.corr_ptr"], want[f"slot_out/{m}.st_ptr"] = ("score", c), ("exact", zeros)

    for dt, xs in (("f32", x), ("u8", xu)):
        g = [O.gram(v.astype(np.float32)) for v in xs[:F]]
        want[f"gram/{dt}.tot"] = ("exact" if dt == "u8" else "gram", np.concatenate([np.concatenate([Rx[np.triu_indices(8)], rx]) for Rx, rx in g]))
        want[f"rgb2gray/{dt}.gray"] = ("exact", O.rgb2gray(I["rgb" + dt].astype(np.float32)))
    want["unpack_rgb8.rgb"] = ("exact", I["rgbu8"].astype(np.float32))
    want["unpack_rgb8.gray"] = ("exact", O.rgb2gray(I["rgbu8"].astype(np.float32)))
    want["pack_rgb8.packed"] = ("exact", np.ascontiguousarray(np.clip(I["rgbf32"], 0, 255).astype(np.uint8).transpose(1, 2, 0)))
    want["unpack16.x"] = ("exact", D.unpack(I["x16"][:F], BITS16))
    want["pack16.v"] = ("exact", D.pack(x[:F], BITS16))
    return want


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same_bits(got, want):
    """names whose arrays differ in shape, dtype or any byte (NaN must sit in the same places with the same bits)"""
    bad = sorted(set(got) ^ set(want))
    for n in sorted(set(got) & set(want)):
        g, w = np.asarray(got[n]), np.asarray(want[n])
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(raw(g), raw(w)):
            bad.append(n)
    return bad


def check_one(kind, got, want):
    """None, or what is wrong"""
    got, want = np.asarray(got), np.asarray(want)
    if kind == "none":
        return None if got.shape == want.shape else f"shape {got.shape} against {want.shape}"
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    if kind == "exact":
        g, w = got, want.astype(got.dtype)
        return None if np.array_equal(raw(g), raw(w)) else f"{int((g != w).sum())} of {g.size} elements differ"
    if kind == "u8":
        d = np.abs(got.astype(int) - want.astype(int))
        ok = d.max() <= 1 and (d != 0).mean() <= TOLERANCES["u8"][0]
        return None if ok else f"max difference {d.max()} LSB, {float((d != 0).mean()):.3g} of the pixels differ"
    g, w = got.astype(np.float64), want.astype(np.float64)
    if kind == "sumsq":
        g, w = g[..., 1:], w[..., 1:]
    fin = np.isfinite(w)
    if not np.array_equal(np.isnan(g), np.isnan(w)) or not np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]):
        return "NaN or infinity in other places"
    d = np.abs(g[fin] - w[fin])
    tol = TOLERANCES[kind][0]
    bound = tol * np.abs(w[fin]) if kind in ("a", "gram", "sumsq") else tol
    if d.size and (d > bound).any():
        i = int(np.argmax(d - bound))
        return f"difference {d[i]:.3g} at {g[fin][i]!r} against {w[fin][i]!r} (bound {tol:g} {'relative' if kind in ('a', 'gram', 'sumsq') else 'absolute'})"
    return None


def check(got, want):
    """[(name, what is wrong)] of a battery dict against expectations()"""
    bad = [(n, "missing on one side") for n in sorted(set(got) ^ set(want))]
    for n in sorted(set(got) & set(want)):
        msg = check_one(want[n][0], got[n], want[n][1])
        if msg:
            bad.append((n, msg))
    return bad


def family_of(name):
    """the call family (FAMILIES) a dict name belongs to"""
    head = name.split("/")[0].split(".")[0]
    return {"host": "host planes", "slot_out": "WM_MEM_SLOT_OUT"}.get(head, "wm_" + head)


# ---- the transitions (data) --------------------------------------------------------------------------------------------------------

S_SEQ, S_STRIP, S_SPLIT, S_TILES, S_TINY = (40, 272), (70, 300), (37, 266), (64, 516), (5, 7)
DEFAULTS = dict(nslots=2, max_frames=1, rps=0, fused=True, handover=False, checked=True)
CUSTOM = dict(nslots=3, max_frames=3, rps=5, fused=False, handover=False, checked=True)
RPS_STOPS = (0, 1, 4096, 5, 0)
RPS_SHAPES = (S_SEQ, S_STRIP, S_SPLIT)
CONFIGURE_STOPS = ((2, 1), (3, 3), (1, 2))

# (kind, shapes the engine walks through, how the last step is made)
REINIT_CASES = (
    ("reinit grow", (S_SEQ, S_TILES), "array"),
    ("reinit shrink", (S_TILES, S_SPLIT), "array"),
    ("reinit same shape", (S_SEQ, S_SEQ), "array"),
    ("reinit fusable switch", (S_SEQ, S_TINY, S_STRIP), "array"),
    ("reinit from file", (S_SPLIT, S_STRIP), "file"),
)
CLONE_VARIANTS = ("checked_off", "handover_on", "band")


def transition_cases(seed=TABLE_SEED):
    """every (kind, target shape, p, settings) at which a battery runs behind a transition.  The settings of the reinit cases and the
    order of the rps legs' (shape, p) pairs are dealt from `seed`"""
    rng = np.random.default_rng(seed)
    cases = []
    for kind, shapes, how in REINIT_CASES:
        for cfg in (DEFAULTS, CUSTOM):
            for s in shapes[1:]:
                cases.append((kind, s, 3, dict(cfg)))
    for (ns, mf) in CONFIGURE_STOPS[1:]:
        cases.append(("configure", S_SEQ, 3, dict(DEFAULTS, nslots=ns, max_frames=mf)))
    pairs = [(s, p) for s in RPS_SHAPES for p in (3, 7)]
    for i in rng.permutation(len(pairs)):
        s, p = pairs[int(i)]
        for rps in RPS_STOPS[1:]:
            cases.append((f"rps {rps}", s, p, dict(DEFAULTS, max_frames=MAX_F, rps=rps)))
    for v in CLONE_VARIANTS[:2]:
        cases.append(("clone", S_SEQ, 3, dict(CUSTOM, checked=v != "checked_off", handover=v == "handover_on")))
    return cases


TRANSITION_KINDS = ("reinit grow", "reinit shrink", "reinit same shape", "reinit fusable switch", "reinit from file", "configure", "rps 1", "rps 4096",
                    "rps 5", "rps 0", "clone")


def names_of(p):
    """the dict names of a battery under window p, without running anything: from the family list of the code above"""
    per_mask = ["embed/{m}/f32/grey/F1", "embed/{m}/u8/rgb/Fq", "detect/{m}/f32/F1", "embed_detect/{m}", "compute_mask/{m}", "detect_keys/{m}/f32",
                "embed_keys/{m}", "detect_offsets/{m}", "detect_tiles/{m}/f32", "detect_keys_tiles/{m}", "embed_signs/{m}", "embed_bits/{m}",
                "detect_bits/{m}", "embed_signs_multi/{m}", "embed_select/{m}", "detect_select/{m}", "embed16/{m}", "detect16/{m}", "host/{m}",
                "slot_out/{m}"]
    flat = ["gram/f32", "rgb2gray/f32", "unpack_rgb8", "pack_rgb8", "unpack16", "pack16"]
    return [n.format(m=m) for m in masks_of(p) for n in per_mask] + flat


def coverage(cases=None):
    """{(transition kind, family): number of batteries that run the family behind such a transition}"""
    cells = {}
    for kind, shape, p, cfg in (transition_cases() if cases is None else cases):
        for fam in sorted({family_of(n) for n in names_of(p)}):
            cells[(kind, fam)] = cells.get((kind, fam), 0) + 1
    return cells
