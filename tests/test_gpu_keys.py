"""wm_detect_keys: one image scored against a bank of watermark keys in one call (k_detect_keys).  Scores against the CPU
oracle (<= 1e-5, the bound of the other detector tests), bit equality with wm_detect on a context whose W is the key (the
kernel keeps k_detect's per-pixel operations and partial-sum grouping), identification of an embedded key, generated keys,
unsolvable frames, enqueue semantics, determinism and the C++ surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from synth import synth_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def seeds_for(K, base=1000):
    return [base + 17 * k for k in range(K)]


def frames_of(R, Cc, F, dtype, first=0):
    return np.stack([synth_frame(R, Cc, frame=first + f, dtype=np.uint8 if dtype == "u8" else np.float32) for f in range(F)])


def oracle_score(x, W, p, mask):
    if x.dtype == np.uint8:
        return O.detect_u8(x, W, p=p, mask=mask)[1]
    return O.detect(x, W, p=p, mask=mask)[1]


SMALL = [(1, 1), (5, 7), (64, 256), (270, 480)]
LARGE = [(1078, 1918), (3838, 2160), (2160, 3840)]
CASES = []
for i, shape in enumerate(SMALL + LARGE):
    masks = [(0, 3), (1, 3)] + ([(1, 5), (1, 7), (1, 9)] if shape in SMALL else [])
    for j, (mk, p) in enumerate(masks):
        for dtype in ("f32", "u8"):
            KF = [(1, 1), (3, 4), (8, 1), (8, 4)][(i + j + (dtype == "u8")) % 4]
            if shape in LARGE:
                KF = (3, 1) if (j + (dtype == "u8")) % 2 == 0 else (3, 4)
            CASES.append((shape, mk, p, dtype) + KF)


@pytest.mark.parametrize("shape,mask,p,dtype,K,F", CASES)
def test_oracle_parity(wm, torch_cuda, shape, mask, p, dtype, K, F):
    torch = torch_cuda
    R, Cc = shape
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K), device=0)
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0, max_frames=F)
    xs = frames_of(R, Cc, F, dtype)
    xt = torch.from_numpy(xs).cuda()
    got = eng.detectKeys(xt if F > 1 else xt[0], keys, wm.MASK_TYPE(mask))
    got = np.asarray(got).reshape(F, K)
    large = shape in LARGE
    for f in range(F):
        for k in range(K):
            if large and F > 1 and f not in (0, F - 1):
                continue  # (oracle time: the first and last frame of a batch at the large shapes)
            ref = oracle_score(xs[f], keys.plane(k), p, mask)
            assert abs(float(got[f, k]) - ref) <= TOL, (shape, mask, p, dtype, f, k, float(got[f, k]), ref)
    keys.close()
    eng.close()


@pytest.mark.parametrize("shape", [(64, 256), (270, 480), (271, 483), (1078, 1918), (2160, 3840)])
@pytest.mark.parametrize("mask,p", [(0, 3), (1, 3), (1, 5), (1, 9)])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("F", [1, 5])
def test_bit_equal_to_wm_detect(wm, torch_cuda, shape, mask, p, dtype, F):
    """the kernel keeps k_detect's per-pixel operation order and partial-sum grouping: key k's score is wm_detect's with key k
    as W, bit for bit (fused kernels off: wm_detect on the batched sweeps)"""
    torch = torch_cuda
    R, Cc = shape
    K = 3
    sd = seeds_for(K, base=77)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    xs = torch.from_numpy(frames_of(R, Cc, F, dtype, first=3)).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), p, 40.0, max_frames=F)
    got = np.asarray(eng.detectKeys(xs, keys, wm.MASK_TYPE(mask))).reshape(F, K)
    for k in range(K):
        ek = wm.Watermark.generated(R, Cc, sd[k], p, 40.0, max_frames=F)
        ek.set_fused(False)
        ref = np.asarray(ek.detectWatermark(xs, wm.MASK_TYPE(mask)), np.float32).reshape(F)
        assert np.array_equal(got[:, k].view(np.uint32), ref.view(np.uint32)), (k, got[:, k], ref)
        ek.close()


@pytest.mark.parametrize("shape", [(270, 480), (2160, 3840)])
def test_identification(wm, torch_cuda, shape):
    """16 keys from seeds; key j embedded at psnr 40: argmax of the scores is j, far above every other key"""
    torch = torch_cuda
    R, Cc = shape
    sd = seeds_for(16, base=5000)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    x = synth_frame(R, Cc, frame=1)
    xt = torch.from_numpy(x).cuda()
    det = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0)
    # threshold from the oracle: the unmarked image's scores against a few keys
    base = max(abs(O.detect(x, keys.plane(k))[1]) for k in (0, 7, 15))
    for j in (0, 5, 11, 15):
        emb = wm.Watermark.generated(R, Cc, sd[j], 3, 40.0)
        y, a = emb.makeWatermark(xt, xt, wm.MASK_TYPE.ME)
        s = det.detectKeys(y, keys, wm.MASK_TYPE.ME)
        assert int(np.argmax(s)) == j, (j, s)
        others = np.delete(np.abs(s), j)
        assert s[j] > 4 * max(base, float(others.max())), (j, s, base)
        assert abs(float(s[j]) - O.detect(y.cpu().numpy(), keys.plane(j))[1]) <= TOL
        emb.close()


def test_generated_keys_equal_wm_create_generated(wm):
    R, Cc = 270, 483
    sd = [0, 1, 12345, 0xFFFFFFFF]
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    for k, s in enumerate(sd):
        e = wm.Watermark.generated(R, Cc, s, 3, 40.0)
        assert np.array_equal(keys.plane(k).view(np.uint32), e.watermark().view(np.uint32)), s
        e.close()


def test_set_and_files(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc = 64, 256
    rng = np.random.default_rng(3)
    ws = [rng.standard_normal((R, Cc)).astype(np.float32) for _ in range(3)]
    paths = []
    for i, w in enumerate(ws):
        pth = tmp_path / f"w{i}.dat"
        w.tofile(pth)
        paths.append(str(pth))
    kf = wm.KeySet.from_files(paths, R, Cc)
    ks = wm.KeySet(R, Cc, 3)
    ks.set(0, ws[0])
    ks.set(1, torch.from_numpy(ws[1]).cuda())
    ks.set(2, torch.from_numpy(ws[2]))
    for k in range(3):
        assert np.array_equal(kf.plane(k), ws[k]) and np.array_equal(ks.plane(k), ws[k])
    L = wm.lib()
    bad = tmp_path / "short.dat"
    np.zeros(10, np.float32).tofile(bad)
    assert L.wm_keys_load_file(kf.handle, 0, str(bad).encode()) == wm.WM_ERR_W_SIZE
    assert L.wm_keys_load_file(kf.handle, 0, str(tmp_path / "none.dat").encode()) == wm.WM_ERR_W_OPEN
    with pytest.raises(RuntimeError):
        wm.KeySet.from_files([str(bad)], R, Cc)
    # a bank of another shape is refused
    eng = wm.Watermark(R, Cc, ws[0], 3, 40.0)
    other = wm.KeySet(R + 1, Cc, 2)
    x = torch.from_numpy(synth_frame(R, Cc)).cuda()
    with pytest.raises(RuntimeError):
        eng.detectKeys(x, other, wm.MASK_TYPE.ME)
    s = eng.detectKeys(x, kf, wm.MASK_TYPE.ME)
    for k in range(3):
        assert abs(float(s[k]) - O.detect(synth_frame(R, Cc), ws[k])[1]) <= TOL


def test_unsolvable_frame_in_batch(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, F, K = 270, 480, 5, 3
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K))
    xs = frames_of(R, Cc, F, "f32")
    xs[2] = 100.0  # constant frame: singular prediction system
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    corr = np.full(F * K, 7.0, np.float32)
    st = np.full(F, -5, np.int32)
    eng.detect_keys_async(torch.from_numpy(xs).cuda(), keys, wm.MASK_TYPE.ME, 0, corr, st)
    assert eng.sync(0) == wm.WM_UNSOLVABLE
    corr = corr.reshape(F, K)
    assert list(st) == [0, 0, 1, 0, 0]
    assert np.all(corr[2] == 0.0)
    for f in (1, 3):
        for k in range(K):
            assert abs(float(corr[f, k]) - O.detect(xs[f], keys.plane(k))[1]) <= TOL


def test_enqueue_semantics(wm, torch_cuda):
    torch = torch_cuda
    L = wm.lib()
    R, Cc, K = 270, 480, 4
    sd = seeds_for(K, base=300)
    keys = wm.KeySet.from_seeds(R, Cc, sd)
    x = synth_frame(R, Cc, frame=2)
    W0 = keys.plane(1)
    eng = wm.Watermark(R, Cc, W0, 3, 40.0, nslots=2)
    xt = torch.from_numpy(x).cuda()
    y0 = torch.empty_like(xt)
    y1 = torch.empty_like(xt)
    a0, a1 = (C.c_float * 1)(), (C.c_float * 1)()
    c_det = (C.c_float * 1)()
    ck0 = np.zeros(K, np.float32)
    ck1 = np.zeros(K, np.float32)
    torch.cuda.synchronize()
    # slot 0: embed, detect_keys of its output, detect; slot 1: detect_keys first, then an embed
    eng.embed_async(xt, xt, y0, wm.MASK_TYPE.ME, 0, a0)
    eng.detect_keys_async(y0, keys, wm.MASK_TYPE.ME, 1 - 1, ck0)
    eng.detect_keys_async(xt, keys, wm.MASK_TYPE.NVF, 1, ck1)
    eng.detect_async(y0, wm.MASK_TYPE.ME, 0, c_det)
    eng.embed_async(xt, xt, y1, wm.MASK_TYPE.NVF, 1, a1)
    eng.sync(1)
    eng.sync(0)
    yo = y0.cpu().numpy()
    for k in range(K):
        assert abs(float(ck0[k]) - O.detect(yo, keys.plane(k))[1]) <= TOL
        assert abs(float(ck1[k]) - O.detect(x, keys.plane(k), mask=1)[1]) <= TOL
    assert int(np.argmax(ck0)) == 1 and abs(c_det[0] - float(ck0[1])) <= 2e-7
    # WM_MEM_HOST input
    hx = np.ascontiguousarray(x)
    ph = wm.wm_plane(hx.ctypes.data, R, Cc, 1, wm.WM_F32, wm.WM_MEM_HOST, 1, Cc, 0, 0)
    ch = np.zeros(K, np.float32)
    eng.detect_keys_async(ph, keys, wm.MASK_TYPE.ME, wm.WM_SLOT_SYNC, ch)
    ref = eng.detectKeys(xt, keys, wm.MASK_TYPE.ME)
    assert np.array_equal(ch, ref)
    # WM_MEM_SLOT_OUT after an embed, hand-over off and on (2 frames: the hand-over applies to batched embeds)
    F = 2
    engb = wm.Watermark(R, Cc, W0, 3, 40.0, nslots=1, max_frames=F)
    xb = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    yb = torch.empty_like(xb)
    for ho in (False, True):
        engb.set_handover(ho)
        engb.embed_async(xb, xb, yb, wm.MASK_TYPE.ME, 0)
        ps = wm.wm_plane(None, R, Cc, 1, wm.WM_F32, wm.WM_MEM_SLOT_OUT, F, Cc, 0, R * Cc)
        cs = np.zeros(F * K, np.float32)
        engb.detect_keys_async(ps, keys, wm.MASK_TYPE.ME, 0, cs)
        engb.sync(0)
        ys = yb.cpu().numpy()
        for f in range(F):
            for k in (0, 1):
                assert abs(float(cs[f * K + k]) - O.detect(ys[f], keys.plane(k))[1]) <= TOL, (ho, f, k)
        assert int(np.argmax(cs[:K])) == 1
    # result capacity: frames x keys count against 4096 un-synced results per slot
    big = wm.KeySet(R, Cc, 4096)
    cb = np.zeros(4096, np.float32)
    eng.detect_async(xt, wm.MASK_TYPE.ME, 0, c_det)
    with pytest.raises(RuntimeError, match="un-synced"):
        eng.detect_keys_async(xt, big, wm.MASK_TYPE.ME, 0, cb)
    eng.sync(0)
    big.close()


def test_deterministic(wm, torch_cuda):
    torch = torch_cuda
    R, Cc, F, K = 1078, 1918, 4, 5
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K))
    xs = torch.from_numpy(frames_of(R, Cc, F, "f32")).cuda()
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0, max_frames=F)
    for mk in (wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF):
        a = eng.detectKeys(xs, keys, mk)
        b = eng.detectKeys(xs, keys, mk)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


CPP = r'''
#include "Watermark.hpp"
#include <cstdio>
#include <vector>
int main(int argc, char** argv)
{
    const int R = 270, C = 480, K = 6;
    std::vector<float> x((size_t)R * C);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 2;
    fclose(f);
    Watermark w(R, C, argv[2], 3, 40.0f);
    WatermarkKeys keys(R, C, K);
    for (int k = 0; k < K; ++k) keys.generate(k, 1000 + 17 * k);
    WatermarkKeys moved(std::move(keys));
    const wm::Image img = wm::Image::fromHost(x.data(), R, C);
    for (int m = 0; m < 2; ++m) {
        const std::vector<float> s = w.detectWatermarkKeys(img, moved, m == 0 ? ME : NVF);
        for (float v : s) printf("%.9g\n", v);
    }
    try { WatermarkKeys bad(R, C, 0); return 3; } catch (const std::runtime_error&) {}
    return 0;
}
'''


def test_cpp_surface(wm, torch_cuda, tmp_path):
    torch = torch_cuda
    R, Cc, K = 270, 480, 6
    src = tmp_path / "keys.cpp"
    src.write_text(CPP)
    exe = tmp_path / "keys"
    libdir = os.path.dirname(wm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lwm_hip", "-Wl,-rpath," + libdir])
    x = synth_frame(R, Cc, frame=6)
    xf = tmp_path / "x.f32"
    x.tofile(xf)
    wf = tmp_path / "w.dat"
    np.zeros((R, Cc), np.float32).tofile(wf)
    out = subprocess.run([str(exe), str(xf), str(wf)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.array([float(v) for v in out.stdout.split()], np.float32).reshape(2, K)
    keys = wm.KeySet.from_seeds(R, Cc, seeds_for(K))
    eng = wm.Watermark(R, Cc, np.zeros((R, Cc), np.float32), 3, 40.0)
    xt = torch.from_numpy(x).cuda()
    for m, mk in enumerate((wm.MASK_TYPE.ME, wm.MASK_TYPE.NVF)):
        assert np.array_equal(got[m], eng.detectKeys(xt, keys, mk)), (m, got[m])
