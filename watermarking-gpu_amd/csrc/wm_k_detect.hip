// wm_k_detect.hip -- detector kernel k_detect with its fold tail corr_finalize_frame (see wm_k_gram.hip header)
#include "wm_detect_march.hpp"
#include <cstdlib>

namespace wmk {

// corr_fold (tail of k_detect; take_ticket, wm_device.hpp): the last wave of a strip folds the strip's records, the last
// strip's wave folds the frame:
// corr = (float)dot / (float)(||e_w|| * ||e_u||)   (Watermark.cpp:230); unsolvable => 0.0f (:246-247)
// publish a frame's score -- or, in the checking instance (CK = 1), only when the digest of the plane this sweep read equals the
// one the embed left (DigCheck); else flag the frame for the redo launches
template <int CK>
__device__ __forceinline__ void corr_publish(int frame, double a0, double a1, double a2, unsigned long long dg,
                                             const int* __restrict__ status, OpResult* res, RawSums* raw, const DigCheck& dc)
{
    if constexpr (CK == 1) {
        const bool ok = dg == dc.want[frame];
        dc.redo[frame] = ok ? 0 : 1;
        atomicAdd(dc.count + (ok ? 0 : 1), 1ull);
        if (!ok) return;
    }
    const int st = status[frame];
    float corr = 0.0f;
    if (st == 0) corr = (float)a0 / (float)(sqrt(a2) * sqrt(a1));
    res[frame].status = st;
    res[frame].value = corr;
    RawSums rw;
    rw.v[0] = a0; rw.v[1] = a1; rw.v[2] = a2; rw.v[3] = 0.0;
    raw[frame] = rw;
}

template <int CK>
__device__ __forceinline__ void corr_fold(int frame, const WaveJob& j, const double* pcorr, int nrec,
                                          const int* __restrict__ status, const CorrTail& tl, const DigCheck& dc)
{
    const int lane = j.lane;
    if (!take_ticket(tl.ticket_strip + (frame * tl.nstrips + j.strip) * TKS, (unsigned)tl.nsegs, lane)) return;
    unsigned long long dg = 0;
    if constexpr (CK == 1) {
        for (int s0 = lane; s0 < tl.nsegs; s0 += WAVE) dg += ld_agent(dc.pdig + (long long)frame * nrec + (long long)s0 * tl.nstrips + j.strip);
        dg = wave_sum_u64(dg);
        if (lane == 0) st_agent(dc.sdig + (long long)frame * tl.nstrips + j.strip, dg);
    }
    // all loads of a batch are issued before the first is used (index clamped, surplus terms dropped): agent-scope loads
    // come from the memory side, a dependent chain of them costs a memory latency per term
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int s0 = lane; s0 < tl.nsegs; s0 += 2 * WAVE) {
        double v[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double* p = pcorr + ((long long)frame * nrec + (long long)min(s0 + u * WAVE, tl.nsegs - 1) * tl.nstrips + j.strip) * 3;
            v[u][0] = ld_agent(p); v[u][1] = ld_agent(p + 1); v[u][2] = ld_agent(p + 2);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool in = s0 + u * WAVE < tl.nsegs;
            a0 += in ? v[u][0] : 0.0; a1 += in ? v[u][1] : 0.0; a2 += in ? v[u][2] : 0.0;
        }
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane == 0) {
        double* q = tl.scorr + ((long long)frame * tl.nstrips + j.strip) * 3;
        st_agent(q, a0); st_agent(q + 1, a1); st_agent(q + 2, a2);
    }
    if (!take_ticket(tl.ticket + frame * TKS, (unsigned)tl.nstrips, lane)) return;
    a0 = 0.0; a1 = 0.0; a2 = 0.0;
    dg = 0;
    for (int s0 = lane; s0 < tl.nstrips; s0 += WAVE) {
        const double* q = tl.scorr + ((long long)frame * tl.nstrips + s0) * 3;
        const double v0 = ld_agent(q), v1 = ld_agent(q + 1), v2 = ld_agent(q + 2);
        a0 += v0; a1 += v1; a2 += v2;
        if constexpr (CK == 1) dg += ld_agent(dc.sdig + (long long)frame * tl.nstrips + s0);
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if constexpr (CK == 1) dg = wave_sum_u64(dg);
    if (lane == 0) corr_publish<CK>(frame, a0, a1, a2, dg, status, tl.res, tl.raw, dc);
}

// corr_finalize_frame (tail of k_detect, run by the frame's last block):
// corr = (float)dot / (float)(||e_w|| * ||e_u||)   (Watermark.cpp:230); unsolvable => 0.0f (:246-247)
template <int CK>
__device__ __forceinline__ void corr_finalize_frame(int frame, const double* pcorr, int nblk, const int* __restrict__ status,
                                                    OpResult* __restrict__ res, RawSums* __restrict__ raw, const DigCheck& dc)
{
    __shared__ double s[3][BLOCK];
    const int t = threadIdx.x;
    unsigned long long dg = 0;
    if constexpr (CK == 1) {
        if (t < WAVE) {
            for (int b = t; b < nblk; b += WAVE) dg += ld_agent(dc.pdig + (long long)frame * nblk + b);
            dg = wave_sum_u64(dg);
        }
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    // 2 x 3 partials in flight per thread (index clamped, surplus terms dropped), see solve_frame
    for (int b0 = t; b0 < nblk; b0 += 2 * BLOCK) {
        double v[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double* p = pcorr + ((long long)frame * nblk + min(b0 + u * BLOCK, nblk - 1)) * 3;
            v[u][0] = ld_agent(p); v[u][1] = ld_agent(p + 1); v[u][2] = ld_agent(p + 2);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool in = b0 + u * BLOCK < nblk;
            a0 += in ? v[u][0] : 0.0; a1 += in ? v[u][1] : 0.0; a2 += in ? v[u][2] : 0.0;
        }
    }
    s[0][t] = a0; s[1][t] = a1; s[2][t] = a2;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (t < o) { s[0][t] += s[0][t + o]; s[1][t] += s[1][t + o]; s[2][t] += s[2][t + o]; }
        __syncthreads();
    }
    if (t == 0) corr_publish<CK>(frame, s[0][0], s[1][0], s[2][0], dg, status, res, raw, dc);
}

// CK: 0 = the ordinary sweep; 1 = the checking instance of a checked hand-over (DigCheck, wm_kernels.hpp: every frame's march
// runs -- an unsolvable one too, its sums dropped -- for the digest); 2 = k_detect_redo (frames with dc.redo[f] == 0 leave first)
template <typename T, int MASK, int PAD, int HC, bool VEC, int CK>
__device__ __forceinline__ void detect_body(const T* __restrict__ x, long long pitch, long long fstride, const float* __restrict__ W,
                                            const Geom& g, const float* __restrict__ coef, const int* __restrict__ status,
                                            double* pcorr, const CorrTail& tail, const DigCheck& dc)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * RowBuf<1>::N];
    __shared__ double s_red[WPB][3];
    __shared__ unsigned long long s_dig[WPB];
    const WaveJob j = make_job(g);
    const int frame = j.frame;
    if constexpr (CK == 2) {
        // quad: the waves of a block are different frames (surplus waves of a short last quad have none) -- a wave-uniform exit, no
        // barrier on that path; else the block is one frame (its waves past the last segment still take part in the barrier)
        if (g.quad ? (!j.valid || dc.redo[frame] == 0) : dc.redo[frame] == 0) return;
    }
    float dot = 0.0f, nu = 0.0f, nw = 0.0f;
    unsigned long long dig = 0;
    const int st = j.valid ? status[frame] : 1;
    if (j.valid && (CK == 1 || st == 0)) {
        float c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
        const T* xf = x + (long long)frame * fstride;
        constexpr bool DPP_OK = HC == 1;  // the halo of p = 9 (HC = 2) exceeds one neighbour chunk: LDS path only
        constexpr bool V = VEC && DPP_OK;
        constexpr bool D = CK == 1;
        if (MASK != 0 || strip_on_edge<V>(g, j)) detect_march<T, MASK, PAD, HC, V, true, D>(xf, pitch, W, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw, dig);
        else detect_march<T, MASK, PAD, HC, V, (MASK != 0), D>(xf, pitch, W, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw, dig);
        if (CK == 1 && st != 0) { dot = 0.0f; nu = 0.0f; nw = 0.0f; }  // (what the ordinary sweep sums for an unsolvable frame)
    }
    const double d0 = wave_sum((double)dot), d1 = wave_sum((double)nu), d2 = wave_sum((double)nw);
    if constexpr (CK == 1) dig = wave_sum_u64(dig);
    if (g.quad) {
        // the waves of this block are 4 frames: one record per wave, folded per strip and then per frame (corr_fold)
        if (!j.valid) return;  // surplus wave of a short last quad (wave-uniform; no barrier below)
        if (j.lane == 0) {
            double* p = pcorr + ((long long)frame * g.nrec + j.rec) * 3;
            st_agent(p, d0); st_agent(p + 1, d1); st_agent(p + 2, d2);
            if constexpr (CK == 1) st_agent(dc.pdig + (long long)frame * g.nrec + j.rec, dig);
        }
        corr_fold<CK>(frame, j, pcorr, g.nrec, status, tail, dc);
        return;
    }
    // the waves of this block are 4 segments of one frame: one record per block, folded by the frame's last block
    if (j.lane == 0) { s_red[j.wave][0] = d0; s_red[j.wave][1] = d1; s_red[j.wave][2] = d2; s_dig[j.wave] = dig; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        st_agent(pcorr + ((long long)frame * g.nblk_total + g.pb0 + j.tile) * 3 + k, ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k]);
    }
    if (CK == 1 && threadIdx.x == 3)
        st_agent(dc.pdig + (long long)frame * g.nblk_total + g.pb0 + j.tile, s_dig[0] + s_dig[1] + s_dig[2] + s_dig[3]);
    if (last_block_of_frame(tail.ticket + frame * TKS, (unsigned)tail.expected))
        corr_finalize_frame<CK>(frame, pcorr, g.nblk_total, status, tail.res, tail.raw, dc);
}

// occupancy floor: 4 waves per SIMD for the aligned 3x3 instances (105 / 106 / 91 VGPRs); the generic instances (LDS re-lay,
// halo predictions of their own) need ~150 registers -- bound to 4 they spilled 48-70 VGPRs to scratch, at 3 they do not
#define WM_DET_BOUNDS (PAD == 1 && HC == 1 ? (VEC ? WM_DET_WAVES : 3) : 1)
template <typename T, int MASK, int PAD, int HC, bool VEC, int CK = 0>
__global__ __launch_bounds__(BLOCK, WM_DET_BOUNDS) void k_detect(const T* __restrict__ x, long long pitch, long long fstride,
                                                                 const float* __restrict__ W, Geom g,
                                                                 const float* __restrict__ coef, const int* __restrict__ status,
                                                                 double* pcorr, CorrTail tail, DigCheck dc)
{
    detect_body<T, MASK, PAD, HC, VEC, CK>(x, pitch, fstride, W, g, coef, status, pcorr, tail, dc);
}
// the fallback of a checked hand-over: k_detect over the frames whose digest did not match (a kernel of its own for profiles)
template <typename T, int MASK, int PAD, int HC, bool VEC>
__global__ __launch_bounds__(BLOCK, WM_DET_BOUNDS) void k_detect_redo(const T* __restrict__ x, long long pitch, long long fstride,
                                                                      const float* __restrict__ W, Geom g,
                                                                      const float* __restrict__ coef, const int* __restrict__ status,
                                                                      double* pcorr, CorrTail tail, DigCheck dc)
{
    detect_body<T, MASK, PAD, HC, VEC, 2>(x, pitch, fstride, W, g, coef, status, pcorr, tail, dc);
}
#undef WM_DET_BOUNDS

// results of a mask-only op: status + coefficients
__global__ void k_mask_result(const int* __restrict__ status, const float* __restrict__ coef, OpResult* __restrict__ res,
                              float* __restrict__ coef_out)
{
    const int frame = blockIdx.x, t = threadIdx.x;
    if (t == 0) { res[frame].status = status ? status[frame] : 0; res[frame].value = 0.0f; }
    if (t < 8) coef_out[frame * 8 + t] = coef ? coef[frame * 8 + t] : 0.0f;
}

// launchers
template <typename T>
static void launch_detect_t(const Sweep& sw, const DetectPlan& pl, const float* W, double* pcorr, const CorrTail& tail, const DigCheck& dc)
{
    const PlaneDesc& x = sw.x;
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_detect<T, decltype(m)::value, decltype(p)::value, decltype(hc)::value, decltype(vec)::value>), sp.grid, dim3(BLOCK),
                   0, sw.s, (const T*)x.p, x.pitch, x.fstride, W, sp.g, sw.coef, sw.status, pcorr, tail, dc);
    });
}
bool detect_checkable(const Sweep& sw, int aligned_w)
{
    return sw.x.dtype == 0 && sw.mask == 0 && sw.pad == 1 && detect_plan(sw, aligned_w).overlap;
}
void launch_detect(const Sweep& sw, const KeyBank& w, double* pcorr, unsigned* ticket, unsigned* ticket_strip, double* scorr, OpResult* res,
                   RawSums* raw, const DigCheck* dc, int mode)
{
    const PlaneDesc& x = sw.x;
    if (mode != 0) {
        // the checking instance and its redo launch: f32, ME, overlapped strips (detect_checkable, checked by the caller)
        const LaunchGeom ld = overlap_geom(sw.lg);
        const CorrTail tail{ticket, ticket_strip, ld.nblk, ld.nsegs, ld.nstrips, scorr, res, raw};
        const SweepPart pv = sweep_part_overlap(ld, sw.frames, 1);
        if (mode == 1) WM_KLAUNCH((k_detect<float, 0, 1, 1, true, 1>), pv.grid, dim3(BLOCK), 0, sw.s, (const float*)x.p, x.pitch, x.fstride, w.W, pv.g, sw.coef, sw.status, pcorr, tail, *dc);
        else WM_KLAUNCH((k_detect_redo<float, 0, 1, 1, true>), pv.grid, dim3(BLOCK), 0, sw.s, (const float*)x.p, x.pitch, x.fstride, w.W, pv.g, sw.coef, sw.status, pcorr, tail, *dc);
        return;
    }
    const DigCheck none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const DetectPlan pl = detect_plan(sw, w.aligned_w);
    const LaunchGeom& ld = pl.ld;
    const CorrTail tail{ticket, ticket_strip, ld.nblk, ld.nsegs, ld.nstrips, scorr, res, raw};
    WM_DISPATCH_T(x.dtype, launch_detect_t<T>(sw, pl, w.W, pcorr, tail, none));
}

// ---- W on the device: the counter-based N(0,1) generator of csrc/app/wm_genw.cpp (the replacement of the reference's
// CommonRandomMatrix tool, CommonRandomMatrix/main.cpp:34-51): element (r, c) is a pure function of (seed, r, c) -- a 32-bit
// hash, two uniforms, Box-Muller in f64 -- so every GPU of a node fills its own copy without a file, an upload or a broadcast
__device__ __forceinline__ uint32_t genw_mix(uint32_t h)
{
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t genw_hash(uint32_t seed, uint32_t stream, uint32_t r, uint32_t c)
{
    const uint32_t h = genw_mix(seed ^ genw_mix(stream * 0x9E3779B1u + r));
    return genw_mix(h ^ genw_mix(c + 0x85EBCA6Bu));
}
__global__ void k_gen_w(float* __restrict__ w, int rows, int cols, uint32_t seed)
{
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / cols), c = (uint32_t)(i - (long long)r * cols);
        const double u1 = ((double)genw_hash(seed, 0x5741u, r, c) + 1.0) / 4294967297.0;
        const double u2 = (double)genw_hash(seed, 0x5742u, r, c) / 4294967296.0;
        w[i] = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2));
    }
}
void launch_gen_w(hipStream_t s, float* w, int rows, int cols, uint32_t seed)
{
    hipLaunchKernelGGL(k_gen_w, dim3(2048), dim3(256), 0, s, w, rows, cols, seed);
}

// ---- exhaustive self-test of the NVF quotient (nvf_quot, wm_device.hpp): every f32 bit pattern in [lo, hi) as `var`,
// the sequence's var / (1 + var) against the compiler's IEEE division (hipcc divides f32 correctly rounded by default).
// out2[0] = values whose results differ in any bit (NaN results compare equal), out2[1] = the smallest such bit pattern
template <int VARIANT>
__global__ void k_selftest_quot(uint32_t lo, uint32_t hi, unsigned long long* out2)
{
    unsigned long long bad = 0, first = ~0ull;
    for (unsigned long long b = (unsigned long long)lo + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b < hi;
         b += (unsigned long long)gridDim.x * blockDim.x) {
        const float var = __uint_as_float((uint32_t)b);
        const float d = 1.0f + var;
        const float ref = var / d;
        const float got = nvf_quot_variant<VARIANT>(var, d);
        const bool same = __float_as_uint(ref) == __float_as_uint(got) || (ref != ref && got != got);
        if (!same) { ++bad; if (b < first) first = b; }
    }
    if (bad) { atomicAdd(out2, bad); atomicMin(out2 + 1, first); }
}
void launch_selftest_quot(hipStream_t s, int variant, uint32_t bits_lo, uint32_t bits_hi, unsigned long long* out2)
{
    if (variant == 0) hipLaunchKernelGGL(k_selftest_quot<0>, dim3(4096), dim3(256), 0, s, bits_lo, bits_hi, out2);
    else if (variant == 1) hipLaunchKernelGGL(k_selftest_quot<1>, dim3(4096), dim3(256), 0, s, bits_lo, bits_hi, out2);
    else if (variant == 2) hipLaunchKernelGGL(k_selftest_quot<2>, dim3(4096), dim3(256), 0, s, bits_lo, bits_hi, out2);
    else hipLaunchKernelGGL(k_selftest_quot<3>, dim3(4096), dim3(256), 0, s, bits_lo, bits_hi, out2);
}

// ---- memory-system yardstick (wm_membench, wm.h): grid-stride streams of 16-byte elements, 2048 blocks x 256 threads like
// the sweeps' grids; stores are non-temporal buffer stores (store4's form), loads plain 16-byte buffer-free global loads
template <int KIND, int UNR>
__global__ __launch_bounds__(256) void k_membench(const float4* __restrict__ src, float4* __restrict__ dst, size_t n16, unsigned long long* sink)
{
    typedef float f4v __attribute__((ext_vector_type(4)));
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    float acc = 0.0f;
    // UNR elements in flight per thread and trip
    for (; i + (UNR - 1) * stride < n16; i += UNR * stride) {
        float4 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (KIND == 0) v[u] = make_float4((float)i, 1.0f, 2.0f, (float)u);
            else v[u] = src[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (KIND == 2) acc += v[u].x + v[u].w;
            else {
                f4v w; w.x = v[u].x; w.y = v[u].y; w.z = v[u].z; w.w = v[u].w;
                __builtin_nontemporal_store(w, reinterpret_cast<f4v*>(dst + i + u * stride));
            }
        }
    }
    for (; i < n16; i += stride) {
        const float4 v = KIND == 0 ? make_float4((float)i, 1.0f, 2.0f, 3.0f) : src[i];
        if (KIND == 2) acc += v.x + v.w;
        else { f4v w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; __builtin_nontemporal_store(w, reinterpret_cast<f4v*>(dst + i)); }
    }
    if (KIND == 2 && acc == 123456.789f) atomicAdd(sink, 1ull);  // (keeps the loads alive)
}
void launch_membench(hipStream_t s, int kind, const void* src, void* dst, size_t n16, unsigned long long* sink, hipEvent_t a, hipEvent_t b)
{
    // two grid shapes (kind / 3): 0 = 2048 blocks x 4 elements in flight per thread, a grid like the sweeps' own (a few waves per
    // SIMD that stay for the whole launch); 1 = 65536 blocks x 1 element per thread, the shape that streams fastest on MI355X
    // (tools/membench_sweep.py: store 6.6, copy 6.2, read 6.4 TB/s against 4.4-5.0 / 4.3-5.0 / 5.3 in shape 0).  The environment
    // overrides both for that sweep
    const int shape = kind / 3;
    kind %= 3;
    static const int env_blocks = getenv("WM_MEMBENCH_BLOCKS") ? atoi(getenv("WM_MEMBENCH_BLOCKS")) : 0;
    static const int env_unr = getenv("WM_MEMBENCH_UNROLL") ? atoi(getenv("WM_MEMBENCH_UNROLL")) : 0;
    const int blocks = env_blocks > 0 ? env_blocks : (shape ? 65536 : 2048);
    const int unr = env_unr > 0 ? env_unr : (shape ? 1 : 4);
    const dim3 grid(blocks), block(256);
#define MB_LAUNCH(K, U) hipExtLaunchKernelGGL((k_membench<K, U>), grid, block, 0, s, a, b, 0, (const float4*)src, (float4*)dst, n16, sink)
#define MB_KIND(U) do { if (kind == 0) MB_LAUNCH(0, U); else if (kind == 1) MB_LAUNCH(1, U); else MB_LAUNCH(2, U); } while (0)
    if (unr <= 1) MB_KIND(1); else if (unr == 2) MB_KIND(2); else if (unr <= 4) MB_KIND(4); else MB_KIND(8);
#undef MB_KIND
#undef MB_LAUNCH
}

void launch_mask_result(hipStream_t s, int frames, const int* status, const float* coef, OpResult* res, float* coef_out)
{
    hipLaunchKernelGGL(k_mask_result, dim3(frames), dim3(64), 0, s, status, coef, res, coef_out);
}

}  // namespace wmk
