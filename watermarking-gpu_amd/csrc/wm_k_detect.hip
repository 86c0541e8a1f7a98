// wm_k_detect.hip -- detector kernel k_detect (body and fold tails: detect_body, wm_detect_march.hpp; see wm_k_gram.hip header)
#include "wm_detect_march.hpp"
#include <cstdlib>

namespace wmk {

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
