// wm_k_detect_keys.hip -- k_detect_keys: the detector of ONE image against a bank of K watermark keys (wm_detect_keys, wm.h)
// with its fold kernel k_keys_fold.
//
// Everything on the image side of the detector is independent of the key (Watermark.cpp:221-250): the coefficients c (one
// Gram sweep + solve, wm_api.hip gram_sweep), e_w = x - c.nbrs(x), the mask m (ME: |e_w|, NVF: nvf(x)) and ||e_w||^2.  Only
// u_k = m W_k, e_u_k = u_k - c.nbrs(u_k), <e_u_k, e_w> and ||e_u_k||^2 change with the key.  k_detect_keys is k_detect's strip
// march (wm_k_detect.hip detect_march) with a compile-time group of KG keys inside every row step (group_march,
// wm_keys_march.hpp, shared with k_detect_keys_tiles and k_detect_offsets, as are the lines around it and the record tail):
// x, e_w and m are formed once per row, then every key of the group loads its W row, forms its rolling u window and runs its
// residual4 chain.  K > KG
// is a grid axis over key groups (x is marched again per group; the groups of one tile run back to back on one XCD, so those
// re-reads are L2 hits).  Per key the per-pixel operations, their order and the partial-sum grouping are k_detect's: a key's
// score is bit-identical to wm_detect's with that key as W (tests/test_gpu_keys.py).
#include "wm_keys_march.hpp"

namespace wmk {

struct KeysArgs {
    const float* W;     // the bank [nkeys][rows][cols]
    long long kstride;  // elements between key planes
    int nkeys;
    int ngroups;        // key groups = grid blocks per tile
    int rstride;        // partial records per (frame, key): >= the sweep's blocks (nblk_total) and wave records (nrec)
    double* part;       // [frames][nkeys][rstride][2]  {<e_u,e_w>, ||e_u||^2}
    double* partw;      // [frames][rstride]            ||e_w||^2 (written by key group 0)
};

// occupancy floor: the aligned 3x3 instances hold two keys' u windows and W rings besides k_detect's registers -- 4 waves per
// SIMD for u8 planes (122 / 124 VGPRs), 3 for f32 ones (at 4 they spill 17 VGPRs); the generic instances 2 (LDS re-lay, halo
// predictions of their own)
template <typename T, int MASK, int PAD, int HC, bool VEC>
__global__ __launch_bounds__(BLOCK, (PAD == 1 && HC == 1 ? (VEC ? (sizeof(T) == 1 ? 4 : 3) : 2) : 1)) void k_detect_keys(
    const T* __restrict__ x, long long pitch, long long fstride, KeysArgs ka, Geom g, const float* __restrict__ coef,
    const int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * KG * RowBuf<1>::N];
    int grp;
    const WaveJob j = keys_job(g, ka.ngroups, grp);
    const int frame = j.frame;
    const int k0 = grp * KG;
    float dot[KG], nu[KG], nw = 0.0f;
#pragma unroll
    for (int q = 0; q < KG; ++q) { dot[q] = 0.0f; nu[q] = 0.0f; }
    if (j.valid && status[frame] == 0) {
        WM_GROUP_DETECT_FRAME;
        // keys beyond the bank (a short last group) repeat its last key; their sums are not stored
        const float* Wk[KG];
#pragma unroll
        for (int q = 0; q < KG; ++q) Wk[q] = ka.W + (long long)min(k0 + q, ka.nkeys - 1) * ka.kstride;
        WM_GROUP_DETECT_MARCH(KG, false, PFK, Wk, g.cols);
    }
    // one record per wave (quad) or per block; the group's keys are k0 .. of the bank's nkeys, those below nkeys are stored; key
    // group 0 records ||e_w||^2
    WM_GROUP_RECORDS(KG, k0, ka.nkeys, k0, ka.nkeys, ka.rstride, grp == 0, ka.part, ka.partw);
}

// one block per (frame, key): the records folded in k_detect's order -- corr_finalize_frame's over the blocks, or (quad)
// corr_fold's over the segments of each strip, then over the strips -- into corr = (float)dot / (float)(||e_w|| * ||e_u||)
// (Watermark.cpp:230); unsolvable => 0.0f (:246-247)
__global__ __launch_bounds__(BLOCK) void k_keys_fold(const double* __restrict__ part, const double* __restrict__ partw, int rstride,
                                                     int nkeys, int quad, int nblk, int nsegs, int nstrips,
                                                     const int* __restrict__ status, OpResult* __restrict__ res)
{
    __shared__ double s[3][BLOCK];
    const int frame = blockIdx.x / nkeys, key = blockIdx.x - frame * nkeys;
    const double* pk = part + ((long long)frame * nkeys + key) * rstride * 2;
    const double* pw = partw + (long long)frame * rstride;
    const int t = threadIdx.x;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    if (!quad) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int b0 = t; b0 < nblk; b0 += 2 * BLOCK) {
            double v[2][3];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int b = min(b0 + u * BLOCK, nblk - 1);
                v[u][0] = pk[2 * b]; v[u][1] = pk[2 * b + 1]; v[u][2] = pw[b];
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
        r0 = s[0][0]; r1 = s[1][0]; r2 = s[2][0];
    } else {
        __shared__ double ss[3][KEYS_MAX_STRIPS];
        const int lane = t & (WAVE - 1), wave = t / WAVE;
        for (int st = wave; st < nstrips; st += WPB) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int s0 = lane; s0 < nsegs; s0 += 2 * WAVE) {
                double v[2][3];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int rec = min(s0 + u * WAVE, nsegs - 1) * nstrips + st;
                    v[u][0] = pk[2 * rec]; v[u][1] = pk[2 * rec + 1]; v[u][2] = pw[rec];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bool in = s0 + u * WAVE < nsegs;
                    a0 += in ? v[u][0] : 0.0; a1 += in ? v[u][1] : 0.0; a2 += in ? v[u][2] : 0.0;
                }
            }
            a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
            if (lane == 0) { ss[0][st] = a0; ss[1][st] = a1; ss[2][st] = a2; }
        }
        __syncthreads();
        if (wave == 0) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int s0 = lane; s0 < nstrips; s0 += WAVE) { a0 += ss[0][s0]; a1 += ss[1][s0]; a2 += ss[2][s0]; }
            r0 = wave_sum(a0); r1 = wave_sum(a1); r2 = wave_sum(a2);
        }
    }
    if (t == 0) {
        const int st = status[frame];
        float corr = 0.0f;
        if (st == 0) corr = (float)r0 / (float)(sqrt(r2) * sqrt(r1));
        OpResult o;
        o.status = st; o.value = corr;
        res[blockIdx.x] = o;
    }
}

template <typename T>
static void launch_detect_keys_t(const Sweep& sw, const DetectPlan& pl, const KeysArgs& ka)
{
    const PlaneDesc& x = sw.x;
    // every grid times the key groups
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_detect_keys<T, decltype(m)::value, decltype(p)::value, decltype(hc)::value, decltype(vec)::value>),
                   dim3(sp.grid.x * (unsigned)ka.ngroups), dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, ka, sp.g, sw.coef, sw.status);
    });
}

int detect_keys_group(void) { return KG; }

int launch_detect_keys(const Sweep& sw, const KeyBank& bank, double* part, int rstride, OpResult* res)
{
    const DetectPlan pl = detect_plan(sw, bank.aligned_w);
    const LaunchGeom& ld = pl.ld;
    const int frames = sw.frames, nkeys = bank.nkeys;
    const bool quad = frames >= 4;
    if (ld.nblk > rstride || ld.nstrips * ld.nsegs > rstride || ld.nstrips > KEYS_MAX_STRIPS) return -1;
    KeysArgs ka;
    ka.W = bank.W; ka.kstride = bank.kstride; ka.nkeys = nkeys; ka.ngroups = group_count(nkeys, KG); ka.rstride = rstride;
    ka.part = part; ka.partw = part + (size_t)frames * nkeys * rstride * 2;
    WM_DISPATCH_T(sw.x.dtype, launch_detect_keys_t<T>(sw, pl, ka));
    launch_keys_fold(sw.s, ka.part, ka.partw, rstride, frames, nkeys, quad ? 1 : 0, ld.nblk, ld.nsegs, ld.nstrips, sw.status, res);
    return 0;
}

void launch_keys_fold(hipStream_t s, const double* part, const double* partw, int rstride, int frames, int nkeys, int quad, int nblk,
                      int nsegs, int nstrips, const int* status, OpResult* res)
{
    WM_KLAUNCH(k_keys_fold, dim3((unsigned)(frames * nkeys)), dim3(BLOCK), 0, s, part, partw, rstride, nkeys, quad, nblk, nsegs, nstrips,
               status, res);
}

}  // namespace wmk
