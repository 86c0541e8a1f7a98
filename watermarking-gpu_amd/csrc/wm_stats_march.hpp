// wm_stats_march.hpp -- me_stats_march and nvf_stats_march, the stats sweeps' marches over one wave's segment, their fold tails
// (stats_fold, embed_scalars_frame) and WM_ME_STATS_BODY / WM_NVF_STATS_BODY, the kernel bodies around them: shared by k_me_stats /
// k_nvf_stats (wm_k_embed.hip) and k_me_stats_sel / k_nvf_stats_sel (wm_k_select.hip), which differ only in where W comes from
#pragma once
#include "wm_embed_march.hpp"

namespace wmk {

// =================================================================================================
// stats_fold (tail of k_me_stats / k_nvf_stats; take_ticket, wm_device.hpp): after a wave stored its record, the
// last wave of a strip folds the strip, the last strip's wave folds the frame:
//      a = sF / (float)(||u|| / sqrt(N))   (Watermark.cpp:170)
//   ME : ||u|| = sqrt(sum (|e| W)^2) / max|e|     NVF: ||u|| = sqrt(sum (m W)^2)
// Sums run in record order over the lanes, then through the fixed DPP tree: deterministic.
// =================================================================================================
__device__ __forceinline__ void stats_fold(int frame, const WaveJob& j, const float* pmax, const double* pss, int nrec,
                                           const int* __restrict__ status, const ScalarsTail& tl)
{
    const int lane = j.lane;
    if (!take_ticket(tl.ticket_strip + (frame * tl.nstrips + j.strip) * TKS, (unsigned)tl.nsegs, lane)) return;
    // ---- this strip's wave records: index seg * nstrips + strip.  All loads of a batch are issued before the first is
    // used (index clamped, surplus terms dropped): agent-scope loads come from the memory side, a dependent chain of
    // them costs a memory latency per term
    float mx = 0.0f;
    double ss = 0.0;
    for (int s0 = lane; s0 < tl.nsegs; s0 += 4 * WAVE) {
        float vm[4];
        double vs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long idx = (long long)frame * nrec + (long long)min(s0 + u * WAVE, tl.nsegs - 1) * tl.nstrips + j.strip;
            vm[u] = pmax ? ld_agent(pmax + idx) : 0.0f;
            vs[u] = ld_agent(pss + idx);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = s0 + u * WAVE < tl.nsegs;
            mx = fmaxf(mx, in ? vm[u] : 0.0f);
            ss += in ? vs[u] : 0.0;
        }
    }
    mx = wave_max(mx);
    ss = wave_sum(ss);
    if (lane == 0) {
        if (pmax) st_agent(tl.smax + frame * tl.nstrips + j.strip, mx);
        st_agent(tl.sss + frame * tl.nstrips + j.strip, ss);
    }
    if (!take_ticket(tl.ticket + frame * TKS, (unsigned)tl.nstrips, lane)) return;
    // ---- the frame's strip records
    mx = 0.0f; ss = 0.0;
    for (int s0 = lane; s0 < tl.nstrips; s0 += WAVE) {
        const float vm = pmax ? ld_agent(tl.smax + frame * tl.nstrips + s0) : 0.0f;
        const double vs = ld_agent(tl.sss + frame * tl.nstrips + s0);
        mx = fmaxf(mx, vm);
        ss += vs;
    }
    mx = wave_max(mx);
    ss = wave_sum(ss);
    if (lane == 0) {
        const int st = status ? status[frame] : 0;
        EmbedScalars s;
        s.maxe = pmax ? mx : 1.0f;
        const double nrm = pmax ? sqrt(ss) / (double)s.maxe : sqrt(ss);
        s.a = tl.sF / (float)(nrm / tl.sqrt_n);
        tl.scal[frame] = s;
        tl.res[frame].status = st;
        tl.res[frame].value = s.a;
        RawSums rw;
        rw.v[0] = (double)s.maxe; rw.v[1] = ss; rw.v[2] = 0.0; rw.v[3] = 0.0;
        tl.raw[frame] = rw;
    }
}

// =================================================================================================
// embed_scalars_frame (tail of k_me_stats / k_nvf_stats, run by the frame's last block): fold the stats partials
//   a = sF / (float)(||u|| / sqrt(N))   (Watermark.cpp:170)
//   ME : ||u|| = sqrt(sum (|e| W)^2) / max|e|     NVF: ||u|| = sqrt(sum (m W)^2)
// =================================================================================================
__device__ __forceinline__ void embed_scalars_frame(int frame, const float* pmax, const double* pss, int nblk,
                                                    const int* __restrict__ status, const ScalarsTail& tl)
{
    __shared__ float s_mx[BLOCK];
    __shared__ double s_ss[BLOCK];
    const int t = threadIdx.x;
    float mx = 0.0f;
    double ss = 0.0;
    // 4 partials in flight per thread (index clamped, surplus terms dropped), see solve_frame
    for (int b0 = t; b0 < nblk; b0 += 4 * BLOCK) {
        float vm[4];
        double vs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long idx = (long long)frame * nblk + min(b0 + u * BLOCK, nblk - 1);
            vm[u] = pmax ? ld_agent(pmax + idx) : 0.0f;
            vs[u] = ld_agent(pss + idx);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = b0 + u * BLOCK < nblk;
            mx = fmaxf(mx, in ? vm[u] : 0.0f);
            ss += in ? vs[u] : 0.0;
        }
    }
    s_mx[t] = mx; s_ss[t] = ss;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (t < o) { s_mx[t] = fmaxf(s_mx[t], s_mx[t + o]); s_ss[t] += s_ss[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        const int st = status ? status[frame] : 0;
        EmbedScalars s;
        s.maxe = pmax ? s_mx[0] : 1.0f;
        const double nrm = pmax ? sqrt(s_ss[0]) / (double)s.maxe : sqrt(s_ss[0]);
        s.a = tl.sF / (float)(nrm / tl.sqrt_n);
        tl.scal[frame] = s;
        tl.res[frame].status = st;
        tl.res[frame].value = s.a;
        RawSums rw;
        rw.v[0] = (double)s.maxe; rw.v[1] = s_ss[0]; rw.v[2] = 0.0; rw.v[3] = 0.0;
        tl.raw[frame] = rw;
    }
}

// =================================================================================================
// k_me_stats: e = x - c.nbrs;  per block: max|e| and sum (|e| W)^2
// =================================================================================================
template <typename T, bool VEC, bool EDGE>
__device__ __forceinline__ void me_stats_march(const T* __restrict__ xf, long long pitch, const float* __restrict__ W,
                                               const Geom& g, const WaveJob& j, float* lds, const float (&c)[8], float& mx,
                                               float& ss)
{
    constexpr int RG = VEC ? WM_RING3 : UNROLL;
    XMarch<T, 1, 1, 3, VEC, PFX, EDGE, false, RG> xm;
    PMarch<float, VEC, PFW> wm_;
    const int nout = j.re - j.rs, n = nout + 2;
    xm.start(xf, pitch, g, j, lds, j.rs - 1, n);
    wm_.start(W, g.cols, g.cols, j, j.rs, nout);
    const int c0 = j.c0s + 4 * j.lane;
    const bool own = !EDGE || 4 * j.lane >= j.dup;  // duplicate lanes of a shifted last strip do not count
    march_n<2, RG>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            constexpr int SLOT = (Q + 4 * UNROLL - 2) % PFW;
            const float4 w = wm_.template take<SLOT>();
            const float* up = xm.template row<Q>(0);
            const float* mid = xm.template row<Q>(1);
            const float* dn = xm.template row<Q>(2);
            float pr[4];
            predict4<4>(up, mid, dn, c, pr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (VEC ? own : c0 + k < g.cols) {
                    const float e = mid[4 + k] - pr[k];
                    const float ae = fabsf(e);
                    mx = fmaxf(mx, ae);
                    const float t = ae * f4get(w, k);
                    ss = fmaf(t, t, ss);
                }
            }
            wm_.template refill<SLOT>(i - 2);
        }
    });
}

// WM_ME_STATS_BODY: the body of k_me_stats and k_me_stats_sel -- the frame's coefficients, the choice between the edge and the no-edge
// instance of the march, the wave's / block's record and the fold tail.  It expands inside a kernel with k_me_stats' template
// parameters (T, VEC) and the names x, pitch, fstride, W, g, coef, status, pmax, pss, tail in scope.  A macro for WM_EMBED_BODY's reason
// (wm_embed_march.hpp): expanded in place, every k_me_stats instance compiles to what it compiled to when the lines stood in the kernel
#define WM_ME_STATS_BODY()                                                                                                               \
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];                                                          \
    __shared__ float s_mx[WPB];                                                                                                          \
    __shared__ double s_ss[WPB];                                                                                                         \
    const WaveJob j = make_job(g);                                                                                                       \
    const int frame = j.frame;                                                                                                           \
    float mx = 0.0f, ss = 0.0f;                                                                                                          \
    if (j.valid && status[frame] == 0) {                                                                                                 \
        float c[8];                                                                                                                      \
        _Pragma("unroll") for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];                                                        \
        const T* xf = x + (long long)frame * fstride;                                                                                    \
        if (strip_on_edge<VEC>(g, j)) me_stats_march<T, VEC, true>(xf, pitch, W, g, j, s_row[j.wave], c, mx, ss);                         \
        else me_stats_march<T, VEC, false>(xf, pitch, W, g, j, s_row[j.wave], c, mx, ss);                                                 \
    }                                                                                                                                    \
    mx = wave_max(mx);                                                                                                                   \
    const double ssd = wave_sum((double)ss);                                                                                             \
    if (g.quad) {                                                                                                                        \
        /* the waves of this block are 4 frames: one record per wave, folded per strip and then per frame (stats_fold) */                \
        if (!j.valid) return;  /* surplus wave of a short last quad (wave-uniform; no barrier below) */                                  \
        if (j.lane == 0) {                                                                                                               \
            const long long pb = (long long)frame * g.nrec + j.rec;                                                                      \
            st_agent(pmax + pb, mx);                                                                                                     \
            st_agent(pss + pb, ssd);                                                                                                     \
        }                                                                                                                                \
        stats_fold(frame, j, pmax, pss, g.nrec, status, tail);                                                                           \
        return;                                                                                                                          \
    }                                                                                                                                    \
    /* the waves of this block are 4 segments of one frame: one record per block, folded by the frame's last block */                    \
    if (j.lane == 0) { s_mx[j.wave] = mx; s_ss[j.wave] = ssd; }                                                                          \
    __syncthreads();                                                                                                                     \
    if (threadIdx.x == 0) {                                                                                                              \
        const long long pb = (long long)frame * g.nblk_total + g.pb0 + j.tile;                                                           \
        st_agent(pmax + pb, fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3])));                                                    \
        st_agent(pss + pb, ((s_ss[0] + s_ss[1]) + s_ss[2]) + s_ss[3]);                                                                   \
    }                                                                                                                                    \
    if (last_block_of_frame(tail.ticket + frame * TKS, (unsigned)tail.expected))                                                         \
        embed_scalars_frame(frame, pmax, pss, g.nblk_total, status, tail)

// =================================================================================================
// k_nvf_stats: per block sum (m_nvf W)^2          (p = 2*PAD+1)
// =================================================================================================
template <typename T, int PAD, bool VEC>
__device__ __forceinline__ void nvf_stats_march(const T* __restrict__ xf, long long pitch, const float* __restrict__ W,
                                                const Geom& g, const WaveJob& j, float* lds, float& ss)
{
    constexpr int NR = 2 * PAD + 1;
    XMarch<T, 1, PAD, NR, VEC, PFX> xm;
    PMarch<float, VEC, PFW> wm_;
    const int nout = j.re - j.rs, n = nout + 2 * PAD;
    xm.start(xf, pitch, g, j, lds, j.rs - PAD, n);
    wm_.start(W, g.cols, g.cols, j, j.rs, nout);
    const int c0 = j.c0s + 4 * j.lane;
    march<2 * PAD>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            constexpr int SLOT = (Q + 2 * UNROLL - 2 * PAD) % PFW;
            const float4 w = wm_.template take<SLOT>();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (VEC ? 4 * j.lane >= j.dup : c0 + k < g.cols) {
                    const float t = nvf_value<PAD, 4, Q>(xm, k) * f4get(w, k);
                    ss = fmaf(t, t, ss);
                }
            }
            wm_.template refill<SLOT>(i - 2 * PAD);
        }
    });
}

// WM_NVF_STATS_BODY: the body of k_nvf_stats and k_nvf_stats_sel (template parameters T, PAD, VEC; the names x, pitch, fstride, W, g,
// pss, tail in scope), as WM_ME_STATS_BODY
#define WM_NVF_STATS_BODY()                                                                                                              \
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];                                                          \
    __shared__ double s_ss[WPB];                                                                                                         \
    const WaveJob j = make_job(g);                                                                                                       \
    const int frame = j.frame;                                                                                                           \
    float ss = 0.0f;                                                                                                                     \
    if (j.valid) {                                                                                                                       \
        const T* xf = x + (long long)frame * fstride;                                                                                    \
        nvf_stats_march<T, PAD, VEC>(xf, pitch, W, g, j, s_row[j.wave], ss);                                                             \
    }                                                                                                                                    \
    const double ssd = wave_sum((double)ss);                                                                                             \
    if (g.quad) {                                                                                                                        \
        if (!j.valid) return;                                                                                                            \
        if (j.lane == 0) st_agent(pss + (long long)frame * g.nrec + j.rec, ssd);                                                         \
        stats_fold(frame, j, nullptr, pss, g.nrec, nullptr, tail);                                                                       \
        return;                                                                                                                          \
    }                                                                                                                                    \
    if (j.lane == 0) s_ss[j.wave] = ssd;                                                                                                 \
    __syncthreads();                                                                                                                     \
    if (threadIdx.x == 0) st_agent(pss + (long long)frame * g.nblk_total + g.pb0 + j.tile, ((s_ss[0] + s_ss[1]) + s_ss[2]) + s_ss[3]);    \
    if (last_block_of_frame(tail.ticket + frame * TKS, (unsigned)tail.expected))                                                         \
        embed_scalars_frame(frame, nullptr, pss, g.nblk_total, nullptr, tail)

// ---- the key plane of a wave's frame (the *_sel sweeps, wm_k_select.hip): W_f = bank.W + kidx[frame] * bank.kstride.  The frame is
// make_job's (wave-uniform, so the table entry is one scalar load per wave and the pointer stays in SGPRs: make_rsrc's condition);
// a surplus wave of a short last quad has no frame and no table entry -- it takes key 0 and marches nothing
__device__ __forceinline__ const float* select_plane(const KeyBank& bank, const int* __restrict__ kidx, const Geom& g)
{
    const WaveJob j = make_job(g);
    const int k = j.frame < g.frames ? kidx[j.frame] : 0;
    return bank.W + (long long)k * bank.kstride;
}

}  // namespace wmk
