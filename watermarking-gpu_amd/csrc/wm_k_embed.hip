// wm_k_embed.hip -- embed-side kernels: k_me_stats, k_nvf_stats (fold tail embed_scalars_frame), k_embed, k_mask (see wm_k_gram.hip header)
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

template <typename T, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_me_stats(const T* __restrict__ x, long long pitch, long long fstride,
                                                    const float* __restrict__ W, Geom g,
                                                    const float* __restrict__ coef, const int* __restrict__ status,
                                                    float* pmax, double* pss, ScalarsTail tail)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];
    __shared__ float s_mx[WPB];
    __shared__ double s_ss[WPB];
    const WaveJob j = make_job(g);
    const int frame = j.frame;
    float mx = 0.0f, ss = 0.0f;
    if (j.valid && status[frame] == 0) {
        float c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
        const T* xf = x + (long long)frame * fstride;
        if (strip_on_edge<VEC>(g, j)) me_stats_march<T, VEC, true>(xf, pitch, W, g, j, s_row[j.wave], c, mx, ss);
        else me_stats_march<T, VEC, false>(xf, pitch, W, g, j, s_row[j.wave], c, mx, ss);
    }
    mx = wave_max(mx);
    const double ssd = wave_sum((double)ss);
    if (g.quad) {
        // the waves of this block are 4 frames: one record per wave, folded per strip and then per frame (stats_fold)
        if (!j.valid) return;  // surplus wave of a short last quad (wave-uniform; no barrier below)
        if (j.lane == 0) {
            const long long pb = (long long)frame * g.nrec + j.rec;
            st_agent(pmax + pb, mx);
            st_agent(pss + pb, ssd);
        }
        stats_fold(frame, j, pmax, pss, g.nrec, status, tail);
        return;
    }
    // the waves of this block are 4 segments of one frame: one record per block, folded by the frame's last block
    if (j.lane == 0) { s_mx[j.wave] = mx; s_ss[j.wave] = ssd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long pb = (long long)frame * g.nblk_total + g.pb0 + j.tile;
        st_agent(pmax + pb, fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3])));
        st_agent(pss + pb, ((s_ss[0] + s_ss[1]) + s_ss[2]) + s_ss[3]);
    }
    if (last_block_of_frame(tail.ticket + frame * TKS, (unsigned)tail.expected))
        embed_scalars_frame(frame, pmax, pss, g.nblk_total, status, tail);
}

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

template <typename T, int PAD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_nvf_stats(const T* __restrict__ x, long long pitch, long long fstride,
                                                     const float* __restrict__ W, Geom g, double* pss, ScalarsTail tail)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];
    __shared__ double s_ss[WPB];
    const WaveJob j = make_job(g);
    const int frame = j.frame;
    float ss = 0.0f;
    if (j.valid) {
        const T* xf = x + (long long)frame * fstride;
        nvf_stats_march<T, PAD, VEC>(xf, pitch, W, g, j, s_row[j.wave], ss);
    }
    const double ssd = wave_sum((double)ss);
    if (g.quad) {
        if (!j.valid) return;
        if (j.lane == 0) st_agent(pss + (long long)frame * g.nrec + j.rec, ssd);
        stats_fold(frame, j, nullptr, pss, g.nrec, nullptr, tail);
        return;
    }
    if (j.lane == 0) s_ss[j.wave] = ssd;
    __syncthreads();
    if (threadIdx.x == 0) st_agent(pss + (long long)frame * g.nblk_total + g.pb0 + j.tile, ((s_ss[0] + s_ss[1]) + s_ss[2]) + s_ss[3]);
    if (last_block_of_frame(tail.ticket + frame * TKS, (unsigned)tail.expected))
        embed_scalars_frame(frame, nullptr, pss, g.nblk_total, nullptr, tail);
}

// =================================================================================================
// k_embed: y = clamp(base + a * m * W, 0, 255) with the mask recomputed on the fly (WM_EMBED_BODY / embed_march, wm_embed_march.hpp)
//   MASK 0 (ME): m = |e| / max|e|;  MASK 1 (NVF): m = nvf(x);  HO: with the Gram hand-over
// =================================================================================================
#ifndef WM_HO_BLOCKS
#define WM_HO_BLOCKS 1
#endif
template <typename TX, typename TB, int NCH, int MASK, int PAD, bool VEC, bool BX, bool HO = false>
__global__ __launch_bounds__(BLOCK, HO ? WM_HO_BLOCKS : 1) void k_embed(const TX* __restrict__ x, long long pitch, long long fstride,
                                                 const float* __restrict__ W, PlaneDesc base, PlaneDesc out, Geom g,
                                                 const float* __restrict__ coef, const int* __restrict__ status,
                                                 const EmbedScalars* __restrict__ scal, HandOver ho)
{
    WM_EMBED_BODY(HO, false, ho, nullptr);
}

// =================================================================================================
// k_mask: materialise the mask (and the error sequence) -- parity-test building block
// =================================================================================================
template <typename T, int MASK, int PAD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_mask(const T* __restrict__ x, long long pitch, long long fstride, Geom g,
                                                const float* __restrict__ coef, const int* __restrict__ status,
                                                const EmbedScalars* __restrict__ scal, PlaneDesc mo, PlaneDesc eo)
{
    constexpr int NR = MASK == 0 ? 3 : 2 * PAD + 1;
    constexpr int HR = MASK == 0 ? 1 : PAD;
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];
    const WaveJob j = make_job(g);
    const int frame = j.frame;
    if (!j.valid) return;
    if (MASK == 0 && status[frame] != 0) return;
    float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float maxe = 1.0f;
    if (MASK == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
        maxe = scal[frame].maxe;
    }
    const float inv_maxe = 1.0f / maxe;
    float* mptr = static_cast<float*>(const_cast<void*>(mo.p)) + (long long)frame * mo.fstride;
    float* eptr = eo.p ? static_cast<float*>(const_cast<void*>(eo.p)) + (long long)frame * eo.fstride : nullptr;
    const int nout = j.re - j.rs, n = nout + 2 * HR;
    const int c0 = j.c0s + 4 * j.lane;
    const T* xf = x + (long long)frame * fstride;
    {
        XMarch<T, 1, HR, NR, VEC, PFX> xm;
        xm.start(xf, pitch, g, j, s_row[j.wave], j.rs - HR, n);
        march<2 * HR>(n, [&](int i, auto qc, auto emit) {
            constexpr int Q = decltype(qc)::value;
            xm.template step<Q>(i);
            if (decltype(emit)::value) {
                float mv[4], ev[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (MASK == 0) {
                        const float* mid = xm.template row<Q>(1);
                        ev[k] = mid[4 + k] - predict<4>(xm.template row<Q>(0), mid, xm.template row<Q>(2), k, c);
                        mv[k] = div_by(fabsf(ev[k]), maxe, inv_maxe);  // as k_embed computes it
                    } else {
                        ev[k] = 0.0f;
                        mv[k] = nvf_value<PAD, 4, Q>(xm, k);
                    }
                }
                if (4 * j.lane < j.dup) return;  // duplicate lanes of a shifted last strip (j.dup = 0 otherwise)
                store4<float, false>(mptr, mo.pitch, j.rs + i - 2 * HR, c0, g.cols, make_float4(mv[0], mv[1], mv[2], mv[3]));
                if (MASK == 0 && eptr)
                    store4<float, false>(eptr, eo.pitch, j.rs + i - 2 * HR, c0, g.cols, make_float4(ev[0], ev[1], ev[2], ev[3]));
            }
        });
    }
}

// launchers
static ScalarsTail scalars_tail(const LaunchGeom& lg, unsigned* ticket, unsigned* ticket_strip, float* smax, double* sss, float sF,
                                double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw)
{
    // ticket: [frames] frame-level counters followed (at ticket_strip) by [frames][nstrips] strip-level counters
    return ScalarsTail{ticket, ticket_strip, lg.nblk, lg.nsegs, lg.nstrips, smax, sss, sF, sqrt_n, scal, res, raw};
}

void launch_me_stats(const Sweep& sw, const KeyBank& w, float* pmax, double* pss, unsigned* ticket, unsigned* ticket_strip, float* smax,
                     double* sss, float sF, double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw)
{
    const PlaneDesc& x = sw.x;
    const int al = align_mode(sw.lg, x.aligned && w.aligned_w);
    const ScalarsTail tail = scalars_tail(sw.lg, ticket, ticket_strip, smax, sss, sF, sqrt_n, scal, res, raw);
    WM_DISPATCH_T(x.dtype, for_each_sweep_part(sw, al, 1, [&](auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_me_stats<T, decltype(vec)::value>), sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, w.W, sp.g, sw.coef,
                   sw.status, pmax, pss, tail);
    }));
}

template <typename T>
static void launch_nvf_stats_t(const Sweep& sw, const KeyBank& w, double* pss, const ScalarsTail& tail)
{
    const PlaneDesc& x = sw.x;
    const int al = align_mode(sw.lg, x.aligned && w.aligned_w);
    for_mask_pad(1, sw.pad, [&](auto, auto p) {
        for_each_sweep_part(sw, al, 1, [&](auto vec, const SweepPart& sp) {
            WM_KLAUNCH((k_nvf_stats<T, decltype(p)::value, decltype(vec)::value>), sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch,
                       x.fstride, w.W, sp.g, pss, tail);
        });
    });
}
void launch_nvf_stats(const Sweep& sw, const KeyBank& w, double* pss, unsigned* ticket, unsigned* ticket_strip, double* sss, float sF,
                      double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw)
{
    const ScalarsTail tail = scalars_tail(sw.lg, ticket, ticket_strip, nullptr, sss, sF, sqrt_n, scal, res, raw);
    WM_DISPATCH_T(sw.x.dtype, launch_nvf_stats_t<T>(sw, w, pss, tail));
}

template <typename TX, typename TB, int NCH>
static bool launch_embed_tt(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const HandOver* ho)
{
    const LaunchGeom& lg = sw.lg;
    const PlaneDesc& x = sw.x;
    const int al = align_mode(lg, x.aligned && w.aligned_w && ep.base.aligned && ep.out.aligned);
    const bool bx = NCH == 1 && std::is_same<TX, TB>::value && same_plane(x, ep.base);
    const HandOver none{nullptr, 0, nullptr, nullptr, nullptr};
    if constexpr (NCH == 1 && std::is_same<TX, float>::value && std::is_same<TB, float>::value) {
        // Gram hand-over: every strip on the aligned path (one launch), 3x3 windows, a core, segments of two rows or more; two
        // frames or more (measured at 4K: one frame -3 %, two +2 %, four +6..9 %, eight and more +9..11 % -- a one-frame launch of
        // k_gram_ho is as latency-bound as the k_gram it replaces)
        if (ho && ho->rec && ho->dig && sw.frames >= 2 && al == 2 && lg.nfull > 0 && sw.pad == 1 && lg.rps >= 2 && lg.rows >= 4 && lg.cols >= 5 && lg.row_lo == 0 && lg.row_hi == lg.rows) {
            const SweepPart pv_ = sweep_part(lg, sw.frames, true, al, 1);
            const Geom g = pv_.g;
#define EMB_HO(MASK)                                                                                                            \
            do {                                                                                                                \
                if (bx) WM_KLAUNCH((k_embed<float, float, 1, MASK, 1, true, true, true>), pv_.grid, dim3(BLOCK), 0, sw.s, (const float*)x.p, x.pitch, \
                                   x.fstride, w.W, ep.base, ep.out, g, sw.coef, sw.status, ep.scal, *ho);                        \
                else WM_KLAUNCH((k_embed<float, float, 1, MASK, 1, true, false, true>), pv_.grid, dim3(BLOCK), 0, sw.s, (const float*)x.p, x.pitch,  \
                                x.fstride, w.W, ep.base, ep.out, g, sw.coef, sw.status, ep.scal, *ho);                           \
            } while (0)
            if (sw.mask == 0) EMB_HO(0); else EMB_HO(1);
#undef EMB_HO
            return true;
        }
    }
    for_each_embed_launch<NCH>(sw, al, bx, [&](auto m, auto p, auto vec, auto nch, auto base_is_x, const SweepPart& sp) {
        WM_KLAUNCH((k_embed<TX, TB, decltype(nch)::value, decltype(m)::value, decltype(p)::value, decltype(vec)::value, decltype(base_is_x)::value>),
                   sp.grid, dim3(BLOCK), 0, sw.s, (const TX*)x.p, x.pitch, x.fstride, w.W, ep.base, ep.out, sp.g, sw.coef, sw.status, ep.scal, none);
    });
    return false;
}
bool launch_embed(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const HandOver* ho)
{
    bool handed = false;
    for_embed_planes(sw.x, ep.base, [&](auto t, auto nch) {
        handed = launch_embed_tt<decltype(t), decltype(t), decltype(nch)::value>(sw, w, ep, ho);
    });
    return handed;
}

template <typename T>
static void launch_mask_t(const Sweep& sw, const EmbedScalars* scal, const PlaneDesc& mo, const PlaneDesc& eo)
{
    const PlaneDesc& x = sw.x;
    // exercises the same two input paths as the production kernels (DPP for aligned full strips, LDS otherwise)
    const int al = align_mode(sw.lg, x.aligned != 0);
    for_mask_pad(sw.mask, sw.pad, [&](auto m, auto p) {
        for_each_sweep_part(sw, al, 0, [&](auto vec, const SweepPart& sp) {
            WM_KLAUNCH((k_mask<T, decltype(m)::value, decltype(p)::value, decltype(vec)::value>), sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p,
                       x.pitch, x.fstride, sp.g, sw.coef, sw.status, scal, mo, eo);
        });
    });
}
void launch_mask(const Sweep& sw, const EmbedScalars* scal, const PlaneDesc& mo, const PlaneDesc& eo)
{
    WM_DISPATCH_T(sw.x.dtype, launch_mask_t<T>(sw, scal, mo, eo));
}

}  // namespace wmk
