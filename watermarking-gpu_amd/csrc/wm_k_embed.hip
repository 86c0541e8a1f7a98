// wm_k_embed.hip -- embed-side kernels: k_me_stats, k_nvf_stats (marches and fold tails: wm_stats_march.hpp), k_embed, k_mask (see wm_k_gram.hip header)
#include "wm_stats_march.hpp"

namespace wmk {

// =================================================================================================
// k_me_stats: e = x - c.nbrs;  per block: max|e| and sum (|e| W)^2   (WM_ME_STATS_BODY / me_stats_march, wm_stats_march.hpp)
// =================================================================================================
template <typename T, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_me_stats(const T* __restrict__ x, long long pitch, long long fstride,
                                                    const float* __restrict__ W, Geom g,
                                                    const float* __restrict__ coef, const int* __restrict__ status,
                                                    float* pmax, double* pss, ScalarsTail tail)
{
    WM_ME_STATS_BODY();
}

// =================================================================================================
// k_nvf_stats: per block sum (m_nvf W)^2          (p = 2*PAD+1)   (WM_NVF_STATS_BODY / nvf_stats_march, wm_stats_march.hpp)
// =================================================================================================
template <typename T, int PAD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_nvf_stats(const T* __restrict__ x, long long pitch, long long fstride,
                                                     const float* __restrict__ W, Geom g, double* pss, ScalarsTail tail)
{
    WM_NVF_STATS_BODY();
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
