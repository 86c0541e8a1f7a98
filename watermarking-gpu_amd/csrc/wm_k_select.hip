// wm_k_select.hip -- a key per frame of a batch (wm_embed_select / wm_detect_select, wm.h): k_me_stats_sel, k_nvf_stats_sel,
// k_embed_sel, k_detect_sel
//
// Everything on the image side of an embed or a detect is independent of the key; the sweeps that read W take it as one pointer.
// These four are the single-key sweeps with that pointer resolved per frame from a bank and a device table kidx [frames]:
//     W_f = bank.W + (long long)kidx[frame] * bank.kstride          (select_plane, wm_stats_march.hpp)
// They instantiate the single-key kernels' own bodies (WM_ME_STATS_BODY, WM_NVF_STATS_BODY, WM_EMBED_BODY, detect_body) on the
// launch plans of their twins -- the same geometry, block order, frame-quad mapping, per-pixel arithmetic, partial-sum grouping,
// fold tails and tickets -- so frame f's output, strength and score are, bit for bit, what the single-key sweep of the same batch
// gives with key kidx[f] as W (tests/test_gpu_select.py).  Launch bounds are the twins'.  No hand-over and no checking / redo
// instances: the calls never take them.
//
// What changes physically: in a single-key batch the four waves of a frame-quad block read the same W rows at the same time and the
// frames of a launch share one W plane through L2; with distinct keys every frame streams its own plane from memory.  Runs of
// equal keys in the table get the sharing back by themselves (the block order keeps consecutive frames together).
#include "wm_stats_march.hpp"
#include "wm_detect_march.hpp"

namespace wmk {

template <typename T, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_me_stats_sel(const T* __restrict__ x, long long pitch, long long fstride, KeyBank bank,
                                                        const int* __restrict__ kidx, Geom g, const float* __restrict__ coef,
                                                        const int* __restrict__ status, float* pmax, double* pss, ScalarsTail tail)
{
    const float* __restrict__ W = select_plane(bank, kidx, g);
    WM_ME_STATS_BODY();
}

template <typename T, int PAD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_nvf_stats_sel(const T* __restrict__ x, long long pitch, long long fstride, KeyBank bank,
                                                         const int* __restrict__ kidx, Geom g, double* pss, ScalarsTail tail)
{
    const float* __restrict__ W = select_plane(bank, kidx, g);
    WM_NVF_STATS_BODY();
}

template <typename TX, typename TB, int NCH, int MASK, int PAD, bool VEC, bool BX>
__global__ __launch_bounds__(BLOCK, 1) void k_embed_sel(const TX* __restrict__ x, long long pitch, long long fstride, KeyBank bank,
                                                        const int* __restrict__ kidx, PlaneDesc base, PlaneDesc out, Geom g,
                                                        const float* __restrict__ coef, const int* __restrict__ status,
                                                        const EmbedScalars* __restrict__ scal)
{
    const float* __restrict__ W = select_plane(bank, kidx, g);
    const HandOver none{nullptr, 0, nullptr, nullptr, nullptr};
    WM_EMBED_BODY(false, false, none, nullptr);
}

template <typename T, int MASK, int PAD, int HC, bool VEC>
__global__ __launch_bounds__(BLOCK, WM_DET_BOUNDS) void k_detect_sel(const T* __restrict__ x, long long pitch, long long fstride,
                                                                     KeyBank bank, const int* __restrict__ kidx, Geom g,
                                                                     const float* __restrict__ coef, const int* __restrict__ status,
                                                                     double* pcorr, CorrTail tail)
{
    const DigCheck none{nullptr, nullptr, nullptr, nullptr, nullptr};
    detect_body<T, MASK, PAD, HC, VEC, 0>(x, pitch, fstride, select_plane(bank, kidx, g), g, coef, status, pcorr, tail, none);
}
#undef WM_DET_BOUNDS

// launchers: the twins' (launch_me_stats, launch_nvf_stats, launch_embed without hand-over, launch_detect's ordinary sweep)
void launch_me_stats_sel(const Sweep& sw, const KeyBank& bank, const int* kidx, float* pmax, double* pss, unsigned* ticket,
                         unsigned* ticket_strip, float* smax, double* sss, float sF, double sqrt_n, EmbedScalars* scal, OpResult* res,
                         RawSums* raw)
{
    const PlaneDesc& x = sw.x;
    const LaunchGeom& lg = sw.lg;
    const int al = align_mode(lg, x.aligned && bank.aligned_w);
    const ScalarsTail tail{ticket, ticket_strip, lg.nblk, lg.nsegs, lg.nstrips, smax, sss, sF, sqrt_n, scal, res, raw};
    WM_DISPATCH_T(x.dtype, for_each_sweep_part(sw, al, 1, [&](auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_me_stats_sel<T, decltype(vec)::value>), sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, bank, kidx, sp.g,
                   sw.coef, sw.status, pmax, pss, tail);
    }));
}

template <typename T>
static void launch_nvf_stats_sel_t(const Sweep& sw, const KeyBank& bank, const int* kidx, double* pss, const ScalarsTail& tail)
{
    const PlaneDesc& x = sw.x;
    const int al = align_mode(sw.lg, x.aligned && bank.aligned_w);
    for_mask_pad(1, sw.pad, [&](auto, auto p) {
        for_each_sweep_part(sw, al, 1, [&](auto vec, const SweepPart& sp) {
            WM_KLAUNCH((k_nvf_stats_sel<T, decltype(p)::value, decltype(vec)::value>), sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch,
                       x.fstride, bank, kidx, sp.g, pss, tail);
        });
    });
}
void launch_nvf_stats_sel(const Sweep& sw, const KeyBank& bank, const int* kidx, double* pss, unsigned* ticket, unsigned* ticket_strip,
                          double* sss, float sF, double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw)
{
    const LaunchGeom& lg = sw.lg;
    const ScalarsTail tail{ticket, ticket_strip, lg.nblk, lg.nsegs, lg.nstrips, nullptr, sss, sF, sqrt_n, scal, res, raw};
    WM_DISPATCH_T(sw.x.dtype, launch_nvf_stats_sel_t<T>(sw, bank, kidx, pss, tail));
}

void launch_embed_sel(const Sweep& sw, const KeyBank& bank, const EmbedPlanes& ep, const int* kidx)
{
    const PlaneDesc& x = sw.x;
    const int al = align_mode(sw.lg, x.aligned && bank.aligned_w && ep.base.aligned && ep.out.aligned);
    for_embed_planes(x, ep.base, [&](auto t, auto nch_base) {
        using T = decltype(t);
        constexpr int NCH = decltype(nch_base)::value;
        const bool bx = NCH == 1 && same_plane(x, ep.base);
        for_each_embed_launch<NCH>(sw, al, bx, [&](auto m, auto p, auto vec, auto nch, auto base_is_x, const SweepPart& sp) {
            WM_KLAUNCH((k_embed_sel<T, T, decltype(nch)::value, decltype(m)::value, decltype(p)::value, decltype(vec)::value, decltype(base_is_x)::value>),
                       sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, bank, kidx, ep.base, ep.out, sp.g, sw.coef, sw.status, ep.scal);
        });
    });
}

template <typename T>
static void launch_detect_sel_t(const Sweep& sw, const DetectPlan& pl, const KeyBank& bank, const int* kidx, double* pcorr, const CorrTail& tail)
{
    const PlaneDesc& x = sw.x;
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_detect_sel<T, decltype(m)::value, decltype(p)::value, decltype(hc)::value, decltype(vec)::value>), sp.grid, dim3(BLOCK),
                   0, sw.s, (const T*)x.p, x.pitch, x.fstride, bank, kidx, sp.g, sw.coef, sw.status, pcorr, tail);
    });
}
void launch_detect_sel(const Sweep& sw, const KeyBank& bank, const int* kidx, double* pcorr, unsigned* ticket, unsigned* ticket_strip,
                       double* scorr, OpResult* res, RawSums* raw)
{
    const DetectPlan pl = detect_plan(sw, bank.aligned_w);
    const LaunchGeom& ld = pl.ld;
    const CorrTail tail{ticket, ticket_strip, ld.nblk, ld.nsegs, ld.nstrips, scorr, res, raw};
    WM_DISPATCH_T(sw.x.dtype, launch_detect_sel_t<T>(sw, pl, bank, kidx, pcorr, tail));
}

}  // namespace wmk
