// wm_k_bits.hip -- a payload in the mark (wm_embed_signs / wm_embed_bits, wm_detect_bits): k_embed_signs + k_bits_fold
//
// The detector's score is signed and local (wm_k_detect_tiles.hip), and the strength a = sF / (||m W|| / sqrt(N)) does not see
// the sign of W.  A frame whose tile (ty, tx) is marked with s W, s = +-1, therefore carries one bit per tile.
//   k_embed_signs  y = clamp(base + a s(ty, tx) m W, 0, 255): k_embed's last sweep with u = m W multiplied by the sign of the
//                  pixel's tile.  It is an entry point of its own around the body and the march it shares with k_embed
//                  (wm_embed_march.hpp: WM_EMBED_BODY, embed_march with SIGNS, never the Gram hand-over).  The product with +-1 or 0
//                  is exact, so fmaf(u, a, b) gives wm_embed's bits with W (+1), with -W (-1) and with a zero W (0).
//   k_bits_fold    one wave per (frame, bit) adds the three f64 sums of the bit's tiles (k_tiles_fold's output) in ascending tile
//                  index, one add after the other, and writes the bit's soft value as a result record.
#include "wm_embed_march.hpp"

namespace wmk {

template <typename TX, typename TB, int NCH, int MASK, int PAD, bool VEC, bool BX>
__global__ __launch_bounds__(BLOCK) void k_embed_signs(const TX* __restrict__ x, long long pitch, long long fstride,
                                                       const float* __restrict__ W, PlaneDesc base, PlaneDesc out, Geom g,
                                                       const float* __restrict__ coef, const int* __restrict__ status,
                                                       const EmbedScalars* __restrict__ scal, SignTable sg)
{
    const HandOver none{nullptr, 0, nullptr, nullptr, nullptr};
    WM_EMBED_BODY(false, true, none, &sg);
}

// =================================================================================================
// k_bits_fold: one wave per (frame, bit).  tiles [start[b], start[b + 1]) of `idx` are the bit's tiles in ascending index; the
// lanes load 64 of them at a time, then every lane adds them one after the other in that order (the value of lane k by
// __shfl): ((s_0 + s_1) + s_2) + ..., starting from s_0 -- the sequential f64 sum, no tree, no atomics.
//   soft = (float)dot / (float)(sqrt(nw) * sqrt(nu))   (Watermark.cpp:230); no tile => 0 / 0 = NaN; unsolvable => 0.0f
// =================================================================================================
__global__ __launch_bounds__(BLOCK) void k_bits_fold(const double* __restrict__ sums, int ntiles, int frames, int nbits,
                                                     const int* __restrict__ start, const int* __restrict__ idx,
                                                     const int* __restrict__ status, OpResult* __restrict__ res)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long id = (long long)blockIdx.x * WPB + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (id >= (long long)frames * nbits) return;  // wave-uniform
    const int frame = (int)(id / nbits), bit = (int)(id - (long long)frame * nbits);
    const int st = status[frame];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (st == 0) {
        const int t0 = start[bit], t1 = start[bit + 1];
        const double* sf = sums + (long long)frame * ntiles * 3;
        for (int b0 = t0; b0 < t1; b0 += WAVE) {
            const int cnt = min(WAVE, t1 - b0);
            double v0 = 0.0, v1 = 0.0, v2 = 0.0;
            if (lane < cnt) {
                const double* q = sf + (long long)idx[b0 + lane] * 3;
                v0 = q[0]; v1 = q[1]; v2 = q[2];
            }
            for (int k = 0; k < cnt; ++k) {
                const double s0 = __shfl(v0, k), s1 = __shfl(v1, k), s2 = __shfl(v2, k);
                if (b0 == t0 && k == 0) { a0 = s0; a1 = s1; a2 = s2; }
                else { a0 += s0; a1 += s1; a2 += s2; }
            }
        }
    }
    if (lane != 0) return;
    OpResult r;
    r.status = st;
    r.value = st == 0 ? (float)a0 / (float)(sqrt(a2) * sqrt(a1)) : 0.0f;
    res[id] = r;
}

// launchers
void launch_embed_signs(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const signed char* signs, const TileShape& ts)
{
    const PlaneDesc& x = sw.x;
    const SignTable sg{signs, ts.th, ts.tw, ts.ny, ts.nx};
    const int al = align_mode(sw.lg, x.aligned && w.aligned_w && ep.base.aligned && ep.out.aligned);
    for_embed_planes(x, ep.base, [&](auto t, auto nch_base) {
        using T = decltype(t);
        constexpr int NCH = decltype(nch_base)::value;
        const bool bx = NCH == 1 && same_plane(x, ep.base);
        for_each_embed_launch<NCH>(sw, al, bx, [&](auto m, auto p, auto vec, auto nch, auto base_is_x, const SweepPart& sp) {
            WM_KLAUNCH((k_embed_signs<T, T, decltype(nch)::value, decltype(m)::value, decltype(p)::value, decltype(vec)::value, decltype(base_is_x)::value>),
                       sp.grid, dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, w.W, ep.base, ep.out, sp.g, sw.coef, sw.status, ep.scal, sg);
        });
    });
}

void launch_bits_fold(hipStream_t s, int frames, int nbits, int ntiles, const double* sums, const int* start, const int* idx,
                      const int* status, OpResult* res)
{
    const long long n = (long long)frames * nbits;
    WM_KLAUNCH(k_bits_fold, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(BLOCK), 0, s, sums, ntiles, frames, nbits, start, idx, status, res);
}

}  // namespace wmk
