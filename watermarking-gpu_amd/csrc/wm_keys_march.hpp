// wm_keys_march.hpp -- keys_march, the detector's march over one wave's segment for a compile-time group of keys: shared by
// k_detect_keys (wm_k_detect_keys.hip) and k_detect_keys_tiles (wm_k_detect_keys_tiles.hip), which differ only in what becomes
// of the 2 KG + 1 sums
#pragma once
#include "wm_march.hpp"

#ifndef WM_KEYS_G
#define WM_KEYS_G 2   // keys per group (registers vs. x re-reads)
#endif
#ifndef WM_PFW_KEYS
#define WM_PFW_KEYS 2  // W rows in flight per key (must divide UNROLL): 2 keys x 2 rows keep as many W loads in flight per wave as
                       // k_detect's 3 rows, and with 3 rows the f32 ME instance spills at 3 waves per SIMD
#endif

namespace wmk {

constexpr int KG = WM_KEYS_G;
constexpr int PFK = WM_PFW_KEYS;
static_assert(UNROLL % PFK == 0, "the W prefetch ring must divide the march group");

// the march of detect_march (wm_k_detect.hip) with the key-dependent half repeated for the KG keys of the group
template <typename T, int MASK, int PAD, int HC, bool VEC, bool EDGE>
__device__ __forceinline__ void keys_march(const T* __restrict__ xf, long long pitch, const float* const (&Wk)[KG],
                                           const Geom& g, const WaveJob& j, float* lds_x, float* lds_u,
                                           const float (&c)[8], float (&dot)[KG], float (&nu)[KG], float& nw)
{
    constexpr int HRX = MASK == 0 ? 1 : PAD;
    constexpr int NR = 2 * HRX + 1;
    constexpr int O = 4 * HC;
    constexpr int MID = HRX;
    const int R = g.rows, C = g.cols;
    float nc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) nc[k] = -c[k];
    const int t0 = j.rs > 0 ? j.rs - 1 : 0;
    const int t1 = j.re < R ? j.re : R - 1;
    const int nu_rows = t1 - t0 + 1;
    const int n = nu_rows + 2 * HRX;
    constexpr bool HALO1 = VEC && HC == 1 && (MASK == 0 || PAD <= 3);
    XMarch<T, HC, HALO1 ? HRX : HRX + 1, NR, VEC, PFX, EDGE, HALO1, UNROLL> xm;
    PMarch<float, VEC, PFK> wm_[KG];
    const int c0 = j.c0s + 4 * j.lane;
    const bool left_edge = EDGE && j.c0s == 0;
    const bool has_right = !EDGE || j.c0s + STRIP <= C - 1;
    xm.start(xf, pitch, g, j, lds_x, t0 - HRX, n);
#pragma unroll
    for (int q = 0; q < KG; ++q) wm_[q].start(Wk[q], C, C, j, t0, nu_rows);
    const int wh_col = j.lane == WAVE - 1 ? (j.c0s + STRIP < C ? j.c0s + STRIP : C - 1) : (j.c0s > 0 ? j.c0s - 1 : 0);
    const unsigned wh_off = (unsigned)wh_col * 4u;
    auto load_wh = [&](int q, int r) -> float {
        if constexpr (HALO1) return 0.0f;
        else if constexpr (VEC) return buf_load<float>(wm_[q].ps.rs, wh_off, (unsigned)r * wm_[q].ps.pitch_b);
        else return Wk[q][wh_col + (long long)r * C];
    };
    float whpre[KG][PFK];
#pragma unroll
    for (int q = 0; q < KG; ++q)
#pragma unroll
        for (int s = 0; s < PFK; ++s) whpre[q][s] = load_wh(q, min(t0 + s, t1));
    float uw[KG][3][6];
    float eww[3][4];
#pragma unroll
    for (int q = 0; q < KG; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) uw[q][a][b] = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) eww[a][b] = 0.f;
    const int last_col_local = C - 1 - j.c0s;
    const bool own = HALO1 || !EDGE || 4 * j.lane >= j.dup;
    march_n<2 * HRX, UNROLL>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            const int o = i - 2 * HRX;
            const int t = t0 + o;
            constexpr int SLOT = (Q + 2 * UNROLL - 2 * HRX) % PFK;
            const float* xup = xm.template row<Q>(MID - 1);
            const float* xmid = xm.template row<Q>(MID);
            const float* xdn = xm.template row<Q>(MID + 1);
            // ---- the image side, once per row: e_w and the mask of the 4 own pixels (and, LDS path, of the strip's halo columns)
            float* ew = eww[Q % 3];
            float ewn[4], m[4];
            residual4<O>(xup, xmid, xdn, nc, ewn);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ew[k] = ewn[k];
                m[k] = MASK == 0 ? fabsf(ew[k]) : nvf_value<PAD, O, Q>(xm, k);
            }
            float mh = 0.0f;  // (LDS path) lane 0: the mask at column c0s - 1, lane 63: at column c0s + STRIP
            if constexpr (!HALO1) {
                if (j.lane == 0 && !left_edge) {
                    const float eh = residual1<O>(xup, xmid, xdn, -1, nc);
                    mh = MASK == 0 ? fabsf(eh) : nvf_value<PAD, O, Q>(xm, -1);
                }
                if (j.lane == WAVE - 1 && has_right) {
                    const float eh = residual1<O>(xup, xmid, xdn, 4, nc);
                    mh = MASK == 0 ? fabsf(eh) : nvf_value<PAD, O, Q>(xm, 4);
                }
            }
            const int r = t - 1;
            const bool emit_r = r >= j.rs && r < j.re;
            const bool last_row = j.re == R && t == R - 1;
            // ---- the key side: k_detect's operations for every key of the group
#pragma unroll
            for (int q = 0; q < KG; ++q) {
                const float4 w = wm_[q].template take<SLOT>();
                const float wh = HALO1 ? 0.0f : pinned(whpre[q][SLOT]);
                float uu[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) uu[k] = m[k] * f4get(w, k);
                float* un = uw[q][Q % 3];
                if constexpr (HALO1) {
                    if constexpr (EDGE) {
                        un[0] = dpp_from_prev(uu[3], uu[0]);
                        const float nx = dpp_from_next(uu[0], uu[3]);
                        un[5] = xm.xs.rsel ? uu[3] : nx;
                    } else {
                        un[0] = dpp_from_prev_any(uu[3]);
                        un[5] = dpp_from_next_any(uu[0]);
                    }
                } else {
#pragma unroll
                    for (int k = 1; k < 4; ++k)
                        if (c0 + k >= C) uu[k] = uu[k - 1];
                    float* urow = lds_u + (2 * q + (Q & 1)) * RowBuf<1>::N;
                    reinterpret_cast<float4*>(urow)[1 + j.lane] = make_float4(uu[0], uu[1], uu[2], uu[3]);
                    if (j.lane == 0) urow[3] = left_edge ? uu[0] : mh * wh;
                    if (j.lane == WAVE - 1 && has_right) urow[4 + STRIP] = mh * wh;
                    if (!has_right) {
                        const int lk = last_col_local - 4 * j.lane;
                        if (lk >= 0 && lk < 4) urow[4 + last_col_local + 1] = uu[lk];
                    }
                    wave_lds_fence();
                    un[0] = urow[3 + 4 * j.lane];
                    un[5] = urow[8 + 4 * j.lane];
                }
                un[1] = uu[0]; un[2] = uu[1]; un[3] = uu[2]; un[4] = uu[3];
                if (o == 0 && j.rs == 0) {
#pragma unroll
                    for (int b = 0; b < 6; ++b) uw[q][(Q + 2) % 3][b] = un[b];
                }
                if (emit_r) {
                    const float* um = uw[q][(Q + 1) % 3];
                    const float* u0 = uw[q][(Q + 2) % 3];
                    const float* ewp = eww[(Q + 2) % 3];
                    float eun[4];
                    residual4<1>(um, u0, un, nc, eun);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (VEC ? own : (c0 + k < C && c0 + k >= j.own_c0)) {
                            const float eu = eun[k];
                            dot[q] = fmaf(eu, ewp[k], dot[q]);
                            nu[q] = fmaf(eu, eu, nu[q]);
                            if (q == 0) nw = fmaf(ewp[k], ewp[k], nw);
                        }
                    }
                }
                if (last_row) {
                    const float* u0 = uw[q][(Q + 2) % 3];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (VEC ? own : (c0 + k < C && c0 + k >= j.own_c0)) {
                            const float eu = residual1<1>(u0, un, un, k, nc);
                            dot[q] = fmaf(eu, ew[k], dot[q]);
                            nu[q] = fmaf(eu, eu, nu[q]);
                            if (q == 0) nw = fmaf(ew[k], ew[k], nw);
                        }
                    }
                }
                wm_[q].template refill<SLOT>(o);
                if constexpr (!HALO1) {
                    __builtin_amdgcn_sched_barrier(0);
                    whpre[q][SLOT] = load_wh(q, min(t + PFK, t1));
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    });
    if constexpr (HALO1) {
        const bool mine = j.lane >= j.lo && j.lane <= j.hi;
#pragma unroll
        for (int q = 0; q < KG; ++q) { dot[q] = mine ? dot[q] : 0.0f; nu[q] = mine ? nu[q] : 0.0f; }
        nw = mine ? nw : 0.0f;
    }
}

}  // namespace wmk
