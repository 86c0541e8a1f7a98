// wm_keys_march.hpp -- what the group detectors share: group_march, the detector's march over one wave's segment for a
// compile-time group of G members -- the keys of a bank (k_detect_keys, wm_k_detect_keys.hip; k_detect_keys_tiles,
// wm_k_detect_keys_tiles.hip) or horizontally adjacent window offsets into one key plane (k_detect_offsets,
// wm_k_detect_offsets.hip) --, WM_GROUP_DETECT_FRAME / WM_GROUP_DETECT_MARCH, the kernels' lines around it, and WM_GROUP_RECORDS,
// the record tail of the two kernels that reduce their 2 G + 1 sums per wave or block.  The kernels differ in where a member's W
// lies and in what becomes of the sums
#pragma once
#include "wm_march.hpp"

#ifndef WM_KEYS_G
#define WM_KEYS_G 2   // keys per group (registers vs. x re-reads)
#endif
#ifndef WM_PFW_KEYS
#define WM_PFW_KEYS 2  // W rows in flight per key (must divide UNROLL): 2 keys x 2 rows keep as many W loads in flight per wave as
                       // k_detect's 3 rows, and with 3 rows the f32 ME instance spills at 3 waves per SIMD
#endif
#ifndef WM_OFFS_G
#define WM_OFFS_G 4     // offsets per group on the aligned 3x3 path (registers vs. W bytes per offset)
#endif
#ifndef WM_PFW_OFFS
#define WM_PFW_OFFS 2   // W rows in flight per group (must divide UNROLL): a row step does G members' arithmetic, so two rows
                        // ahead are as far ahead in time as k_detect_keys' two rows per key
#endif

namespace wmk {

// (the two depths are knobs of their own; both feed group_march's PF)
constexpr int KG = WM_KEYS_G;
constexpr int PFK = WM_PFW_KEYS;
constexpr int OG = WM_OFFS_G;
constexpr int PFO = WM_PFW_OFFS;
static_assert(OG >= 2 && OG <= 4, "the shared row is one 16-byte load and one load of 1..3 values");
static_assert(UNROLL % PFK == 0 && UNROLL % PFO == 0, "the W prefetch ring must divide the march group");

// the G - 1 key values behind a lane's float4
template <int N> struct ExtVec;
template <> struct ExtVec<1> { using type = float; };
template <> struct ExtVec<2> { using type = float2; };
template <> struct ExtVec<3> { using type = float3; };
__device__ __forceinline__ void ext_unpack(float v, float* o) { o[0] = pinned(v); }
__device__ __forceinline__ void ext_unpack(const float2& v, float* o) { o[0] = pinned(v.x); o[1] = pinned(v.y); }
__device__ __forceinline__ void ext_unpack(const float3& v, float* o) { o[0] = pinned(v.x); o[1] = pinned(v.y); o[2] = pinned(v.z); }

// PMarch's ring (wm_march.hpp) for the shared W row of a group of G offsets: per row the lane's 4 + G - 1 key values
template <int G, int PF>
struct WShare {
    using Ext = typename ExtVec<G - 1>::type;
    BufRsrc rs;
    unsigned pitch_b, off;
    float4 pa[PF];
    Ext pb[PF];
    int r0, last;
    // base: the key at (row offset, the group's first column offset); lanes beyond the image re-read its last 4 columns
    __device__ __forceinline__ void start(const float* base, int kc, int cols, const WaveJob& j, int first_row, int count)
    {
        rs = make_rsrc(base); pitch_b = (unsigned)kc * 4u;
        off = (unsigned)min(j.c0s + 4 * j.lane, cols - 4) * 4u;
        r0 = first_row; last = first_row + count - 1;
#pragma unroll
        for (int q = 0; q < PF; ++q) issue(q, min(r0 + q, last));
    }
    __device__ __forceinline__ void issue(int slot, int r)
    {
        pa[slot] = buf_load<float4>(rs, off, (unsigned)r * pitch_b);
        pb[slot] = buf_load<Ext>(rs, off + 16u, (unsigned)r * pitch_b);
    }
    template <int SLOT>
    __device__ __forceinline__ void take(float (&v)[4 + G - 1]) const
    {
        const float4 a = pinned(pa[SLOT]);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        ext_unpack(pb[SLOT], v + 4);
    }
    template <int SLOT>
    __device__ __forceinline__ void refill(int o)
    {
        __builtin_amdgcn_sched_barrier(0);
        issue(SLOT, min(r0 + o + PF, last));
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch where it is written (see XMarch::step)
    }
};
struct WShareNone {};

// the march of detect_march (wm_k_detect.hip) with the member-dependent half repeated for the G members of the group.  Member q's
// W is the plane at Wm[q], wpitch elements between its rows and g.cols wide: a key of a bank (wpitch = cols), or a window of a
// larger key plane (wpitch = the plane's pitch; the (LDS path) halo column is clamped to the WINDOW: its replicate border, never
// the key's next column).  SHARE (aligned path, G > 1, the members are windows one column apart: Wm[q] = Wm[0] + q): one row
// stream for the group, a lane's 4 + G - 1 values per row of which member q takes q .. q + 3; else one PMarch (and, LDS path, one
// halo stream) per member.  PF: W rows in flight per stream
template <typename T, int MASK, int PAD, int HC, bool VEC, bool EDGE, int G, bool SHARE, int PF>
__device__ __forceinline__ void group_march(const T* __restrict__ xf, long long pitch, const float* const (&Wm)[G], int wpitch,
                                            const Geom& g, const WaveJob& j, float* lds_x, float* lds_u,
                                            const float (&c)[8], float (&dot)[G], float (&nu)[G], float& nw)
{
    constexpr int HRX = MASK == 0 ? 1 : PAD;
    constexpr int NR = 2 * HRX + 1;
    constexpr int O = 4 * HC;
    constexpr int MID = HRX;
    constexpr bool HALO1 = VEC && HC == 1 && (MASK == 0 || PAD <= 3);
    static_assert(!SHARE || (HALO1 && G > 1), "the shared row serves the overlapped strips: no halo loads");
    constexpr int NM = SHARE ? 1 : G;  // per-member streams
    const int R = g.rows, C = g.cols;
    float nc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) nc[k] = -c[k];
    const int t0 = j.rs > 0 ? j.rs - 1 : 0;
    const int t1 = j.re < R ? j.re : R - 1;
    const int nu_rows = t1 - t0 + 1;
    const int n = nu_rows + 2 * HRX;
    XMarch<T, HC, HALO1 ? HRX : HRX + 1, NR, VEC, PFX, EDGE, HALO1, UNROLL> xm;
    PMarch<float, VEC, PF> wm_[NM];
    typename std::conditional<SHARE, WShare<SHARE ? G : 2, PF>, WShareNone>::type ws;
    const int c0 = j.c0s + 4 * j.lane;
    const bool left_edge = EDGE && j.c0s == 0;
    const bool has_right = !EDGE || j.c0s + STRIP <= C - 1;
    xm.start(xf, pitch, g, j, lds_x, t0 - HRX, n);
    if constexpr (SHARE) ws.start(Wm[0], wpitch, C, j, t0, nu_rows);
    else {
#pragma unroll
        for (int q = 0; q < G; ++q) wm_[q].start(Wm[q], wpitch, C, j, t0, nu_rows);
    }
    const int wh_col = j.lane == WAVE - 1 ? (j.c0s + STRIP < C ? j.c0s + STRIP : C - 1) : (j.c0s > 0 ? j.c0s - 1 : 0);
    const unsigned wh_off = (unsigned)wh_col * 4u;
    auto load_wh = [&](int q, int r) -> float {
        if constexpr (HALO1) return 0.0f;
        else if constexpr (VEC) return buf_load<float>(wm_[q].ps.rs, wh_off, (unsigned)r * wm_[q].ps.pitch_b);
        else return wm_[q].ps.base[wh_col + r * wm_[q].ps.pitch];
    };
    float whpre[G][PF];
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
        for (int s = 0; s < PF; ++s) whpre[q][s] = load_wh(q, min(t0 + s, t1));
    float uw[G][3][6];
    float eww[3][4];
#pragma unroll
    for (int q = 0; q < G; ++q)
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
            constexpr int SLOT = (Q + 2 * UNROLL - 2 * HRX) % PF;
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
            // ---- the member side: (shared row) the row's 4 + G - 1 key values once, then k_detect's operations for every member
            float wv[4 + G - 1];
            if constexpr (SHARE) ws.template take<SLOT>(wv);
#pragma unroll
            for (int q = 0; q < G; ++q) {
                float4 w;
                if constexpr (SHARE) w = make_float4(wv[q], wv[q + 1], wv[q + 2], wv[q + 3]);
                else w = wm_[q].template take<SLOT>();
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
                if constexpr (!SHARE) {
                    wm_[q].template refill<SLOT>(o);
                    if constexpr (!HALO1) {
                        __builtin_amdgcn_sched_barrier(0);
                        whpre[q][SLOT] = load_wh(q, min(t + PF, t1));
                        asm volatile("" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if constexpr (SHARE) ws.template refill<SLOT>(o);
        }
    });
    if constexpr (HALO1) {
        const bool mine = j.lane >= j.lo && j.lane <= j.hi;
#pragma unroll
        for (int q = 0; q < G; ++q) { dot[q] = mine ? dot[q] : 0.0f; nu[q] = mine ? nu[q] : 0.0f; }
        nw = mine ? nw : 0.0f;
    }
}

// the kernels' lines around the march.  They expand inside a kernel with the template parameters T, MASK, PAD, HC, VEC and the
// arguments x, pitch, fstride, g, coef, the job j of keys_job, `frame`, the wave's LDS rows s_row / s_u and the sums dot, nu, nw.
// WM_GROUP_DETECT_FRAME leaves the frame's coefficients c and plane xf behind; between the two the kernel says where its members'
// W planes lie; WM_GROUP_DETECT_MARCH chooses between the edge and the no-edge instance (SHARE holds on the instances that can
// share a row).  Macros for WM_EMBED_BODY's reason: as one function around the kernel's own lines the
// scalar prologue of all 18 k_detect_keys_tiles instances came out in another order
#define WM_GROUP_DETECT_FRAME                                                                                                             \
    float c[8];                                                                                                                          \
    _Pragma("unroll") for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];                                                            \
    const T* xf = x + (long long)frame * fstride
#define WM_GROUP_DETECT_MARCH(G, SHARE, PF, WM, WPITCH)                                                                                   \
    constexpr bool V = VEC && HC == 1; /* (as in detect_body: the halo of p = 9 exceeds one neighbour chunk) */                          \
    if (MASK != 0 || strip_on_edge<V>(g, j))                                                                                             \
        group_march<T, MASK, PAD, HC, V, true, G, (SHARE) && V, PF>(xf, pitch, WM, WPITCH, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, \
                                                                    nw);                                                                 \
    else                                                                                                                                 \
        group_march<T, MASK, PAD, HC, V, (MASK != 0), G, (SHARE) && V, PF>(xf, pitch, WM, WPITCH, g, j, s_row[j.wave], s_u[j.wave], c,   \
                                                                           dot, nu, nw)

// WM_GROUP_RECORDS: the record tail of k_detect_keys and k_detect_offsets.  It expands behind the march, where every wave of the
// block arrives, reads frame, g, j and the sums dot, nu, nw of the kernel, declares s_red, and ends the kernel (its returns are
// the kernel's).  Member q of the group is member M0 + q of the frame's NM, with the records PART [frames][NM][RSTRIDE][2]; of
// its members the group stores those whose number lies in [MLO, MHI): a short last group of keys runs past the bank
// ([k0, nkeys)), a group of offsets moved left to be full starts below its own columns ([o0 + first, o0 + G)).  WRITE_W: this
// block records ||e_w||^2 in PARTW [frames][RSTRIDE].  A macro for WM_EMBED_BODY's reason: as a function,
// or with the range given as slots of the group, 18 of the 19 kernels of wm_k_detect_keys.hip came out with other registers
#define WM_GROUP_RECORDS(G, M0, NM, MLO, MHI, RSTRIDE, WRITE_W, PART, PARTW)                                                              \
    __shared__ double s_red[WPB][2 * (G) + 1];                                                                                           \
    double d[2 * (G) + 1];                                                                                                               \
    _Pragma("unroll") for (int q = 0; q < (G); ++q) { d[2 * q] = wave_sum((double)dot[q]); d[2 * q + 1] = wave_sum((double)nu[q]); }     \
    d[2 * (G)] = wave_sum((double)nw);                                                                                                   \
    if (g.quad) {                                                                                                                        \
        /* the waves of this block are 4 frames: one record per wave (k_detect's corr_fold order, folded by k_keys_fold) */              \
        if (!j.valid || j.lane != 0) return;                                                                                             \
        _Pragma("unroll") for (int q = 0; q < (G); ++q) {                                                                                \
            if ((M0) + q < (MLO)) continue;                                                                                              \
            if ((M0) + q >= (MHI)) break;                                                                                                \
            double* p = (PART) + (((long long)frame * (NM) + (M0) + q) * (RSTRIDE) + j.rec) * 2;                                         \
            p[0] = d[2 * q]; p[1] = d[2 * q + 1];                                                                                        \
        }                                                                                                                                \
        if (WRITE_W) (PARTW)[(long long)frame * (RSTRIDE) + j.rec] = d[2 * (G)];                                                         \
        return;                                                                                                                          \
    }                                                                                                                                    \
    /* the waves of this block are 4 segments of one frame: one record per block, k_detect's ((w0 + w1) + w2) + w3 */                    \
    if (j.lane == 0) {                                                                                                                   \
        _Pragma("unroll") for (int v = 0; v < 2 * (G) + 1; ++v) s_red[j.wave][v] = d[v];                                                 \
    }                                                                                                                                    \
    __syncthreads();                                                                                                                     \
    const int v = threadIdx.x;                                                                                                           \
    if (v < 2 * (G) + 1) {                                                                                                               \
        const double s = ((s_red[0][v] + s_red[1][v]) + s_red[2][v]) + s_red[3][v];                                                      \
        const long long blk = g.pb0 + j.tile;                                                                                            \
        if (v == 2 * (G)) { if (WRITE_W) (PARTW)[(long long)frame * (RSTRIDE) + blk] = s; }                                              \
        else if ((M0) + v / 2 >= (MLO) && (M0) + v / 2 < (MHI))                                                                          \
            (PART)[(((long long)frame * (NM) + (M0) + v / 2) * (RSTRIDE) + blk) * 2 + (v & 1)] = s;                                      \
    }                                                                                                                                    \
    (void)0

}  // namespace wmk
