// wm_k_detect_offsets.hip -- k_detect_offsets: the detector of ONE image against a rectangle of window offsets into ONE key
// plane that is larger than the image (wm_detect_offsets, wm.h): where in its key does a cropped copy lie?
//
// Offset (oy, ox) scores the image against W = key[oy : oy + rows, ox : ox + cols].  The image side is wm_detect_keys' (Gram
// sweep, solve; e_w, the mask and ||e_w||^2 once per row of the march); the sweep is k_detect_keys' march (wm_k_detect_keys.hip
// keys_march) whose members are G horizontally adjacent offsets of one row offset instead of KG keys.  The point of the kernel:
// on the aligned path the G members SHARE ONE W ROW STREAM.  A lane's four pixels need, for the offsets ox .. ox + G - 1, the
// 4 + G - 1 consecutive key values key[oy + r][ox + c .. ox + c + 3 + G - 1]: one 16-byte load and one load of the G - 1 values
// behind it (the bytes the next lane loads as its own: a vector-cache hit).  Member q takes values q .. q + 3 of them; all that
// follows -- u = m w, the rolling u window with ITS OWN halos (the replicate border is the window's edge, never the key's next
// column), residual4, the dot / nu chains and the partial-sum grouping -- is keys_march's per member, so a score is bit for bit
// wm_detect_keys' on a bank that holds the window copied out (tests/test_gpu_offsets.py).  The records are laid out
// [frames][ny * nx][rstride][2] and folded by k_keys_fold with nkeys = ny * nx.
//
// Bounds.  The buffer descriptor's range check is open (make_rsrc), so every address is kept inside the key plane by
// arithmetic: a lane's column is clamped to cols - 4 (PStream's clamp), every group is FULL (a short last group starts
// G - nx % G columns further left and does not store the members it shares with its left neighbour; a remainder of at most
// G / 2 columns runs as a second launch of the G = 1 instance instead, which is cheaper), and the extra load is
// exactly G - 1 values wide -- so the last value a group touches is key column ox + cols - 4 + 3 + G - 1, the last column of
// its last member's window, which wm_detect_offsets has checked to lie inside the plane.  nx < G runs the G = 1 instance, as do
// the generic, split-remainder and NVF p > 3 instances: their members would each need a W stream and a halo stream of their
// own, and at G = 1 they are k_detect's march with a pitch.
#include "wm_march.hpp"

#ifndef WM_OFFS_G
#define WM_OFFS_G 4     // offsets per group on the aligned 3x3 path (registers vs. W bytes per offset)
#endif
#ifndef WM_PFW_OFFS
#define WM_PFW_OFFS 2   // W rows in flight per group (must divide UNROLL): a row step does G members' arithmetic, so two rows
                        // ahead are as far ahead in time as k_detect_keys' two rows per key
#endif

namespace wmk {

constexpr int OG = WM_OFFS_G;
constexpr int PFO = WM_PFW_OFFS;
static_assert(OG >= 2 && OG <= 4, "the shared row is one 16-byte load and one load of 1..3 values");
static_assert(UNROLL % PFO == 0, "the W prefetch ring must divide the march group");

struct OffsArgs {
    const float* key;   // the searched key plane [KR][KC]
    int kc;             // its pitch (elements)
    int oy0, ox0;       // first offset
    int ny, nx;         // offsets: (oy0 + i, ox0 + j), i < ny, j < nx; record index i * nx + j
    int jx_lo, nxl;     // this launch scores the columns [jx_lo, jx_lo + nxl) of every row offset in groups of its G
    int ngx;            // column groups per row offset = ceil(nxl / G)
    int ngroups;        // ny * ngx = grid blocks per tile
    int write_w;        // this launch records ||e_w||^2 (one launch of a sweep part does)
    int rstride;        // partial records per (frame, offset)
    double* part;       // [frames][ny * nx][rstride][2]  {<e_u,e_w>, ||e_u||^2}
    double* partw;      // [frames][rstride]              ||e_w||^2 (written by group 0 of the write_w launch)
};

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

// keys_march (wm_k_detect_keys.hip) with the G members' W rows taken from the window pitch kc apart: Wg = the key at the
// group's (row offset, first column offset), member q's window starts q columns further right.  SHARED (aligned path, G > 1):
// one row stream for the group; else one PMarch (and, LDS path, one halo stream) per member
template <typename T, int MASK, int PAD, int HC, bool VEC, bool EDGE, int G>
__device__ __forceinline__ void offsets_march(const T* __restrict__ xf, long long pitch, const float* __restrict__ Wg, int kc,
                                              const Geom& g, const WaveJob& j, float* lds_x, float* lds_u,
                                              const float (&c)[8], float (&dot)[G], float (&nu)[G], float& nw)
{
    constexpr int HRX = MASK == 0 ? 1 : PAD;
    constexpr int NR = 2 * HRX + 1;
    constexpr int O = 4 * HC;
    constexpr int MID = HRX;
    constexpr bool HALO1 = VEC && HC == 1 && (MASK == 0 || PAD <= 3);
    constexpr bool SHARED = VEC && G > 1;
    static_assert(!SHARED || HALO1, "the shared row serves the overlapped strips: no halo loads");
    constexpr int NM = SHARED ? 1 : G;  // per-member streams
    const int R = g.rows, C = g.cols;
    float nc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) nc[k] = -c[k];
    const int t0 = j.rs > 0 ? j.rs - 1 : 0;
    const int t1 = j.re < R ? j.re : R - 1;
    const int nu_rows = t1 - t0 + 1;
    const int n = nu_rows + 2 * HRX;
    XMarch<T, HC, HALO1 ? HRX : HRX + 1, NR, VEC, PFX, EDGE, HALO1, UNROLL> xm;
    PMarch<float, VEC, PFO> wm_[NM];
    typename std::conditional<SHARED, WShare<SHARED ? G : 2, PFO>, WShareNone>::type ws;
    const int c0 = j.c0s + 4 * j.lane;
    const bool left_edge = EDGE && j.c0s == 0;
    const bool has_right = !EDGE || j.c0s + STRIP <= C - 1;
    xm.start(xf, pitch, g, j, lds_x, t0 - HRX, n);
    if constexpr (SHARED) ws.start(Wg, kc, C, j, t0, nu_rows);
    else {
#pragma unroll
        for (int q = 0; q < G; ++q) wm_[q].start(Wg + q, kc, C, j, t0, nu_rows);
    }
    // (LDS path) the window's column beside the strip, clamped to the WINDOW: its replicate border, not the key's next column
    const int wh_col = j.lane == WAVE - 1 ? (j.c0s + STRIP < C ? j.c0s + STRIP : C - 1) : (j.c0s > 0 ? j.c0s - 1 : 0);
    const unsigned wh_off = (unsigned)wh_col * 4u;
    auto load_wh = [&](int q, int r) -> float {
        if constexpr (HALO1) return 0.0f;
        else if constexpr (VEC) return buf_load<float>(wm_[q].ps.rs, wh_off, (unsigned)r * wm_[q].ps.pitch_b);
        else return Wg[q + wh_col + (long long)r * kc];
    };
    float whpre[G][PFO];
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
        for (int s = 0; s < PFO; ++s) whpre[q][s] = load_wh(q, min(t0 + s, t1));
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
            constexpr int SLOT = (Q + 2 * UNROLL - 2 * HRX) % PFO;
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
            // ---- the key side: the row's 4 + G - 1 key values once (shared row), then k_detect's operations for every member
            float wv[4 + G - 1];
            if constexpr (SHARED) ws.template take<SLOT>(wv);
#pragma unroll
            for (int q = 0; q < G; ++q) {
                float wq[4];
                if constexpr (SHARED) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) wq[k] = wv[q + k];
                } else {
                    const float4 w = wm_[q].template take<SLOT>();
#pragma unroll
                    for (int k = 0; k < 4; ++k) wq[k] = f4get(w, k);
                }
                const float wh = HALO1 ? 0.0f : pinned(whpre[q][SLOT]);
                float uu[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) uu[k] = m[k] * wq[k];
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
                if constexpr (!SHARED) {
                    wm_[q].template refill<SLOT>(o);
                    if constexpr (!HALO1) {
                        __builtin_amdgcn_sched_barrier(0);
                        whpre[q][SLOT] = load_wh(q, min(t + PFO, t1));
                        asm volatile("" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if constexpr (SHARED) ws.template refill<SLOT>(o);
        }
    });
    if constexpr (HALO1) {
        const bool mine = j.lane >= j.lo && j.lane <= j.hi;
#pragma unroll
        for (int q = 0; q < G; ++q) { dot[q] = mine ? dot[q] : 0.0f; nu[q] = mine ? nu[q] : 0.0f; }
        nw = mine ? nw : 0.0f;
    }
}

// occupancy floor: G = 1 is k_detect_keys' budget with one member less; the shared-row instances hold G u windows
// (18 VGPRs each) beside the image side's registers
constexpr int offsets_min_blocks(int pad, int hc, bool vec, int tsize, int G)
{
    if (!(pad == 1 && hc == 1)) return 1;
    if (!vec) return 2;
    if (G == 1) return 4;
    return G <= 2 ? (tsize == 1 ? 4 : 3) : 2;
}

template <typename T, int MASK, int PAD, int HC, bool VEC, int G>
__global__ __launch_bounds__(BLOCK, offsets_min_blocks(PAD, HC, VEC, (int)sizeof(T), G)) void k_detect_offsets(
    const T* __restrict__ x, long long pitch, long long fstride, OffsArgs oa, Geom g, const float* __restrict__ coef,
    const int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * G * RowBuf<1>::N];
    __shared__ double s_red[WPB][2 * G + 1];
    int grp;  // (offset group: iy * ngx + gx, column groups fastest)
    const WaveJob j = keys_job(g, oa.ngroups, grp);
    const int frame = j.frame;
    const int iy = grp / oa.ngx, gx = grp - iy * oa.ngx;
    // every group is full: a short last group starts further left and recomputes the members below `first`, which it does not store
    const int jl0 = min(gx * G, oa.nxl - G);
    const int first = gx * G - jl0;
    const int jx0 = oa.jx_lo + jl0;
    const int noff = oa.ny * oa.nx;
    const int o0 = iy * oa.nx + jx0;  // record index of member 0
    float dot[G], nu[G], nw = 0.0f;
#pragma unroll
    for (int q = 0; q < G; ++q) { dot[q] = 0.0f; nu[q] = 0.0f; }
    if (j.valid && status[frame] == 0) {
        float c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
        const T* xf = x + (long long)frame * fstride;
        const float* Wg = oa.key + (long long)(oa.oy0 + iy) * oa.kc + (oa.ox0 + jx0);
        constexpr bool V = VEC && HC == 1;
        if (MASK != 0 || strip_on_edge<V>(g, j)) offsets_march<T, MASK, PAD, HC, V, true, G>(xf, pitch, Wg, oa.kc, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw);
        else offsets_march<T, MASK, PAD, HC, V, (MASK != 0), G>(xf, pitch, Wg, oa.kc, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw);
    }
    double d[2 * G + 1];
#pragma unroll
    for (int q = 0; q < G; ++q) { d[2 * q] = wave_sum((double)dot[q]); d[2 * q + 1] = wave_sum((double)nu[q]); }
    d[2 * G] = wave_sum((double)nw);
    if (g.quad) {
        // the waves of this block are 4 frames: one record per wave (k_detect's corr_fold order, folded by k_keys_fold)
        if (!j.valid || j.lane != 0) return;
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (q < first) continue;
            double* p = oa.part + (((long long)frame * noff + o0 + q) * oa.rstride + j.rec) * 2;
            p[0] = d[2 * q]; p[1] = d[2 * q + 1];
        }
        if (grp == 0 && oa.write_w) oa.partw[(long long)frame * oa.rstride + j.rec] = d[2 * G];
        return;
    }
    // the waves of this block are 4 segments of one frame: one record per block, k_detect's ((w0 + w1) + w2) + w3
    if (j.lane == 0) {
#pragma unroll
        for (int v = 0; v < 2 * G + 1; ++v) s_red[j.wave][v] = d[v];
    }
    __syncthreads();
    const int v = threadIdx.x;
    if (v < 2 * G + 1) {
        const double s = ((s_red[0][v] + s_red[1][v]) + s_red[2][v]) + s_red[3][v];
        const long long blk = g.pb0 + j.tile;
        if (v == 2 * G) { if (grp == 0 && oa.write_w) oa.partw[(long long)frame * oa.rstride + blk] = s; }
        else if (v / 2 >= first) oa.part[(((long long)frame * noff + o0 + v / 2) * oa.rstride + blk) * 2 + (v & 1)] = s;
    }
}

template <typename T>
static void launch_detect_offsets_t(const Sweep& sw, const DetectPlan& pl, const OffsArgs& oa1)
{
    const PlaneDesc& x = sw.x;
    // columns(): the columns [lo, lo + n) of every row offset in groups of G
    auto columns = [&](int G, int lo, int n, int write_w) {
        OffsArgs a = oa1;
        a.jx_lo = lo; a.nxl = n; a.write_w = write_w;
        a.ngx = group_count(n, G); a.ngroups = a.ny * a.ngx;
        return a;
    };
    // the aligned instance of the 3x3 windows: the shared row when a full group exists.  A remainder of nx % G columns costs a
    // whole group when the last group is moved left to be full; up to G / 2 columns are cheaper as one offset per block (the
    // G = 1 instance) in a launch of their own
    const int rem = oa1.nx % OG, tail = oa1.nx >= OG && 2 * rem <= OG ? rem : 0;
    const OffsArgs all1 = columns(1, 0, oa1.nx, 1);  // every offset a block of its own
    // every grid times the offset groups of its instance
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        constexpr int MASK = decltype(m)::value, PAD = decltype(p)::value, HC = decltype(hc)::value;
        constexpr bool VEC = decltype(vec)::value;
        auto go = [&](auto g, const OffsArgs& oa) {
            WM_KLAUNCH((k_detect_offsets<T, MASK, PAD, HC, VEC, decltype(g)::value>), dim3(sp.grid.x * (unsigned)oa.ngroups), dim3(BLOCK), 0, sw.s,
                       (const T*)x.p, x.pitch, x.fstride, oa, sp.g, sw.coef, sw.status);
        };
        if constexpr (VEC && PAD == 1) {
            if (oa1.nx >= OG) {
                go(IC<OG>{}, columns(OG, 0, oa1.nx - tail, 1));
                if (tail) go(IC<1>{}, columns(1, oa1.nx - tail, tail, 0));
                return;
            }
        }
        go(IC<1>{}, all1);
    });
}

int detect_offsets_group(void) { return OG; }

int launch_detect_offsets(const Sweep& sw, const KeyBank& key, int key_cols, int oy0, int ox0, int ny, int nx, double* part, int rstride,
                          OpResult* res)
{
    // the geometry comes from the IMAGE plane alone (detect_plan, as for every detector)
    const DetectPlan pl = detect_plan(sw, key.aligned_w);
    const LaunchGeom& ld = pl.ld;
    const int frames = sw.frames;
    const bool quad = frames >= 4;
    if (ld.nblk > rstride || ld.nstrips * ld.nsegs > rstride || ld.nstrips > KEYS_MAX_STRIPS) return -1;
    const int noff = ny * nx;
    OffsArgs oa;
    oa.key = key.W; oa.kc = key_cols; oa.oy0 = oy0; oa.ox0 = ox0; oa.ny = ny; oa.nx = nx; oa.jx_lo = 0; oa.nxl = nx; oa.ngx = nx; oa.ngroups = noff; oa.write_w = 1;
    oa.rstride = rstride; oa.part = part; oa.partw = part + (size_t)frames * noff * rstride * 2;
    WM_DISPATCH_T(sw.x.dtype, launch_detect_offsets_t<T>(sw, pl, oa));
    launch_keys_fold(sw.s, oa.part, oa.partw, rstride, frames, noff, quad ? 1 : 0, ld.nblk, ld.nsegs, ld.nstrips, sw.status, res);
    return 0;
}

}  // namespace wmk
