// wm_k_embed_signs_multi.hip -- ONE frame, many payload copies (wm_embed_signs_multi / wm_embed_bits_multi, wm.h): k_embed_signs_multi
//
// A distributor marks one frame for K recipients, every copy with its own sign table and all of them with one key.  Nothing on the
// image side depends on the table: the Gram sums, the coefficients, the mask, max|e| and -- since ||m W|| does not see the signs --
// the strength a are the frame's.  k_embed_signs_multi is k_embed_signs' march (embed_march with SIGNS, wm_embed_march.hpp) with the
// copy-dependent tail inside the row step: m, the W row, u = m W and the base row are formed once per row, then every copy of a
// compile-time group takes its tile's sign, us = u s (exact), y = clamp(fmaf(us, a, b), 0, 255) in embed_march's expression order,
// and stores its plane.  Copy groups are a grid axis in k_embed_keys' block order (keys_job): the groups of one (tile, frame) are
// consecutive blocks of one XCD, so their re-reads of x, W and base are L2 hits.  One channel of the base per launch, as k_embed_keys.
#include "wm_embed_march.hpp"

#ifndef WM_EMBED_SIGNS_G
#define WM_EMBED_SIGNS_G 2   // copies per group: the largest that keeps the aligned ME f32 instances at k_embed_signs' waves per SIMD
                             // (5 with base = input, 4 with a grey base; 3 and 4 copies lose the fifth wave: DESIGN.md section 17)
#endif

namespace wmk {

constexpr int SMG = WM_EMBED_SIGNS_G;

struct SignsMultiArgs {
    const signed char* signs;  // [frames][ncopies][ny][nx], -1 | 0 | +1
    int th, tw, ny, nx;
    int ncopies;
    int ngroups;               // copy groups = grid blocks per tile
};

// SignWalk (wm_embed_march.hpp) for the SMG tables of a group.  The tile column of a lane is fixed over its march and the tile row is
// wave-uniform (SignWalk's argument, unchanged), so the walks share ty / next_row -- the scalar bookkeeping runs once per row -- and
// differ in their table and in cur / nxt.  The tables of a frame's copies lie T = ny * nx apart: one base, one offset per copy.
struct SignWalkGroup {
    const signed char* p;  // this lane's column of the group's first table
    int off[SMG];          // table of copy q from there (wave-uniform)
    int nx, th, ny;
    int ty, next_row;      // current tile row; first row of the next one (INT_MAX in the last)
    float cur[SMG];
    int nxt[SMG];          // raw signs of tile row ty + 1 (converted when it becomes current)
    __device__ __forceinline__ void start(const signed char* table, const int (&off_)[SMG], int th_, int tw, int ny_, int nx_, int c0, int row)
    {
        nx = nx_; th = th_; ny = ny_;
        p = table + min(c0 / tw, nx - 1);
        ty = min(row / th, ny - 1);
#pragma unroll
        for (int q = 0; q < SMG; ++q) {
            off[q] = off_[q];
            cur[q] = (float)p[off[q] + ty * nx];
            nxt[q] = p[off[q] + min(ty + 1, ny - 1) * nx];
        }
        next_row = ty < ny - 1 ? (ty + 1) * th : 0x7fffffff;
    }
    // move to row `row` (rows arrive in ascending order); cur[q] is then the sign of copy q there
    __device__ __forceinline__ void advance(int row)
    {
        if (row >= next_row) {  // wave-uniform
            ++ty;
            next_row = ty < ny - 1 ? next_row + th : 0x7fffffff;
            const int r2 = min(ty + 1, ny - 1) * nx;
#pragma unroll
            for (int q = 0; q < SMG; ++q) {
                cur[q] = (float)nxt[q];
                nxt[q] = p[off[q] + r2];
            }
        }
    }
};

// embed_march's plain instance (no hand-over) on one channel, with the sign, fmaf, clamp and store repeated for the copies of the group
template <typename T, int MASK, int PAD, bool VEC, bool BX, bool EDGE>
__device__ __forceinline__ void embed_signs_multi_march(const T* __restrict__ xf, long long pitch, const float* __restrict__ W,
                                                        const T* __restrict__ bptr, T* const (&optr)[SMG], int nk, const PlaneDesc& base,
                                                        const PlaneDesc& out, const Geom& g, const WaveJob& j, float* lds, float* obuf,
                                                        const float (&c)[8], float a, float maxe, const signed char* table,
                                                        const int (&toff)[SMG], const SignsMultiArgs& sa)
{
    constexpr int NR = MASK == 0 ? 3 : 2 * PAD + 1;
    constexpr int HR = MASK == 0 ? 1 : PAD;  // halo rows above/below = halo columns left/right
    constexpr int RG = VEC && NR == 3 ? WM_RING3 : UNROLL;
    XMarch<T, 1, HR, NR, VEC, PFX, EDGE, false, RG> xm;
    PMarch<float, VEC, PFW> wm_;
    PMarch<T, VEC, PFW> bm;               // (BX: the base is the grey input, read from the stencil window)
    const float inv_maxe = 1.0f / maxe;   // (k_embed's m = |e| / max|e|: one reciprocal per wave, then div_by per pixel)
    const int nout = j.re - j.rs, n = nout + 2 * HR;
    const int c0 = j.c0s + 4 * j.lane;
    const bool own = !EDGE || 4 * j.lane >= j.dup;  // duplicate lanes of a shifted last strip: the previous strip stores these pixels
    xm.start(xf, pitch, g, j, lds, j.rs - HR, n);
    wm_.start(W, g.cols, g.cols, j, j.rs, nout);
    if (!BX) bm.start(bptr, base.pitch, g.cols, j, j.rs, nout);
    SignWalkGroup sw;
    sw.start(table, toff, sa.th, sa.tw, sa.ny, sa.nx, c0, j.rs);
    march_n<2 * HR, RG>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            const int o = i - 2 * HR;
            constexpr int SLOT = (Q + 4 * UNROLL - 2 * HR) % PFW;
            // ---- the image side, once per row: u = m W of the lane's 4 pixels and the base row
            const float4 w = wm_.template take<SLOT>();
            sw.advance(j.rs + o);
            float u[4];
            float pr[4] = {0.f, 0.f, 0.f, 0.f};
            if (MASK == 0) predict4<4>(xm.template row<Q>(0), xm.template row<Q>(1), xm.template row<Q>(2), c, pr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float m;
                if (MASK == 0) {
                    const float* mid = xm.template row<Q>(1);
                    const float e = mid[4 + k] - pr[k];
                    m = div_by(fabsf(e), maxe, inv_maxe);
                } else {
                    m = nvf_value<PAD, 4, Q>(xm, k);
                }
                u[k] = m * f4get(w, k);  // Watermark.cpp:169
            }
            float4 b;
            if (BX) {
                const float* ctr = xm.template row<Q>(HR);  // the output row itself
                b = make_float4(ctr[4], ctr[5], ctr[6], ctr[7]);
            } else {
                b = bm.template take<SLOT>();
            }
            // ---- the copy side: k_embed_signs' sign, y and store for every copy of the group
#pragma unroll
            for (int q = 0; q < SMG; ++q) {
                if (q < nk) {  // (wave-uniform: copies beyond ncopies store nothing)
                    const float sgn = sw.cur[q];
                    float4 y;
                    y.x = fminf(fmaxf(fmaf(u[0] * sgn, a, b.x), 0.0f), 255.0f);  // (u s: times the tile's sign, exact)
                    y.y = fminf(fmaxf(fmaf(u[1] * sgn, a, b.y), 0.0f), 255.0f);
                    y.z = fminf(fmaxf(fmaf(u[2] * sgn, a, b.z), 0.0f), 255.0f);
                    y.w = fminf(fmaxf(fmaf(u[3] * sgn, a, b.w), 0.0f), 255.0f);
                    if constexpr (VEC) {
                        if (own) store4<T, true>(optr[q], out.pitch, j.rs + o, c0, g.cols, y);
                    } else {
                        store_row_generic<T>(optr[q], out.pitch, j.rs + o, j.c0s, j.lane, g.cols, y, obuf);
                    }
                }
            }
            if (!BX) bm.template refill<SLOT>(o);
            wm_.template refill<SLOT>(o);
        }
    });
}

// base / out: one channel (PlaneDesc::p at that channel, cstride unused)
template <typename T, int MASK, int PAD, bool VEC, bool BX>
__global__ __launch_bounds__(BLOCK) void k_embed_signs_multi(const T* __restrict__ x, long long pitch, long long fstride,
                                                             const float* __restrict__ W, PlaneDesc base, PlaneDesc out, Geom g,
                                                             const float* __restrict__ coef, const int* __restrict__ status,
                                                             const EmbedScalars* __restrict__ scal, SignsMultiArgs sa)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];
    __shared__ __attribute__((aligned(16))) float s_out[VEC ? 1 : WPB][VEC ? 4 : STRIP];  // generic path: store re-layout rows
    int grp;
    const WaveJob j = keys_job(g, sa.ngroups, grp);
    if (!j.valid) return;
    const int frame = j.frame;
    const int k0 = grp * SMG;
    const int nk = min(SMG, sa.ncopies - k0);
    // copy (frame, k) is frame index frame * ncopies + k of `out`; copies beyond ncopies repeat the last one and store nothing
    const T* bptr = static_cast<const T*>(base.p) + (long long)frame * base.fstride;
    const int T_ = sa.ny * sa.nx;
    T* optr[SMG];
    int toff[SMG];
#pragma unroll
    for (int q = 0; q < SMG; ++q) {
        const int kq = min(k0 + q, sa.ncopies - 1);
        optr[q] = static_cast<T*>(const_cast<void*>(out.p)) + ((long long)frame * sa.ncopies + kq) * out.fstride;
        toff[q] = (kq - k0) * T_;
    }
    if (MASK == 0 && status[frame] != 0) {
        // unsolvable: every copy = base bit-exact (Watermark.cpp:164-165)
        const int c0 = j.c0s + 4 * j.lane;
#pragma unroll
        for (int q = 0; q < SMG; ++q) {
            if (q >= nk) break;
            for (int r = j.rs; r < j.re; ++r) {
                const T* rb = bptr + (long long)r * base.pitch;
                T* ro = optr[q] + (long long)r * out.pitch;
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < g.cols) ro[c0 + k] = rb[c0 + k];
            }
        }
        return;
    }
    float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MASK == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
    }
    const float a = applied_strength(scal[frame].a);  // (one strength per frame: ||m W|| does not see the signs)
    const float maxe = scal[frame].maxe;
    const T* xf = x + (long long)frame * fstride;
    const signed char* table = sa.signs + ((long long)frame * sa.ncopies + k0) * T_;  // (under the quad mapping: this wave's frame)
    if (MASK != 0 || strip_on_edge<VEC>(g, j))
        embed_signs_multi_march<T, MASK, PAD, VEC, BX, true>(xf, pitch, W, bptr, optr, nk, base, out, g, j, s_row[j.wave], s_out[VEC ? 0 : j.wave], c, a,
                                                             maxe, table, toff, sa);
    else
        embed_signs_multi_march<T, MASK, PAD, VEC, BX, (MASK != 0)>(xf, pitch, W, bptr, optr, nk, base, out, g, j, s_row[j.wave], s_out[VEC ? 0 : j.wave],
                                                                    c, a, maxe, table, toff, sa);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static inline int signs_multi_groups(int ncopies) { return (ncopies + SMG - 1) / SMG; }

// does every grid of the sweep, times the copy groups, fit a launch grid of 31 bits (from the shapes alone: under any alignment)?
bool embed_signs_multi_grid_fits(const LaunchGeom& lg, int frames, int ncopies)
{
    const long long ng = signs_multi_groups(ncopies);
    bool ok = true;
    for (int al = 0; al <= 2; ++al)
        for (int vec = 0; vec <= 1; ++vec) {
            const SweepPart sp = sweep_part(lg, frames, vec != 0, al, 1);
            ok = ok && (!sp.run || (long long)sp.grid.x * ng <= 0x7fffffffLL);
        }
    return ok;
}

void launch_embed_signs_multi(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const signed char* signs, int ncopies, const TileShape& ts)
{
    const PlaneDesc& x = sw.x;
    const SignsMultiArgs sa{signs, ts.th, ts.tw, ts.ny, ts.nx, ncopies, signs_multi_groups(ncopies)};
    // k_embed_signs' launch plan, once per channel of the base, every grid times the copy groups
    WM_DISPATCH_T(x.dtype, for_each_embed_group_launch<T>(sw, w.aligned_w, ep, sa.ngroups, [&](auto m, auto p, auto vec, auto base_is_x, dim3 grid, const Geom& g,
                                                                                              const PlaneDesc& bc, const PlaneDesc& oc) {
        WM_KLAUNCH((k_embed_signs_multi<T, decltype(m)::value, decltype(p)::value, decltype(vec)::value, decltype(base_is_x)::value>), grid, dim3(BLOCK), 0,
                   sw.s, (const T*)x.p, x.pitch, x.fstride, w.W, bc, oc, g, sw.coef, sw.status, ep.scal, sa);
    }));
}

int embed_signs_group(void) { return SMG; }

}  // namespace wmk
