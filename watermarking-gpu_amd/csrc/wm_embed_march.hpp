// wm_embed_march.hpp -- embed_march, the embed sweep's march over one wave's segment, and WM_EMBED_BODY, the kernel body around it:
// shared by k_embed (wm_k_embed.hip; plain and with the Gram hand-over) and k_embed_signs (wm_k_bits.hip; the tile's sign in the
// row step), with the launch loop the two have in common; and embed_group_march with WM_EMBED_GROUP_BODY / WM_EMBED_GROUP_MARCH, the
// same march and body on one channel with the copy-dependent tail repeated for a group of copies: shared by the multi-copy embed
// kernels k_embed_keys (wm_k_embed_keys.hip) and k_embed_signs_multi (wm_k_embed_signs_multi.hip), with their per-channel launch loop
#pragma once
#include "wm_march.hpp"

#ifndef WM_RING3
#define WM_RING3 UNROLL   // ring length of the 3-row x windows of k_me_stats / k_embed (rows in flight per wave = ring - 3)
#endif

#ifndef WM_HO_PFW
#define WM_HO_PFW 3   // W / base rows in flight per wave in the hand-over instantiation of k_embed: 3 instead of 6 brings it from
                      // 174 to 162 VGPRs, i.e. three waves per SIMD instead of two (+0.8 % frames/s on the hand-over leg)
#endif

namespace wmk {

// =================================================================================================
// Gram hand-over (HandOver, wm_kernels.hpp): the lag products of y that stay inside this wave's tile, accumulated as
// k_gram's march accumulates them (f64 FMAs of exact products; window of rows q, q+1, q+2 x columns c0-2 .. c0+5 in rotating
// slots).  The partner rows behind the segment (q+1, q+2 of its last q rows) are computed here as well -- the march runs two
// rows further, without storing them -- so that no product is left open between vertically adjacent tiles; what a lane cannot
// see is y in other strips (lanes 0 / 63 get zeros for the neighbour they do not have): k_gram_ho's column seams (wm_k_gram.hip),
// for which the lanes at a strip's two ends also store their two outermost columns of every row to a compact array (read back
// from the plane, those 16 bytes per row and boundary would cost two 128-byte lines each).
// =================================================================================================
struct HoState {
    double w[3][8];
    double acc[13];
    bool cv[4];
};
// the products of q row `w0` with itself (dr = 0), with `w1` (dr = 1) and with `w2` (dr = 2)
__device__ __forceinline__ void ho_products(HoState& h, const double* w0, const double* w1, const double* w2)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xq = h.cv[k] ? w0[2 + k] : 0.0;
        h.acc[0] = fma(xq, w0[2 + k], h.acc[0]);
        h.acc[1] = fma(xq, w0[3 + k], h.acc[1]);
        h.acc[2] = fma(xq, w0[4 + k], h.acc[2]);
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            h.acc[3 + b] = fma(xq, w1[k + b], h.acc[3 + b]);
            h.acc[8 + b] = fma(xq, w2[k + b], h.acc[8 + b]);
        }
    }
}
// row r of y enters slot S; q row r - 2 (slot S + 1) is complete when `qvalid` (a core row of this segment)
template <int S>
__device__ __forceinline__ void ho_row(HoState& h, const float4& y, bool qvalid)
{
    double* s2 = h.w[S];
    s2[0] = (double)dpp_from_prev(y.z, 0.0f); s2[1] = (double)dpp_from_prev(y.w, 0.0f);
    s2[2] = (double)y.x; s2[3] = (double)y.y; s2[4] = (double)y.z; s2[5] = (double)y.w;
    s2[6] = (double)dpp_from_next(y.x, 0.0f); s2[7] = (double)dpp_from_next(y.y, 0.0f);
    if (qvalid) ho_products(h, h.w[(S + 1) % 3], h.w[(S + 2) % 3], s2);
}

// =================================================================================================
// The sign of a pixel's tile (k_embed_signs).  Tile geometry is wm_tiles_shape's: pixel (r, c) belongs to tile
// (min(r / th, ny - 1), min(c / tw, nx - 1)).
//  * column: a lane's four columns start at c0 = c0s + 4 lane, and c0s is a multiple of 4 in every strip this sweep launches (full
//    strips at multiples of 256; the shifted last strip at cols - 256 with cols a multiple of 4, align_mode; the generic strips at
//    multiples of 256 as well).  tw is a multiple of 4, so the four columns lie in ONE tile column, fixed over the march.
//  * row: wave-uniform, changes every th rows; segments need not line up with tiles.  A lane holds the sign of the current tile
//    row and, already loaded, that of the next one: the load for tile row ty + 2 is issued when the march enters ty + 1, at least
//    th >= 32 rows ahead of its use.
// =================================================================================================
struct SignWalk {
    const signed char* p;  // this lane's column of the frame's [ny][nx] table
    int nx, th, ny;
    int ty, next_row;      // current tile row; first row of the next one (INT_MAX in the last)
    float cur;
    int nxt;               // raw sign of tile row ty + 1 (converted when it becomes current)
    __device__ __forceinline__ void start(const signed char* table, int th_, int tw, int ny_, int nx_, int c0, int row)
    {
        nx = nx_; th = th_; ny = ny_;
        p = table + min(c0 / tw, nx - 1);
        ty = min(row / th, ny - 1);
        cur = (float)p[ty * nx];
        nxt = p[min(ty + 1, ny - 1) * nx];
        next_row = ty < ny - 1 ? (ty + 1) * th : 0x7fffffff;
    }
    // the sign of row `row` (rows arrive in ascending order)
    __device__ __forceinline__ float at(int row)
    {
        if (row >= next_row) {  // wave-uniform
            cur = (float)nxt;
            ++ty;
            next_row = ty < ny - 1 ? next_row + th : 0x7fffffff;
            nxt = p[min(ty + 1, ny - 1) * nx];
        }
        return cur;
    }
};

// SignWalk for the G tables of a copy group (k_embed_signs_multi).  The tile column of a lane is fixed over its march and the tile row
// is wave-uniform (SignWalk's argument, unchanged), so the walks share ty / next_row -- the scalar bookkeeping runs once per row -- and
// differ in their table and in cur / nxt.  The tables of a frame's copies lie ny * nx apart: one base, one offset per copy.
template <int G>
struct SignWalkGroup {
    const signed char* p;  // this lane's column of the group's first table
    int off[G];            // table of copy q from there (wave-uniform)
    int nx, th, ny;
    int ty, next_row;      // current tile row; first row of the next one (INT_MAX in the last)
    float cur[G];
    int nxt[G];            // raw signs of tile row ty + 1 (converted when it becomes current)
    __device__ __forceinline__ void start(const signed char* table, const int* off_, int th_, int tw, int ny_, int nx_, int c0, int row)
    {
        nx = nx_; th = th_; ny = ny_;
        p = table + min(c0 / tw, nx - 1);
        ty = min(row / th, ny - 1);
#pragma unroll
        for (int q = 0; q < G; ++q) {
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
            for (int q = 0; q < G; ++q) {
                cur[q] = (float)nxt[q];
                nxt[q] = p[off[q] + r2];
            }
        }
    }
};

struct SignTable {
    const signed char* signs;  // [frames][ny][nx], -1 | 0 | +1
    int th, tw, ny, nx;
};

// =================================================================================================
// embed_march: y = clamp(base + a * m * W, 0, 255) with the mask recomputed on the fly
//   MASK 0 (ME): m = |e| / max|e|;  MASK 1 (NVF): m = nvf(x)
//   HO:    the Gram hand-over above (k_embed's hand-over instance)
//   SIGNS: u = m W times the sign of the pixel's tile (k_embed_signs).  The product with +-1 or 0 is exact, so fmaf(u, a, b) gives
//          the plain march's bits with W (+1), with -W (-1) and with a zero W (0)
// =================================================================================================
template <typename TX, typename TB, int NCH, int MASK, int PAD, bool VEC, bool BX, bool EDGE, bool HO = false, bool SIGNS = false>
__device__ __forceinline__ void embed_march(const TX* __restrict__ xf, long long pitch, const float* __restrict__ W,
                                            const TB* __restrict__ bptr, TB* __restrict__ optr, const PlaneDesc& base,
                                            const PlaneDesc& out, const Geom& g, const WaveJob& j, float* lds, float* obuf,
                                            const float (&c)[8], float a, float maxe, bool pass = false, double* horec = nullptr,
                                            float* hoseam = nullptr, unsigned long long* hodig = nullptr,
                                            const SignTable* sg = nullptr)
{
    static_assert(!HO || (VEC && NCH == 1 && sizeof(TB) == 4), "hand-over: grey f32 planes on the aligned path");
    static_assert(!(HO && SIGNS), "the signed embed never hands over");
    constexpr int NR = MASK == 0 ? 3 : 2 * PAD + 1;
    constexpr int HR = MASK == 0 ? 1 : PAD;  // halo rows above/below = halo columns left/right
    constexpr int RG = VEC && NR == 3 ? WM_RING3 : UNROLL;
    XMarch<TX, 1, HR, NR, VEC, PFX, EDGE, false, RG> xm;
    constexpr int PW = HO ? WM_HO_PFW : PFW;  // rows of W / base in flight per wave
    PMarch<float, VEC, PW> wm_;
    // m = |e| / max|e| (Watermark.cpp:213-214): one reciprocal per wave, then div_by() per pixel (same quotient)
    const float inv_maxe = 1.0f / maxe;
    // BX: the base IS the grey input plane (video frames, grey images): its pixels are already in the stencil window,
    // so the base stream -- a third of this kernel's loads -- is not issued at all
    PMarch<TB, VEC, PW> bm[BX ? 1 : NCH];
    // (hand-over: up to two rows of y behind the segment are computed, not stored -- the partner rows of its last q rows)
    const int nout = j.re - j.rs, nrow = nout + (HO ? min(2, g.rows - j.re) : 0), n = nrow + 2 * HR;
    const int c0 = j.c0s + 4 * j.lane;
    xm.start(xf, pitch, g, j, lds, j.rs - HR, n);
    wm_.start(W, g.cols, g.cols, j, j.rs, nrow);
    if (!BX) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) bm[ch].start(bptr + (long long)ch * base.cstride, base.pitch, g.cols, j, j.rs, nrow);
    }
    HoState ho;
    if constexpr (HO) {
        static_assert(!HO || (HR == 1 && RG % 3 == 0), "hand-over: 3x3 windows (one x row ahead of the output row)");
#pragma unroll
        for (int a_ = 0; a_ < 3; ++a_)
#pragma unroll
            for (int b_ = 0; b_ < 8; ++b_) ho.w[a_][b_] = 0.0;
#pragma unroll
        for (int l = 0; l < 13; ++l) ho.acc[l] = 0.0;
        // q pixels: the core columns 2 .. C-3 this lane owns (k_gram's column factor)
#pragma unroll
        for (int k = 0; k < 4; ++k) ho.cv[k] = !EDGE || (c0 + k >= 2 && c0 + k <= g.cols - 3 && 4 * j.lane >= j.dup);
    }
    // digest of the stored y (dig_add, wm_device.hpp): the pixels this lane stores, as stored
    unsigned long long dig = 0;
    const uint32_t dcb = HO ? dig_col_key4(c0) : 0u;
    // this lane's entry of the seam array, or null: lane 63 holds columns S-2, S-1 of the boundary behind its strip, the first
    // lane that owns pixels (lane 0, or dup / 4 in a shifted last strip) holds columns S, S+1 of the boundary in front of it
    float* seamp = nullptr;
    bool seam_right = false;  // this lane stores its LAST two columns (the boundary behind the strip), else its first two
    if constexpr (HO) {
        const long long per_frame = (long long)(g.nstrips_total - 1) * g.rows * 4;
        if (j.lane == WAVE - 1 && j.strip < g.nstrips_total - 1) { seamp = hoseam + (long long)j.frame * per_frame + (long long)j.strip * g.rows * 4; seam_right = true; }
        else if (4 * j.lane == j.dup && j.strip > 0) seamp = hoseam + (long long)j.frame * per_frame + (long long)(j.strip - 1) * g.rows * 4 + 2;
    }
    SignWalk sw;
    if constexpr (SIGNS) sw.start(sg->signs + (long long)j.frame * sg->ny * sg->nx, sg->th, sg->tw, sg->ny, sg->nx, c0, j.rs);
    march_n<2 * HR, RG>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            const int o = i - 2 * HR;
            constexpr int SLOT = (Q + 4 * UNROLL - 2 * HR) % PW;
            const float4 w = wm_.template take<SLOT>();
            float sgn = 1.0f;
            if constexpr (SIGNS) sgn = sw.at(j.rs + o);
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
                if constexpr (SIGNS) u[k] *= sgn;  // times the tile's sign (exact)
            }
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                float4 b;
                if (BX) {
                    const float* ctr = xm.template row<Q>(HR);  // the output row itself
                    b = make_float4(ctr[4], ctr[5], ctr[6], ctr[7]);
                } else {
                    b = bm[ch].template take<SLOT>();
                }
                float4 y;
                y.x = fminf(fmaxf(fmaf(u[0], a, b.x), 0.0f), 255.0f);
                y.y = fminf(fmaxf(fmaf(u[1], a, b.y), 0.0f), 255.0f);
                y.z = fminf(fmaxf(fmaf(u[2], a, b.z), 0.0f), 255.0f);
                y.w = fminf(fmaxf(fmaf(u[3], a, b.w), 0.0f), 255.0f);
                if constexpr (HO) {
                    if (pass) y = b;  // unsolvable frame: out = base bit-exact (Watermark.cpp:164-165), and that is the plane the detector reads
                    const int rq = j.rs + o - 2;  // the q row that row o completes (core rows 1 .. R-3; rq < re by construction)
                    ho_row<Q % 3>(ho, y, o >= 2 && rq >= 1 && rq < g.rows - 2);
                    if (seamp && o < nout)
                        *reinterpret_cast<float2*>(seamp + (long long)(j.rs + o) * 4) = seam_right ? make_float2(y.z, y.w) : make_float2(y.x, y.y);
                    if (o < nout && (!EDGE || 4 * j.lane >= j.dup))  // (duplicate lanes of a shifted last strip store nothing)
                        dig_add4(dig, y.x, y.y, y.z, y.w, dig_row_key(j.rs + o), dcb);
                }
                if constexpr (VEC) {
                    if ((!EDGE || 4 * j.lane >= j.dup) && (!HO || o < nout))  // duplicate lanes of a shifted last strip: the previous strip stores these pixels
                        store4<TB, true>(optr + (long long)ch * out.cstride, out.pitch, j.rs + o, c0, g.cols, y);
                } else {
                    store_row_generic<TB>(optr + (long long)ch * out.cstride, out.pitch, j.rs + o, j.c0s, j.lane, g.cols, y, obuf);
                }
                if (!BX) bm[ch].template refill<SLOT>(o);
            }
            wm_.template refill<SLOT>(o);
        }
    });
    if constexpr (HO) {
        int idx;
        const double t = wave_sum_multi<13>(ho.acc, j.lane, idx);
        if (idx < 13) horec[idx] = t;
        const unsigned long long dw = wave_sum_u64(dig);
        if (j.lane == 0) *hodig = dw;
    }
}

// WM_EMBED_BODY: the body of k_embed and k_embed_signs -- the frame's planes, the unsolvable pass-through, coefficients and scalars, and
// the choice between the edge and the no-edge instance of the march.  It expands inside a kernel with k_embed's template parameters
// (TX, TB, NCH, MASK, PAD, VEC, BX) and arguments (x, pitch, fstride, W, base, out, g, coef, status, scal).  HO / ho: the hand-over
// instance and its HandOver; SIGNS / sg: the signed instance and a pointer to its SignTable (else null).
// A macro where k_detect and k_detect_redo share a __forceinline__ function (detect_body): a function is optimised on its own before
// it is inlined, and with the body as a function 64 of k_embed's 104 instances compiled to other code than with these lines in the
// kernel (scalar selects became branches, the pass-through copy of the u8 planar-RGB generic instance grew by 166 instructions).
// Expanded in place, every k_embed instance compiles to what it compiled to when the lines stood in the kernel.
#define WM_EMBED_BODY(HO, SIGNS, ho, sg)                                                                                                   \
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];                                                          \
    __shared__ __attribute__((aligned(16))) float s_out[VEC ? 1 : WPB][VEC ? 4 : STRIP]; /* generic path: store re-layout rows */         \
    const WaveJob j = make_job(g);                                                                                                       \
    const int frame = j.frame;                                                                                                           \
    if (!j.valid) return;                                                                                                                \
    const TB* bptr = static_cast<const TB*>(base.p) + (long long)frame * base.fstride;                                                    \
    TB* optr = static_cast<TB*>(const_cast<void*>(out.p)) + (long long)frame * out.fstride;                                               \
    const int st = MASK == 0 ? status[frame] : 0;                                                                                        \
    if (!HO && st != 0) {                                                                                                                \
        /* unsolvable: out = base bit-exact (Watermark.cpp:164-165) */                                                                   \
        if (bptr != optr) {                                                                                                              \
            const int c0 = j.c0s + 4 * j.lane;                                                                                           \
            for (int ch = 0; ch < NCH; ++ch)                                                                                             \
                for (int r = j.rs; r < j.re; ++r) {                                                                                      \
                    const TB* rb = bptr + (long long)ch * base.cstride + (long long)r * base.pitch;                                       \
                    TB* ro = optr + (long long)ch * out.cstride + (long long)r * out.pitch;                                               \
                    for (int k = 0; k < 4; ++k)                                                                                          \
                        if (c0 + k < g.cols) ro[c0 + k] = rb[c0 + k];                                                                    \
                }                                                                                                                        \
        }                                                                                                                                \
        return;                                                                                                                          \
    }                                                                                                                                    \
    float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                                                                               \
    if (MASK == 0) {                                                                                                                     \
        _Pragma("unroll") for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];                                                        \
    }                                                                                                                                    \
    const float a = applied_strength(scal[frame].a);                                                                                     \
    const float maxe = scal[frame].maxe;                                                                                                 \
    const TX* xf = x + (long long)frame * fstride;                                                                                       \
    /* hand-over: an unsolvable frame runs the march too (y = base, selected per row) -- its lag sums are the detector's */              \
    const bool pass = HO && st != 0;                                                                                                     \
    double* horec = HO ? (ho).rec + ((long long)frame * (ho).stride + j.rec) * 13 : nullptr;                                              \
    float* hoseam = HO ? (ho).seam : nullptr;                                                                                            \
    unsigned long long* hodig = HO ? (ho).dig + (long long)frame * (ho).stride + j.rec : nullptr;                                         \
    /* NVF windows (PAD > 1) keep the single instance: their halo fix-up is a small share of the step */                                 \
    if (MASK != 0 || strip_on_edge<VEC>(g, j))                                                                                           \
        embed_march<TX, TB, NCH, MASK, PAD, VEC, BX, true, HO, SIGNS>(xf, pitch, W, bptr, optr, base, out, g, j, s_row[j.wave],           \
                                                                      s_out[VEC ? 0 : j.wave], c, a, maxe, pass, horec, hoseam, hodig, sg); \
    else                                                                                                                                 \
        embed_march<TX, TB, NCH, MASK, PAD, VEC, BX, (MASK != 0), HO, SIGNS>(xf, pitch, W, bptr, optr, base, out, g, j, s_row[j.wave],    \
                                                                             s_out[VEC ? 0 : j.wave], c, a, maxe, pass, horec, hoseam, hodig, sg)

// =================================================================================================
// embed_group_march: the multi-copy embed (k_embed_keys, k_embed_signs_multi) -- embed_march's plain instance (no hand-over) on ONE
// channel of the base, with the copy-dependent tail of the row step repeated for a compile-time group of G copies.  The image side --
// the mask m and the base row b -- is formed once per row.  The copy side is one of two:
//   SIGNS false (k_embed_keys):        a W stream with PW rows in flight and a strength per copy (W, a: arrays of G):
//                                      y_q = clamp(fmaf(m W_q, a_q, b), 0, 255)
//   SIGNS true  (k_embed_signs_multi): one W stream and one strength (W, a: scalars) and a sign table per copy (SignWalkGroup:
//                                      `table` of the group's first copy, toff[q] from there to copy q's, st for the tile geometry):
//                                      u = m W once, y_q = clamp(fmaf(u s_q, a, b), 0, 255) -- u s exact, as embed_march's SIGNS
// G, PW and SIGNS are template parameters, not constants of the function: a generic lambda discards an `if constexpr` branch on the
// former when the march is instantiated, on the latter only when the lambda is called -- by then it has captured what the branch
// names, and 31 of the 40 k_embed_keys instances compiled to other code.  The W take and the sign advance stand in front of the mask
// for SIGNS, u = m W inside the mask loop: the order k_embed_signs_multi was written in, and the one its instances compile the same with.
// =================================================================================================
template <typename V, int N>
__device__ __forceinline__ V copy_of(const V (&v)[N], int q) { return v[q]; }  // copy q's W plane / strength: one per copy ...
template <typename V>
__device__ __forceinline__ V copy_of(const V& v, int) { return v; }            // ... or one for all

template <typename T, int MASK, int PAD, bool VEC, bool BX, bool EDGE, int G, int PW, bool SIGNS, typename WT, typename AT>
__device__ __forceinline__ void embed_group_march(const T* __restrict__ xf, long long pitch, const WT& W, const T* __restrict__ bptr,
                                                  T* const (&optr)[G], int nk, const PlaneDesc& base, const PlaneDesc& out,
                                                  const Geom& g, const WaveJob& j, float* lds, float* obuf, const float (&c)[8],
                                                  const AT& a, float maxe, const signed char* table, const int* toff,
                                                  const SignTable* st)
{
    constexpr int NR = MASK == 0 ? 3 : 2 * PAD + 1;
    constexpr int HR = MASK == 0 ? 1 : PAD;  // halo rows above/below = halo columns left/right
    constexpr int RG = VEC && NR == 3 ? WM_RING3 : UNROLL;
    constexpr int NW = SIGNS ? 1 : G;        // W streams
    static_assert(UNROLL % PW == 0 && RG % PW == 0, "the W prefetch ring must divide the march group");
    XMarch<T, 1, HR, NR, VEC, PFX, EDGE, false, RG> xm;
    PMarch<float, VEC, PW> wm_[NW];
    PMarch<T, VEC, PFW> bm;               // (BX: the base is the grey input, read from the stencil window)
    const float inv_maxe = 1.0f / maxe;   // (k_embed's m = |e| / max|e|: one reciprocal per wave, then div_by per pixel)
    const int nout = j.re - j.rs, n = nout + 2 * HR;
    const int c0 = j.c0s + 4 * j.lane;
    const bool own = !EDGE || 4 * j.lane >= j.dup;  // duplicate lanes of a shifted last strip: the previous strip stores these pixels
    xm.start(xf, pitch, g, j, lds, j.rs - HR, n);
#pragma unroll
    for (int q = 0; q < NW; ++q) wm_[q].start(copy_of(W, q), g.cols, g.cols, j, j.rs, nout);
    if (!BX) bm.start(bptr, base.pitch, g.cols, j, j.rs, nout);
    SignWalkGroup<G> sw;
    if constexpr (SIGNS) sw.start(table, toff, st->th, st->tw, st->ny, st->nx, c0, j.rs);
    march_n<2 * HR, RG>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            const int o = i - 2 * HR;
            constexpr int SB = (Q + 4 * UNROLL - 2 * HR) % PFW;
            constexpr int SW = (Q + 4 * UNROLL - 2 * HR) % PW;
            // ---- the image side, once per row: the mask of the lane's 4 pixels and the base row
            float4 w;
            float m[4], u[4];
            if constexpr (SIGNS) {
                w = wm_[0].template take<SW>();
                sw.advance(j.rs + o);
            }
            float pr[4] = {0.f, 0.f, 0.f, 0.f};
            if (MASK == 0) predict4<4>(xm.template row<Q>(0), xm.template row<Q>(1), xm.template row<Q>(2), c, pr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (MASK == 0) {
                    const float* mid = xm.template row<Q>(1);
                    m[k] = div_by(fabsf(mid[4 + k] - pr[k]), maxe, inv_maxe);
                } else {
                    m[k] = nvf_value<PAD, 4, Q>(xm, k);
                }
                if constexpr (SIGNS) u[k] = m[k] * f4get(w, k);  // Watermark.cpp:169
            }
            float4 b;
            if (BX) {
                const float* ctr = xm.template row<Q>(HR);  // the output row itself
                b = make_float4(ctr[4], ctr[5], ctr[6], ctr[7]);
            } else {
                b = bm.template take<SB>();
            }
            // ---- the copy side: k_embed's u and y for every copy of the group
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if constexpr (!SIGNS) {
                    w = wm_[q].template take<SW>();
#pragma unroll
                    for (int k = 0; k < 4; ++k) u[k] = m[k] * f4get(w, k);  // Watermark.cpp:169
                }
                if (q < nk) {  // (wave-uniform: copies beyond the last store nothing)
                    const float aq = copy_of(a, q);
                    float us[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        us[k] = u[k];
                        if constexpr (SIGNS) us[k] *= sw.cur[q];  // times the tile's sign (exact)
                    }
                    float4 y;
                    y.x = fminf(fmaxf(fmaf(us[0], aq, b.x), 0.0f), 255.0f);
                    y.y = fminf(fmaxf(fmaf(us[1], aq, b.y), 0.0f), 255.0f);
                    y.z = fminf(fmaxf(fmaf(us[2], aq, b.z), 0.0f), 255.0f);
                    y.w = fminf(fmaxf(fmaf(us[3], aq, b.w), 0.0f), 255.0f);
                    if constexpr (VEC) {
                        if (own) store4<T, true>(optr[q], out.pitch, j.rs + o, c0, g.cols, y);
                    } else {
                        store_row_generic<T>(optr[q], out.pitch, j.rs + o, j.c0s, j.lane, g.cols, y, obuf);
                    }
                }
                if constexpr (!SIGNS) wm_[q].template refill<SW>(o);
            }
            if (!BX) bm.template refill<SB>(o);
            if constexpr (SIGNS) wm_[0].template refill<SW>(o);
        }
    });
}

// WM_EMBED_GROUP_BODY: the body of k_embed_keys and k_embed_signs_multi in front of the march -- WM_EMBED_BODY's lines for a group of G
// copies: the wave's job and copy group (keys_job), the base and the group's out planes, the unsolvable pass-through of every copy, the
// coefficients.  It expands inside a kernel with the template parameters T, MASK, PAD, VEC, BX and the arguments x, pitch, fstride, base,
// out (one channel: PlaneDesc::p at that channel, cstride unused), g, coef, status, and leaves j, frame, k0 (the group's first copy), nk
// (its copies), kq[] (the copy index of slot q), bptr, optr[] and c behind.  Copy (frame, k) is frame index frame * ncopies + k of `out`;
// slots beyond the last copy (a short last group) repeat it and store nothing.  A macro for WM_EMBED_BODY's reason.
#define WM_EMBED_GROUP_BODY(G, ngroups, ncopies)                                                                                          \
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];                                                          \
    __shared__ __attribute__((aligned(16))) float s_out[VEC ? 1 : WPB][VEC ? 4 : STRIP]; /* generic path: store re-layout rows */         \
    int grp;                                                                                                                             \
    const WaveJob j = keys_job(g, ngroups, grp);                                                                                         \
    if (!j.valid) return;                                                                                                                \
    const int frame = j.frame;                                                                                                           \
    const int k0 = grp * (G);                                                                                                            \
    const int nk = min((G), (ncopies) - k0);                                                                                             \
    const T* bptr = static_cast<const T*>(base.p) + (long long)frame * base.fstride;                                                     \
    T* optr[G];                                                                                                                          \
    int kq[G];                                                                                                                           \
    _Pragma("unroll") for (int q = 0; q < (G); ++q) {                                                                                    \
        kq[q] = min(k0 + q, (ncopies) - 1);                                                                                              \
        optr[q] = static_cast<T*>(const_cast<void*>(out.p)) + ((long long)frame * (ncopies) + kq[q]) * out.fstride;                      \
    }                                                                                                                                    \
    if (MASK == 0 && status[frame] != 0) {                                                                                               \
        /* unsolvable: every copy = base bit-exact (Watermark.cpp:164-165) */                                                            \
        const int c0 = j.c0s + 4 * j.lane;                                                                                               \
        _Pragma("unroll") for (int q = 0; q < (G); ++q) {                                                                                \
            if (q >= nk) break;                                                                                                          \
            for (int r = j.rs; r < j.re; ++r) {                                                                                          \
                const T* rb = bptr + (long long)r * base.pitch;                                                                          \
                T* ro = optr[q] + (long long)r * out.pitch;                                                                              \
                for (int k = 0; k < 4; ++k)                                                                                              \
                    if (c0 + k < g.cols) ro[c0 + k] = rb[c0 + k];                                                                        \
            }                                                                                                                            \
        }                                                                                                                                \
        return;                                                                                                                          \
    }                                                                                                                                    \
    float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                                                                               \
    if (MASK == 0) {                                                                                                                     \
        _Pragma("unroll") for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];                                                        \
    }                                                                                                                                    \
    (void)0
// ... and behind the kernel's own lines (W, a, maxe, xf; table, toff, st as embed_group_march takes them: the sign tables of SIGNS,
// null without): the choice between the edge and the no-edge instance
#define WM_EMBED_GROUP_MARCH(G, PW, SIGNS, W, a, maxe, table, toff, st)                                                                      \
    if (MASK != 0 || strip_on_edge<VEC>(g, j))                                                                                           \
        embed_group_march<T, MASK, PAD, VEC, BX, true, G, PW, SIGNS>(xf, pitch, W, bptr, optr, nk, base, out, g, j, s_row[j.wave],       \
                                                                     s_out[VEC ? 0 : j.wave], c, a, maxe, table, toff, st);              \
    else                                                                                                                                 \
        embed_group_march<T, MASK, PAD, VEC, BX, (MASK != 0), G, PW, SIGNS>(xf, pitch, W, bptr, optr, nk, base, out, g, j, s_row[j.wave], \
                                                                            s_out[VEC ? 0 : j.wave], c, a, maxe, table, toff, st)

// ---- launch: what launch_embed (without hand-over) and launch_embed_signs share ----------------------------------------------------
// the planes of an embed sweep: f(T{}, IC<channels of the base>{}) with T = float or uint8_t, the element type of x, base and out.
// Mixed f32/u8 planes are rejected by the API layer (the reference converts whole frames, main.cpp:355-357): f is not called
template <typename F>
static inline void for_embed_planes(const PlaneDesc& x, const PlaneDesc& base, F&& f)
{
    if (x.dtype != base.dtype || (x.dtype != 0 && x.dtype != 1)) return;
    WM_DISPATCH_T(x.dtype, if (base.channels == 3) f(T{}, IC<3>{}); else f(T{}, IC<1>{}));
}
// the launches of one embed sweep over planes of NCH channels: go(IC<MASK>, IC<PAD>, vec, IC<channels of the instance>, base_is_x, part)
// for the aligned and the generic part.  al: align_mode of all four planes; bx: the base is the grey input plane (same_plane)
template <int NCH, typename F>
static inline void for_each_embed_launch(const Sweep& sw, int al, bool bx, F&& go)
{
    for_mask_pad(sw.mask, sw.pad, [&](auto m, auto p) {
        auto sweep = [&](auto base_is_x) {
            for_each_sweep_part(sw, al, 1, [&](auto vec, const SweepPart& sp) {
                go(m, p, vec, IC<(decltype(base_is_x)::value ? 1 : NCH)>{}, base_is_x, sp);
            });
        };
        if (bx) sweep(std::true_type{}); else sweep(std::false_type{});
    });
}
// the launches of a multi-copy embed sweep (k_embed_keys, k_embed_signs_multi): the plan above once per channel of the base, on
// one-channel views of base and out, every grid times the copy groups: go(IC<MASK>, IC<PAD>, vec, base_is_x, grid, Geom, base view, out view).
// T: the planes' element type (the API layer admits same-dtype planes only, as for wm_embed)
template <typename T, typename F>
static inline void for_each_embed_group_launch(const Sweep& sw, int aligned_w, const EmbedPlanes& ep, int ngroups, F&& go)
{
    const PlaneDesc &base = ep.base, &out = ep.out;
    const int al = align_mode(sw.lg, sw.x.aligned && aligned_w && base.aligned && out.aligned);
    const bool bx = base.channels == 1 && same_plane(sw.x, base);
    for (int ch = 0; ch < base.channels; ++ch) {
        PlaneDesc bc = base, oc = out;
        bc.p = static_cast<const T*>(base.p) + (long long)ch * base.cstride;
        oc.p = static_cast<const T*>(out.p) + (long long)ch * out.cstride;
        bc.channels = oc.channels = 1;
        for_each_embed_launch<1>(sw, al, bx, [&](auto m, auto p, auto vec, auto, auto base_is_x, const SweepPart& sp) {
            go(m, p, vec, base_is_x, dim3(sp.grid.x * (unsigned)ngroups), sp.g, bc, oc);
        });
    }
}

}  // namespace wmk
