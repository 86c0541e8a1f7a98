// wm_k_bits.hip -- a payload in the mark (wm_embed_signs / wm_embed_bits, wm_detect_bits): k_embed_signs + k_bits_fold
//
// The detector's score is signed and local (wm_k_detect_tiles.hip), and the strength a = sF / (||m W|| / sqrt(N)) does not see
// the sign of W.  A frame whose tile (ty, tx) is marked with s W, s = +-1, therefore carries one bit per tile.
//   k_embed_signs  y = clamp(base + a s(ty, tx) m W, 0, 255): k_embed's last sweep (wm_k_embed.hip embed_march without the Gram
//                  hand-over) with u = m W multiplied by the sign of the pixel's tile.  The product with +-1 or 0 is exact, so
//                  fmaf(u, a, b) gives wm_embed's bits with W (+1), with -W (-1) and with a zero W (0).  The march is this file's
//                  own: wm_k_embed.hip is not touched and k_embed's instances compile to what they compiled to before.
//   k_bits_fold    one wave per (frame, bit) adds the three f64 sums of the bit's tiles (k_tiles_fold's output) in ascending tile
//                  index, one add after the other, and writes the bit's soft value as a result record.
#include "wm_march.hpp"

namespace wmk {

// Tile geometry is wm_tiles_shape's: pixel (r, c) belongs to tile (min(r / th, ny - 1), min(c / tw, nx - 1)).
//  * column: a lane's four columns start at c0 = c0s + 4 lane, and c0s is a multiple of 4 in every strip this sweep launches (full
//    strips at multiples of 256; the shifted last strip at cols - 256 with cols a multiple of 4, align_mode; the generic strips at
//    multiples of 256 as well).  tw is a multiple of 4, so the four columns lie in ONE tile column, fixed over the march.
//  * row: wave-uniform, changes every th rows; segments need not line up with tiles.  A lane holds the sign of the current tile
//    row and, already loaded, that of the next one: the load for tile row ty + 2 is issued when the march enters ty + 1, at least
//    th >= 32 rows ahead of its use.
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

struct SignTable {
    const signed char* signs;  // [frames][ny][nx], -1 | 0 | +1
    int th, tw, ny, nx;
};

template <typename TX, typename TB, int NCH, int MASK, int PAD, bool VEC, bool BX, bool EDGE>
__device__ __forceinline__ void embed_signs_march(const TX* __restrict__ xf, long long pitch, const float* __restrict__ W,
                                                  const TB* __restrict__ bptr, TB* __restrict__ optr, const PlaneDesc& base,
                                                  const PlaneDesc& out, const Geom& g, const WaveJob& j, float* lds, float* obuf,
                                                  const float (&c)[8], float a, float maxe, const SignTable& sg)
{
    constexpr int NR = MASK == 0 ? 3 : 2 * PAD + 1;
    constexpr int HR = MASK == 0 ? 1 : PAD;  // halo rows above/below = halo columns left/right
    constexpr int RG = UNROLL;
    XMarch<TX, 1, HR, NR, VEC, PFX, EDGE, false, RG> xm;
    PMarch<float, VEC, PFW> wm_;
    const float inv_maxe = 1.0f / maxe;
    PMarch<TB, VEC, PFW> bm[BX ? 1 : NCH];  // BX: the base IS the grey input plane, taken from the stencil window
    const int nout = j.re - j.rs, n = nout + 2 * HR;
    const int c0 = j.c0s + 4 * j.lane;
    xm.start(xf, pitch, g, j, lds, j.rs - HR, n);
    wm_.start(W, g.cols, g.cols, j, j.rs, nout);
    if (!BX) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) bm[ch].start(bptr + (long long)ch * base.cstride, base.pitch, g.cols, j, j.rs, nout);
    }
    SignWalk sw;
    sw.start(sg.signs + (long long)j.frame * sg.ny * sg.nx, sg.th, sg.tw, sg.ny, sg.nx, c0, j.rs);
    march_n<2 * HR, RG>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            const int o = i - 2 * HR;
            constexpr int SLOT = (Q + 4 * UNROLL - 2 * HR) % PFW;
            const float4 w = wm_.template take<SLOT>();
            const float sgn = sw.at(j.rs + o);
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
                u[k] = (m * f4get(w, k)) * sgn;  // Watermark.cpp:169, times the tile's sign (exact)
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
                if constexpr (VEC) {
                    if (!EDGE || 4 * j.lane >= j.dup)  // duplicate lanes of a shifted last strip: the previous strip stores these pixels
                        store4<TB, true>(optr + (long long)ch * out.cstride, out.pitch, j.rs + o, c0, g.cols, y);
                } else {
                    store_row_generic<TB>(optr + (long long)ch * out.cstride, out.pitch, j.rs + o, j.c0s, j.lane, g.cols, y, obuf);
                }
                if (!BX) bm[ch].template refill<SLOT>(o);
            }
            wm_.template refill<SLOT>(o);
        }
    });
}

template <typename TX, typename TB, int NCH, int MASK, int PAD, bool VEC, bool BX>
__global__ __launch_bounds__(BLOCK) void k_embed_signs(const TX* __restrict__ x, long long pitch, long long fstride,
                                                       const float* __restrict__ W, PlaneDesc base, PlaneDesc out, Geom g,
                                                       const float* __restrict__ coef, const int* __restrict__ status,
                                                       const EmbedScalars* __restrict__ scal, SignTable sg)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];
    __shared__ __attribute__((aligned(16))) float s_out[VEC ? 1 : WPB][VEC ? 4 : STRIP];  // generic path: store re-layout rows
    const WaveJob j = make_job(g);
    const int frame = j.frame;
    if (!j.valid) return;
    const TB* bptr = static_cast<const TB*>(base.p) + (long long)frame * base.fstride;
    TB* optr = static_cast<TB*>(const_cast<void*>(out.p)) + (long long)frame * out.fstride;
    const int st = MASK == 0 ? status[frame] : 0;
    if (st != 0) {
        // unsolvable: out = base bit-exact (Watermark.cpp:164-165)
        if (bptr != optr) {
            const int c0 = j.c0s + 4 * j.lane;
            for (int ch = 0; ch < NCH; ++ch)
                for (int r = j.rs; r < j.re; ++r) {
                    const TB* rb = bptr + (long long)ch * base.cstride + (long long)r * base.pitch;
                    TB* ro = optr + (long long)ch * out.cstride + (long long)r * out.pitch;
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
    const float a = applied_strength(scal[frame].a);
    const float maxe = scal[frame].maxe;
    const TX* xf = x + (long long)frame * fstride;
    // k_embed's choice of instances: NVF windows keep the single (edge) instance
    if (MASK != 0 || strip_on_edge<VEC>(g, j))
        embed_signs_march<TX, TB, NCH, MASK, PAD, VEC, BX, true>(xf, pitch, W, bptr, optr, base, out, g, j, s_row[j.wave], s_out[VEC ? 0 : j.wave], c, a, maxe, sg);
    else
        embed_signs_march<TX, TB, NCH, MASK, PAD, VEC, BX, (MASK != 0)>(xf, pitch, W, bptr, optr, base, out, g, j, s_row[j.wave], s_out[VEC ? 0 : j.wave], c, a, maxe, sg);
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
template <typename TX, typename TB, int NCH>
static void launch_embed_signs_tt(hipStream_t s, const LaunchGeom& lg, int frames, int mask, int pad, const PlaneDesc& x,
                                  const float* W, int aligned_w, const PlaneDesc& base, const PlaneDesc& out, const float* coef,
                                  const int* status, const EmbedScalars* scal, const SignTable& sg)
{
    const int al = align_mode(lg, x.aligned && aligned_w && base.aligned && out.aligned);
    const bool bx = NCH == 1 && std::is_same<TX, TB>::value && same_plane(x, base);
    for_mask_pad(mask, pad, [&](auto m, auto p) {
        auto sweep = [&](auto base_is_x) {
            for_each_sweep_part(lg, frames, al, 1, [&](auto vec, const SweepPart& sp) {
                constexpr bool BX = decltype(base_is_x)::value;
                WM_KLAUNCH((k_embed_signs<TX, TB, (BX ? 1 : NCH), decltype(m)::value, decltype(p)::value, decltype(vec)::value, BX>), sp.grid,
                           dim3(BLOCK), 0, s, (const TX*)x.p, x.pitch, x.fstride, W, base, out, sp.g, coef, status, scal, sg);
            });
        };
        if (bx) sweep(std::true_type{}); else sweep(std::false_type{});
    });
}

void launch_embed_signs(hipStream_t s, const LaunchGeom& lg, int frames, int mask, int pad, const PlaneDesc& x, const float* W,
                        int aligned_w, const PlaneDesc& base, const PlaneDesc& out, const float* coef, const int* status,
                        const EmbedScalars* scal, const signed char* signs, int tile_rows, int tile_cols, int ny, int nx)
{
    const SignTable sg{signs, tile_rows, tile_cols, ny, nx};
    // mixed f32/u8 planes are rejected by the API layer
    if (x.dtype == 0 && base.dtype == 0) {
        if (base.channels == 3) launch_embed_signs_tt<float, float, 3>(s, lg, frames, mask, pad, x, W, aligned_w, base, out, coef, status, scal, sg);
        else launch_embed_signs_tt<float, float, 1>(s, lg, frames, mask, pad, x, W, aligned_w, base, out, coef, status, scal, sg);
    } else if (x.dtype == 1 && base.dtype == 1) {
        if (base.channels == 3) launch_embed_signs_tt<uint8_t, uint8_t, 3>(s, lg, frames, mask, pad, x, W, aligned_w, base, out, coef, status, scal, sg);
        else launch_embed_signs_tt<uint8_t, uint8_t, 1>(s, lg, frames, mask, pad, x, W, aligned_w, base, out, coef, status, scal, sg);
    }
}

void launch_bits_fold(hipStream_t s, int frames, int nbits, int ntiles, const double* sums, const int* start, const int* idx,
                      const int* status, OpResult* res)
{
    const long long n = (long long)frames * nbits;
    WM_KLAUNCH(k_bits_fold, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(BLOCK), 0, s, sums, ntiles, frames, nbits, start, idx, status, res);
}

}  // namespace wmk
