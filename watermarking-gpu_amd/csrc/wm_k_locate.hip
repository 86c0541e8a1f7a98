// wm_k_locate.hip -- the image and key side of the locate family around the transform of wm_k_fft.hip.  Image side: k_locate_e (the
// frame's prediction error and NVF mask), k_locate_h (h = m * F^T e_w, the exact adjoint of the replicate-border stencil, laid into
// a zeroed complex plane) and, for wm_clip_pool, k_clip_pool (the frames of a clip pooled into one image-side plane, h formed by
// k_locate_e's and k_locate_h's helpers).  Key side: k_locate_lay, one kernel body over three sources -- a dense real plane (a key of
// wm_locate, or a pool), a key masked to the tiles of two payload bits (wm_locate_bits), two keys of a bank with a flag per key that
// is not all zero (wm_locate_keys) --, one source per half of a complex plane.  Behind the inverse transform: k_locate_map (one map,
// or the two of a pair, and their block folds) and k_locate_records (a map's four numbers) for wm_locate and wm_locate_keys;
// k_locate_bits_acc (the two maps, the energy map and their block folds) and k_locate_bits_fold (the records) for wm_locate_bits.
// All of them fold through the same pieces: peak_take, peak_tree, peak_fold, peak_z_around, peak_records.
//
// With c solved, the detector's numerator is linear in W: <e_u, e_w>(oy, ox) = sum_q h(q) W(q + (oy, ox)), one 2-D cross-correlation
// of h with the key plane.  Every workgroup works on its own pixels or its own chunk of the map; the fold
// runs in a fixed order in f64, without atomics: a frame's map and numbers do not depend on the batch or on repetition.
#include "wm_march.hpp"

namespace wmk {

namespace {

constexpr int LB = 256;          // threads per workgroup
constexpr int LTX = 64, LTY = 4; // ... as 64 columns x 4 rows of pixels
constexpr int PEAK_PER = 16;     // map values per thread of k_locate_map: a workgroup folds 4096 consecutive values

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- the arithmetic of one pixel of the image side, shared by k_locate_e / k_locate_h and k_clip_pool: the kernels differ in where
// the taps come from (global memory or an LDS tile), never in the sequence of operations, so their e, m and h agree bit for bit

// the NVF value of the window 2 PAD + 1 around a pixel: nvf_from_sums over row-major taps, as nvf_value forms it (the first tap
// starts both chains).  at(a, b): the pixel value at row offset a, column offset b
template <int PAD, typename At>
__device__ __forceinline__ float locate_nvf(At&& at)
{
    float sum = 0.0f, sumsq = 0.0f;
#pragma unroll
    for (int a = -PAD; a <= PAD; ++a)
#pragma unroll
        for (int b = -PAD; b <= PAD; ++b) {
            const float v = at(a, b);
            if (a == -PAD && b == -PAD) { sum = v; sumsq = v * v; }
            else { sum += v; sumsq = fmaf(v, v, sumsq); }
        }
    return nvf_from_sums<PAD>(sum, sumsq);
}

// the pixels p of one axis with clamp(p + d) == q: q - d when it is in range, and the border pixel once more when q is that
// border and d points outwards.  Returns their count (0 .. 2)
__device__ __forceinline__ int adjoint_set(int q, int d, int n, int (&out)[2])
{
    int cnt = 0;
    const int p = q - d;
    if (p >= 0 && p < n) out[cnt++] = p;
    if (d == -1 && q == 0) out[cnt++] = 0;
    if (d == 1 && q == n - 1) out[cnt++] = n - 1;
    return cnt;
}

// g(q) = e(q) - sum_k c_k sum_{p : clamp(p + d_k) = q} e(p) at q = (r, c): the exact adjoint of the replicate-border stencil.
// ec = e(q); e_at(pr, pc): e at image coordinates
template <typename EAt>
__device__ __forceinline__ float locate_g(float ec, int r, int c, int rows, int cols, const float* __restrict__ coef, EAt&& e_at)
{
    float g = ec;
    if (r >= 1 && r < rows - 1 && c >= 1 && c < cols - 1) {
        // off the border every set is the one pixel q - d_k: the same operations as below (0.0f + e included), without the sets
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = k < 4 ? k : k + 1;
            const float s = 0.0f + e_at(r - (t / 3 - 1), c - (t % 3 - 1));
            g = fmaf(-coef[k], s, g);
        }
        return g;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int t = k < 4 ? k : k + 1;  // the 3x3 taps in row-major order without the centre
        const int dr = t / 3 - 1, dc = t % 3 - 1;
        int pr_[2], pc_[2];
        const int nr = adjoint_set(r, dr, rows, pr_), ncn = adjoint_set(c, dc, cols, pc_);
        float s = 0.0f;
        for (int a = 0; a < nr; ++a)
            for (int b = 0; b < ncn; ++b) s += e_at(pr_[a], pc_[b]);
        g = fmaf(-coef[k], s, g);
    }
    return g;
}

// h = m g with m = |e| (ME) or the NVF value
template <int MASK>
__device__ __forceinline__ float locate_h_value(float ec, float m, float g) { return (MASK == 0 ? fabsf(ec) : m) * g; }

// k_locate_e: e = x - sum_k c_k x(clamp(p + d_k)) with the detector's rounding sequence (residual1: the chain starts at the centre
// and runs over the negated coefficients), and under NVF the mask of the window 2 PAD + 1 (locate_nvf).  One pixel per lane,
// replicate borders by clamped indices; x of any type, pitch and frame stride.
// e, m: dense [rows][cols] f32 planes of ONE frame (m unused under ME).  An unsolvable frame is skipped: k_locate_h writes zeros
template <typename T, int MASK, int PAD>
__global__ __launch_bounds__(LB) void k_locate_e(const T* __restrict__ x, long long pitch, int rows, int cols, const float* __restrict__ coef,
                                                 const int* __restrict__ status, float* __restrict__ e, float* __restrict__ m)
{
    if (status[0] != 0) return;
    const int c = blockIdx.x * LTX + threadIdx.x % LTX, r = blockIdx.y * LTY + threadIdx.x / LTX;
    if (r >= rows || c >= cols) return;
    float nc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) nc[k] = -coef[k];
    float win[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            win[a][b] = Elem<T>::cvt1(x[(long long)clampi(r + a - 1, rows) * pitch + clampi(c + b - 1, cols)]);
    e[(size_t)r * cols + c] = residual1<1>(win[0], win[1], win[2], 0, nc);
    if (MASK == 1)
        m[(size_t)r * cols + c] = locate_nvf<PAD>([&](int a, int b) {
            return PAD == 1 ? win[a + 1][b + 1] : Elem<T>::cvt1(x[(long long)clampi(r + a, rows) * pitch + clampi(c + b, cols)]);
        });
}

// k_locate_h: g(q) = e(q) - sum_k c_k sum_{p : clamp(p + d_k) = q} e(p), h = m g with m = |e| (ME) or the NVF plane, written as
// (h, 0) into the [pr][pc] complex plane; every element outside the image, and the whole plane of an unsolvable frame, is (0, 0)
template <int MASK>
__global__ __launch_bounds__(LB) void k_locate_h(const float* __restrict__ e, const float* __restrict__ m, int rows, int cols,
                                                 const float* __restrict__ coef, const int* __restrict__ status, float2* __restrict__ plane, int pc)
{
    const int c = blockIdx.x * LTX + threadIdx.x % LTX, r = blockIdx.y * LTY + threadIdx.x / LTX;  // (the grid covers pr x pc exactly)
    float h = 0.0f;
    if (r < rows && c < cols && status[0] == 0) {
        const float ec = e[(size_t)r * cols + c];
        const float g = locate_g(ec, r, c, rows, cols, coef, [&](int pr_, int pc_) { return e[(size_t)pr_ * cols + pc_]; });
        h = locate_h_value<MASK>(ec, MASK == 0 ? 0.0f : m[(size_t)r * cols + c], g);
    }
    plane[(size_t)r * pc + c] = make_float2(h, 0.0f);
}

// ---- wm_clip_pool: the frames of a clip pooled on the image side ----------------------------------------

constexpr int CTX = 64, CTY = 16;        // k_clip_pool: a workgroup's tile of output pixels, 64 columns x 16 rows
constexpr int CPER = CTY / (LB / CTX);   // ... 4 pixels per lane: column t % 64, rows t / 64 + 4 k

// k_clip_pool: pool(q) = fmaf(w_f, h_f(q), pool(q)) over the solvable frames f ascending, from 0.0f (accumulate == 0) or from the
// plane's content; h_f is k_locate_e's and k_locate_h's, through the same helpers.  A workgroup owns a CTX x CTY tile and loops
// over the frames: x with a halo of H = max(2, PAD) (indices clamped to the image) into LDS, e on the tile plus one pixel of halo
// once per pixel into LDS, then per output pixel g, m, h and one fmaf into a register.  The pool is read and written once per
// call.  Workgroup (0, 0) also writes the frames' status records.  x of any type, pitch and frame stride
template <typename T, int MASK, int PAD>
__global__ __launch_bounds__(LB) void k_clip_pool(const T* __restrict__ x, long long pitch, long long fstride, int frames, int rows, int cols,
                                                  const float* __restrict__ coef, const int* __restrict__ status, const float* __restrict__ weights,
                                                  float* __restrict__ pool, int accumulate, OpResult* __restrict__ res)
{
    constexpr int H = PAD > 2 ? PAD : 2;
    constexpr int XW = CTX + 2 * H, XH = CTY + 2 * H, EW = CTX + 2, EH = CTY + 2;
    __shared__ float s_x[XH * XW];
    __shared__ float s_e[EH * EW];
    const int t = threadIdx.x, tx = t % CTX, ty = t / CTX;
    const int c0 = blockIdx.x * CTX, r0 = blockIdx.y * CTY;
    const int c = c0 + tx;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int f = t; f < frames; f += LB) res[f] = OpResult{status[f], 0.0f};
    float acc[CPER];
#pragma unroll
    for (int k = 0; k < CPER; ++k) {
        const int r = r0 + ty + k * (LB / CTX);
        acc[k] = accumulate && r < rows && c < cols ? pool[(size_t)r * cols + c] : 0.0f;
    }
    for (int f = 0; f < frames; ++f) {
        if (status[f] != 0) continue;  // (the same in every lane)
        const T* __restrict__ xf = x + (long long)f * fstride;
        const float* __restrict__ cf = coef + 8 * f;
        const float w = weights[f];
        for (int i = t; i < XH * XW; i += LB) {
            const int lr = i / XW, lc = i % XW;
            s_x[i] = Elem<T>::cvt1(xf[(long long)clampi(r0 - H + lr, rows) * pitch + clampi(c0 - H + lc, cols)]);
        }
        __syncthreads();
        float nc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) nc[k] = -cf[k];
        for (int i = t; i < EH * EW; i += LB) {
            const int lr = i / EW, lc = i % EW;
            const int r = r0 - 1 + lr, cc = c0 - 1 + lc;
            float e = 0.0f;  // (a halo pixel outside the image: no adjoint set names it)
            if (r >= 0 && r < rows && cc >= 0 && cc < cols) {
                const float* up = s_x + (lr + H - 2) * XW + (lc + H - 2);  // the window's top left tap: x at (r - 1, cc - 1)
                e = residual1<1>(up, up + XW, up + 2 * XW, 0, nc);
            }
            s_e[i] = e;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CPER; ++k) {
            // (the row is the same in every lane of a wave; pinned to a vector register, or the row conditions of the four pixels
            // overfill the scalar registers)
            const int lr = (int)pinned((uint32_t)(ty + k * (LB / CTX))), r = r0 + lr;
            if (r < rows && c < cols) {
                const float ec = s_e[(lr + 1) * EW + tx + 1];
                const float g = locate_g(ec, r, c, rows, cols, cf, [&](int pr_, int pc_) { return s_e[(pr_ - r0 + 1) * EW + (pc_ - c0 + 1)]; });
                float m = 0.0f;
                if (MASK == 1) m = locate_nvf<PAD>([&](int a, int b) { return s_x[(lr + H + a) * XW + tx + H + b]; });
                acc[k] = fmaf(w, locate_h_value<MASK>(ec, m, g), acc[k]);
            }
        }
        if (MASK == 1) __syncthreads();  // (the next frame's x replaces the windows the NVF values read)
    }
#pragma unroll
    for (int k = 0; k < CPER; ++k) {
        const int r = r0 + ty + k * (LB / CTX);
        if (r < rows && c < cols) pool[(size_t)r * cols + c] = acc[k];
    }
}

// k_clip_pool_gather: k_clip_pool's result bit for bit without the LDS tiles -- one pixel per lane; per frame the 5 x 5 window of x
// (a window of 2 PAD + 1 beside it under NVF p > 5) is gathered from cache with clamped indices and the nine e values around the
// pixel are formed in registers.  The yardstick k_clip_pool's tiles are held against (wm_clip_pool_bench); no call takes it
__device__ __forceinline__ float pick3(float a, float b, float c, int i) { return i == 0 ? a : (i == 1 ? b : c); }
template <typename T, int MASK, int PAD>
__global__ __launch_bounds__(LB) void k_clip_pool_gather(const T* __restrict__ x, long long pitch, long long fstride, int frames, int rows, int cols,
                                                         const float* __restrict__ coef, const int* __restrict__ status,
                                                         const float* __restrict__ weights, float* __restrict__ pool, int accumulate,
                                                         OpResult* __restrict__ res)
{
    const int c = blockIdx.x * LTX + threadIdx.x % LTX, r = blockIdx.y * LTY + threadIdx.x / LTX;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int f = threadIdx.x; f < frames; f += LB) res[f] = OpResult{status[f], 0.0f};
    if (r >= rows || c >= cols) return;
    float acc = accumulate ? pool[(size_t)r * cols + c] : 0.0f;
    for (int f = 0; f < frames; ++f) {
        if (status[f] != 0) continue;
        const T* __restrict__ xf = x + (long long)f * fstride;
        const float* __restrict__ cf = coef + 8 * f;
        float nc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) nc[k] = -cf[k];
        float win[5][5];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) win[a][b] = Elem<T>::cvt1(xf[(long long)clampi(r + a - 2, rows) * pitch + clampi(c + b - 2, cols)]);
        float ee[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) ee[a][b] = residual1<1>(win[a] + b, win[a + 1] + b, win[a + 2] + b, 0, nc);
        const float ec = ee[1][1];
        const float g = locate_g(ec, r, c, rows, cols, cf, [&](int pr_, int pc_) {
            const int j = pc_ - c + 1;
            return pick3(pick3(ee[0][0], ee[0][1], ee[0][2], j), pick3(ee[1][0], ee[1][1], ee[1][2], j), pick3(ee[2][0], ee[2][1], ee[2][2], j), pr_ - r + 1);
        });
        float m = 0.0f;
        if (MASK == 1)
            m = locate_nvf<PAD>([&](int a, int b) {
                return PAD <= 2 ? win[a + 2][b + 2] : Elem<T>::cvt1(xf[(long long)clampi(r + a, rows) * pitch + clampi(c + b, cols)]);
            });
        acc = fmaf(weights[f], locate_h_value<MASK>(ec, m, g), acc);
    }
    pool[(size_t)r * cols + c] = acc;
}

// ---- k_locate_lay: a real source laid into a zeroed [pr][pc] complex plane, (0, 0) outside the source's rows x cols.  The source is
// a functor: src(r, c, i), i = r * cols + c, gives the plane's element of source pixel (r, c); FLAGS: the kernel also raises src.nz.
// Its members arrive as plain kernel arguments and it is put together in the kernel: pointers that come inside a struct argument
// are addressed as flat ones, which costs registers

// one dense real plane as the real part: a key of wm_locate, or a pooled image side in the place of h
struct LayPlane {
    static constexpr bool FLAGS = false;
    const float* key;
    __device__ __forceinline__ float2 operator()(int, int, size_t i) const { return make_float2(key[i], 0.0f); }
};
// wm_locate_bits: (key [tb(tile) == b0], key [tb(tile) == b1]).  The tiles lie on the KEY plane by the rule of wm_tiles_shape: tile
// (min(r / th, tny - 1), min(c / tw, tnx - 1)), the last one of an axis takes the remainder.  b1 = -2 (no entry of the table is below
// -1): the odd last bit rides alone
struct LayBits {
    static constexpr bool FLAGS = false;
    const float* key;
    const int* tb;
    int th, tw, tny, tnx, b0, b1;
    __device__ __forceinline__ float2 operator()(int r, int c, size_t i) const
    {
        const int bit = tb[min(r / th, tny - 1) * tnx + min(c / tw, tnx - 1)];
        const float w = key[i];
        return make_float2(bit == b0 ? w : 0.0f, bit == b1 ? w : 0.0f);
    }
};
// wm_locate_keys: (keyA, keyB); keyB null: the odd last key rides alone.  nz[0] / nz[1] (cleared on the stream at the start of the
// call) is set to 1 by every workgroup that saw a value of key A / key B other than 0: the workgroups store the same value, a later
// kernel on the stream reads it
struct LayKeys {
    static constexpr bool FLAGS = true;
    const float *keyA, *keyB;
    int* nz;
    __device__ __forceinline__ float2 operator()(int, int, size_t i) const { return make_float2(keyA[i], keyB ? keyB[i] : 0.0f); }
};

template <typename Src, typename... A>
__global__ __launch_bounds__(LB) void k_locate_lay(int rows, int cols, float2* __restrict__ plane, int pc, A... a)
{
    const Src src{a...};
    const int c = blockIdx.x * LTX + threadIdx.x % LTX, r = blockIdx.y * LTY + threadIdx.x / LTX;  // (the grid covers pr x pc exactly)
    float2 v = make_float2(0.0f, 0.0f);
    if (r < rows && c < cols) v = src(r, c, (size_t)r * cols + c);
    plane[(size_t)r * pc + c] = v;
    if constexpr (Src::FLAGS) {
        const int anyA = __syncthreads_or(v.x != 0.0f), anyB = __syncthreads_or(v.y != 0.0f);
        if (threadIdx.x == 0) {
            if (anyA) src.nz[0] = 1;
            if (anyB) src.nz[1] = 1;
        }
    }
}

// ---- the fold of a map: records, their tree, the z rule ---------------------------------------------------------------------------

// one block's or one frame's fold: argmax (ties to the smallest index), sum and sum of squares in f64
struct PeakRec {
    double sum, sumsq;
    long long idx;
    float val;
    int pad;
};
__device__ __forceinline__ bool peak_better(float v, long long i, float bv, long long bi) { return v > bv || (v == bv && i < bi); }
// map value v at index i as a record of its own, and the record of nothing (idx -1)
__device__ __forceinline__ PeakRec peak_of(float v, long long i) { return PeakRec{(double)v, (double)v * (double)v, i, v, 0}; }
__device__ __forceinline__ PeakRec peak_none() { return PeakRec{0.0, 0.0, -1, 0.0f, 0}; }
// record o taken into the running record me
__device__ __forceinline__ void peak_take(PeakRec& me, const PeakRec& o)
{
    me.sum += o.sum; me.sumsq += o.sumsq;
    if (o.idx >= 0 && (me.idx < 0 || peak_better(o.val, o.idx, me.val, me.idx))) { me.val = o.val; me.idx = o.idx; }
}

// a workgroup's 256 records folded pairwise in a fixed tree; the result is in s_rec[0]
__device__ __forceinline__ void peak_tree(PeakRec* s_rec, int t)
{
    for (int half = LB / 2; half > 0; half >>= 1) {
        __syncthreads();
        if (t < half) {
            PeakRec me = s_rec[t];
            peak_take(me, s_rec[t + half]);
            s_rec[t] = me;
        }
    }
    __syncthreads();
}
// a workgroup's fold of the nblk block records of one map: thread t takes t, t + 256, ... in ascending order, then the tree
__device__ __forceinline__ void peak_fold(const PeakRec* __restrict__ part, int nblk, PeakRec* s_rec, int t)
{
    PeakRec me = peak_none();
    for (int b = t; b < nblk; b += LB) peak_take(me, part[b]);
    s_rec[t] = me;
    peak_tree(s_rec, t);
}

// z of a peak against the offsets that remain in (sum, sumsq, cnt) once the 3 x 3 block around it is taken out: (val - mu) / sigma in
// f64 (population sigma), NaN when fewer than two offsets remain or they do not vary
__device__ __forceinline__ float peak_z(double sum, double sumsq, long long cnt, float val)
{
    float z = __builtin_nanf("");
    if (cnt >= 2) {
        const double mu = sum / (double)cnt;
        const double var = sumsq / (double)cnt - mu * mu;
        if (var > 0.0) z = (float)(((double)val - mu) / sqrt(var));
    }
    return z;
}
// ... with (sum, sumsq) still over all ny x nx offsets: the values at(i, j) of the 3 x 3 block around (oy, ox) are taken out first
template <typename At>
__device__ __forceinline__ float peak_z_around(double sum, double sumsq, int oy, int ox, int ny, int nx, float val, At&& at)
{
    long long cnt = (long long)ny * nx;
    for (int i = max(oy - 1, 0); i <= min(oy + 1, ny - 1); ++i)
        for (int j = max(ox - 1, 0); j <= min(ox + 1, nx - 1); ++j) {
            const double v = (double)at(i, j);
            sum -= v; sumsq -= v * v; --cnt;
        }
    return peak_z(sum, sumsq, cnt, val);
}
// the four records {oy, ox, peak, z} of a map; an unsolvable frame (st != 0): its status and zeros
__device__ __forceinline__ void peak_records(OpResult* __restrict__ res, int st, int oy, int ox, float val, float z)
{
    res[0] = OpResult{st, st ? 0.0f : (float)oy};
    res[1] = OpResult{st, st ? 0.0f : (float)ox};
    res[2] = OpResult{st, st ? 0.0f : val};
    res[3] = OpResult{st, st ? 0.0f : z};
}

// the value of one half of a complex plane at an offset: the product with 1 / (pr pc), or exactly zero for a half that carries no
// key (its flag is clear, or the odd last key has no partner) -- not the rounding residue of the other half
__device__ __forceinline__ float keys_half(const float2 v, int half, float scale, bool use) { return use ? (half ? v.y : v.x) * scale : 0.0f; }

// k_locate_map: the ny x nx admissible offsets of an inverse plane times scale = 1 / (pr pc) (the transforms are not normalised): the
// real parts are key A's map and, under PAIR, the imaginary parts key B's (mapA / mapB null: not stored).  Workgroup b folds values
// [4096 b, 4096 (b + 1)) of each map into partA[b] / partB[b].  nz: the pair's flags (k_locate_lay), null: key A is in use (wm_locate).
// Without PAIR there is no second half: no load, no record, no LDS for it.  An unsolvable frame's maps are zero
template <bool PAIR>
__global__ __launch_bounds__(LB) void k_locate_map(const float2* __restrict__ plane, int pc, int ny, int nx, float scale, const int* __restrict__ status,
                                                   const int* __restrict__ nz, float* __restrict__ mapA, float* __restrict__ mapB,
                                                   PeakRec* __restrict__ partA, PeakRec* __restrict__ partB)
{
    __shared__ PeakRec s_rec[PAIR ? 2 : 1][LB];
    const int t = threadIdx.x;
    const long long n = (long long)ny * nx;
    const long long i0 = (long long)blockIdx.x * (LB * PEAK_PER);
    const bool dead = status[0] != 0;
    const bool useA = !nz || nz[0] != 0, useB = PAIR && nz[1] != 0;
    PeakRec a = peak_none(), b = peak_none();
#pragma unroll 4
    for (int k = 0; k < PEAK_PER; ++k) {
        const long long i = i0 + t + (long long)k * LB;
        if (i >= n) break;
        const int oy = (int)(i / nx), ox = (int)(i % nx);
        float2 v = make_float2(0.0f, 0.0f);
        if (!dead) {
            if (PAIR) v = plane[(size_t)oy * pc + ox];
            else v.x = plane[(size_t)oy * pc + ox].x;
        }
        const float re = keys_half(v, 0, scale, useA);
        if (mapA) mapA[i] = re;
        peak_take(a, peak_of(re, i));
        if (PAIR) {
            const float im = keys_half(v, 1, scale, useB);
            if (mapB) mapB[i] = im;
            peak_take(b, peak_of(im, i));
        }
    }
    s_rec[0][t] = a;
    peak_tree(s_rec[0], t);
    if (t == 0) partA[blockIdx.x] = s_rec[0][0];
    if constexpr (PAIR) {
        s_rec[1][t] = b;
        peak_tree(s_rec[1], t);
        if (t == 0) partB[blockIdx.x] = s_rec[1][0];
    }
}

// k_locate_records: workgroup h folds the nblk block records of half h of a (pair, frame) (part + h * nblk; grid 1: key A alone),
// takes the values of the 3 x 3 block around the argmax out of the sums -- formed as k_locate_map formed them, so they are the map's
// bits -- and writes the half's four records {oy, ox, peak, z} to res + 4 h: z = (peak - mu) / sigma over the offsets outside that
// block (peak_z).  nz as in k_locate_map
__global__ __launch_bounds__(LB) void k_locate_records(const PeakRec* __restrict__ part, int nblk, const float2* __restrict__ plane, int pc, int ny,
                                                       int nx, float scale, const int* __restrict__ status, const int* __restrict__ nz,
                                                       OpResult* __restrict__ res)
{
    __shared__ PeakRec s_rec[LB];
    const int t = threadIdx.x, half = (int)blockIdx.x;
    peak_fold(part + (size_t)half * nblk, nblk, s_rec, t);
    if (t != 0) return;
    const int st = status[0];
    const bool use = !nz || nz[half] != 0;
    const PeakRec tot = s_rec[0];
    const int oy = (int)(tot.idx / nx), ox = (int)(tot.idx % nx);
    float z = 0.0f;
    if (st == 0)
        z = peak_z_around(tot.sum, tot.sumsq, oy, ox, ny, nx, tot.val,
                          [&](int i, int j) { return keys_half(plane[(size_t)i * pc + j], half, scale, use); });
    peak_records(res + 4 * half, st, oy, ox, tot.val, z);
}

// ---- wm_locate_bits: one map per payload bit, two bits per transform -----------------------------------

// one block's sums of the two maps of a pair: sum and sum of squares in f64
struct BitsRec {
    double s0, q0, s1, q1;
};
__device__ __forceinline__ void bits_tree(BitsRec* s_b, int t)
{
    for (int half = LB / 2; half > 0; half >>= 1) {
        __syncthreads();
        if (t < half) {
            const BitsRec o = s_b[t + half];
            BitsRec me = s_b[t];
            me.s0 += o.s0; me.q0 += o.q0; me.s1 += o.s1; me.q1 += o.q1;
            s_b[t] = me;
        }
    }
    __syncthreads();
}

// k_locate_bits_acc: the ny x nx admissible offsets of the pair's inverse plane times 1 / (pr pc): the real parts are bit b0's map,
// the imaginary parts bit b1's.  Stores both maps, E = re^2 + im^2 for the first pair and E += re^2 + im^2 for the later ones (f32,
// in the order of the pairs: E's bits do not depend on the batch), and folds each map's sum and sum of squares over the workgroup's
// 4096 consecutive values into part[block].  use0 / use1 = 0: the bit has no tile (or, use1, the odd last pair has no second bit):
// its map is exactly zero, not the rounding residue of its partner.  epart (the last pair only): the block's fold of the finished E,
// as k_locate_map folds a map.  An unsolvable frame's maps and E are zero
template <bool FIRST>
__global__ __launch_bounds__(LB) void k_locate_bits_acc(const float2* __restrict__ plane, int pc, int ny, int nx, float scale, const int* __restrict__ status,
                                                        int use0, int use1, float* __restrict__ map0, float* __restrict__ map1, float* __restrict__ E,
                                                        BitsRec* __restrict__ part, PeakRec* __restrict__ epart)
{
    __shared__ BitsRec s_b[LB];
    __shared__ PeakRec s_rec[LB];
    const int t = threadIdx.x;
    const long long n = (long long)ny * nx;
    const long long i0 = (long long)blockIdx.x * (LB * PEAK_PER);
    const bool dead = status[0] != 0;
    BitsRec me{0.0, 0.0, 0.0, 0.0};
    PeakRec pk = peak_none();
#pragma unroll 4
    for (int k = 0; k < PEAK_PER; ++k) {
        const long long i = i0 + t + (long long)k * LB;
        if (i >= n) break;
        const int oy = (int)(i / nx), ox = (int)(i % nx);
        const float2 v = dead ? make_float2(0.0f, 0.0f) : plane[(size_t)oy * pc + ox];
        const float re = keys_half(v, 0, scale, use0), im = keys_half(v, 1, scale, use1);
        map0[i] = re;
        if (map1) map1[i] = im;
        const float e2 = fmaf(im, im, re * re);
        const float e = FIRST ? e2 : E[i] + e2;
        E[i] = e;
        me.s0 += (double)re; me.q0 += (double)re * (double)re;
        me.s1 += (double)im; me.q1 += (double)im * (double)im;
        if (epart) peak_take(pk, peak_of(e, i));
    }
    s_b[t] = me;
    bits_tree(s_b, t);
    if (t == 0) part[blockIdx.x] = s_b[0];
    if (epart) {  // (the same in every lane: a kernel argument)
        s_rec[t] = pk;
        peak_tree(s_rec, t);
        if (t == 0) epart[blockIdx.x] = s_rec[0];
    }
}

// k_locate_bits_fold: workgroup 0 writes the frame's four records of E by k_locate_records' rule, workgroup 1 + b the soft value of
// bit b.  Every workgroup folds E's nblk block records itself (peak_fold): all agree on the argmax o* without waiting for each
// other.  Bit b: its block records folded in the same order, the values of the 3 x 3 block around o* taken out of the sums --
// re-read from the stored map, so they are the map's bits --, and soft = (map_b(o*) - mu_b) / sigma_b by peak_z.
// part: [pairs][nblk], maps: [nbits][ny nx].  An unsolvable frame: its status and zeros
__global__ __launch_bounds__(LB) void k_locate_bits_fold(const PeakRec* __restrict__ epart, const BitsRec* __restrict__ part, int nblk,
                                                         const float* __restrict__ E, const float* __restrict__ maps, int ny, int nx,
                                                         const int* __restrict__ status, OpResult* __restrict__ loc, OpResult* __restrict__ soft)
{
    __shared__ PeakRec s_rec[LB];
    __shared__ double s_sum[LB], s_sq[LB];
    const int t = threadIdx.x;
    peak_fold(epart, nblk, s_rec, t);
    const PeakRec tot = s_rec[0];
    const int st = status[0];
    const int oy = (int)(tot.idx / nx), ox = (int)(tot.idx % nx);
    if (blockIdx.x == 0) {
        if (t != 0) return;
        float z = 0.0f;
        if (st == 0) z = peak_z_around(tot.sum, tot.sumsq, oy, ox, ny, nx, tot.val, [&](int i, int j) { return E[(size_t)i * nx + j]; });
        peak_records(loc, st, oy, ox, tot.val, z);
        return;
    }
    const int bit = (int)blockIdx.x - 1;
    const BitsRec* __restrict__ pp = part + (size_t)(bit / 2) * nblk;
    double sum = 0.0, sumsq = 0.0;
    for (int b = t; b < nblk; b += LB) {
        const BitsRec o = pp[b];
        sum += bit % 2 ? o.s1 : o.s0; sumsq += bit % 2 ? o.q1 : o.q0;
    }
    s_sum[t] = sum; s_sq[t] = sumsq;
    for (int half = LB / 2; half > 0; half >>= 1) {
        __syncthreads();
        if (t < half) { s_sum[t] += s_sum[t + half]; s_sq[t] += s_sq[t + half]; }
    }
    if (t != 0) return;
    if (st != 0) {
        soft[bit] = OpResult{st, 0.0f};
        return;
    }
    const float* __restrict__ mp = maps + (size_t)bit * ((size_t)ny * nx);
    soft[bit] = OpResult{0, peak_z_around(s_sum[0], s_sq[0], oy, ox, ny, nx, mp[tot.idx], [&](int i, int j) { return mp[(size_t)i * nx + j]; })};
}

// the block records of a map of ny x nx offsets, and the scale of an unnormalised forward + inverse transform pair
int locate_nblk(int ny, int nx) { return (int)(((long long)ny * nx + LB * PEAK_PER - 1) / (LB * PEAK_PER)); }
float locate_scale(int pr, int pc) { return 1.0f / ((float)pr * (float)pc); }  // (a power of two: the scaling is exact)

using LayF = const float* __restrict__;
using LayI = const int* __restrict__;
template <typename Src, typename... A>
void launch_lay(hipStream_t s, int rows, int cols, float* plane, int pr, int pc, A... a)
{
    WM_KLAUNCH((k_locate_lay<Src, A...>), dim3(pc / LTX, pr / LTY), dim3(LB), 0, s, rows, cols, reinterpret_cast<float2*>(plane), pc, a...);
}

}  // namespace

size_t locate_part_bytes(int ny, int nx) { return (size_t)locate_nblk(ny, nx) * sizeof(PeakRec); }
size_t locate_bits_part_bytes(int ny, int nx) { return (size_t)locate_nblk(ny, nx) * sizeof(BitsRec); }

void launch_locate_lay(hipStream_t s, const float* src, int rows, int cols, float* plane, int pr, int pc)
{
    launch_lay<LayPlane, LayF>(s, rows, cols, plane, pr, pc, src);
}

void launch_locate_lay_bits(hipStream_t s, const float* key, int key_rows, int key_cols, const int* tile_bit, const TileShape& ts, int b0, int b1,
                            float* plane, int pr, int pc)
{
    launch_lay<LayBits, LayF, LayI, int, int, int, int, int, int>(s, key_rows, key_cols, plane, pr, pc, key, tile_bit, ts.th, ts.tw, ts.ny, ts.nx, b0, b1);
}

void launch_locate_lay_keys(hipStream_t s, const float* key_a, const float* key_b, int key_rows, int key_cols, float* plane, int pr, int pc, int* nz)
{
    launch_lay<LayKeys, LayF, LayF, int*>(s, key_rows, key_cols, plane, pr, pc, key_a, key_b, nz);
}

void launch_locate_map(hipStream_t s, const float* plane, int pr, int pc, int ny, int nx, const int* status, const int* nz, bool pair, float* map_a,
                       float* map_b, void* part, OpResult* res)
{
    const float scale = locate_scale(pr, pc);
    const int nblk = locate_nblk(ny, nx);
    const float2* pl = reinterpret_cast<const float2*>(plane);
    PeakRec* pa = static_cast<PeakRec*>(part);
    if (pair) WM_KLAUNCH(k_locate_map<true>, dim3(nblk), dim3(LB), 0, s, pl, pc, ny, nx, scale, status, nz, map_a, map_b, pa, pa + nblk);
    else WM_KLAUNCH(k_locate_map<false>, dim3(nblk), dim3(LB), 0, s, pl, pc, ny, nx, scale, status, nz, map_a, nullptr, pa, nullptr);
    if (res) WM_KLAUNCH(k_locate_records, dim3(pair ? 2 : 1), dim3(LB), 0, s, pa, nblk, pl, pc, ny, nx, scale, status, nz, res);
}

void launch_locate_bits_acc(hipStream_t s, const float* plane, int pr, int pc, int ny, int nx, const int* status, bool first, bool use0, bool use1,
                            float* map0, float* map1, float* energy, void* part, void* epart)
{
    const float scale = locate_scale(pr, pc);
    const int nblk = locate_nblk(ny, nx);
    const float2* pl = reinterpret_cast<const float2*>(plane);
    if (first)
        WM_KLAUNCH(k_locate_bits_acc<true>, dim3(nblk), dim3(LB), 0, s, pl, pc, ny, nx, scale, status, use0 ? 1 : 0, use1 ? 1 : 0, map0, map1, energy,
                   static_cast<BitsRec*>(part), static_cast<PeakRec*>(epart));
    else
        WM_KLAUNCH(k_locate_bits_acc<false>, dim3(nblk), dim3(LB), 0, s, pl, pc, ny, nx, scale, status, use0 ? 1 : 0, use1 ? 1 : 0, map0, map1, energy,
                   static_cast<BitsRec*>(part), static_cast<PeakRec*>(epart));
}

void launch_locate_bits_fold(hipStream_t s, const void* epart, const void* part, int ny, int nx, int nbits, const float* energy, const float* maps,
                             const int* status, OpResult* loc, OpResult* soft)
{
    WM_KLAUNCH(k_locate_bits_fold, dim3(1 + nbits), dim3(LB), 0, s, static_cast<const PeakRec*>(epart), static_cast<const BitsRec*>(part),
               locate_nblk(ny, nx), energy, maps, ny, nx, status, loc, soft);
}

void launch_locate_e(const Sweep& sw, int frame, float* e, float* m)
{
    const PlaneDesc& x = sw.x;
    const int rows = sw.lg.rows, cols = sw.lg.cols;
    const dim3 grid((cols + LTX - 1) / LTX, (rows + LTY - 1) / LTY);
    WM_DISPATCH_T(x.dtype, for_mask_pad(sw.mask, sw.pad, [&](auto mk, auto p) {
        WM_KLAUNCH((k_locate_e<T, decltype(mk)::value, decltype(p)::value>), grid, dim3(LB), 0, sw.s, (const T*)x.p + (long long)frame * x.fstride,
                   x.pitch, rows, cols, sw.coef + 8 * frame, sw.status + frame, e, m);
    }));
}

void launch_locate_h(const Sweep& sw, int frame, const float* e, const float* m, float* plane, int pr, int pc)
{
    const dim3 grid(pc / LTX, pr / LTY);
    if (sw.mask == 0)
        WM_KLAUNCH(k_locate_h<0>, grid, dim3(LB), 0, sw.s, e, m, sw.lg.rows, sw.lg.cols, sw.coef + 8 * frame, sw.status + frame,
                   reinterpret_cast<float2*>(plane), pc);
    else
        WM_KLAUNCH(k_locate_h<1>, grid, dim3(LB), 0, sw.s, e, m, sw.lg.rows, sw.lg.cols, sw.coef + 8 * frame, sw.status + frame,
                   reinterpret_cast<float2*>(plane), pc);
}

void launch_clip_pool(const Sweep& sw, const float* weights, float* pool, bool accumulate, OpResult* res)
{
    const PlaneDesc& x = sw.x;
    const int rows = sw.lg.rows, cols = sw.lg.cols;
    const dim3 grid((cols + CTX - 1) / CTX, (rows + CTY - 1) / CTY);
    WM_DISPATCH_T(x.dtype, for_mask_pad(sw.mask, sw.pad, [&](auto mk, auto p) {
        WM_KLAUNCH((k_clip_pool<T, decltype(mk)::value, decltype(p)::value>), grid, dim3(LB), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, sw.frames, rows,
                   cols, sw.coef, sw.status, weights, pool, accumulate ? 1 : 0, res);
    }));
}

void launch_clip_pool_gather(const Sweep& sw, const float* weights, float* pool, bool accumulate, OpResult* res)
{
    const PlaneDesc& x = sw.x;
    const int rows = sw.lg.rows, cols = sw.lg.cols;
    const dim3 grid((cols + LTX - 1) / LTX, (rows + LTY - 1) / LTY);
    WM_DISPATCH_T(x.dtype, for_mask_pad(sw.mask, sw.pad, [&](auto mk, auto p) {
        WM_KLAUNCH((k_clip_pool_gather<T, decltype(mk)::value, decltype(p)::value>), grid, dim3(LB), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, sw.frames,
                   rows, cols, sw.coef, sw.status, weights, pool, accumulate ? 1 : 0, res);
    }));
}

}  // namespace wmk
