// wm_k_fft.hip -- the 2-D complex f32 transform behind wm_locate and wm_fft2: k_fft_rows (batched power-of-two rows through LDS),
// k_fft_transpose (tiled LDS transpose), k_locate_mul (the spectrum product) and k_locate_mul3 (the product into a third plane).
//
// A 2-D transform of a [pr][pc] plane is: rows of length pc, transpose, rows of length pr -- the spectrum then lies TRANSPOSED
// ([pc][pr]); wm_locate multiplies and starts the inverse in that layout, so a forward and an inverse transform need one transpose
// each.  Every workgroup works on its own rows or tile: no waits between workgroups, no atomics, a fixed order of operations.
#include "wm_kernels.hpp"
#include <vector>

namespace wmk {

namespace {

constexpr int FFT_BLOCK = 256;
constexpr int FFT_MIN_ELEMS = 1024;  // complex elements a workgroup holds at least: rows shorter than that share one (1024 / P rows)

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a * w, or a * conj(w) for the inverse direction (the table holds exp(-2 pi i t / P))
template <bool INV>
__device__ __forceinline__ float2 ctw(float2 a, float2 w)
{
    const float wy = INV ? -w.y : w.y;
    return make_float2(a.x * w.x - a.y * wy, a.x * wy + a.y * w.x);
}
// -i a (forward) or +i a (inverse): the quarter turn of the radix-4 butterfly
template <bool INV>
__device__ __forceinline__ float2 cquarter(float2 a) { return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }

// One Stockham pass of radix R over the ROWS rows of length P a workgroup holds: butterfly b of the workgroup (b = t + 256 i) is
// butterfly j = b % (P / R) of row b / (P / R).  It reads elements j + r P / R, turns them by exp(-+2 pi i r (j % NS) / (NS R)),
// and writes the radix-R DFT to (j / NS) NS R + j % NS + r NS: after the passes whose radices multiply to P the row is in natural
// order (autosort: no bit reversal).  All reads of a pass are in registers before `mid` runs (the barrier of an in-place LDS pass)
template <int LOGP, int R, int NS, bool INV, int NB, typename Load, typename Mid, typename Store>
__device__ __forceinline__ void fft_pass(const float2* __restrict__ tw, int t, Load load, Mid mid, Store store)
{
    constexpr int P = 1 << LOGP;
    constexpr int PER_ROW = P / R;            // butterflies per row
    constexpr int TSTEP = P / (NS * R);       // table step of this pass
    float2 v[NB][R];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = t + FFT_BLOCK * i;
        const int row = b / PER_ROW, j = b % PER_ROW;
#pragma unroll
        for (int r = 0; r < R; ++r) v[i][r] = load(row, j + r * PER_ROW);
    }
    mid();
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = t + FFT_BLOCK * i;
        const int row = b / PER_ROW, j = b % PER_ROW;
        const int w = j % NS;
        if (NS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) v[i][r] = ctw<INV>(v[i][r], tw[r * w * TSTEP]);
        }
        const int d = (j / NS) * (NS * R) + w;
        if constexpr (R == 2) {
            store(row, d, cadd(v[i][0], v[i][1]));
            store(row, d + NS, csub(v[i][0], v[i][1]));
        } else {
            const float2 a0 = cadd(v[i][0], v[i][2]), a1 = csub(v[i][0], v[i][2]);
            const float2 a2 = cadd(v[i][1], v[i][3]), a3 = cquarter<INV>(csub(v[i][1], v[i][3]));
            store(row, d, cadd(a0, a2));
            store(row, d + NS, cadd(a1, a3));
            store(row, d + 2 * NS, csub(a0, a2));
            store(row, d + 3 * NS, csub(a1, a3));
        }
    }
}

// the passes behind the first one: radix 4 with NS = 2^LOGNS, the last of them stores to memory
template <int LOGP, int LOGNS, bool INV, int NB4, typename LdsLoad, typename LdsStore, typename MemStore>
__device__ __forceinline__ void fft_tail(const float2* __restrict__ tw, int t, LdsLoad lload, LdsStore lstore, MemStore mstore)
{
    if constexpr (LOGNS + 2 == LOGP) {
        fft_pass<LOGP, 4, (1 << LOGNS), INV, NB4>(tw, t, lload, [] {}, mstore);
    } else {
        // in place: every element of the row buffer is read before any is overwritten, and written before the next pass reads
        fft_pass<LOGP, 4, (1 << LOGNS), INV, NB4>(tw, t, lload, [] { __syncthreads(); }, lstore);
        __syncthreads();
        fft_tail<LOGP, LOGNS + 2, INV, NB4>(tw, t, lload, lstore, mstore);
    }
}

// k_fft_rows: in-place transform of every row of a dense [nrows][P] complex plane, P = 2^LOGP in 64 .. 8192.  One workgroup of 256
// holds ROWS = max(1, 1024 / P) whole rows in LDS as float2 (64 KiB at P = 8192).  The first pass reads memory and the last one
// writes it, both at unit stride across the lanes; the passes between them go through the row buffer with 8-byte accesses.
// Radix 4, with one radix-2 pass in front when log2 P is odd (its turn factors are all 1).  tw: [P] exp(-2 pi i t / P), built on the
// host in f64
template <int LOGP, bool INV>
__global__ __launch_bounds__(FFT_BLOCK) void k_fft_rows(float2* __restrict__ data, const float2* __restrict__ tw)
{
    constexpr int P = 1 << LOGP;
    constexpr int ROWS = P >= FFT_MIN_ELEMS ? 1 : FFT_MIN_ELEMS / P;
    constexpr int NB4 = ROWS * P / 4 / FFT_BLOCK;
    __shared__ float2 s_row[ROWS * P];
    const int t = threadIdx.x;
    float2* __restrict__ base = data + (size_t)blockIdx.x * (ROWS * P);
    auto mload = [&](int row, int idx) { return base[row * P + idx]; };
    auto mstore = [&](int row, int idx, float2 v) { base[row * P + idx] = v; };
    auto lload = [&](int row, int idx) { return s_row[row * P + idx]; };
    auto lstore = [&](int row, int idx, float2 v) { s_row[row * P + idx] = v; };
    if constexpr (LOGP % 2 == 1) {
        fft_pass<LOGP, 2, 1, INV, 2 * NB4>(tw, t, mload, [] {}, lstore);
        __syncthreads();
        fft_tail<LOGP, 1, INV, NB4>(tw, t, lload, lstore, mstore);
    } else {
        fft_pass<LOGP, 4, 1, INV, NB4>(tw, t, mload, [] {}, lstore);
        __syncthreads();
        fft_tail<LOGP, 2, INV, NB4>(tw, t, lload, lstore, mstore);
    }
}

// k_fft_transpose: dst [ncols][nrows] = src [nrows][ncols]^T in tiles of 64 x 64 complex elements through LDS (rows padded to 65:
// the column reads of the store phase fall on different banks).  nrows and ncols are multiples of 64
constexpr int TT = 64;
__global__ __launch_bounds__(FFT_BLOCK) void k_fft_transpose(const float2* __restrict__ src, float2* __restrict__ dst, int nrows, int ncols)
{
    __shared__ float2 s_tile[TT][TT + 1];
    const int tx = threadIdx.x % TT, ty = threadIdx.x / TT;  // 64 x 4
    const int r0 = blockIdx.y * TT, c0 = blockIdx.x * TT;
#pragma unroll
    for (int i = 0; i < TT; i += FFT_BLOCK / TT) s_tile[ty + i][tx] = src[(size_t)(r0 + ty + i) * ncols + c0 + tx];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TT; i += FFT_BLOCK / TT) dst[(size_t)(c0 + ty + i) * nrows + r0 + tx] = s_tile[tx][ty + i];
}

// k_locate_mul: a = conj(a) * b per element (two elements per lane: 16-byte accesses); n2 = pairs
__global__ __launch_bounds__(FFT_BLOCK) void k_locate_mul(float4* __restrict__ a, const float4* __restrict__ b, size_t n2)
{
    const size_t i = (size_t)blockIdx.x * FFT_BLOCK + threadIdx.x;
    if (i >= n2) return;
    const float4 h = a[i], w = b[i];
    a[i] = make_float4(h.x * w.x + h.y * w.y, h.x * w.y - h.y * w.x, h.z * w.z + h.w * w.w, h.z * w.w - h.w * w.z);
}

// k_locate_mul3: out = conj(h) * k per element, h and k kept (wm_locate_bits multiplies one frame's spectrum with every key pair's)
__global__ __launch_bounds__(FFT_BLOCK) void k_locate_mul3(const float4* __restrict__ hs, const float4* __restrict__ ks, float4* __restrict__ out, size_t n2)
{
    const size_t i = (size_t)blockIdx.x * FFT_BLOCK + threadIdx.x;
    if (i >= n2) return;
    const float4 h = hs[i], w = ks[i];
    out[i] = make_float4(h.x * w.x + h.y * w.y, h.x * w.y - h.y * w.x, h.z * w.z + h.w * w.w, h.z * w.w - h.w * w.z);
}

template <int LOGP>
void launch_rows_p(hipStream_t s, float2* data, int nrows, const float2* tw, bool inverse)
{
    constexpr int P = 1 << LOGP;
    constexpr int ROWS = P >= FFT_MIN_ELEMS ? 1 : FFT_MIN_ELEMS / P;
    if (inverse) WM_KLAUNCH((k_fft_rows<LOGP, true>), dim3(nrows / ROWS), dim3(FFT_BLOCK), 0, s, data, tw);
    else WM_KLAUNCH((k_fft_rows<LOGP, false>), dim3(nrows / ROWS), dim3(FFT_BLOCK), 0, s, data, tw);
}

}  // namespace

int fft_log2(int n)
{
    for (int l = FFT_LOG_MIN; l <= FFT_LOG_MAX; ++l)
        if (n == (1 << l)) return l;
    return -1;
}

void fft_twiddles(int P, float* out)
{
    const double step = -2.0 * 3.14159265358979323846264338327950288 / (double)P;
    for (int t = 0; t < P; ++t) {
        out[2 * t] = (float)cos(step * t);
        out[2 * t + 1] = (float)sin(step * t);
    }
}

hipError_t fft_twiddles_upload(float* tw_dev, int pr, int pc)
{
    std::vector<float> tw((size_t)2 * (pr + pc));
    fft_twiddles(pr, tw.data());
    fft_twiddles(pc, tw.data() + (size_t)2 * pr);
    return hipMemcpy(tw_dev, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice);
}

void launch_fft_rows(hipStream_t s, float* data, int nrows, int P, const float* tw, bool inverse)
{
    float2* d = reinterpret_cast<float2*>(data);
    const float2* w = reinterpret_cast<const float2*>(tw);
    switch (fft_log2(P)) {
    case 6: launch_rows_p<6>(s, d, nrows, w, inverse); break;
    case 7: launch_rows_p<7>(s, d, nrows, w, inverse); break;
    case 8: launch_rows_p<8>(s, d, nrows, w, inverse); break;
    case 9: launch_rows_p<9>(s, d, nrows, w, inverse); break;
    case 10: launch_rows_p<10>(s, d, nrows, w, inverse); break;
    case 11: launch_rows_p<11>(s, d, nrows, w, inverse); break;
    case 12: launch_rows_p<12>(s, d, nrows, w, inverse); break;
    case 13: launch_rows_p<13>(s, d, nrows, w, inverse); break;
    default: break;  // (the callers have checked the length)
    }
}

void launch_fft_transpose(hipStream_t s, const float* src, float* dst, int nrows, int ncols)
{
    WM_KLAUNCH(k_fft_transpose, dim3(ncols / TT, nrows / TT), dim3(FFT_BLOCK), 0, s, reinterpret_cast<const float2*>(src),
               reinterpret_cast<float2*>(dst), nrows, ncols);
}

void launch_locate_mul(hipStream_t s, float* a, const float* b, size_t n)
{
    const size_t n2 = n / 2;
    WM_KLAUNCH(k_locate_mul, dim3((unsigned)((n2 + FFT_BLOCK - 1) / FFT_BLOCK)), dim3(FFT_BLOCK), 0, s, reinterpret_cast<float4*>(a),
               reinterpret_cast<const float4*>(b), n2);
}

void launch_locate_mul3(hipStream_t s, const float* h, const float* k, float* out, size_t n)
{
    const size_t n2 = n / 2;
    WM_KLAUNCH(k_locate_mul3, dim3((unsigned)((n2 + FFT_BLOCK - 1) / FFT_BLOCK)), dim3(FFT_BLOCK), 0, s, reinterpret_cast<const float4*>(h),
               reinterpret_cast<const float4*>(k), reinterpret_cast<float4*>(out), n2);
}

}  // namespace wmk
