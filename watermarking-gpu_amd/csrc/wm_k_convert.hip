// wm_k_convert.hip -- the pixel-format front (wm_rgb2gray, wm_unpack_rgb8, wm_pack_rgb8): element-wise, memory-bound kernels.
//
// One lane handles four consecutive pixels of one row; a block is 256 lanes (1024 pixels of a row), the grid is
// (column chunks, rows, frames).  A planar f32 plane moves as one 16-byte access per lane and channel, a planar u8 plane as one
// dword, packed pixels as one 12-byte access (a wave covers 768 contiguous bytes).  Which planes may be accessed that way is
// decided on the host per plane (vec_ok's rule, PlaneDesc::aligned / PackedDesc::aligned: f32 rows only need 4-byte alignment,
// tools/ubench/unaligned.hip); the flags are uniform over the launch, so only the wave at a ragged right edge diverges.  A lane whose four
// pixels reach past the right edge, and every lane of a plane that does not qualify, takes the per-pixel form of the same access.
// Row addresses are 64-bit.  No LDS, no atomics, nothing shared between lanes.
//
// Arithmetic of the grey (wmo_rgb2gray's order; the library is built with -ffp-contract=off): (wr * R + wg * G) + wb * B in f32.
#include "wm_kernels.hpp"

namespace wmk {
namespace {

constexpr int CV_LANES = 256;  // lanes per block; 4 pixels each

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));          // 16 bytes at a 4-byte aligned address
struct __attribute__((aligned(4))) P12 { unsigned int a, b, c; };          // four packed pixels: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3

struct Px4 { float v[4]; };  // one channel of a lane's four pixels

template <class T> struct Ld;
template <> struct Ld<float> {
    static __device__ __forceinline__ Px4 vec(const float* p)
    {
        const f4u t = *reinterpret_cast<const f4u*>(p);
        return Px4{{t.x, t.y, t.z, t.w}};
    }
    static __device__ __forceinline__ float one(const float* p) { return *p; }
};
template <> struct Ld<unsigned char> {
    static __device__ __forceinline__ Px4 vec(const unsigned char* p)
    {
        const unsigned int w = *reinterpret_cast<const unsigned int*>(p);
        return Px4{{(float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24)}};
    }
    static __device__ __forceinline__ float one(const unsigned char* p) { return (float)*p; }
};

// n: pixels of the lane inside the row (4, or 1..3 at the right edge)
template <class T>
__device__ __forceinline__ Px4 load4(const T* p, bool vec, int n)
{
    if (vec && n == 4) return Ld<T>::vec(p);
    Px4 r{{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) r.v[i] = Ld<T>::one(p + i);
    return r;
}

// f32 -> 8 bits: clamp to [0, 255], truncate toward zero, NaN gives 0 (what v_cvt_u32_f32 and a min give)
__device__ __forceinline__ unsigned int to_u8(float v)
{
    return (unsigned int)__builtin_fminf(__builtin_fmaxf(v, 0.0f), 255.0f);
}

__device__ __forceinline__ void store4(float* p, bool vec, int n, const Px4& x)
{
    if (vec && n == 4) {
        f4u t; t.x = x.v[0]; t.y = x.v[1]; t.z = x.v[2]; t.w = x.v[3];
        *reinterpret_cast<f4u*>(p) = t;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) p[i] = x.v[i];
}
// (a planar u8 output of wm_unpack_rgb8 holds values that came from bytes: the conversion is exact)
__device__ __forceinline__ void store4(unsigned char* p, bool vec, int n, const Px4& x)
{
    if (vec && n == 4) {
        *reinterpret_cast<unsigned int*>(p) = to_u8(x.v[0]) | (to_u8(x.v[1]) << 8) | (to_u8(x.v[2]) << 16) | (to_u8(x.v[3]) << 24);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) p[i] = (unsigned char)to_u8(x.v[i]);
}

__device__ __forceinline__ Px4 gray_of(const Px4& R, const Px4& G, const Px4& B, float wr, float wg, float wb)
{
    Px4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) y.v[i] = (wr * R.v[i] + wg * G.v[i]) + wb * B.v[i];
    return y;
}

// the lane's place: first column c0, pixels n (0: the lane is outside the row), row and frame from the grid
struct Lane { int c0, n; long long r, f; };
__device__ __forceinline__ Lane lane_of(int cols)
{
    Lane l;
    l.c0 = (blockIdx.x * CV_LANES + threadIdx.x) * 4;
    l.n = min(4, cols - l.c0);
    l.r = blockIdx.y; l.f = blockIdx.z;
    return l;
}
template <class T>
__device__ __forceinline__ T* at(const PlaneDesc& d, const Lane& l)
{
    return const_cast<T*>(static_cast<const T*>(d.p)) + l.f * d.fstride + l.r * d.pitch + l.c0;
}
__device__ __forceinline__ unsigned char* at(const PackedDesc& d, const Lane& l)
{
    return const_cast<unsigned char*>(static_cast<const unsigned char*>(d.p)) + l.f * d.fstride + l.r * d.pitch + 3LL * l.c0;
}

}  // namespace

template <class T>
__global__ __launch_bounds__(CV_LANES) void k_rgb2gray(int cols, PlaneDesc rgb, PlaneDesc gray, float wr, float wg, float wb)
{
    const Lane l = lane_of(cols);
    if (l.n <= 0) return;
    const T* src = at<T>(rgb, l);
    const Px4 R = load4(src, rgb.aligned, l.n), G = load4(src + rgb.cstride, rgb.aligned, l.n), B = load4(src + 2 * rgb.cstride, rgb.aligned, l.n);
    store4(at<float>(gray, l), gray.aligned, l.n, gray_of(R, G, B, wr, wg, wb));
}

// interleaved bytes -> planar (T; rgb.p may be null) and grey (gray.p may be null), every source byte read once
template <class T>
__global__ __launch_bounds__(CV_LANES) void k_unpack_rgb8(int cols, PackedDesc pk, PlaneDesc rgb, PlaneDesc gray, float wr, float wg, float wb)
{
    const Lane l = lane_of(cols);
    if (l.n <= 0) return;
    const unsigned char* src = at(pk, l);
    Px4 R{{0.0f, 0.0f, 0.0f, 0.0f}}, G = R, B = R;
    if (pk.aligned && l.n == 4) {
        const P12 w = *reinterpret_cast<const P12*>(src);
        R.v[0] = (float)(w.a & 0xffu);         G.v[0] = (float)((w.a >> 8) & 0xffu);  B.v[0] = (float)((w.a >> 16) & 0xffu);
        R.v[1] = (float)(w.a >> 24);           G.v[1] = (float)(w.b & 0xffu);         B.v[1] = (float)((w.b >> 8) & 0xffu);
        R.v[2] = (float)((w.b >> 16) & 0xffu); G.v[2] = (float)(w.b >> 24);           B.v[2] = (float)(w.c & 0xffu);
        R.v[3] = (float)((w.c >> 8) & 0xffu);  G.v[3] = (float)((w.c >> 16) & 0xffu); B.v[3] = (float)(w.c >> 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < l.n) { R.v[i] = (float)src[3 * i]; G.v[i] = (float)src[3 * i + 1]; B.v[i] = (float)src[3 * i + 2]; }
    }
    if (rgb.p) {
        T* dst = at<T>(rgb, l);
        store4(dst, rgb.aligned, l.n, R);
        store4(dst + rgb.cstride, rgb.aligned, l.n, G);
        store4(dst + 2 * rgb.cstride, rgb.aligned, l.n, B);
    }
    if (gray.p) store4(at<float>(gray, l), gray.aligned, l.n, gray_of(R, G, B, wr, wg, wb));
}

// planar (T) -> interleaved bytes.  The packed rows are read next by the host or a copy engine: non-temporal stores
template <class T>
__global__ __launch_bounds__(CV_LANES) void k_pack_rgb8(int cols, PlaneDesc rgb, PackedDesc pk)
{
    const Lane l = lane_of(cols);
    if (l.n <= 0) return;
    const T* src = at<T>(rgb, l);
    const Px4 R = load4(src, rgb.aligned, l.n), G = load4(src + rgb.cstride, rgb.aligned, l.n), B = load4(src + 2 * rgb.cstride, rgb.aligned, l.n);
    unsigned int r[4], g[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = to_u8(R.v[i]); g[i] = to_u8(G.v[i]); b[i] = to_u8(B.v[i]); }
    unsigned char* dst = at(pk, l);
    if (pk.aligned && l.n == 4) {
        unsigned int* d = reinterpret_cast<unsigned int*>(dst);
        __builtin_nontemporal_store(r[0] | (g[0] << 8) | (b[0] << 16) | (r[1] << 24), d);
        __builtin_nontemporal_store(g[1] | (b[1] << 8) | (r[2] << 16) | (g[2] << 24), d + 1);
        __builtin_nontemporal_store(b[2] | (r[3] << 8) | (g[3] << 16) | (b[3] << 24), d + 2);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < l.n) { dst[3 * i] = (unsigned char)r[i]; dst[3 * i + 1] = (unsigned char)g[i]; dst[3 * i + 2] = (unsigned char)b[i]; }
}

static dim3 convert_grid(int rows, int cols, int frames) { return dim3((unsigned)(((cols + 3) / 4 + CV_LANES - 1) / CV_LANES), (unsigned)rows, (unsigned)frames); }

bool convert_grid_fits(int rows, int frames) { return rows >= 1 && rows <= 65535 && frames >= 1 && frames <= 65535; }

void launch_rgb2gray(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& rgb, const PlaneDesc& gray, const float* w)
{
    const dim3 grid = convert_grid(rows, cols, frames), block(CV_LANES);
    if (rgb.dtype == 0) WM_KLAUNCH(k_rgb2gray<float>, grid, block, 0, s, cols, rgb, gray, w[0], w[1], w[2]);
    else WM_KLAUNCH(k_rgb2gray<unsigned char>, grid, block, 0, s, cols, rgb, gray, w[0], w[1], w[2]);
}

void launch_unpack_rgb8(hipStream_t s, int rows, int cols, int frames, const PackedDesc& pk, const PlaneDesc& rgb, const PlaneDesc& gray, const float* w)
{
    const dim3 grid = convert_grid(rows, cols, frames), block(CV_LANES);
    if (rgb.dtype == 0) WM_KLAUNCH(k_unpack_rgb8<float>, grid, block, 0, s, cols, pk, rgb, gray, w[0], w[1], w[2]);
    else WM_KLAUNCH(k_unpack_rgb8<unsigned char>, grid, block, 0, s, cols, pk, rgb, gray, w[0], w[1], w[2]);
}

void launch_pack_rgb8(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& rgb, const PackedDesc& pk)
{
    const dim3 grid = convert_grid(rows, cols, frames), block(CV_LANES);
    if (rgb.dtype == 0) WM_KLAUNCH(k_pack_rgb8<float>, grid, block, 0, s, cols, rgb, pk);
    else WM_KLAUNCH(k_pack_rgb8<unsigned char>, grid, block, 0, s, cols, rgb, pk);
}

}  // namespace wmk
