// wm_k_convert16.hip -- samples of 9 to 16 bits (wm_unpack16, wm_pack16; wm.h): element-wise, memory-bound.
//
// wm_k_convert.hip's lane mapping: one lane handles four consecutive pixels of one row, a block is 256 lanes (1024 pixels of a
// row), the grid is (column chunks, rows, frames x channels).  A lane's four f32 values move as one 16-byte access (vec_ok's rule:
// a 4-byte aligned base), its four u16 samples as one 8-byte access when the plane's base is a multiple of 4 bytes and its pitch
// and used strides are even (PlaneDesc::aligned, decided on the host per plane and uniform over the launch).  A lane whose four
// pixels reach past the right edge, and every lane of a plane that does not qualify, takes the per-pixel form of the same access.
// Row addresses are 64-bit.  No LDS, no atomics, nothing shared between lanes.
//
// Arithmetic (the library is built with -ffp-contract=off; each is ONE f32 multiply):
//   unpack: g = (float)min(v >> shift, maxv) * k_in          shift = 16 - bits for msb-aligned samples, else 0
//   pack:   v = (unsigned)rint(fmin(fmax(g * k_out, 0), maxv)) << shift      rint: ties to even (v_rndne_f32); NaN gives 0
#include "wm_kernels.hpp"

namespace wmk {
namespace {

constexpr int CV_LANES = 256;  // lanes per block; 4 pixels each

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));         // 16 bytes at a 4-byte aligned address
typedef unsigned int u2u __attribute__((ext_vector_type(2), aligned(4)));  // four u16 samples: 8 bytes at a 4-byte aligned address

// the lane's place: first column c0, pixels n (<= 0: the lane is outside the row); the element offset of its first pixel in a plane
struct Lane { int c0, n; long long r, f, ch; };
__device__ __forceinline__ Lane lane_of(int cols, int channels)
{
    Lane l;
    l.c0 = (blockIdx.x * CV_LANES + threadIdx.x) * 4;
    l.n = min(4, cols - l.c0);
    l.r = blockIdx.y; l.f = blockIdx.z / (unsigned)channels; l.ch = blockIdx.z % (unsigned)channels;
    return l;
}
template <class T>
__device__ __forceinline__ T* at(const PlaneDesc& d, const Lane& l)
{
    return const_cast<T*>(static_cast<const T*>(d.p)) + l.f * d.fstride + l.ch * d.cstride + l.r * d.pitch + l.c0;
}

}  // namespace

__global__ __launch_bounds__(CV_LANES) void k_unpack16(int cols, PlaneDesc src, PlaneDesc out, int shift, unsigned int maxv, float k_in)
{
    const Lane l = lane_of(cols, src.channels);
    if (l.n <= 0) return;
    const unsigned short* sp = at<unsigned short>(src, l);
    unsigned int v[4] = {0u, 0u, 0u, 0u};
    if (src.aligned && l.n == 4) {
        const u2u w = *reinterpret_cast<const u2u*>(sp);
        v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < l.n) v[i] = sp[i];
    }
    float g[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = (float)min(v[i] >> shift, maxv) * k_in;
    // (the Gram sweep reads this plane at once: ordinary stores)
    float* dp = at<float>(out, l);
    if (out.aligned && l.n == 4) {
        f4u t; t.x = g[0]; t.y = g[1]; t.z = g[2]; t.w = g[3];
        *reinterpret_cast<f4u*>(dp) = t;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < l.n) dp[i] = g[i];
}

// The samples are read next by the host, a copy engine or an encoder: non-temporal stores
__global__ __launch_bounds__(CV_LANES) void k_pack16(int cols, PlaneDesc src, PlaneDesc out, int shift, float maxv, float k_out)
{
    const Lane l = lane_of(cols, src.channels);
    if (l.n <= 0) return;
    const float* sp = at<float>(src, l);
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (src.aligned && l.n == 4) {
        const f4u t = *reinterpret_cast<const f4u*>(sp);
        g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < l.n) g[i] = sp[i];
    }
    unsigned int q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float t = __builtin_fminf(__builtin_fmaxf(g[i] * k_out, 0.0f), maxv);  // (fmax(NaN, 0) is 0)
        q[i] = (unsigned int)__builtin_rintf(t) << shift;
    }
    unsigned short* dp = at<unsigned short>(out, l);
    if (out.aligned && l.n == 4) {
        u2u w; w.x = q[0] | (q[1] << 16); w.y = q[2] | (q[3] << 16);
        __builtin_nontemporal_store(w, reinterpret_cast<u2u*>(dp));
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < l.n) __builtin_nontemporal_store((unsigned short)q[i], dp + i);
}

static dim3 convert16_grid(int rows, int cols, int planes) { return dim3((unsigned)(((cols + 3) / 4 + CV_LANES - 1) / CV_LANES), (unsigned)rows, (unsigned)planes); }

// planes = frames x channels; shift / maxv from bits and msb_aligned (wm.h)
void launch_unpack16(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& src, const PlaneDesc& out, int bits, int msb_aligned, float k_in)
{
    WM_KLAUNCH(k_unpack16, convert16_grid(rows, cols, frames * src.channels), dim3(CV_LANES), 0, s, cols, src, out, msb_aligned ? 16 - bits : 0, (1u << bits) - 1u, k_in);
}

void launch_pack16(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& src, const PlaneDesc& out, int bits, int msb_aligned, float k_out)
{
    WM_KLAUNCH(k_pack16, convert16_grid(rows, cols, frames * src.channels), dim3(CV_LANES), 0, s, cols, src, out, msb_aligned ? 16 - bits : 0, (float)((1u << bits) - 1u), k_out);
}

}  // namespace wmk
