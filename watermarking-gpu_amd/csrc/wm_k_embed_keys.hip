// wm_k_embed_keys.hip -- the embed of ONE image with every key of a bank (wm_embed_keys, wm.h): k_stats_keys, its fold
// k_embed_keys_fold, and k_embed_keys.
//
// Of makeWatermark (Watermark.cpp:156-172) only u_k = m W_k, ||u_k|| (and with it the strength a_k) and
// y_k = clamp(base + a_k u_k, 0, 255) depend on the key.  The image side -- the Gram sweep and solve (launch_gram), e and max|e|
// (ME) or the NVF mask -- is the same for every key.  k_stats_keys is k_me_stats' / k_nvf_stats' strip march (wm_k_embed.hip)
// with a compile-time group of EKG keys inside the row step: the mask of the row is formed once, then every key of the group
// takes its W row and runs its own sum of (m W_k)^2 in k_me_stats' per-lane order.  Its records are k_me_stats' (one per block,
// or one per wave under the quad mapping), one set per key; k_embed_keys_fold folds them per (frame, key) in
// embed_scalars_frame's (stats_fold's) order, so a_k is wm_embed's with key k as W bit for bit.  k_embed_keys is k_embed's march
// with the key-dependent half inside the row step: m and the base row are formed / read once, then every key of the group takes
// its W row and stores its copy of y.  That march (embed_group_march) and the kernel body around it (WM_EMBED_GROUP_BODY) live in
// wm_embed_march.hpp, shared with k_embed_signs_multi; the kernel here says where W, a and max|e| come from.  Key groups are a grid
// axis, as in k_detect_keys (keys_job): the groups of one tile are consecutive blocks of one XCD, so the re-reads of x and base are
// L2 hits.
#include "wm_embed_march.hpp"   // (WM_RING3, the ring length of the 3-row x windows on the aligned path; the group march, body and launch loop)

#ifndef WM_EMBED_KEYS_G
#define WM_EMBED_KEYS_G 4   // keys per group (registers vs. x / base re-reads)
#endif
#ifndef WM_PFW_EMBED_KEYS
#define WM_PFW_EMBED_KEYS 2  // W rows in flight per key (must divide UNROLL and WM_RING3)
#endif

namespace wmk {

constexpr int EKG = WM_EMBED_KEYS_G;
constexpr int EPFK = WM_PFW_EMBED_KEYS;

static_assert(UNROLL % EPFK == 0 && WM_RING3 % EPFK == 0, "the W prefetch ring must divide the march group");
constexpr int EKEYS_MAX_STRIPS = 256;  // strip records the quad-mode fold holds in LDS (a 32768-column image has 128 strips)

struct EKeysArgs {
    const float* W;      // the bank [nkeys][rows][cols]
    long long kstride;   // elements between key planes
    int nkeys;
    int ngroups;         // key groups = grid blocks per tile
    int rstride;         // records per (frame, key): >= the sweep's blocks (nblk_total) and wave records (nrec)
    float* pmax;         // [frames][rstride]         max|e| records (ME; written by key group 0)
    double* pss;         // [frames][nkeys][rstride]  sum (m W_k)^2 records
    EmbedScalars* scal;  // [frames][nkeys]           written by k_embed_keys_fold
};

// (the wave's job and key group: keys_job, wm_device.hpp)

// =================================================================================================
// k_stats_keys: me_stats_march / nvf_stats_march with the sum of (m W)^2 repeated for the keys of the group
// =================================================================================================
template <typename T, bool VEC, bool EDGE>
__device__ __forceinline__ void me_stats_keys_march(const T* __restrict__ xf, long long pitch, const float* const (&Wk)[EKG],
                                                    const Geom& g, const WaveJob& j, float* lds, const float (&c)[8], float& mx,
                                                    float (&ss)[EKG])
{
    constexpr int RG = VEC ? WM_RING3 : UNROLL;
    XMarch<T, 1, 1, 3, VEC, PFX, EDGE, false, RG> xm;
    PMarch<float, VEC, EPFK> wm_[EKG];
    const int nout = j.re - j.rs, n = nout + 2;
    xm.start(xf, pitch, g, j, lds, j.rs - 1, n);
#pragma unroll
    for (int q = 0; q < EKG; ++q) wm_[q].start(Wk[q], g.cols, g.cols, j, j.rs, nout);
    const int c0 = j.c0s + 4 * j.lane;
    const bool own = !EDGE || 4 * j.lane >= j.dup;  // duplicate lanes of a shifted last strip do not count
    march_n<2, RG>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            constexpr int SLOT = (Q + 4 * UNROLL - 2) % EPFK;
            const float* mid = xm.template row<Q>(1);
            float pr[4], ae[4];
            bool in[4];
            predict4<4>(xm.template row<Q>(0), mid, xm.template row<Q>(2), c, pr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                in[k] = VEC ? own : c0 + k < g.cols;
                ae[k] = fabsf(mid[4 + k] - pr[k]);
                if (in[k]) mx = fmaxf(mx, ae[k]);
            }
#pragma unroll
            for (int q = 0; q < EKG; ++q) {
                const float4 w = wm_[q].template take<SLOT>();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (in[k]) {
                        const float t = ae[k] * f4get(w, k);
                        ss[q] = fmaf(t, t, ss[q]);
                    }
                }
                wm_[q].template refill<SLOT>(i - 2);
            }
        }
    });
}

template <typename T, int PAD, bool VEC>
__device__ __forceinline__ void nvf_stats_keys_march(const T* __restrict__ xf, long long pitch, const float* const (&Wk)[EKG],
                                                     const Geom& g, const WaveJob& j, float* lds, float (&ss)[EKG])
{
    constexpr int NR = 2 * PAD + 1;
    XMarch<T, 1, PAD, NR, VEC, PFX> xm;
    PMarch<float, VEC, EPFK> wm_[EKG];
    const int nout = j.re - j.rs, n = nout + 2 * PAD;
    xm.start(xf, pitch, g, j, lds, j.rs - PAD, n);
#pragma unroll
    for (int q = 0; q < EKG; ++q) wm_[q].start(Wk[q], g.cols, g.cols, j, j.rs, nout);
    const int c0 = j.c0s + 4 * j.lane;
    march<2 * PAD>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            constexpr int SLOT = (Q + 2 * UNROLL - 2 * PAD) % EPFK;
            float m[4];
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                in[k] = VEC ? 4 * j.lane >= j.dup : c0 + k < g.cols;
                m[k] = nvf_value<PAD, 4, Q>(xm, k);
            }
#pragma unroll
            for (int q = 0; q < EKG; ++q) {
                const float4 w = wm_[q].template take<SLOT>();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (in[k]) {
                        const float t = m[k] * f4get(w, k);
                        ss[q] = fmaf(t, t, ss[q]);
                    }
                }
                wm_[q].template refill<SLOT>(i - 2 * PAD);
            }
        }
    });
}

template <typename T, int MASK, int PAD, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_stats_keys(const T* __restrict__ x, long long pitch, long long fstride, EKeysArgs ka,
                                                      Geom g, const float* __restrict__ coef, const int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<1>::N];
    __shared__ float s_mx[WPB];
    __shared__ double s_ss[WPB][EKG];
    int grp;
    const WaveJob j = keys_job(g, ka.ngroups, grp);
    const int frame = j.frame;
    const int k0 = grp * EKG;
    float mx = 0.0f, ss[EKG];
#pragma unroll
    for (int q = 0; q < EKG; ++q) ss[q] = 0.0f;
    if (j.valid && (MASK != 0 || status[frame] == 0)) {
        const T* xf = x + (long long)frame * fstride;
        // keys beyond the bank (a short last group) repeat its last key; their sums are not stored
        const float* Wk[EKG];
#pragma unroll
        for (int q = 0; q < EKG; ++q) Wk[q] = ka.W + (long long)min(k0 + q, ka.nkeys - 1) * ka.kstride;
        if constexpr (MASK == 0) {
            float c[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
            if (strip_on_edge<VEC>(g, j)) me_stats_keys_march<T, VEC, true>(xf, pitch, Wk, g, j, s_row[j.wave], c, mx, ss);
            else me_stats_keys_march<T, VEC, false>(xf, pitch, Wk, g, j, s_row[j.wave], c, mx, ss);
        } else {
            nvf_stats_keys_march<T, PAD, VEC>(xf, pitch, Wk, g, j, s_row[j.wave], ss);
        }
    }
    mx = wave_max(mx);
    double d[EKG];
#pragma unroll
    for (int q = 0; q < EKG; ++q) d[q] = wave_sum((double)ss[q]);
    if (g.quad) {
        // the waves of this block are 4 frames: one record per wave (k_me_stats' records, folded by k_embed_keys_fold)
        if (!j.valid || j.lane != 0) return;
        if (MASK == 0 && grp == 0) ka.pmax[(long long)frame * ka.rstride + j.rec] = mx;
#pragma unroll
        for (int q = 0; q < EKG; ++q)
            if (k0 + q < ka.nkeys) ka.pss[((long long)frame * ka.nkeys + k0 + q) * ka.rstride + j.rec] = d[q];
        return;
    }
    // the waves of this block are 4 segments of one frame: one record per block, k_me_stats' ((w0 + w1) + w2) + w3
    if (j.lane == 0) {
        s_mx[j.wave] = mx;
#pragma unroll
        for (int q = 0; q < EKG; ++q) s_ss[j.wave][q] = d[q];
    }
    __syncthreads();
    const int v = threadIdx.x;
    const long long blk = g.pb0 + j.tile;
    if (v < EKG) {
        if (k0 + v < ka.nkeys)
            ka.pss[((long long)frame * ka.nkeys + k0 + v) * ka.rstride + blk] = ((s_ss[0][v] + s_ss[1][v]) + s_ss[2][v]) + s_ss[3][v];
    } else if (v == EKG && MASK == 0 && grp == 0) {
        ka.pmax[(long long)frame * ka.rstride + blk] = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    }
}

// one block per (frame, key): the records folded in the order of k_me_stats' / k_nvf_stats' tails -- embed_scalars_frame's over
// the blocks, or (quad) stats_fold's over the segments of each strip, then over the strips -- into
//   a = sF / (float)(||u|| / sqrt(N))   (Watermark.cpp:170);  ME: ||u|| = sqrt(sum (|e| W)^2) / max|e|, NVF: sqrt(sum (m W)^2)
__global__ __launch_bounds__(BLOCK) void k_embed_keys_fold(EKeysArgs ka, int quad, int nblk, int nsegs, int nstrips, int me, float sF,
                                                           double sqrt_n, const int* __restrict__ status, OpResult* __restrict__ res)
{
    __shared__ float s_mx[BLOCK];
    __shared__ double s_ss[BLOCK];
    const int frame = blockIdx.x / ka.nkeys;
    const float* pm = ka.pmax + (long long)frame * ka.rstride;
    const double* ps = ka.pss + (long long)blockIdx.x * ka.rstride;
    const int t = threadIdx.x;
    float mx = 0.0f;
    double ss = 0.0;
    if (!quad) {
        for (int b0 = t; b0 < nblk; b0 += 4 * BLOCK) {
            float vm[4];
            double vs[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int b = min(b0 + u * BLOCK, nblk - 1);
                vm[u] = me ? pm[b] : 0.0f;
                vs[u] = ps[b];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = b0 + u * BLOCK < nblk;
                mx = fmaxf(mx, in ? vm[u] : 0.0f);
                ss += in ? vs[u] : 0.0;
            }
        }
        s_mx[t] = mx; s_ss[t] = ss;
        __syncthreads();
        for (int o = BLOCK / 2; o > 0; o >>= 1) {
            if (t < o) { s_mx[t] = fmaxf(s_mx[t], s_mx[t + o]); s_ss[t] += s_ss[t + o]; }
            __syncthreads();
        }
        mx = s_mx[0]; ss = s_ss[0];
    } else {
        // strip records in the first EKEYS_MAX_STRIPS entries of the block-mode arrays
        const int lane = t & (WAVE - 1), wave = t / WAVE;
        for (int st = wave; st < nstrips; st += WPB) {
            float m = 0.0f;
            double s = 0.0;
            for (int s0 = lane; s0 < nsegs; s0 += 4 * WAVE) {
                float vm[4];
                double vs[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int rec = min(s0 + u * WAVE, nsegs - 1) * nstrips + st;
                    vm[u] = me ? pm[rec] : 0.0f;
                    vs[u] = ps[rec];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool in = s0 + u * WAVE < nsegs;
                    m = fmaxf(m, in ? vm[u] : 0.0f);
                    s += in ? vs[u] : 0.0;
                }
            }
            m = wave_max(m);
            s = wave_sum(s);
            if (lane == 0) { s_mx[st] = m; s_ss[st] = s; }
        }
        __syncthreads();
        if (wave == 0) {
            for (int s0 = lane; s0 < nstrips; s0 += WAVE) { mx = fmaxf(mx, s_mx[s0]); ss += s_ss[s0]; }
            mx = wave_max(mx);
            ss = wave_sum(ss);
        }
    }
    if (t == 0) {
        EmbedScalars s;
        s.maxe = me ? mx : 1.0f;
        const double nrm = me ? sqrt(ss) / (double)s.maxe : sqrt(ss);
        s.a = sF / (float)(nrm / sqrt_n);
        ka.scal[blockIdx.x] = s;
        OpResult o;
        o.status = me ? status[frame] : 0;
        o.value = s.a;
        res[blockIdx.x] = o;
    }
}

// =================================================================================================
// k_embed_keys: the group march (embed_group_march, wm_embed_march.hpp) with a W stream and a strength per key, on ONE channel of the
// base (a planar-RGB base is three launches, one per channel: y of a channel depends on that channel's base only)
// =================================================================================================
template <typename T, int MASK, int PAD, bool VEC, bool BX>
__global__ __launch_bounds__(BLOCK) void k_embed_keys(const T* __restrict__ x, long long pitch, long long fstride, EKeysArgs ka,
                                                      PlaneDesc base, PlaneDesc out, Geom g, const float* __restrict__ coef,
                                                      const int* __restrict__ status)
{
    WM_EMBED_GROUP_BODY(EKG, ka.ngroups, ka.nkeys);
    const float* Wk[EKG];
    float a[EKG];
#pragma unroll
    for (int q = 0; q < EKG; ++q) {
        Wk[q] = ka.W + (long long)kq[q] * ka.kstride;
        a[q] = applied_strength(ka.scal[(long long)frame * ka.nkeys + kq[q]].a);  // (per key: a zero key leaves its copy = base)
    }
    const float maxe = ka.scal[(long long)frame * ka.nkeys + k0].maxe;  // (the same for every key of the frame)
    const T* xf = x + (long long)frame * fstride;
    WM_EMBED_GROUP_MARCH(EKG, EPFK, false, Wk, a, maxe, nullptr, nullptr, nullptr);  // (no sign tables)
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static EKeysArgs ekeys_args(const float* Wbank, long long kstride, int nkeys, int frames, void* scratch, int rstride)
{
    EKeysArgs ka;
    ka.W = Wbank; ka.kstride = kstride; ka.nkeys = nkeys; ka.ngroups = group_count(nkeys, EKG); ka.rstride = rstride;
    char* p = static_cast<char*>(scratch);
    ka.pss = reinterpret_cast<double*>(p);
    p += (size_t)frames * nkeys * rstride * sizeof(double);
    ka.scal = reinterpret_cast<EmbedScalars*>(p);
    p += (size_t)frames * nkeys * sizeof(EmbedScalars);
    ka.pmax = reinterpret_cast<float*>(p);
    return ka;
}
size_t embed_keys_scratch_bytes(int frames, int nkeys, int rstride)
{
    return (size_t)frames * nkeys * rstride * sizeof(double) + (size_t)frames * nkeys * sizeof(EmbedScalars) + (size_t)frames * rstride * sizeof(float);
}

template <typename T>
static void launch_stats_keys_t(const Sweep& sw, int al, const EKeysArgs& ka)
{
    const PlaneDesc& x = sw.x;
    // every grid times the key groups
    for_mask_pad(sw.mask, sw.pad, [&](auto m, auto p) {
        for_each_sweep_part(sw, al, 1, [&](auto vec, const SweepPart& sp) {
            WM_KLAUNCH((k_stats_keys<T, decltype(m)::value, decltype(p)::value, decltype(vec)::value>), dim3(sp.grid.x * (unsigned)ka.ngroups),
                       dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, ka, sp.g, sw.coef, sw.status);
        });
    });
}

int launch_stats_keys(const Sweep& sw, const KeyBank& bank, void* scratch, int rstride)
{
    const LaunchGeom& lg = sw.lg;
    // k_me_stats' / k_nvf_stats' geometry and record layout (launch_me_stats): the fold's order depends on it
    if (lg.nblk > rstride || lg.nstrips * lg.nsegs > rstride || lg.nstrips > EKEYS_MAX_STRIPS) return -1;
    const EKeysArgs ka = ekeys_args(bank.W, bank.kstride, bank.nkeys, sw.frames, scratch, rstride);
    const int al = align_mode(lg, sw.x.aligned && bank.aligned_w);
    WM_DISPATCH_T(sw.x.dtype, launch_stats_keys_t<T>(sw, al, ka));
    return 0;
}

void launch_embed_keys_fold(const Sweep& sw, int nkeys, void* scratch, int rstride, float sF, double sqrt_n, OpResult* res)
{
    const LaunchGeom& lg = sw.lg;
    const EKeysArgs ka = ekeys_args(nullptr, 0, nkeys, sw.frames, scratch, rstride);
    const int quad = sw.frames >= 4 ? 1 : 0;  // (sweep_part's quad mapping of the stats sweep)
    WM_KLAUNCH(k_embed_keys_fold, dim3((unsigned)(sw.frames * nkeys)), dim3(BLOCK), 0, sw.s, ka, quad, lg.nblk, lg.nsegs, lg.nstrips,
               sw.mask == 0 ? 1 : 0, sF, sqrt_n, sw.mask == 0 ? sw.status : nullptr, res);
}

void launch_embed_keys(const Sweep& sw, const KeyBank& bank, const EmbedPlanes& ep, void* scratch, int rstride)
{
    const PlaneDesc& x = sw.x;
    const EKeysArgs ka = ekeys_args(bank.W, bank.kstride, bank.nkeys, sw.frames, scratch, rstride);
    WM_DISPATCH_T(x.dtype, for_each_embed_group_launch<T>(sw, bank.aligned_w, ep, ka.ngroups, [&](auto m, auto p, auto vec, auto base_is_x, dim3 grid, const Geom& g,
                                                                                                 const PlaneDesc& bc, const PlaneDesc& oc) {
        WM_KLAUNCH((k_embed_keys<T, decltype(m)::value, decltype(p)::value, decltype(vec)::value, decltype(base_is_x)::value>), grid, dim3(BLOCK), 0,
                   sw.s, (const T*)x.p, x.pitch, x.fstride, ka, bc, oc, g, sw.coef, sw.status);
    }));
}

int embed_keys_group(void) { return EKG; }

}  // namespace wmk
