// wm_k_detect_keys_tiles.hip -- the detector's sums kept per tile of the frame AND per key of a bank (wm_detect_keys_tiles):
// k_detect_keys_tiles + k_keys_tiles_fold
//
// wm_detect_keys shares the image side of the detector (c, e_w, m, ||e_w||^2) between the keys of a bank; wm_detect_tiles keeps
// the positions of the three sums.  k_detect_keys_tiles is k_detect_keys' march (group_march with the lines around it,
// wm_keys_march.hpp: the same instances, key groups, block order and fmaf order) on wm_detect_tiles' geometry (tiles_plan:
// segments whose height divides tile_rows) with k_detect_tiles' end: no wave reduction, no LDS fold, no block barrier -- every
// lane stores its 2 KG + 1 f32 partials into
//     rec [frame][group][segment][strip][2 KG + 1][64 lanes]     {dot_q, nu_q} per key q of the group, then nw
// with plain vector stores (a lane that owns no pixels stores zeros).  k_keys_tiles_fold then adds the records of each
// (frame, key, tile) in k_tiles_fold's fixed index order in f64: key k's map and sums are wm_detect_tiles' with key k as W, bit
// for bit (tests/test_gpu_keys_tiles.py).
#include "wm_keys_march.hpp"
#include <algorithm>

namespace wmk {

constexpr int KT_NV = 2 * KG + 1;  // f32 partials per lane: dot, nu per key of the group, then nw

// the same occupancy floors as k_detect_keys' instances (wm_k_detect_keys.hip)
template <typename T, int MASK, int PAD, int HC, bool VEC>
__global__ __launch_bounds__(BLOCK, (PAD == 1 && HC == 1 ? (VEC ? (sizeof(T) == 1 ? 4 : 3) : 2) : 1)) void k_detect_keys_tiles(
    const T* __restrict__ x, long long pitch, long long fstride, const float* __restrict__ Wbank, long long kstride, int nkeys,
    int ngroups, Geom g, const float* __restrict__ coef, const int* __restrict__ status, float* __restrict__ rec)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * KG * RowBuf<1>::N];
    int grp;
    const WaveJob j = keys_job(g, ngroups, grp);
    // wave-uniform exits (the kernel has no block barrier): a surplus wave, or a frame the fold answers from its status alone
    if (!j.valid || status[j.frame] != 0) return;
    const int frame = j.frame;
    const int k0 = grp * KG;
    float dot[KG], nu[KG], nw = 0.0f;
#pragma unroll
    for (int q = 0; q < KG; ++q) { dot[q] = 0.0f; nu[q] = 0.0f; }
    WM_GROUP_DETECT_FRAME;
    // keys beyond the bank (a short last group) repeat its last key; the fold never reads their slots
    const float* Wk[KG];
#pragma unroll
    for (int q = 0; q < KG; ++q) Wk[q] = Wbank + (long long)min(k0 + q, nkeys - 1) * kstride;
    WM_GROUP_DETECT_MARCH(KG, false, PFK, Wk, g.cols);
    // every lane of the wave stores (the lanes that own nothing hold zeros: group_march masks them)
    float* p = rec + ((((long long)frame * ngroups + grp) * g.nrec + j.rec) * KT_NV) * WAVE + j.lane;
#pragma unroll
    for (int q = 0; q < KG; ++q) { p[(2 * q) * WAVE] = dot[q]; p[(2 * q + 1) * WAVE] = nu[q]; }
    p[2 * KG * WAVE] = nw;
}

// k_tiles_fold per (frame, key, tile): TPT threads add the tile's records in the same index order in f64 -- for key k the slots
// 2 (k % KG), 2 (k % KG) + 1 and 2 KG of group k / KG --, the wave its lanes in wave_sum's fixed order and (TPT = 256) thread 0
// the four waves in order.  map / sums [frames][nkeys][ny][nx]; the frame's status record is written once, by (key 0, tile 0)
template <int TPT>
__global__ __launch_bounds__(BLOCK) void k_keys_tiles_fold(const float* __restrict__ rec, TileGeom tg, int frames, int nkeys, int ngroups,
                                                           const int* __restrict__ status, float* __restrict__ map, double* __restrict__ sums,
                                                           OpResult* __restrict__ res)
{
    __shared__ double s_w[WPB][3];
    const int ntiles = tg.ny * tg.nx;
    const long long per_frame = (long long)nkeys * ntiles;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / TPT);
    const int lt = (int)threadIdx.x - sub * TPT;
    const long long id = (long long)blockIdx.x * (BLOCK / TPT) + sub;
    if (id >= (long long)frames * per_frame) return;  // (TPT = 64: wave-uniform; TPT = 256: never)
    const int frame = (int)(id / per_frame);
    const long long kt = id - (long long)frame * per_frame;
    const int key = (int)(kt / ntiles);
    const int t = (int)(kt - (long long)key * ntiles);
    const int ty = t / tg.nx, tx = t - ty * tg.nx;
    const int st = status[frame];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (st == 0) {
        const int seg0 = ty * tg.th / tg.rps, seg1 = ty == tg.ny - 1 ? tg.nsegs : (ty + 1) * tg.th / tg.rps;
        const int g0 = tx * tg.tw / 4, g1 = tx == tg.nx - 1 ? tg.ngroups : (tx + 1) * tg.tw / 4;
        const int ng = g1 - g0, n = (seg1 - seg0) * ng;
        const int grp = key / KG, q = key - grp * KG;
        const float* rf = rec + (((long long)frame * ngroups + grp) * tg.nsegs * tg.nstrips) * (KT_NV * WAVE);
        for (int i = lt; i < n; i += TPT) {
            const int sg = i / ng;
            int strip, lane;
            tile_owner(tg, g0 + (i - sg * ng), strip, lane);
            const float* p = rf + ((long long)(seg0 + sg) * tg.nstrips + strip) * (KT_NV * WAVE) + lane;
            a0 += (double)p[(2 * q) * WAVE]; a1 += (double)p[(2 * q + 1) * WAVE]; a2 += (double)p[2 * KG * WAVE];
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
        if constexpr (TPT == BLOCK) {
            const int w = (int)threadIdx.x >> 6;
            if ((threadIdx.x & (WAVE - 1)) == 0) { s_w[w][0] = a0; s_w[w][1] = a1; s_w[w][2] = a2; }
            __syncthreads();
            a0 = ((s_w[0][0] + s_w[1][0]) + s_w[2][0]) + s_w[3][0];
            a1 = ((s_w[0][1] + s_w[1][1]) + s_w[2][1]) + s_w[3][1];
            a2 = ((s_w[0][2] + s_w[1][2]) + s_w[2][2]) + s_w[3][2];
        }
    }
    if (lt != 0) return;
    map[id] = st == 0 ? (float)a0 / (float)(sqrt(a2) * sqrt(a1)) : 0.0f;
    if (sums) { double* o = sums + id * 3; o[0] = a0; o[1] = a1; o[2] = a2; }
    if (kt == 0) { OpResult r; r.status = st; r.value = 0.0f; res[frame] = r; }
}

size_t keys_tiles_rec_bytes(const TilesPlan& pl, int frames, int nkeys)
{
    const size_t ngroups = (size_t)group_count(nkeys, KG);
    return (size_t)frames * ngroups * pl.ld.nsegs * pl.ld.nstrips * KT_NV * WAVE * sizeof(float);
}

// do both grids of a call fit 31 bits?  Answered from the shapes alone (the caller asks before any device work), so with upper
// bounds of what tiles_plan may choose: a block per (frame, key, tile) in the fold; in the sweep the overlapped strips and one
// generic strip, a block per segment and frame
bool keys_tiles_grids_fit(int rows, int cols, int tile_rows, int frames, int nkeys, int ny, int nx)
{
    const long long lim = 0x7fffffffLL;
    const long long ngroups = group_count(nkeys, KG);
    const int rps = std::min(tiles_segment_rows(tile_rows), rows);
    const long long nsegs = (rows + rps - 1) / rps;
    const long long nstrips = std::max((cols + STRIP - 1) / STRIP, overlap_strips(cols) + 1);
    return (long long)frames * nkeys * ny * nx <= lim && nstrips * nsegs * frames * ngroups <= lim;
}

template <typename T>
static void launch_detect_keys_tiles_t(const Sweep& sw, const TilesPlan& pl, const KeyBank& bank, float* rec)
{
    const PlaneDesc& x = sw.x;
    const int ngroups = group_count(bank.nkeys, KG);
    // every grid times the key groups
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_detect_keys_tiles<T, decltype(m)::value, decltype(p)::value, decltype(hc)::value, decltype(vec)::value>),
                   dim3(sp.grid.x * (unsigned)ngroups), dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, bank.W, bank.kstride, bank.nkeys,
                   ngroups, sp.g, sw.coef, sw.status, rec);
    });
}

void launch_detect_keys_tiles(const Sweep& sw, const TilesPlan& pl, const KeyBank& bank, float* rec)
{
    WM_DISPATCH_T(sw.x.dtype, launch_detect_keys_tiles_t<T>(sw, pl, bank, rec));
}

void launch_keys_tiles_fold(hipStream_t s, const TilesPlan& pl, int frames, int nkeys, const float* rec, const int* status, float* map,
                            double* sums, OpResult* res)
{
    const int ngroups = group_count(nkeys, KG);
    const long long n = (long long)frames * nkeys * pl.tg.ny * pl.tg.nx;
    if (pl.fold_threads == BLOCK) WM_KLAUNCH(k_keys_tiles_fold<BLOCK>, dim3((unsigned)n), dim3(BLOCK), 0, s, rec, pl.tg, frames, nkeys, ngroups, status, map, sums, res);
    else WM_KLAUNCH(k_keys_tiles_fold<WAVE>, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(BLOCK), 0, s, rec, pl.tg, frames, nkeys, ngroups, status, map, sums, res);
}

}  // namespace wmk
