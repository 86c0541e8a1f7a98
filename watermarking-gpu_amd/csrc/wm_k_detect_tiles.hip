// wm_k_detect_tiles.hip -- the detector's sums kept per tile of the frame (wm_detect_tiles): k_detect_tiles + k_tiles_fold
//
// The detector is local once the coefficients are solved: e_w, u = m W and e_u are 3x3 stencils, and k_detect sums <e_u,e_w>,
// ||e_u||^2 and ||e_w||^2 per lane over a segment of rows before its fold throws the positions away.  k_detect_tiles is
// k_detect's march (detect_march, wm_detect_march.hpp: the same instances, chains and fmaf order) with another end: instead of
// the wave reduction and the ticket fold, every lane stores its three f32 partials into a record array
//     rec [frame][segment][strip][3][64 lanes]          (plain vector stores; a lane that owns no pixels stores zeros)
// The segment height divides tile_rows and tile_cols is a multiple of 4, so a lane's record lies inside ONE tile.  k_tiles_fold
// then adds the records of each tile in a fixed index order in f64 and forms the tile's score: no atomics, no arrival order.
#include "wm_detect_march.hpp"
#include <algorithm>

namespace wmk {

// the same occupancy floors as k_detect's instances (WM_DET_BOUNDS, wm_detect_march.hpp)
template <typename T, int MASK, int PAD, int HC, bool VEC>
__global__ __launch_bounds__(BLOCK, WM_DET_BOUNDS) void k_detect_tiles(const T* __restrict__ x, long long pitch, long long fstride,
                                                                       const float* __restrict__ W, Geom g,
                                                                       const float* __restrict__ coef, const int* __restrict__ status,
                                                                       float* __restrict__ rec)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * RowBuf<1>::N];
    const WaveJob j = make_job(g);
    // wave-uniform exits (the kernel has no block barrier): a surplus wave, or a frame the fold answers from its status alone
    if (!j.valid || status[j.frame] != 0) return;
    const int frame = j.frame;
    float dot = 0.0f, nu = 0.0f, nw = 0.0f;
    unsigned long long dig = 0;
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
    const T* xf = x + (long long)frame * fstride;
    constexpr bool V = VEC && HC == 1;  // (as in detect_body: the halo of p = 9 exceeds one neighbour chunk)
    if (MASK != 0 || strip_on_edge<V>(g, j)) detect_march<T, MASK, PAD, HC, V, true>(xf, pitch, W, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw, dig);
    else detect_march<T, MASK, PAD, HC, V, (MASK != 0)>(xf, pitch, W, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw, dig);
    // every lane of the wave stores (the lanes that own nothing hold zeros: detect_march masks them)
    float* p = rec + ((long long)frame * g.nrec + j.rec) * (3 * WAVE) + j.lane;
    p[0] = dot; p[WAVE] = nu; p[2 * WAVE] = nw;
}
#undef WM_DET_BOUNDS

// TPT threads per (frame, tile): thread t adds the tile's records t, t + TPT, ... (record i = segment i / ng, group i % ng of
// the tile) in f64, the wave adds its lanes in wave_sum's fixed order, and (TPT = 256) thread 0 the four waves in order.
//   corr = (float)dot / (float)(sqrt(nw) * sqrt(nu))   (Watermark.cpp:230) per tile; unsolvable => 0.0f and zero sums
template <int TPT>
__global__ __launch_bounds__(BLOCK) void k_tiles_fold(const float* __restrict__ rec, TileGeom tg, int frames, const int* __restrict__ status,
                                                      float* __restrict__ map, double* __restrict__ sums, OpResult* __restrict__ res)
{
    __shared__ double s_w[WPB][3];
    const int ntiles = tg.ny * tg.nx;
    const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / TPT);
    const int lt = (int)threadIdx.x - sub * TPT;
    const long long id = (long long)blockIdx.x * (BLOCK / TPT) + sub;
    if (id >= (long long)frames * ntiles) return;  // (TPT = 64: wave-uniform; TPT = 256: never)
    const int frame = (int)(id / ntiles);
    const int t = (int)(id - (long long)frame * ntiles);
    const int ty = t / tg.nx, tx = t - ty * tg.nx;
    const int st = status[frame];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (st == 0) {
        const int seg0 = ty * tg.th / tg.rps, seg1 = ty == tg.ny - 1 ? tg.nsegs : (ty + 1) * tg.th / tg.rps;
        const int g0 = tx * tg.tw / 4, g1 = tx == tg.nx - 1 ? tg.ngroups : (tx + 1) * tg.tw / 4;
        const int ng = g1 - g0, n = (seg1 - seg0) * ng;
        const float* rf = rec + (long long)frame * tg.nsegs * tg.nstrips * (3 * WAVE);
        for (int i = lt; i < n; i += TPT) {
            const int sg = i / ng;
            int strip, lane;
            tile_owner(tg, g0 + (i - sg * ng), strip, lane);
            const float* p = rf + ((long long)(seg0 + sg) * tg.nstrips + strip) * (3 * WAVE) + lane;
            a0 += (double)p[0]; a1 += (double)p[WAVE]; a2 += (double)p[2 * WAVE];
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
    if (sums) { double* q = sums + id * 3; q[0] = a0; q[1] = a1; q[2] = a2; }
    if (t == 0) { OpResult r; r.status = st; r.value = 0.0f; res[frame] = r; }
}

int tiles_segment_rows(int tile_rows)
{
    for (int d = 48; d >= 8; --d)
        if (tile_rows % d == 0) return d;
    return 0;
}

// the sweep's geometry: segments of tiles_segment_rows(tile_rows) rows -- from the tile shape alone, so that a frame's records
// (and bits) do not depend on the batch it arrives in --, strips as detect_plan chooses them
TilesPlan tiles_plan(const Sweep& sw, int aligned_w, const TileShape& ts)
{
    TilesPlan pl;
    Sweep st = sw;
    LaunchGeom& lt = st.lg;
    lt.rps = std::min(tiles_segment_rows(ts.th), lt.row_hi - lt.row_lo);
    lt.nsegs = (lt.row_hi - lt.row_lo + lt.rps - 1) / lt.rps;
    lt.nblk = lt.nstrips * ((lt.nsegs + WPB - 1) / WPB);
    const DetectPlan dp = detect_plan(st, aligned_w);
    pl.ld = dp.ld; pl.overlap = dp.overlap; pl.split = dp.split;
    const LaunchGeom& ld = pl.ld;
    TileGeom& tg = pl.tg;
    tg.th = ts.th; tg.tw = ts.tw; tg.ny = ts.ny; tg.nx = ts.nx;
    tg.rps = ld.rps; tg.nsegs = ld.nsegs; tg.nstrips = ld.nstrips;
    tg.layout = pl.overlap ? 1 : (pl.split ? 2 : 0);
    tg.nown = pl.overlap ? ld.cols / 4 : (pl.split ? split_own_cols(ld.cols) / 4 : 0);
    tg.ngroups = pl.overlap ? tg.nown : (pl.split ? tg.nown + WAVE : (ld.cols + 3) / 4);
    pl.rec_bytes = (size_t)sw.frames * ld.nsegs * ld.nstrips * 3 * WAVE * sizeof(float);
    // threads per tile from the geometry alone: a wave for tiles of a few hundred records, a block for larger ones (the last
    // tile of each axis takes the remainder; one tile may be the whole plane)
    const long long worst = (long long)(ld.nsegs - (ts.ny - 1) * (ts.th / ld.rps)) * (tg.ngroups - (ts.nx - 1) * (ts.tw / 4));
    pl.fold_threads = worst > 512 ? BLOCK : WAVE;
    return pl;
}

template <typename T>
static void launch_detect_tiles_t(const Sweep& sw, const TilesPlan& pl, const float* W, float* rec)
{
    const PlaneDesc& x = sw.x;
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        WM_KLAUNCH((k_detect_tiles<T, decltype(m)::value, decltype(p)::value, decltype(hc)::value, decltype(vec)::value>), sp.grid,
                   dim3(BLOCK), 0, sw.s, (const T*)x.p, x.pitch, x.fstride, W, sp.g, sw.coef, sw.status, rec);
    });
}

void launch_detect_tiles(const Sweep& sw, const TilesPlan& pl, const KeyBank& w, float* rec)
{
    WM_DISPATCH_T(sw.x.dtype, launch_detect_tiles_t<T>(sw, pl, w.W, rec));
}

void launch_tiles_fold(hipStream_t s, const TilesPlan& pl, int frames, const float* rec, const int* status, float* map, double* sums,
                       OpResult* res)
{
    const long long n = (long long)frames * pl.tg.ny * pl.tg.nx;
    if (pl.fold_threads == BLOCK) WM_KLAUNCH(k_tiles_fold<BLOCK>, dim3((unsigned)n), dim3(BLOCK), 0, s, rec, pl.tg, frames, status, map, sums, res);
    else WM_KLAUNCH(k_tiles_fold<WAVE>, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(BLOCK), 0, s, rec, pl.tg, frames, status, map, sums, res);
}

}  // namespace wmk
