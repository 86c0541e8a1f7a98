// wm_k_quality.hip -- PSNR and SSIM of a marked copy against its base (wm_quality): k_quality, k_quality_fold_cols, k_quality_fold, k_quality_total
//
// A measuring instrument: every difference, square, product and sum is f64.  Per (frame, channel) plane pair and per tile of
// wm_tiles_shape's grid the call leaves {sse, npix, ssim_sum, nwin, max|d|} (wm.h).  SSIM is Wang et al.'s 11 x 11 Gaussian window,
// evaluated separably and only where the window lies wholly inside the plane.
//
// k_quality: one wavefront per block; a block owns a strip of 64 columns x a segment of rps rows (rps divides tile_rows, so a segment
// lies in one tile row), a lane owns ONE column of the strip and marches down it.  Per row of the march (the segment's rows and 5
// halo rows on either side, rows outside the plane read as zero and only feed windows that are not counted):
//   - the wave keeps the row's 74 samples (64 + 5 halo columns a side) of both planes in LDS, converted to f64 once (samples are f32
//     or u8: exact), double-buffered, the next row's global loads in flight while this row is worked on;
//   - the lane forms the five horizontally filtered values of its column, sum g x, g y, g x^2, g y^2, g x y over 11 taps, using the
//     Gaussian's symmetry (taps k and 10 - k share a weight), and puts them into a ring of 11 rows held in REGISTERS (55 doubles;
//     the march is unrolled by 11, so every ring index is a compile-time constant);
//   - the vertical filter over the ring, again with the symmetry, gives the window centred 5 rows up; the SSIM expression follows;
//   - the lane's own pixel of the row adds d^2 and max|d|.
// Arithmetic per pixel: ~75 f64 operations for the row filter (11 taps x {3 products, 5 weighted sums}, halved where the symmetry
// allows), ~55 for the column filter, ~25 for the expression with its division.  No LDS traffic beyond 22 f64 reads per pixel-row.
// At the end the four lanes of a column group of 4 are added in lane order and the group's record {sse, ssim_sum, max|d|} is stored:
//     rec [plane][segment][group][3] f64, group = column / 4             (a tile's width is a multiple of 4: a group lies in one tile)
// k_quality_fold_cols + k_quality_fold: a tile's records are added in two levels, each a wavefront whose lane l takes entries l,
// l + 64, ... in index order followed by a fixed tree over the lanes -- first the groups of one tile column within one segment, then
// the tile's segments -- and the tile's five values are written; npix and nwin follow from the tile's bounds.
// k_quality_total: one wavefront per plane adds the tiles' values in ascending tile index, one after the other, and writes the
// three result records {mse, ssim, max|d|}.  No atomics anywhere; nothing depends on arrival order, the batch or repetition.
// Samples are fetched one element per lane (any base address, pitch, stride; the kernel is arithmetic-bound).
#include "wm_kernels.hpp"

namespace wmk {
namespace {

constexpr int QW = 64;              // lanes of the block = columns of a strip
constexpr int QR = 5;               // window radius
constexpr int QN = 2 * QR + 1;      // taps
constexpr int QROW = QW + 2 * QR;   // samples of a buffered row
constexpr double QC1 = (0.01 * 255.0) * (0.01 * 255.0);
constexpr double QC2 = (0.03 * 255.0) * (0.03 * 255.0);

__device__ __forceinline__ float q_ld(const float* p) { return *p; }
__device__ __forceinline__ float q_ld(const unsigned char* p) { return (float)*p; }

__device__ __forceinline__ double q_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

}  // namespace

template <class TX, class TY>
__global__ __launch_bounds__(QW) void k_quality(PlaneDesc x, PlaneDesc y, QualityGeom q, QualityWeights w, double* __restrict__ rec)
{
    __shared__ double s_x[2][QROW + 6];
    __shared__ double s_y[2][QROW + 6];
    __shared__ double s_red[3][QW];
    const int lane = (int)threadIdx.x;
    const int strip = (int)blockIdx.x, seg = (int)blockIdx.y, z = (int)blockIdx.z;
    const int f = z / q.channels, ch = z - f * q.channels;
    const TX* xp = static_cast<const TX*>(x.p) + (long long)f * x.fstride + (long long)ch * x.cstride;
    const TY* yp = static_cast<const TY*>(y.p) + (long long)f * y.fstride + (long long)ch * y.cstride;
    const int c0 = strip * QW, c = c0 + lane;
    const int r0 = seg * q.rps, r1 = min(r0 + q.rps, q.rows);
    const int niter = r1 - r0 + 2 * QR;
    // the two samples of a buffered row this lane fetches: columns c0 - 5 + lane and (lanes 0..9) c0 + 59 + lane
    const int ca = c - QR, cb = c - QR + QW;
    const bool a_in = ca >= 0 && ca < q.cols, b_in = lane < 2 * QR && cb < q.cols;
    const bool col_own = c < q.cols;                          // the lane's pixel exists
    const bool col_win = c >= QR && c <= q.cols - 1 - QR;     // ... and is the centre of a whole window (columns)

    float fxa = 0.0f, fya = 0.0f, fxb = 0.0f, fyb = 0.0f;
    auto fetch = [&](int i) {  // row r0 - 5 + i of both planes into registers (zero outside the plane)
        const int rr = r0 - QR + i;
        fxa = 0.0f; fya = 0.0f; fxb = 0.0f; fyb = 0.0f;
        if (rr < 0 || rr >= q.rows) return;
        const TX* xr = xp + (long long)rr * x.pitch;
        const TY* yr = yp + (long long)rr * y.pitch;
        if (a_in) { fxa = q_ld(xr + ca); fya = q_ld(yr + ca); }
        if (b_in) { fxb = q_ld(xr + cb); fyb = q_ld(yr + cb); }
    };
    auto stash = [&](int buf) {
        s_x[buf][lane] = (double)fxa; s_y[buf][lane] = (double)fya;
        if (lane < 2 * QR) { s_x[buf][QW + lane] = (double)fxb; s_y[buf][QW + lane] = (double)fyb; }
    };

    double ring[QN][5];
#pragma unroll
    for (int j = 0; j < QN; ++j)
#pragma unroll
        for (int k = 0; k < 5; ++k) ring[j][k] = 0.0;
    double sse = 0.0, dmax = 0.0, ssum = 0.0;

    fetch(0);
    stash(0);
    for (int it = 0; it < niter; it += QN) {
#pragma unroll
        for (int j = 0; j < QN; ++j) {
            const int i = it + j;
            if (i < niter) {  // (uniform over the block)
                const int buf = i & 1;
                if (i + 1 < niter) fetch(i + 1);
                __syncthreads();  // row i is in s_*[buf]; everyone has finished with s_*[buf ^ 1] (row i - 1)
                const double* sx = s_x[buf] + lane;
                const double* sy = s_y[buf] + lane;
                // the row filter at this lane's column: taps k and 10 - k share g[k]
                const double xc = sx[QR], yc = sy[QR];
                double hx = w.g[QR] * xc, hy = w.g[QR] * yc;
                double hxx = w.g[QR] * (xc * xc), hyy = w.g[QR] * (yc * yc), hxy = w.g[QR] * (xc * yc);
#pragma unroll
                for (int k = 0; k < QR; ++k) {
                    const double xa = sx[k], xb = sx[QN - 1 - k];
                    const double ya = sy[k], yb = sy[QN - 1 - k];
                    hx = q_fma(w.g[k], xa + xb, hx);
                    hy = q_fma(w.g[k], ya + yb, hy);
                    hxx = q_fma(w.g[k], q_fma(xa, xa, xb * xb), hxx);
                    hyy = q_fma(w.g[k], q_fma(ya, ya, yb * yb), hyy);
                    hxy = q_fma(w.g[k], q_fma(xa, ya, xb * yb), hxy);
                }
                ring[j][0] = hx; ring[j][1] = hy; ring[j][2] = hxx; ring[j][3] = hyy; ring[j][4] = hxy;
                // the lane's own pixel of this row
                const int rr = r0 - QR + i;
                if (rr >= r0 && rr < r1 && col_own) {
                    const double d = xc - yc;
                    sse += d * d;
                    dmax = fmax(dmax, fabs(d));
                }
                // the window whose last row this is: centre ro = rr - 5, ring rows (j + 1 + k) % 11, k = 0 .. 10, oldest first
                const int ro = rr - QR;
                if (i >= 2 * QR && ro >= QR && ro <= q.rows - 1 - QR) {  // (uniform; ro < r1 by niter)
                    double v[5];
#pragma unroll
                    for (int m = 0; m < 5; ++m) {
                        double acc = w.g[QR] * ring[(j + 1 + QR) % QN][m];
#pragma unroll
                        for (int k = 0; k < QR; ++k) acc = q_fma(w.g[k], ring[(j + 1 + k) % QN][m] + ring[(j + QN - k) % QN][m], acc);
                        v[m] = acc;
                    }
                    const double mx = v[0], my = v[1];
                    const double mxy = mx * my, mxx = mx * mx, myy = my * my;
                    const double vx = v[2] - mxx, vy = v[3] - myy, cxy = v[4] - mxy;
                    const double num = (2.0 * mxy + QC1) * (2.0 * cxy + QC2);
                    const double den = ((mxx + myy) + QC1) * ((vx + vy) + QC2);
                    if (col_win) ssum += num / den;
                }
                if (i + 1 < niter) stash(buf ^ 1);
            }
        }
    }

    // the four lanes of a column group, in lane order
    s_red[0][lane] = sse; s_red[1][lane] = ssum; s_red[2][lane] = dmax;
    __syncthreads();
    if ((lane & 3) == 0 && col_own) {
        const double a = ((s_red[0][lane] + s_red[0][lane + 1]) + s_red[0][lane + 2]) + s_red[0][lane + 3];
        const double b = ((s_red[1][lane] + s_red[1][lane + 1]) + s_red[1][lane + 2]) + s_red[1][lane + 3];
        const double m = fmax(fmax(s_red[2][lane], s_red[2][lane + 1]), fmax(s_red[2][lane + 2], s_red[2][lane + 3]));
        double* p = rec + (((long long)z * q.nsegs + seg) * q.ngroups + (c >> 2)) * 3;
        p[0] = a; p[1] = b; p[2] = m;
    }
}

namespace {
// a wave's three values folded in a fixed tree over the lanes; the totals are in s_*[0] afterwards (every lane calls)
__device__ __forceinline__ void q_tree(double* s_a, double* s_b, double* s_m, int lane, double a, double b, double m)
{
    s_a[lane] = a; s_b[lane] = b; s_m[lane] = m;
    __syncthreads();
    for (int o = QW / 2; o > 0; o >>= 1) {
        if (lane < o) { s_a[lane] += s_a[lane + o]; s_b[lane] += s_b[lane + o]; s_m[lane] = fmax(s_m[lane], s_m[lane + o]); }
        __syncthreads();
    }
}
}  // namespace

// The fold of a tile's records, in two levels so that one tile per 4K plane (65 280 records) is not one wave's serial loop.
// k_quality_fold_cols: one wavefront per (plane, segment, tile column) adds the segment's groups of that tile column -- lane l takes
// groups g0 + l, g0 + l + 64, ... in order, then a fixed tree over the lanes -- into part [plane][segment][nx][3]
__global__ __launch_bounds__(QW) void k_quality_fold_cols(const double* __restrict__ rec, QualityGeom q, TileShape ts, double* __restrict__ part)
{
    __shared__ double s_a[QW], s_b[QW], s_m[QW];
    const int lane = (int)threadIdx.x;
    const int tx = (int)blockIdx.x, seg = (int)blockIdx.y, z = (int)blockIdx.z;
    const int g0 = tx * ts.tw / 4, g1 = tx == ts.nx - 1 ? q.ngroups : (tx + 1) * ts.tw / 4;
    const double* rs = rec + ((long long)z * q.nsegs + seg) * q.ngroups * 3;
    double a = 0.0, b = 0.0, m = 0.0;
    for (int g = g0 + lane; g < g1; g += QW) {
        const double* p = rs + (long long)g * 3;
        a += p[0]; b += p[1]; m = fmax(m, p[2]);
    }
    q_tree(s_a, s_b, s_m, lane, a, b, m);
    if (lane != 0) return;
    double* o = part + (((long long)z * q.nsegs + seg) * ts.nx + tx) * 3;
    o[0] = s_a[0]; o[1] = s_b[0]; o[2] = s_m[0];
}

// k_quality_fold: one wavefront per (plane, tile) adds the tile's segments of part the same way (lane l takes segments seg0 + l,
// seg0 + l + 64, ...).  sums [plane][tile][5] = {sse, npix, ssim_sum, nwin, max|d|}
__global__ __launch_bounds__(QW) void k_quality_fold(const double* __restrict__ part, QualityGeom q, TileShape ts, double* __restrict__ sums)
{
    __shared__ double s_a[QW], s_b[QW], s_m[QW];
    const int lane = (int)threadIdx.x;
    const int t = (int)blockIdx.x, z = (int)blockIdx.y;
    const int ty = t / ts.nx, tx = t - ty * ts.nx;
    const int seg0 = ty * ts.th / q.rps, seg1 = ty == ts.ny - 1 ? q.nsegs : (ty + 1) * ts.th / q.rps;
    const double* pz = part + (long long)z * q.nsegs * ts.nx * 3;
    double a = 0.0, b = 0.0, m = 0.0;
    for (int sg = seg0 + lane; sg < seg1; sg += QW) {
        const double* p = pz + ((long long)sg * ts.nx + tx) * 3;
        a += p[0]; b += p[1]; m = fmax(m, p[2]);
    }
    q_tree(s_a, s_b, s_m, lane, a, b, m);
    if (lane != 0) return;
    // the tile's pixels and the window centres among them (rows 5 .. rows - 6, columns 5 .. cols - 6)
    const int tr0 = ty * ts.th, tr1 = ty == ts.ny - 1 ? q.rows : (ty + 1) * ts.th;
    const int tc0 = tx * ts.tw, tc1 = tx == ts.nx - 1 ? q.cols : (tx + 1) * ts.tw;
    const int wr = max(0, min(tr1, q.rows - QR) - max(tr0, QR)), wc = max(0, min(tc1, q.cols - QR) - max(tc0, QR));
    double* o = sums + ((long long)z * ts.ny * ts.nx + t) * 5;
    o[0] = s_a[0];
    o[1] = (double)(tr1 - tr0) * (double)(tc1 - tc0);
    o[2] = s_b[0];
    o[3] = (double)wr * (double)wc;
    o[4] = s_m[0];
}

// one wavefront per plane: the tiles' values added in ascending tile index, one after the other (64 tiles are loaded at a time and
// every lane adds all of them in order), then res[plane * 3 ..] = {mse, ssim, max|d|} with status 0
__global__ __launch_bounds__(QW) void k_quality_total(const double* __restrict__ sums, int ntiles, OpResult* __restrict__ res)
{
    __shared__ double s_v[5][QW];
    const int lane = (int)threadIdx.x;
    const int z = (int)blockIdx.x;
    const double* sz = sums + (long long)z * ntiles * 5;
    double sse = 0.0, npix = 0.0, ssum = 0.0, nwin = 0.0, dmax = 0.0;
    for (int t0 = 0; t0 < ntiles; t0 += QW) {
        const int n = min(QW, ntiles - t0);
        __syncthreads();
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 5; ++k) s_v[k][lane] = sz[(long long)(t0 + lane) * 5 + k];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            sse += s_v[0][k]; npix += s_v[1][k]; ssum += s_v[2][k]; nwin += s_v[3][k]; dmax = fmax(dmax, s_v[4][k]);
        }
    }
    if (lane != 0) return;
    OpResult r;
    r.status = 0;
    r.value = (float)(sse / npix); res[z * 3 + 0] = r;
    r.value = (float)(ssum / nwin); res[z * 3 + 1] = r;   // (no window: 0 / 0 = NaN, wm.h)
    r.value = (float)dmax; res[z * 3 + 2] = r;
}

QualityGeom quality_geom(int rows, int cols, int channels, int tile_rows)
{
    QualityGeom q;
    q.rows = rows; q.cols = cols; q.channels = channels;
    q.rps = tile_rows > 0 ? tiles_segment_rows(tile_rows) : 48;  // from the tile shape alone: a plane's bits do not depend on the batch
    q.nsegs = (rows + q.rps - 1) / q.rps;
    q.nstrips = (cols + QW - 1) / QW;
    q.ngroups = (cols + 3) / 4;
    return q;
}
// rec [planes][nsegs][ngroups][3] and, behind it, part [planes][nsegs][nx][3]
static size_t quality_rec_doubles(const QualityGeom& q, int planes) { return (size_t)planes * q.nsegs * q.ngroups * 3; }
size_t quality_rec_bytes(const QualityGeom& q, const TileShape& ts, int planes)
{
    return (quality_rec_doubles(q, planes) + (size_t)planes * q.nsegs * ts.nx * 3) * sizeof(double);
}
bool quality_grid_fits(int planes) { return planes >= 1 && planes <= 65535; }

void launch_quality(hipStream_t s, const QualityGeom& q, const QualityWeights& w, const TileShape& ts, int planes, const PlaneDesc& x,
                    const PlaneDesc& y, double* rec, double* sums, OpResult* res)
{
    double* part = rec + quality_rec_doubles(q, planes);
    const dim3 grid((unsigned)q.nstrips, (unsigned)q.nsegs, (unsigned)planes), block(QW);
    if (x.dtype == 0 && y.dtype == 0) hipLaunchKernelGGL((k_quality<float, float>), grid, block, 0, s, x, y, q, w, rec);
    else if (x.dtype == 0) hipLaunchKernelGGL((k_quality<float, unsigned char>), grid, block, 0, s, x, y, q, w, rec);
    else if (y.dtype == 0) hipLaunchKernelGGL((k_quality<unsigned char, float>), grid, block, 0, s, x, y, q, w, rec);
    else hipLaunchKernelGGL((k_quality<unsigned char, unsigned char>), grid, block, 0, s, x, y, q, w, rec);
    hipLaunchKernelGGL(k_quality_fold_cols, dim3((unsigned)ts.nx, (unsigned)q.nsegs, (unsigned)planes), block, 0, s, rec, q, ts, part);
    hipLaunchKernelGGL(k_quality_fold, dim3((unsigned)(ts.ny * ts.nx), (unsigned)planes), block, 0, s, part, q, ts, sums);
    if (res) hipLaunchKernelGGL(k_quality_total, dim3((unsigned)planes), block, 0, s, sums, ts.ny * ts.nx, res);
}

}  // namespace wmk
