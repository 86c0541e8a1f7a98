// wm_k_detect_offsets.hip -- k_detect_offsets: the detector of ONE image against a rectangle of window offsets into ONE key
// plane that is larger than the image (wm_detect_offsets, wm.h): where in its key does a cropped copy lie?
//
// Offset (oy, ox) scores the image against W = key[oy : oy + rows, ox : ox + cols].  The image side is wm_detect_keys' (Gram
// sweep, solve; e_w, the mask and ||e_w||^2 once per row of the march); the sweep is k_detect_keys' march (group_march,
// wm_keys_march.hpp: one body for both, as are the lines around it and the record tail WM_GROUP_RECORDS) whose members are G
// horizontally adjacent offsets of one row offset instead of KG keys.  The point of the kernel:
// on the aligned path the G members SHARE ONE W ROW STREAM.  A lane's four pixels need, for the offsets ox .. ox + G - 1, the
// 4 + G - 1 consecutive key values key[oy + r][ox + c .. ox + c + 3 + G - 1]: one 16-byte load and one load of the G - 1 values
// behind it (the bytes the next lane loads as its own: a vector-cache hit).  Member q takes values q .. q + 3 of them; all that
// follows -- u = m w, the rolling u window with ITS OWN halos (the replicate border is the window's edge, never the key's next
// column), residual4, the dot / nu chains and the partial-sum grouping -- is the march's per member, so a score is bit for bit
// wm_detect_keys' on a bank that holds the window copied out (tests/test_gpu_offsets.py).  The records are laid out
// [frames][ny * nx][rstride][2] and folded by k_keys_fold with nkeys = ny * nx.
//
// Bounds.  The buffer descriptor's range check is open (make_rsrc), so every address is kept inside the key plane by
// arithmetic: a lane's column is clamped to cols - 4 (PStream's clamp), every group is FULL (a short last group starts
// G - nx % G columns further left and does not store the members it shares with its left neighbour; a remainder of at most
// G / 2 columns runs as a second launch of the G = 1 instance instead, which is cheaper), and the extra load is
// exactly G - 1 values wide -- so the last value a group touches is key column ox + cols - 4 + 3 + G - 1, the last column of
// its last member's window, which wm_detect_offsets has checked to lie inside the plane.  nx < G runs the G = 1 instance, as do
// the generic, split-remainder and NVF p > 3 instances: their members would each need a W stream and a halo stream of their
// own, and at G = 1 they are k_detect's march with a pitch.
#include "wm_keys_march.hpp"

namespace wmk {

struct OffsArgs {
    const float* key;   // the searched key plane [KR][KC]
    int kc;             // its pitch (elements)
    int oy0, ox0;       // first offset
    int ny, nx;         // offsets: (oy0 + i, ox0 + j), i < ny, j < nx; record index i * nx + j
    int jx_lo, nxl;     // this launch scores the columns [jx_lo, jx_lo + nxl) of every row offset in groups of its G
    int ngx;            // column groups per row offset = ceil(nxl / G)
    int ngroups;        // ny * ngx = grid blocks per tile
    int write_w;        // this launch records ||e_w||^2 (one launch of a sweep part does)
    int rstride;        // partial records per (frame, offset)
    double* part;       // [frames][ny * nx][rstride][2]  {<e_u,e_w>, ||e_u||^2}
    double* partw;      // [frames][rstride]              ||e_w||^2 (written by group 0 of the write_w launch)
};

// occupancy floor: G = 1 is k_detect_keys' budget with one member less; the shared-row instances hold G u windows
// (18 VGPRs each) beside the image side's registers
constexpr int offsets_min_blocks(int pad, int hc, bool vec, int tsize, int G)
{
    if (!(pad == 1 && hc == 1)) return 1;
    if (!vec) return 2;
    if (G == 1) return 4;
    return G <= 2 ? (tsize == 1 ? 4 : 3) : 2;
}

template <typename T, int MASK, int PAD, int HC, bool VEC, int G>
__global__ __launch_bounds__(BLOCK, offsets_min_blocks(PAD, HC, VEC, (int)sizeof(T), G)) void k_detect_offsets(
    const T* __restrict__ x, long long pitch, long long fstride, OffsArgs oa, Geom g, const float* __restrict__ coef,
    const int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * G * RowBuf<1>::N];
    int grp;  // (offset group: iy * ngx + gx, column groups fastest)
    const WaveJob j = keys_job(g, oa.ngroups, grp);
    const int frame = j.frame;
    const int iy = grp / oa.ngx, gx = grp - iy * oa.ngx;
    // every group is full: a short last group starts further left and recomputes the members below `first`, which it does not store
    const int jl0 = min(gx * G, oa.nxl - G);
    const int first = gx * G - jl0;
    const int jx0 = oa.jx_lo + jl0;
    const int noff = oa.ny * oa.nx;
    const int o0 = iy * oa.nx + jx0;  // record index of member 0
    float dot[G], nu[G], nw = 0.0f;
#pragma unroll
    for (int q = 0; q < G; ++q) { dot[q] = 0.0f; nu[q] = 0.0f; }
    if (j.valid && status[frame] == 0) {
        WM_GROUP_DETECT_FRAME;
        // member q's window starts q columns right of the group's (row offset, first column offset)
        const float* Wg = oa.key + (long long)(oa.oy0 + iy) * oa.kc + (oa.ox0 + jx0);
        const float* Wm[G];
#pragma unroll
        for (int q = 0; q < G; ++q) Wm[q] = Wg + q;
        WM_GROUP_DETECT_MARCH(G, G > 1, PFO, Wm, oa.kc);
    }
    // one record per wave (quad) or per block; the group's offsets are o0 .. of the rectangle's noff, those from `first` on are
    // stored; group 0 of the write_w launch records ||e_w||^2
    WM_GROUP_RECORDS(G, o0, noff, o0 + first, o0 + G, oa.rstride, grp == 0 && oa.write_w, oa.part, oa.partw);
}

template <typename T>
static void launch_detect_offsets_t(const Sweep& sw, const DetectPlan& pl, const OffsArgs& oa1)
{
    const PlaneDesc& x = sw.x;
    // columns(): the columns [lo, lo + n) of every row offset in groups of G
    auto columns = [&](int G, int lo, int n, int write_w) {
        OffsArgs a = oa1;
        a.jx_lo = lo; a.nxl = n; a.write_w = write_w;
        a.ngx = group_count(n, G); a.ngroups = a.ny * a.ngx;
        return a;
    };
    // the aligned instance of the 3x3 windows: the shared row when a full group exists.  A remainder of nx % G columns costs a
    // whole group when the last group is moved left to be full; up to G / 2 columns are cheaper as one offset per block (the
    // G = 1 instance) in a launch of their own
    const int rem = oa1.nx % OG, tail = oa1.nx >= OG && 2 * rem <= OG ? rem : 0;
    const OffsArgs all1 = columns(1, 0, oa1.nx, 1);  // every offset a block of its own
    // every grid times the offset groups of its instance
    for_each_detect_launch(pl, sw, [&](auto m, auto p, auto hc, auto vec, const SweepPart& sp) {
        constexpr int MASK = decltype(m)::value, PAD = decltype(p)::value, HC = decltype(hc)::value;
        constexpr bool VEC = decltype(vec)::value;
        auto go = [&](auto g, const OffsArgs& oa) {
            WM_KLAUNCH((k_detect_offsets<T, MASK, PAD, HC, VEC, decltype(g)::value>), dim3(sp.grid.x * (unsigned)oa.ngroups), dim3(BLOCK), 0, sw.s,
                       (const T*)x.p, x.pitch, x.fstride, oa, sp.g, sw.coef, sw.status);
        };
        if constexpr (VEC && PAD == 1) {
            if (oa1.nx >= OG) {
                go(IC<OG>{}, columns(OG, 0, oa1.nx - tail, 1));
                if (tail) go(IC<1>{}, columns(1, oa1.nx - tail, tail, 0));
                return;
            }
        }
        go(IC<1>{}, all1);
    });
}

int detect_offsets_group(void) { return OG; }

int launch_detect_offsets(const Sweep& sw, const KeyBank& key, int key_cols, int oy0, int ox0, int ny, int nx, double* part, int rstride,
                          OpResult* res)
{
    // the geometry comes from the IMAGE plane alone (detect_plan, as for every detector)
    const DetectPlan pl = detect_plan(sw, key.aligned_w);
    const LaunchGeom& ld = pl.ld;
    const int frames = sw.frames;
    const bool quad = frames >= 4;
    if (ld.nblk > rstride || ld.nstrips * ld.nsegs > rstride || ld.nstrips > KEYS_MAX_STRIPS) return -1;
    const int noff = ny * nx;
    OffsArgs oa;
    oa.key = key.W; oa.kc = key_cols; oa.oy0 = oy0; oa.ox0 = ox0; oa.ny = ny; oa.nx = nx; oa.jx_lo = 0; oa.nxl = nx; oa.ngx = nx; oa.ngroups = noff; oa.write_w = 1;
    oa.rstride = rstride; oa.part = part; oa.partw = part + (size_t)frames * noff * rstride * 2;
    WM_DISPATCH_T(sw.x.dtype, launch_detect_offsets_t<T>(sw, pl, oa));
    launch_keys_fold(sw.s, oa.part, oa.partw, rstride, frames, noff, quad ? 1 : 0, ld.nblk, ld.nsegs, ld.nstrips, sw.status, res);
    return 0;
}

}  // namespace wmk
