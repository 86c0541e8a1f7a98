// wm_k_embed_signs_multi.hip -- ONE frame, many payload copies (wm_embed_signs_multi / wm_embed_bits_multi, wm.h): k_embed_signs_multi
//
// A distributor marks one frame for K recipients, every copy with its own sign table and all of them with one key.  Nothing on the
// image side depends on the table: the Gram sums, the coefficients, the mask, max|e| and -- since ||m W|| does not see the signs --
// the strength a are the frame's.  k_embed_signs_multi is k_embed_signs' march (embed_march with SIGNS, wm_embed_march.hpp) with the
// copy-dependent tail inside the row step: m, the W row, u = m W and the base row are formed once per row, then every copy of a
// compile-time group takes its tile's sign, us = u s (exact), y = clamp(fmaf(us, a, b), 0, 255) in embed_march's expression order,
// and stores its plane.  That march (embed_group_march with SIGNS, beside SignWalkGroup) and the kernel body around it
// (WM_EMBED_GROUP_BODY) live in wm_embed_march.hpp, shared with k_embed_keys; the kernel here says where W, a, max|e| and the sign
// tables come from.  Copy groups are a grid axis in k_embed_keys' block order (keys_job): the groups of one (tile, frame) are
// consecutive blocks of one XCD, so their re-reads of x, W and base are L2 hits.  One channel of the base per launch, as k_embed_keys.
#include "wm_embed_march.hpp"

#ifndef WM_EMBED_SIGNS_G
#define WM_EMBED_SIGNS_G 2   // copies per group: the largest that keeps the aligned ME f32 instances at k_embed_signs' waves per SIMD
                             // (5 with base = input, 4 with a grey base; 3 and 4 copies lose the fifth wave: DESIGN.md section 17)
#endif

namespace wmk {

constexpr int SMG = WM_EMBED_SIGNS_G;

struct SignsMultiArgs {
    SignTable st;              // signs [frames][ncopies][ny][nx], -1 | 0 | +1
    int ncopies;
    int ngroups;               // copy groups = grid blocks per tile
};

// the group march (embed_group_march, wm_embed_march.hpp) with one W stream, one strength and a sign table per copy
// base / out: one channel (PlaneDesc::p at that channel, cstride unused)
template <typename T, int MASK, int PAD, bool VEC, bool BX>
__global__ __launch_bounds__(BLOCK) void k_embed_signs_multi(const T* __restrict__ x, long long pitch, long long fstride,
                                                             const float* __restrict__ W, PlaneDesc base, PlaneDesc out, Geom g,
                                                             const float* __restrict__ coef, const int* __restrict__ status,
                                                             const EmbedScalars* __restrict__ scal, SignsMultiArgs sa)
{
    WM_EMBED_GROUP_BODY(SMG, sa.ngroups, sa.ncopies);
    const int T_ = sa.st.ny * sa.st.nx;  // the tables of a frame's copies lie ny * nx apart
    int toff[SMG];                       // table of copy q from the group's first
#pragma unroll
    for (int q = 0; q < SMG; ++q) toff[q] = (kq[q] - k0) * T_;
    const float a = applied_strength(scal[frame].a);  // (one strength per frame: ||m W|| does not see the signs)
    const float maxe = scal[frame].maxe;
    const T* xf = x + (long long)frame * fstride;
    const signed char* table = sa.st.signs + ((long long)frame * sa.ncopies + k0) * T_;  // (under the quad mapping: this wave's frame)
    WM_EMBED_GROUP_MARCH(SMG, PFW, true, W, a, maxe, table, toff, &sa.st);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// does every grid of the sweep, times the copy groups, fit a launch grid of 31 bits (from the shapes alone: under any alignment)?
bool embed_signs_multi_grid_fits(const LaunchGeom& lg, int frames, int ncopies)
{
    const long long ng = group_count(ncopies, SMG);
    bool ok = true;
    for (int al = 0; al <= 2; ++al)
        for (int vec = 0; vec <= 1; ++vec) {
            const SweepPart sp = sweep_part(lg, frames, vec != 0, al, 1);
            ok = ok && (!sp.run || (long long)sp.grid.x * ng <= 0x7fffffffLL);
        }
    return ok;
}

void launch_embed_signs_multi(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const signed char* signs, int ncopies, const TileShape& ts)
{
    const PlaneDesc& x = sw.x;
    const SignsMultiArgs sa{{signs, ts.th, ts.tw, ts.ny, ts.nx}, ncopies, group_count(ncopies, SMG)};
    // k_embed_signs' launch plan, once per channel of the base, every grid times the copy groups
    WM_DISPATCH_T(x.dtype, for_each_embed_group_launch<T>(sw, w.aligned_w, ep, sa.ngroups, [&](auto m, auto p, auto vec, auto base_is_x, dim3 grid, const Geom& g,
                                                                                              const PlaneDesc& bc, const PlaneDesc& oc) {
        WM_KLAUNCH((k_embed_signs_multi<T, decltype(m)::value, decltype(p)::value, decltype(vec)::value, decltype(base_is_x)::value>), grid, dim3(BLOCK), 0,
                   sw.s, (const T*)x.p, x.pitch, x.fstride, w.W, bc, oc, g, sw.coef, sw.status, ep.scal, sa);
    }));
}

int embed_signs_group(void) { return SMG; }

}  // namespace wmk
