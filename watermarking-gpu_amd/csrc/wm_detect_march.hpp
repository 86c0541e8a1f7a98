// wm_detect_march.hpp -- detect_march, the detector's march over one wave's segment: shared by k_detect (wm_k_detect.hip) and
// k_detect_tiles (wm_k_detect_tiles.hip), which differ only in what becomes of the three sums; and detect_body with its fold
// tails (corr_fold, corr_finalize_frame), k_detect's kernel body, which k_detect_sel (wm_k_select.hip) runs with a W per frame
#pragma once
#include "wm_march.hpp"

#ifndef WM_DET_RING
#define WM_DET_RING 6   // x rows of k_detect's aligned 3x3 path: ring length (rows in flight = ring - 3).  Measured: 9 and 12 (6 and
                        // 9 rows in flight) gain nothing and cost a wave per SIMD
#endif
#ifndef WM_DET_EXP
#define WM_DET_EXP 0   // timing experiments (wrong results): 1 no prediction chains, 3 no e_u chain
#endif
#ifndef WM_DET_WAVES
#define WM_DET_WAVES 4
#endif
#ifndef WM_PFW_DET
#define WM_PFW_DET 3   // W rows are L2 hits (the frames of a block share them): 3 in flight suffice and leave k_detect at 4 waves per SIMD
#endif

namespace wmk {

constexpr int PFWD = WM_PFW_DET;  // rows of W (and of W's halo column) prefetched per wave in k_detect

// =================================================================================================
// k_detect: one fused sweep over the test image and W:
//   e_w = x - c.nbrs(x);  u = m W  (ME: m ~ |e_w|, the max|e_w| normalisation cancels in the
//   correlation; NVF: m = nvf(x));  e_u = u - c.nbrs(u)  with u replicate-padded;
//   per block: <e_u,e_w>, ||e_u||^2, ||e_w||^2          (Watermark.cpp:221-250)
// =================================================================================================
// DIG (the checking instance, f32 on the overlapped aligned path): also the digest of the pixels this wave owns (dig_add,
// wm_device.hpp) -- x rows rs .. re-1, lanes lo .. hi, as loaded
template <typename T, int MASK, int PAD, int HC, bool VEC, bool EDGE, bool DIG = false>
__device__ __forceinline__ void detect_march(const T* __restrict__ xf, long long pitch, const float* __restrict__ W,
                                             const Geom& g, const WaveJob& j, float* lds_x, float* lds_u,
                                             const float (&c)[8], float& dot, float& nu, float& nw, unsigned long long& dig)
{
    constexpr int HRX = MASK == 0 ? 1 : PAD;  // x rows needed above/below a u row
    constexpr int NR = 2 * HRX + 1;
    constexpr int O = 4 * HC;                 // own chunk offset in window rows
    constexpr int MID = HRX;                  // window row of the u row being produced
    const int R = g.rows, C = g.cols;
    float nc[8];  // the negated coefficients of residual4 (wave-uniform: SGPRs)
#pragma unroll
    for (int k = 0; k < 8; ++k) nc[k] = -c[k];
    // u rows t0..t1 are computed; x rows t0-HRX .. t1+HRX are streamed (clamped at load)
    const int t0 = j.rs > 0 ? j.rs - 1 : 0;
    const int t1 = j.re < R ? j.re : R - 1;
    const int nu_rows = t1 - t0 + 1;
    const int n = nu_rows + 2 * HRX;
    // (aligned path, 3x3 masks) OVERLAPPED STRIPS (Geom::sstride / lead, WaveJob::lo / hi): the wave loads 256 consecutive
    // columns of which lanes lo .. hi own theirs; lane 0 and lane 63 (when they are not owners: everywhere but at the image's
    // left border) evaluate e_w and u like every lane and exist to hand them to lanes 1 and 62 by DPP.  Nothing at a strip's
    // halo column is loaded or computed separately: the per-row halo loads (2 of 4 loads), the halo prediction every lane
    // evaluated for the two that used it and the selects that routed its inputs (~25 of ~120 vector instructions per row) are
    // gone, for 2 of 64 lanes that own nothing (4K: 16 strips of 248 columns instead of 15 of 256).  NVF with p = 5, 7 runs the same
    // way since round 4 (the mask's 2 or 3 halo columns lie inside the provider lane's 4 pixels; until then every lane evaluated the
    // mask at a halo column for the two lanes that used it: a third of the row's arithmetic); p = 9 takes the generic path.
    constexpr bool HALO1 = VEC && HC == 1 && (MASK == 0 || PAD <= 3);  // (p = 5, 7 as well: the mask's halo columns lie inside the provider lane)
    constexpr int DR = HALO1 && NR == 3 ? WM_DET_RING : UNROLL;
    XMarch<T, HC, HALO1 ? HRX : HRX + 1, NR, VEC, PFX, EDGE, HALO1, DR> xm;
    PMarch<float, VEC, PFWD> wm_;
    const int c0 = j.c0s + 4 * j.lane;
    const bool left_edge = EDGE && j.c0s == 0;
    const bool has_right = !EDGE || j.c0s + STRIP <= C - 1;  // column c0s+STRIP exists in the image
    xm.start(xf, pitch, g, j, lds_x, t0 - HRX, n);
    wm_.start(W, C, C, j, t0, nu_rows);
    // W at the strip's halo columns c0s-1 (lanes != 63) and c0s+STRIP (lane 63): loaded by every lane, no branch (variants
    // without the gather)
    const int wh_col = j.lane == WAVE - 1 ? (j.c0s + STRIP < C ? j.c0s + STRIP : C - 1) : (j.c0s > 0 ? j.c0s - 1 : 0);
    const unsigned wh_off = (unsigned)wh_col * 4u;
    const float* whp = W + wh_col;
    auto load_wh = [&](int r) -> float {
        if constexpr (HALO1) return 0.0f;
        else if constexpr (VEC) return buf_load<float>(wm_.ps.rs, wh_off, (unsigned)r * wm_.ps.pitch_b);  // (a row of W: scalar offset)
        else return whp[(long long)r * C];
    };
    float whpre[PFWD];
#pragma unroll
    for (int s = 0; s < PFWD; ++s) whpre[s] = load_wh(min(t0 + s, t1));
    // rolling window of u rows (left neighbour, 4 own, right neighbour) in rotating slots, e_w of two rows
    float uw[3][6];
    float eww[3][4];  // (three slots: the ring length DR may be odd)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) uw[a][b] = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) eww[a][b] = 0.f;
    const int last_col_local = C - 1 - j.c0s;  // strip-local index of the image's last column
    // lanes that own their 4 columns: not the duplicate lanes of a shifted last strip (their sums belong to the previous strip),
    // and with overlapped strips (HALO1) only lanes lo .. hi -- those sum everything and are masked once, at the end
    const bool own = HALO1 || !EDGE || 4 * j.lane >= j.dup;
    static_assert(!DIG || (HALO1 && std::is_same<T, float>::value), "digest: f32 planes on the overlapped aligned path");
    const uint32_t dcb = DIG ? dig_col_key4(c0) : 0u;
    march_n<2 * HRX, DR>(n, [&](int i, auto qc, auto emit) {
        constexpr int Q = decltype(qc)::value;
        xm.template step<Q>(i);
        if (decltype(emit)::value) {
            const int o = i - 2 * HRX;  // u row index t = t0 + o; its slots: uw[Q % 3], eww[Q % 2]
            const int t = t0 + o;
            constexpr int SLOT = (Q + 2 * DR - 2 * HRX) % PFWD;
            const float4 w = wm_.template take<SLOT>();
            const float wh = HALO1 ? 0.0f : pinned(whpre[SLOT]);
            const float* xup = xm.template row<Q>(MID - 1);
            const float* xmid = xm.template row<Q>(MID);
            const float* xdn = xm.template row<Q>(MID + 1);
            // ---- e_w and u of row t for the 4 own pixels
            float uu[4];
            float* ew = eww[Q % 3];
            float ewn[4];
#if WM_DET_EXP == 1
            ewn[0] = xup[O]; ewn[1] = xup[O + 1]; ewn[2] = xdn[O + 2]; ewn[3] = xdn[O + 3];  // (timing experiment: no prediction chains)
#else
            residual4<O>(xup, xmid, xdn, nc, ewn);  // e_w = x - c.nbrs(x), the subtraction folded into the chain (wm_device.hpp)
#endif
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ew[k] = ewn[k];
                const float m = MASK == 0 ? fabsf(ew[k]) : nvf_value<PAD, O, Q>(xm, k);
                uu[k] = m * f4get(w, k);
            }
            if constexpr (DIG) {
                if (t >= j.rs && t < j.re) dig_add4(dig, xmid[O], xmid[O + 1], xmid[O + 2], xmid[O + 3], dig_row_key(t), dcb);
            }
            float* un = uw[Q % 3];
            if constexpr (HALO1) {
                // neighbours' u by DPP wave shifts.  Lane 0 / lane 63 keep their own border pixel (the "old" operand): that is
                // the replicate border u(-1) := u(0) where lane 0 owns the image's first column, and never used where they are
                // provider lanes; at the image's right border the lane that holds the last column takes u(C) := u(C-1) itself
                if constexpr (EDGE) {
                    un[0] = dpp_from_prev(uu[3], uu[0]);
                    const float nx = dpp_from_next(uu[0], uu[3]);
                    un[5] = xm.xs.rsel ? uu[3] : nx;
                } else {
                    un[0] = dpp_from_prev_any(uu[3]);
                    un[5] = dpp_from_next_any(uu[0]);
                }
            } else {
                // replicate border inside the own chunk: u(c) := u(C-1) for c >= C
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    if (c0 + k >= C) uu[k] = uu[k - 1];
                // ---- publish the u row through LDS: own chunk, strip halo columns, replicate border
                float* urow = lds_u + (Q & 1) * RowBuf<1>::N;
                reinterpret_cast<float4*>(urow)[1 + j.lane] = make_float4(uu[0], uu[1], uu[2], uu[3]);
                if (j.lane == 0) {
                    float uh;
                    if (left_edge) uh = uu[0];
                    else {
                        const float eh = residual1<O>(xup, xmid, xdn, -1, nc);
                        const float m = MASK == 0 ? fabsf(eh) : nvf_value<PAD, O, Q>(xm, -1);
                        uh = m * wh;
                    }
                    urow[3] = uh;
                }
                if (j.lane == WAVE - 1 && has_right) {
                    const float eh = residual1<O>(xup, xmid, xdn, 4, nc);
                    const float m = MASK == 0 ? fabsf(eh) : nvf_value<PAD, O, Q>(xm, 4);
                    urow[4 + STRIP] = m * wh;
                }
                if (!has_right) {
                    // image's last column lies in this strip: u(C) := u(C-1)
                    const int lk = last_col_local - 4 * j.lane;
                    if (lk >= 0 && lk < 4) urow[4 + last_col_local + 1] = uu[lk];
                }
                wave_lds_fence();
                un[0] = urow[3 + 4 * j.lane];
                un[5] = urow[8 + 4 * j.lane];
            }
            un[1] = uu[0]; un[2] = uu[1]; un[3] = uu[2]; un[4] = uu[3];
            if (o == 0 && j.rs == 0) {
                // u(-1) := u(0): the first computed row is image row 0; seed the slot the next step reads as "um"
#pragma unroll
                for (int b = 0; b < 6; ++b) uw[(Q + 2) % 3][b] = un[b];
            }
            // ---- emit e_u for row r = t-1: u rows r-1, r, r+1 are slots (Q+1)%3, (Q+2)%3, Q%3
            const int r = t - 1;
            if (r >= j.rs && r < j.re) {
                const float* um = uw[(Q + 1) % 3];
                const float* u0 = uw[(Q + 2) % 3];
                const float* ewp = eww[(Q + 2) % 3];
                float eun[4];
#if WM_DET_EXP == 1 || WM_DET_EXP == 3
                eun[0] = um[1]; eun[1] = um[2]; eun[2] = un[3]; eun[3] = un[4];  // (timing experiment)
#else
                residual4<1>(um, u0, un, nc, eun);  // e_u = u - c.nbrs(u)
#endif
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (VEC ? own : (c0 + k < C && c0 + k >= j.own_c0)) {
                        const float eu = eun[k];
                        dot = fmaf(eu, ewp[k], dot);
                        nu = fmaf(eu, eu, nu);
                        nw = fmaf(ewp[k], ewp[k], nw);
                    }
                }
            }
            if (j.re == R && t == R - 1) {
                // last image row: u(R) := u(R-1); window (u(R-2), u(R-1), u(R-1))
                const float* u0 = uw[(Q + 2) % 3];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (VEC ? own : (c0 + k < C && c0 + k >= j.own_c0)) {
                        const float eu = residual1<1>(u0, un, un, k, nc);
                        dot = fmaf(eu, ew[k], dot);
                        nu = fmaf(eu, eu, nu);
                        nw = fmaf(ew[k], ew[k], nw);
                    }
                }
            }
            wm_.template refill<SLOT>(o);
            if constexpr (!HALO1) {
                __builtin_amdgcn_sched_barrier(0);
                whpre[SLOT] = load_wh(min(t + PFWD, t1));
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    });
    if constexpr (HALO1) {
        // the provider lanes (and the lanes beyond the image's last column) summed pixels other lanes own: drop their sums
        const bool mine = j.lane >= j.lo && j.lane <= j.hi;
        dot = mine ? dot : 0.0f; nu = mine ? nu : 0.0f; nw = mine ? nw : 0.0f;
        if constexpr (DIG) dig = mine ? dig : 0ull;
    }
}

// ---- detect_body, the body of k_detect / k_detect_redo (wm_k_detect.hip) and of k_detect_sel (wm_k_select.hip, with the frame's own
// key plane as W), and its fold tails
// corr_fold (tail of k_detect; take_ticket, wm_device.hpp): the last wave of a strip folds the strip's records, the last
// strip's wave folds the frame:
// corr = (float)dot / (float)(||e_w|| * ||e_u||)   (Watermark.cpp:230); unsolvable => 0.0f (:246-247)
// publish a frame's score -- or, in the checking instance (CK = 1), only when the digest of the plane this sweep read equals the
// one the embed left (DigCheck); else flag the frame for the redo launches
template <int CK>
__device__ __forceinline__ void corr_publish(int frame, double a0, double a1, double a2, unsigned long long dg,
                                             const int* __restrict__ status, OpResult* res, RawSums* raw, const DigCheck& dc)
{
    if constexpr (CK == 1) {
        const bool ok = dg == dc.want[frame];
        dc.redo[frame] = ok ? 0 : 1;
        atomicAdd(dc.count + (ok ? 0 : 1), 1ull);
        if (!ok) return;
    }
    const int st = status[frame];
    float corr = 0.0f;
    if (st == 0) corr = (float)a0 / (float)(sqrt(a2) * sqrt(a1));
    res[frame].status = st;
    res[frame].value = corr;
    RawSums rw;
    rw.v[0] = a0; rw.v[1] = a1; rw.v[2] = a2; rw.v[3] = 0.0;
    raw[frame] = rw;
}

template <int CK>
__device__ __forceinline__ void corr_fold(int frame, const WaveJob& j, const double* pcorr, int nrec,
                                          const int* __restrict__ status, const CorrTail& tl, const DigCheck& dc)
{
    const int lane = j.lane;
    if (!take_ticket(tl.ticket_strip + (frame * tl.nstrips + j.strip) * TKS, (unsigned)tl.nsegs, lane)) return;
    unsigned long long dg = 0;
    if constexpr (CK == 1) {
        for (int s0 = lane; s0 < tl.nsegs; s0 += WAVE) dg += ld_agent(dc.pdig + (long long)frame * nrec + (long long)s0 * tl.nstrips + j.strip);
        dg = wave_sum_u64(dg);
        if (lane == 0) st_agent(dc.sdig + (long long)frame * tl.nstrips + j.strip, dg);
    }
    // all loads of a batch are issued before the first is used (index clamped, surplus terms dropped): agent-scope loads
    // come from the memory side, a dependent chain of them costs a memory latency per term
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int s0 = lane; s0 < tl.nsegs; s0 += 2 * WAVE) {
        double v[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double* p = pcorr + ((long long)frame * nrec + (long long)min(s0 + u * WAVE, tl.nsegs - 1) * tl.nstrips + j.strip) * 3;
            v[u][0] = ld_agent(p); v[u][1] = ld_agent(p + 1); v[u][2] = ld_agent(p + 2);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool in = s0 + u * WAVE < tl.nsegs;
            a0 += in ? v[u][0] : 0.0; a1 += in ? v[u][1] : 0.0; a2 += in ? v[u][2] : 0.0;
        }
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane == 0) {
        double* q = tl.scorr + ((long long)frame * tl.nstrips + j.strip) * 3;
        st_agent(q, a0); st_agent(q + 1, a1); st_agent(q + 2, a2);
    }
    if (!take_ticket(tl.ticket + frame * TKS, (unsigned)tl.nstrips, lane)) return;
    a0 = 0.0; a1 = 0.0; a2 = 0.0;
    dg = 0;
    for (int s0 = lane; s0 < tl.nstrips; s0 += WAVE) {
        const double* q = tl.scorr + ((long long)frame * tl.nstrips + s0) * 3;
        const double v0 = ld_agent(q), v1 = ld_agent(q + 1), v2 = ld_agent(q + 2);
        a0 += v0; a1 += v1; a2 += v2;
        if constexpr (CK == 1) dg += ld_agent(dc.sdig + (long long)frame * tl.nstrips + s0);
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if constexpr (CK == 1) dg = wave_sum_u64(dg);
    if (lane == 0) corr_publish<CK>(frame, a0, a1, a2, dg, status, tl.res, tl.raw, dc);
}

// corr_finalize_frame (tail of k_detect, run by the frame's last block):
// corr = (float)dot / (float)(||e_w|| * ||e_u||)   (Watermark.cpp:230); unsolvable => 0.0f (:246-247)
template <int CK>
__device__ __forceinline__ void corr_finalize_frame(int frame, const double* pcorr, int nblk, const int* __restrict__ status,
                                                    OpResult* __restrict__ res, RawSums* __restrict__ raw, const DigCheck& dc)
{
    __shared__ double s[3][BLOCK];
    const int t = threadIdx.x;
    unsigned long long dg = 0;
    if constexpr (CK == 1) {
        if (t < WAVE) {
            for (int b = t; b < nblk; b += WAVE) dg += ld_agent(dc.pdig + (long long)frame * nblk + b);
            dg = wave_sum_u64(dg);
        }
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    // 2 x 3 partials in flight per thread (index clamped, surplus terms dropped), see solve_frame
    for (int b0 = t; b0 < nblk; b0 += 2 * BLOCK) {
        double v[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double* p = pcorr + ((long long)frame * nblk + min(b0 + u * BLOCK, nblk - 1)) * 3;
            v[u][0] = ld_agent(p); v[u][1] = ld_agent(p + 1); v[u][2] = ld_agent(p + 2);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool in = b0 + u * BLOCK < nblk;
            a0 += in ? v[u][0] : 0.0; a1 += in ? v[u][1] : 0.0; a2 += in ? v[u][2] : 0.0;
        }
    }
    s[0][t] = a0; s[1][t] = a1; s[2][t] = a2;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (t < o) { s[0][t] += s[0][t + o]; s[1][t] += s[1][t + o]; s[2][t] += s[2][t + o]; }
        __syncthreads();
    }
    if (t == 0) corr_publish<CK>(frame, s[0][0], s[1][0], s[2][0], dg, status, res, raw, dc);
}

// CK: 0 = the ordinary sweep; 1 = the checking instance of a checked hand-over (DigCheck, wm_kernels.hpp: every frame's march
// runs -- an unsolvable one too, its sums dropped -- for the digest); 2 = k_detect_redo (frames with dc.redo[f] == 0 leave first)
template <typename T, int MASK, int PAD, int HC, bool VEC, int CK>
__device__ __forceinline__ void detect_body(const T* __restrict__ x, long long pitch, long long fstride, const float* __restrict__ W,
                                            const Geom& g, const float* __restrict__ coef, const int* __restrict__ status,
                                            double* pcorr, const CorrTail& tail, const DigCheck& dc)
{
    __shared__ __attribute__((aligned(16))) float s_row[WPB][2 * RowBuf<HC>::N];
    __shared__ __attribute__((aligned(16))) float s_u[WPB][2 * RowBuf<1>::N];
    __shared__ double s_red[WPB][3];
    __shared__ unsigned long long s_dig[WPB];
    const WaveJob j = make_job(g);
    const int frame = j.frame;
    if constexpr (CK == 2) {
        // quad: the waves of a block are different frames (surplus waves of a short last quad have none) -- a wave-uniform exit, no
        // barrier on that path; else the block is one frame (its waves past the last segment still take part in the barrier)
        if (g.quad ? (!j.valid || dc.redo[frame] == 0) : dc.redo[frame] == 0) return;
    }
    float dot = 0.0f, nu = 0.0f, nw = 0.0f;
    unsigned long long dig = 0;
    const int st = j.valid ? status[frame] : 1;
    if (j.valid && (CK == 1 || st == 0)) {
        float c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = coef[frame * 8 + k];
        const T* xf = x + (long long)frame * fstride;
        constexpr bool DPP_OK = HC == 1;  // the halo of p = 9 (HC = 2) exceeds one neighbour chunk: LDS path only
        constexpr bool V = VEC && DPP_OK;
        constexpr bool D = CK == 1;
        if (MASK != 0 || strip_on_edge<V>(g, j)) detect_march<T, MASK, PAD, HC, V, true, D>(xf, pitch, W, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw, dig);
        else detect_march<T, MASK, PAD, HC, V, (MASK != 0), D>(xf, pitch, W, g, j, s_row[j.wave], s_u[j.wave], c, dot, nu, nw, dig);
        if (CK == 1 && st != 0) { dot = 0.0f; nu = 0.0f; nw = 0.0f; }  // (what the ordinary sweep sums for an unsolvable frame)
    }
    const double d0 = wave_sum((double)dot), d1 = wave_sum((double)nu), d2 = wave_sum((double)nw);
    if constexpr (CK == 1) dig = wave_sum_u64(dig);
    if (g.quad) {
        // the waves of this block are 4 frames: one record per wave, folded per strip and then per frame (corr_fold)
        if (!j.valid) return;  // surplus wave of a short last quad (wave-uniform; no barrier below)
        if (j.lane == 0) {
            double* p = pcorr + ((long long)frame * g.nrec + j.rec) * 3;
            st_agent(p, d0); st_agent(p + 1, d1); st_agent(p + 2, d2);
            if constexpr (CK == 1) st_agent(dc.pdig + (long long)frame * g.nrec + j.rec, dig);
        }
        corr_fold<CK>(frame, j, pcorr, g.nrec, status, tail, dc);
        return;
    }
    // the waves of this block are 4 segments of one frame: one record per block, folded by the frame's last block
    if (j.lane == 0) { s_red[j.wave][0] = d0; s_red[j.wave][1] = d1; s_red[j.wave][2] = d2; s_dig[j.wave] = dig; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        st_agent(pcorr + ((long long)frame * g.nblk_total + g.pb0 + j.tile) * 3 + k, ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k]);
    }
    if (CK == 1 && threadIdx.x == 3)
        st_agent(dc.pdig + (long long)frame * g.nblk_total + g.pb0 + j.tile, s_dig[0] + s_dig[1] + s_dig[2] + s_dig[3]);
    if (last_block_of_frame(tail.ticket + frame * TKS, (unsigned)tail.expected))
        corr_finalize_frame<CK>(frame, pcorr, g.nblk_total, status, tail.res, tail.raw, dc);
}

// occupancy floor: 4 waves per SIMD for the aligned 3x3 instances (105 / 106 / 91 VGPRs); the generic instances (LDS re-lay,
// halo predictions of their own) need ~150 registers -- bound to 4 they spilled 48-70 VGPRs to scratch, at 3 they do not
// (expands inside a kernel template with k_detect's parameters PAD, HC, VEC; the file that uses it #undefs it behind its kernels)
#define WM_DET_BOUNDS (PAD == 1 && HC == 1 ? (VEC ? WM_DET_WAVES : 3) : 1)

}  // namespace wmk
