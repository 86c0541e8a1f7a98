// wm_api.hip -- the C ABI of include/wm.h: context, slots, staging, launch sequencing.
//
// No CPU fallback exists here by design: without a HIP device wm_create() fails with
// WM_ERR_NO_DEVICE.  (The CPU oracle lives in oracle/ and is test infrastructure only.)
#include "../../include/wm.h"
#include "wm_kernels.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace wmk;

namespace {

constexpr int RES_CAP = 4096;  // result records a slot can hold between two wm_sync calls
// wavefronts a launch should have at least.  Measured at 4K with one frame per launch: the ME sweeps are fastest with ~1 wave
// per SIMD (segments of 24-32 rows), the NVF sweeps (three times the arithmetic per pixel) with ~2 (16 rows)
constexpr int TARGET_WAVES_ME = 1280;
constexpr int TARGET_WAVES_NVF = 2048;

// the fold steps (solve, embed scalars, correlation) are tails of k_gram / k_*_stats / k_detect: no kernels of their own
// (the checked hand-over of wm_detect: its k_gram_ho launch and the predicated redo launches behind it are counted apart from
// the opt-in hand-over's k_gram_ho and from the Gram sweeps)
enum KernelId { K_GRAM = 0, K_ME_STATS, K_NVF_STATS, K_EMBED, K_DETECT, K_MASK, K_FUSED_EMBED, K_FUSED_DETECT, K_GRAM_HO, K_FUSED_PAIR, K_DETECT_KEYS,
                K_GRAM_HO_CHECKED, K_GRAM_REDO, K_DETECT_REDO, K_STATS_KEYS, K_EMBED_KEYS_FOLD, K_EMBED_KEYS, K_DETECT_OFFSETS, K_DETECT_TILES, K_TILES_FOLD,
                K_COUNT };
const char* const kKernelNames[K_COUNT] = {"k_gram", "k_me_stats", "k_nvf_stats", "k_embed", "k_detect", "k_mask", "k_fused_embed", "k_fused_detect", "k_gram_ho", "k_fused_pair",
                                           "k_detect_keys", "k_gram_ho_checked", "k_gram_redo", "k_detect_redo", "k_stats_keys",
                                           "k_embed_keys_fold", "k_embed_keys", "k_detect_offsets", "k_detect_tiles", "k_tiles_fold"};

// WM_X=1 / WM_X=0 switches: only a value that says the opposite of the default changes it (first character)
bool env_flag(const char* name, bool dflt)
{
    const char* e = getenv(name);
    return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt;
}

// fused single-frame launches use every CU and wait for each other inside the launch: two of them in flight on one device
// could each hold a part of the CUs and starve the other (their spins are bounded, so that would be a slow fallback, not a
// hang).  Synchronous calls hold this lock from launch to completion: a mutex between the threads of this process and an
// advisory file lock (flock on a per-device file named after the device's PCI address, so the same GPU has the same name
// under any HIP_VISIBLE_DEVICES) between processes that share the device.
constexpr int MAX_DEVICES = 64;
std::mutex g_fused_mu[MAX_DEVICES];
constexpr int FUSED_PENDING = -99;  // result record status while a fused launch has not delivered
constexpr int PAIR_RETRY = 100;     // internal: the fused pair of wm_embed_detect did not complete, take the sweeps

struct FusedGuard {
    std::lock_guard<std::mutex> lk;
    int fd;
    bool ok = true;  // false: another process kept the device's lock beyond the deadline -- the caller takes the sweeps
    FusedGuard(int device, int lock_fd) : lk(g_fused_mu[device % MAX_DEVICES]), fd(lock_fd)
    {
        if (fd < 0) return;
        // a holder is normally gone within one call (~30 us); one that is stopped (a debugger, SIGSTOP) must not hang every other
        // process's synchronous calls: non-blocking attempts up to a deadline, then the call proceeds on the sweeps
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            if (flock(fd, LOCK_EX | LOCK_NB) == 0) return;
            if (errno != EWOULDBLOCK && errno != EINTR) break;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
        }
        ok = false; fd = -1;
    }
    ~FusedGuard() { if (fd >= 0) (void)flock(fd, LOCK_UN); }
};

struct WShared {
    float* d_w = nullptr;
    size_t n = 0;
    ~WShared() { if (d_w) (void)hipFree(d_w); }
};

struct Pending {
    int frames;
    int per_frame;  // records per frame: 1, or the keys of wm_detect_keys / wm_embed_keys, or wm_detect_offsets' ny * nx (value_out [frames][per_frame])
    bool keep_value_when_unsolvable;  // embed: `a` stays untouched (Watermark.cpp:164-165)
    int res_off;
    float* value_out;
    int* status_out;  // [frames]
    float* coef_out;  // host destination for 8*frames coefficients (mask-only ops)
};

// the scratch of one call of the locate family inside one allocation (loc_layout): the twiddle tables of the [pr][pc] transform, the
// frames' spectra hs [kept] (transposed; null: the call keeps none), planes a (work: h, its spectrum's way back, the map), kw (the
// key side's spectrum, transposed) and p (the product; the plane a key is laid into), the frame's e and m, and what only some calls
// have (null: not in this layout): the energy map and the per-bit maps of a wm_locate_bits call that passes none, the block records
// (wm_locate: one map's; wm_locate_keys: the two halves' of one (pair, frame), whose fold runs before the next one's map pass;
// wm_locate_bits: the bits' [frames][pairs][blocks]), the energy's block records [frames][blocks], the per-key non-zero flags.
// Every member is 8 bytes wide or one of a pair of ints: two layouts are compared as bytes
struct LocScratch {
    int pr, pc;
    float *tw_r, *tw_c, *hs, *a, *kw, *p, *e, *m, *energy, *maps;
    char *part, *epart;
    int* nz;
    size_t plane_floats;
};
// one allocation of that scratch; at: the layout on a null base that its tables were last filled for (loc_scratch)
struct LocAlloc {
    void* p = nullptr;
    size_t bytes = 0;
    LocScratch at{};
};
enum { LOC_PLAIN, LOC_BITS, LOC_KEYS, LOC_KINDS };  // wm_locate, wm_locate_bits, wm_locate_keys, each with its pooled call

struct Slot {
    hipStream_t own = nullptr, stream = nullptr;
    void* arena = nullptr;  // the one device allocation behind the scratch arrays below (alloc_slots)
    // scratch (sized for max_frames and the worst-case block count)
    double* d_gram = nullptr;    // k_gram main partials [frames][nblk][13]
    double* d_gramb = nullptr;   // k_gram border partials [frames][nbb][44]
    double* d_gramtot = nullptr; // folded sums [frames][44]
    float* d_coef = nullptr;
    int* d_status = nullptr;
    float* d_pmax = nullptr;
    double* d_pss = nullptr;
    double* d_pcorr = nullptr;
    unsigned long long* d_pdig = nullptr;   // [frames][nrec] digest records of a checking k_detect (DigCheck)
    unsigned long long* d_sdig = nullptr;   // [frames][nstrips] its strip records
    int* d_redo = nullptr;                  // [frames] frames a checking k_detect left to the redo launches
    unsigned long long* d_hocnt = nullptr;  // [2] frames trusted / redone by checked hand-overs
    EmbedScalars* d_scal = nullptr;
    float* d_smax = nullptr;       // [max_frames][nstrips] strip records of the stats sweep
    double* d_sss = nullptr;
    double* d_scorr = nullptr;     // [max_frames][nstrips][3] strip records of the detect sweep
    RawSums* d_raw = nullptr;      // [2][max_frames] raw totals of the stats / detect sweeps (band mode reads them)
    double* d_totals = nullptr;    // [max_frames][44] all-reduced Gram totals handed back by wm_band_solve
    unsigned* d_ticket = nullptr;  // [3][max_frames] last-block tickets of the Gram, stats and detect sweeps (zero between ops)
    // result records live in pinned, device-mapped host memory: the finalising kernels store them straight over
    // PCIe, so a call needs no D2H copy node and wm_sync only waits for the stream
    OpResult* h_res = nullptr;   // host view
    OpResult* d_res = nullptr;   // device view of the same memory
    float* h_coefres = nullptr;
    float* d_coefres = nullptr;
    int res_used = 0;
    std::deque<Pending> pending;
    // the device copy of the last embed's output on this slot (WM_MEM_SLOT_OUT planes name it)
    PlaneDesc last_out{};
    int last_out_frames = 0, last_out_dtype = 0;
    // fused single-frame path (wm_k_fused.hip)
    FusedScratch fz{};
    void* fz_block = nullptr;  // one allocation behind fz
    unsigned fz_epoch = 0;
    // Gram hand-over (wm_set_handover): wave + seam records [max_frames][ho_stride_max][13]; ho.valid: the last embed on this
    // slot left the tile-internal lag sums of its output (= last_out) there, for the geometry ho.lg
    // promised: the embed ran under wm_set_handover / wm_embed_detect (a WM_MEM_SLOT_OUT detector may trust the sums); else only
    // the checked hand-over of wm_detect takes them, once (used: a detector or wm_gram has taken them)
    double* d_ho = nullptr;
    float* d_hoseam = nullptr;   // [max_frames][strips - 1][rows][4]: the columns at the strip boundaries (HandOver::seam)
    unsigned long long* d_hodig = nullptr;  // [max_frames][ho_stride_max] digest records, then [max_frames] frame digests (HandOver::dig / fdig)
    struct HoInfo { bool valid = false; bool promised = false; bool used = false; LaunchGeom lg{}; int frames = 0; int stride = 0; } ho;
    // wm_embed_detect: a fused embed whose wait was deferred to the detector's record (the two launches go out back to back)
    struct PairEmbed {
        bool armed = false; int res_index = 0; bool host_out = false; bool out_overlaps_inputs = false;
        // one launch for both halves (k_fused_pair): the embed was NOT launched -- the detector's call launches both
        bool deferred = false; int mask = 0; unsigned epoch = 0; PlaneDesc xd{}, bd{}, od{};
    } pair;
    // staging for WM_MEM_HOST planes
    void* st_in = nullptr; size_t st_in_bytes = 0;
    void* st_base = nullptr; size_t st_base_bytes = 0;
    void* st_out = nullptr; size_t st_out_bytes = 0;
    // wm_detect_keys: per-(frame, key) partial records of k_detect_keys (grown on demand)
    void* keys_part = nullptr; size_t keys_part_bytes = 0;
    // wm_embed_keys: per-(frame, key) stats records and strengths of k_stats_keys (grown on demand)
    void* ekeys_part = nullptr; size_t ekeys_part_bytes = 0;
    // wm_detect_tiles: per-lane records of k_detect_tiles [frames][nsegs][nstrips][3][64] f32 (grown on demand)
    void* tiles_rec = nullptr; size_t tiles_rec_bytes = 0;
    // wm_detect_keys_tiles: per-lane records of k_detect_keys_tiles [frames][ngroups][nsegs][nstrips][2 G + 1][64] f32 (grown on demand)
    void* keys_tiles_rec = nullptr; size_t keys_tiles_rec_bytes = 0;
    // wm_embed_signs / wm_detect_bits: the tables of the slot's un-synced calls (sign tables, tile lists per bit).  A call copies
    // its table into the pinned host arena and queues the upload into the device arena at the same offset, so every queued call
    // keeps its own; wm_sync resets both, table_room grows them on demand
    void* tab_host = nullptr; void* tab_dev = nullptr; size_t tab_bytes = 0, tab_used = 0;
    // wm_detect_bits: what its tile fold writes (sums [frames][ny * nx][3] f64, records [frames], map [frames][ny * nx] f32; grown on demand)
    void* bits_scr = nullptr; size_t bits_scr_bytes = 0;
    // wm_embed16 / wm_detect16: the f32 planes X (the unpacked samples) and Y (the embed's output, what WM_MEM_SLOT_OUT then names),
    // dense in staged_layout's form (grown on demand)
    void* x16 = nullptr; size_t x16_bytes = 0;
    void* y16 = nullptr; size_t y16_bytes = 0;
    // wm_quality: k_quality's records [planes][nsegs][ngroups][3] f64 and the folds' [planes][nsegs][nx][3], then the tile sums [planes][ny * nx][5] f64 of a call that
    // passes no sums_dev (grown on demand)
    void* qual_scr = nullptr; size_t qual_scr_bytes = 0;
    // the locate family's scratch (LocScratch; grown on demand), one allocation per call kind: calls of different kinds alternate
    // on a slot without moving each other's layout, which would make every one of them wait for the stream
    LocAlloc loc[LOC_KINDS];
};

struct ProfRec { int kid; hipEvent_t a, b; bool first; };  // first: the sweep's first launch (counts the call)

}  // namespace

struct wm_ctx {
    int device = 0;
    int rows = 0, cols = 0, p = 3;
    float psnr = 0.f, sF = 0.f;
    std::shared_ptr<WShared> w;
    int nslots = 0, max_frames = 1;
    int rps_override = 0;
    int ncu = 0;
    int fused_mode = env_flag("WM_FUSED", true);  // 1: synchronous one-frame calls take the fused kernels when the shape allows (wm_set_fused)
    // wm_embed_detect on one image: 1 = ONE launch for both halves (k_fused_pair).  Off unless WM_FUSED_PAIR=1: measured 1.5-2 us
    // SLOWER than the two launches back to back at 4K, equal at 1080p
    int fused_pair = env_flag("WM_FUSED_PAIR", false);
    FusedGeom fg{};
    unsigned long long fused_fallbacks = 0;  // fused launches that timed out and were re-run on the sweeps
    unsigned long long fused_lock_skips = 0; // synchronous calls that took the sweeps because another process held the device's lock
    // after a fallback the fused path is skipped for `fused_backoff` calls (8, doubling up to 4096 while the re-probes keep
    // failing; a probe that succeeds clears it): a device on which the workgroups cannot all be resident -- another
    // process's kernels, a CU mask -- costs one time-out per window, not one per call
    int fused_backoff = 0, fused_skip = 0;
    int handover = 0;        // wm_set_handover
    int handover_verify = env_flag("WM_HANDOVER_VERIFY", false);  // debug: re-check every hand-over
    int pair_handover = 0;   // 1 inside wm_embed_detect: its detector reads the embed's output by construction
    int checked_handover = env_flag("WM_CHECKED_HANDOVER", true);  // wm_set_checked_handover
    int pair_mode = 0;       // 1 inside wm_embed_detect: the fused embed does not wait (and the caller holds the FusedGuard)
    int fused_lock_fd = -1;  // per-device lock file shared with other processes (FusedGuard), -1: none
    int max_nblk = 0, max_nrec = 0;  // per-frame capacity of the slots' partial-record arrays (alloc_slots)
    // row band of a larger image (wm_band_configure): planes are the band plus halo rows, sums and stores cover the owned rows
    int band_lo = 0, band_hi = 0;       // owned rows in plane coordinates; band_hi == 0: no band (the whole plane is owned)
    long long band_rows_global = 0;     // rows of the whole image (the strength needs sqrt(N) of the whole image)
    std::vector<Slot> slots;
    std::string last_error;
    bool prof = false;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_free;
    uint64_t prof_n[K_COUNT] = {0};
    double prof_ms[K_COUNT] = {0};
    ~wm_ctx();  // releases streams, scratch and events (also on the error paths of wm_create / wm_clone)
};

// a bank of watermark keys (wm_keys_*): K planes of one shape on one device, one allocation [K][rows][cols]
struct wm_keys {
    int device = 0;
    int rows = 0, cols = 0, nkeys = 0;
    float* d = nullptr;
    ~wm_keys() { if (d) { (void)hipSetDevice(device); (void)hipFree(d); } }
};

namespace {

// a result record as the device left it in mapped host memory: ONE 64-bit acquire load, so status and value belong together
// and nothing that follows is read ahead of it
OpResult load_record(const OpResult* rec)
{
    static_assert(sizeof(OpResult) == 8 && sizeof(std::atomic<uint64_t>) == 8, "the record is one 8-byte word");
    const uint64_t v = reinterpret_cast<const std::atomic<uint64_t>*>(rec)->load(std::memory_order_acquire);
    OpResult r;
    std::memcpy(&r, &v, 8);
    return r;
}

// Wait for a fused launch by polling the result record its folding workgroup writes to device-mapped pinned memory (ONE 8-byte
// store: status and value; embed: after every byte of the output has been written through to memory: load_record).  Returns
// true when the record arrived (copy in *got).  A launch whose hand-off timed out ends WITHOUT writing the record: once
// the call is older than a normal one (150 us) the stream is queried every ~20 us, and a finished stream with the record
// still pending returns false at once (it used to spin for 200 ms).  hipStreamSynchronize costs 5.5 us more per call than
// this poll (tools/ubench/launch_sync.hip), so the normal path never touches the stream.
bool poll_record(const OpResult* rec, int pending, hipStream_t stream, OpResult* got)
{
    auto look = [&]() {
        *got = load_record(rec);
        return got->status != pending;
    };
    const auto t0 = std::chrono::steady_clock::now();
    auto next_query = std::chrono::microseconds(150);
    for (unsigned spins = 0;; ++spins) {
        if (look()) return true;
        if ((spins & 0xff) != 0xff) continue;
        const auto dt = std::chrono::steady_clock::now() - t0;
        if (dt < next_query) continue;
        next_query = std::chrono::duration_cast<std::chrono::microseconds>(dt) + std::chrono::microseconds(20);
        if (hipStreamQuery(stream) != hipErrorNotReady) return look();  // the launch has ended (or failed): the record is final
        if (dt > std::chrono::milliseconds(500)) return false;             // backstop; the caller synchronises the stream
    }
}

}  // namespace
namespace wmk {
LaunchProf*& launch_prof_slot()
{
    static thread_local LaunchProf* slot = nullptr;
    return slot;
}
}  // namespace wmk
namespace {

int fail(wm_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->last_error = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                           \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(ctx, WM_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

int ceil_div(int a, int b) { return (a + b - 1) / b; }
// strips the per-strip record and ticket arrays are sized for: k_detect's overlapped strips are 248 columns apart
// (wm_march.hpp OV_STRIDE), every other sweep's 256
int strips_alloc(int cols) { return ceil_div(cols, 248) + 1; }  // (+1: the generic strip of a width that is not a multiple of 4)
int border_blocks(int rows, int cols, int frames = 1);

// sqrt(N) of Watermark.cpp:170: N counts the pixels of the whole image (a row band knows the image's row count)
double sqrt_n(const wm_ctx* ctx)
{
    const double rows = ctx->band_hi > 0 ? (double)ctx->band_rows_global : (double)ctx->rows;
    return sqrt(rows * (double)ctx->cols);
}

// geometry of one launch: strips of 256 columns, segments of rps rows, 4 segments per block
LaunchGeom make_geom(const wm_ctx* ctx, int frames, int mask = WM_MASK_ME)
{
    const int TARGET_WAVES = mask == WM_MASK_NVF ? TARGET_WAVES_NVF : TARGET_WAVES_ME;
    LaunchGeom lg;
    lg.rows = ctx->rows; lg.cols = ctx->cols;
    lg.nstrips = ceil_div(ctx->cols, 256);
    lg.nfull = ctx->cols / 256;
    lg.row_lo = ctx->band_hi > 0 ? ctx->band_lo : 0;
    lg.row_hi = ctx->band_hi > 0 ? ctx->band_hi : ctx->rows;
    const int owned = lg.row_hi - lg.row_lo;
    int rps = ctx->rps_override;
    if (rps <= 0) {
        // enough wavefronts to fill 256 CUs several times over, but segments long enough to amortise their halo rows
        // (2 of rps for the 3x3 sweeps, 4 of rps for k_detect): 8 .. 48 rows, measured flat from 40 to 64 at 4K
        const long long want = (long long)owned * lg.nstrips * frames;
        rps = (int)((want + TARGET_WAVES - 1) / TARGET_WAVES);
        if (rps < 8) rps = 8;
        if (rps > 48) rps = 48;
        // balance: blocks own 4 segments, so make the segments equal parts of a whole number of blocks
        const int groups = ceil_div(owned, 4 * rps);
        rps = ceil_div(owned, 4 * groups);
        if (rps < 1) rps = 1;
    }
    if (rps > owned) rps = owned;
    lg.rps = rps;
    lg.nsegs = ceil_div(owned, rps);
    lg.nblk = lg.nstrips * ceil_div(lg.nsegs, 4);
    lg.nbb = border_blocks(ctx->rows, ctx->cols, frames);
    return lg;
}

// blocks of 256 threads for the border frame of k_gram: 5 full rows + 6 side columns (or everything for tiny images)
int border_blocks(int rows, int cols, int frames)
{
    const bool core_empty = rows < 4 || cols < 5;
    const long long nfull = core_empty ? rows + 2 : 5;
    const long long cpr = (cols + 2 + 63) / 64;
    const long long rpc = core_empty ? 0 : (rows - 3 + 63) / 64;
    long long nb = (nfull * cpr + 6 * rpc + 7) / 8;  // 2 chunks per wave: the pass is latency-bound, so short waves, many of them
    // ... but every block leaves a 44-sum record that the frame's last block folds before it can solve, and that fold
    // is the exposed tail of the launch: at most 32 blocks per frame (4 chunks per wave at 4K), 16 in batched launches,
    // where the other frames' blocks hide the longer border waves (4K: k_gram 7.6 -> 7.3 us per frame; one frame per
    // launch loses 7 % with 16)
    const long long cap = frames >= 8 ? 16 : 32;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    return (int)nb;
}

// make_geom + the guarantee the kernels index by: a launch's per-block / per-wave record counts fit the slot's arrays
int geom_checked(wm_ctx* ctx, int frames, int mask, LaunchGeom* lg)
{
    *lg = make_geom(ctx, frames, mask);
    if (lg->nblk > ctx->max_nblk || lg->nstrips * lg->nsegs > ctx->max_nrec || lg->nbb > border_blocks(ctx->rows, ctx->cols))
        return fail(ctx, WM_ERR_RUNTIME, "launch geometry exceeds the slot's partial-record arrays (nblk " + std::to_string(lg->nblk) + "/" +
                                             std::to_string(ctx->max_nblk) + ", nrec " + std::to_string(lg->nstrips * lg->nsegs) + "/" +
                                             std::to_string(ctx->max_nrec) + ")");
    return WM_OK;
}

int worst_nsegs(int rows, int rps_override);
int worst_nblk(int rows, int cols, int rps_override)
{
    return strips_alloc(cols) * ceil_div(worst_nsegs(rows, rps_override), 4);
}

void free_slot(Slot& s)
{
    if (s.own) (void)hipStreamDestroy(s.own);
    (void)hipFree(s.arena);  // (d_gram ... d_ticket point into it)
    if (s.h_res) (void)hipHostFree(s.h_res);
    if (s.h_coefres) (void)hipHostFree(s.h_coefres);
    (void)hipFree(s.st_in); (void)hipFree(s.st_base); (void)hipFree(s.st_out); (void)hipFree(s.fz_block); (void)hipFree(s.d_ho); (void)hipFree(s.d_hoseam);
    (void)hipFree(s.d_hodig); (void)hipFree(s.keys_part); (void)hipFree(s.ekeys_part); (void)hipFree(s.tiles_rec); (void)hipFree(s.keys_tiles_rec);
    if (s.tab_host) (void)hipHostFree(s.tab_host);
    (void)hipFree(s.tab_dev); (void)hipFree(s.bits_scr); (void)hipFree(s.x16); (void)hipFree(s.y16); (void)hipFree(s.qual_scr);
    for (LocAlloc& al : s.loc) (void)hipFree(al.p);
    s = Slot();
}

// last-block / last-wave tickets of a slot: [3][max_frames] frame-level (Gram, stats, detect) + [2][max_frames][nstrips]
// strip-level (stats, detect)
size_t ticket_words(const wm_ctx* ctx)
{
    return ((size_t)3 * ctx->max_frames + (size_t)2 * ctx->max_frames * strips_alloc(ctx->cols)) * TKS;  // one counter per 128-byte line
}
unsigned* strip_tickets(const wm_ctx* ctx, const Slot& s, int which)  // which: 0 stats, 1 detect
{
    return s.d_ticket + ((size_t)3 * ctx->max_frames + (size_t)which * ctx->max_frames * strips_alloc(ctx->cols)) * TKS;
}

// per-wave partial records of the stats / detect sweeps: strips x segments, for the LARGEST segment count make_geom can
// produce.  make_geom starts from rps0 >= 8 rows and then balances: groups = ceil(owned / (4 rps0)), rps = ceil(owned /
// (4 groups)), which may end below 8, so nsegs = ceil(owned / rps) <= 4 groups <= 4 ceil(rows / 32) (not ceil(rows / 8)).
int worst_nsegs(int rows, int rps_override)
{
    if (rps_override > 0) return ceil_div(rows, rps_override > rows ? rows : rps_override);
    return 4 * ceil_div(rows, 32);
}
int worst_nrec(int rows, int cols, int rps_override) { return strips_alloc(cols) * worst_nsegs(rows, rps_override); }

// Gram hand-over: records per frame of a slot's hand-over array = the wave records + the seam-block records of the largest geometry
int ho_stride_max(const wm_ctx* ctx) { return ctx->max_nrec + 2 * ((ctx->max_nrec + 3) / 4) + 2; }
// all arrays of a slot or none: a slot with records but no seam array would send k_embed<HO>'s edge lanes to address 0
bool ho_ready(const Slot& s) { return s.d_ho && s.d_hoseam && s.d_hodig; }
int ho_alloc_slot(wm_ctx* ctx, Slot& s)
{
    if (ho_ready(s)) return WM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    s.ho.valid = false;
    (void)hipFree(s.d_ho); (void)hipFree(s.d_hoseam); (void)hipFree(s.d_hodig);
    s.d_ho = nullptr; s.d_hoseam = nullptr; s.d_hodig = nullptr;
    void* rec = nullptr; void* seam = nullptr; void* dig = nullptr;
    hipError_t e = hipMalloc(&rec, (size_t)ctx->max_frames * ho_stride_max(ctx) * 13 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&seam, (size_t)ctx->max_frames * ceil_div(ctx->cols, 256) * ctx->rows * 4 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dig, (size_t)ctx->max_frames * (ho_stride_max(ctx) + 1) * sizeof(unsigned long long));
    if (e != hipSuccess) {
        (void)hipFree(rec); (void)hipFree(seam); (void)hipFree(dig);
        (void)hipGetLastError();
        return fail(ctx, WM_ERR_ALLOC, std::string("hand-over arrays: ") + hipGetErrorString(e));
    }
    s.d_ho = (double*)rec; s.d_hoseam = (float*)seam; s.d_hodig = (unsigned long long*)dig;
    return WM_OK;
}
int ho_alloc(wm_ctx* ctx)
{
    for (auto& s : ctx->slots) {
        s.ho.valid = false;
        const int rc = ho_alloc_slot(ctx, s);
        if (rc != WM_OK) return rc;
    }
    return WM_OK;
}
HandOver handover_of(const wm_ctx* ctx, const Slot& s, int stride)
{
    return HandOver{s.d_ho, stride, s.d_hoseam, s.d_hodig, s.d_hodig + (size_t)ctx->max_frames * ho_stride_max(ctx)};
}

int alloc_slots(wm_ctx* ctx, int nslots, int max_frames)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // a slot that runs on the caller's stream (wm_set_stream) keeps it across the rebuild, as long as its index still exists: the
    // ordering against the caller's collectives must not end because a rank tunes rps or reinitialises
    std::vector<hipStream_t> caller_stream;
    for (auto& s : ctx->slots) caller_stream.push_back(s.stream != s.own ? s.stream : nullptr);
    for (auto& s : ctx->slots) free_slot(s);
    ctx->slots.clear();
    ctx->nslots = nslots; ctx->max_frames = max_frames;
    ctx->max_nblk = worst_nblk(ctx->rows, ctx->cols, ctx->rps_override);
    ctx->max_nrec = worst_nrec(ctx->rows, ctx->cols, ctx->rps_override);
    ctx->slots.resize(nslots);
    const size_t nb = (size_t)ctx->max_nblk * max_frames;
    if (ctx->ncu == 0 && hipDeviceGetAttribute(&ctx->ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) ctx->ncu = 0;
    ctx->fg = fused_geometry(ctx->rows, ctx->cols, ctx->ncu);
    if (ctx->fg.fusable && ctx->fused_lock_fd < 0 && env_flag("WM_FUSED_XPROC_LOCK", true)) {
        char bus[64] = "dev";
        if (hipDeviceGetPCIBusId(bus, sizeof bus, ctx->device) != hipSuccess) snprintf(bus, sizeof bus, "ordinal%d", ctx->device);
        for (char* q = bus; *q; ++q) if (*q == ':' || *q == '/' || *q == '.') *q = '_';
        // a lock directory that every user of the machine shares: /run/lock where it exists, else TMPDIR / /tmp.  The file is
        // opened read-only (flock works on read-only descriptors, so a file another user created with any umask can still be
        // locked), never through a symbolic link, and made 0666 by whoever creates it
        const char* dir = getenv("WM_FUSED_LOCK_DIR") ? getenv("WM_FUSED_LOCK_DIR")
                          : access("/run/lock", W_OK | X_OK) == 0 ? "/run/lock" : (getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp");
        const std::string path = std::string(dir) + "/wm_fused_" + bus + ".lock";
        ctx->fused_lock_fd = open(path.c_str(), O_CREAT | O_RDONLY | O_NOFOLLOW | O_CLOEXEC, 0666);  // (-1: no cross-process serialisation, the bounded spins still hold)
        if (ctx->fused_lock_fd >= 0) (void)fchmod(ctx->fused_lock_fd, 0666);  // (fails quietly when the file is another user's: it is 0666 already)
    }
    for (auto& s : ctx->slots) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&s.own, hipStreamNonBlocking));
        s.stream = s.own;
        // The slot's device scratch is ONE allocation (a multiple of 2 MiB, the arrays on 4 KiB boundaries inside it), not a
        // dozen small ones: small hipMallocs are sub-allocated wherever the runtime's pools have room, and where the partial
        // records and ticket counters of the fold tails landed decided 10-20 % of k_gram / k_detect -- the first context a
        // process created ran them in 120 / 130 us, the second and third in 105 / 110 us, same code, same frames
        // (tools/data_probe2.py).  An arena of its own gets its own large, aligned mapping, the same for every context.
        const size_t nr = (size_t)ctx->max_nrec * max_frames;
        const size_t nsr = (size_t)max_frames * strips_alloc(ctx->cols);
        struct Part { void** p; size_t bytes; };
        const Part parts[] = {
            {(void**)&s.d_gram, nb * 13 * sizeof(double)},
            {(void**)&s.d_gramb, (size_t)border_blocks(ctx->rows, ctx->cols) * max_frames * NGRAM * sizeof(double)},
            {(void**)&s.d_gramtot, (size_t)max_frames * NGRAM * sizeof(double)},
            {(void**)&s.d_coef, (size_t)max_frames * 8 * sizeof(float)},
            {(void**)&s.d_status, (size_t)max_frames * sizeof(int)},
            {(void**)&s.d_pmax, nr * sizeof(float)},
            {(void**)&s.d_pss, nr * sizeof(double)},
            {(void**)&s.d_pcorr, nr * 3 * sizeof(double)},
            {(void**)&s.d_pdig, nr * sizeof(unsigned long long)},
            {(void**)&s.d_sdig, nsr * sizeof(unsigned long long)},
            {(void**)&s.d_redo, (size_t)max_frames * sizeof(int)},
            {(void**)&s.d_hocnt, 2 * sizeof(unsigned long long)},
            {(void**)&s.d_scal, (size_t)max_frames * sizeof(EmbedScalars)},
            {(void**)&s.d_smax, nsr * sizeof(float)},
            {(void**)&s.d_sss, nsr * sizeof(double)},
            {(void**)&s.d_scorr, nsr * 3 * sizeof(double)},
            {(void**)&s.d_raw, (size_t)2 * max_frames * sizeof(RawSums)},
            {(void**)&s.d_totals, (size_t)max_frames * NGRAM * sizeof(double)},
            {(void**)&s.d_ticket, ticket_words(ctx) * sizeof(unsigned)},
        };
        auto up = [](size_t v, size_t a) { return (v + a - 1) / a * a; };
        size_t total = 0;
        for (const Part& pt : parts) total += up(pt.bytes, 4096);
        total = up(total, (size_t)2 << 20);
        HIPCHK(ctx, hipMalloc(&s.arena, total));
        HIPCHK(ctx, hipMemsetAsync(s.arena, 0, total, s.stream));  // (tickets and status words start at zero)
        {
            char* q = (char*)s.arena;
            for (const Part& pt : parts) { *pt.p = q; q += up(pt.bytes, 4096); }
        }
        HIPCHK(ctx, hipHostMalloc((void**)&s.h_res, (size_t)RES_CAP * sizeof(OpResult), hipHostMallocMapped));
        HIPCHK(ctx, hipHostMalloc((void**)&s.h_coefres, (size_t)RES_CAP * 8 * sizeof(float), hipHostMallocMapped));
        HIPCHK(ctx, hipHostGetDevicePointer((void**)&s.d_res, s.h_res, 0));
        HIPCHK(ctx, hipHostGetDevicePointer((void**)&s.d_coefres, s.h_coefres, 0));
        if (ctx->fg.fusable) {
            // [27 counter lines | 32 granules | workgroup records | stamps]
            const size_t G = (size_t)ctx->fg.G;
            const bool want_stamps = getenv("WM_FUSED_STAMPS") != nullptr;
            const size_t ndbl = G * (2 * (13 + NGRAM) + 4 + 8 + 1) + (want_stamps ? G * 16 + 16 + NGRAM : 0);
            const size_t bytes = up(FUSED_CNT_BYTES + 64 * 8 + ndbl * sizeof(double), (size_t)2 << 20);  // (an arena of its own, like the sweeps' scratch)
            HIPCHK(ctx, hipMalloc(&s.fz_block, bytes));
            HIPCHK(ctx, hipMemsetAsync(s.fz_block, 0, bytes, s.stream));
            char* b = (char*)s.fz_block;
            s.fz.cnt = (unsigned*)b;
            s.fz.gran = (unsigned long long*)(b + FUSED_CNT_BYTES);
            double* d = (double*)(b + FUSED_CNT_BYTES + 64 * 8);
            s.fz.pmain = d; d += 2 * G * (13 + NGRAM);
            s.fz.gstat = (unsigned long long*)d; d += G * 4;
            s.fz.gcorr = (unsigned long long*)d; d += G * 8;
            s.fz.gdone = (unsigned long long*)d; d += G;
            s.fz.stamps = want_stamps ? (unsigned long long*)d : nullptr;
            s.fz.dbg = getenv("WM_FUSED_DBG") ? atoi(getenv("WM_FUSED_DBG")) : 0;  // development / test switches of the fused kernels
            if (!want_stamps) s.fz.dbg &= ~3;  // bits 0, 1 give wrong results (timing experiments): only with the stamps switched on
        }
    }
    HIPCHK(ctx, hipDeviceSynchronize());  // (the scratch is cleared before any stream, the caller's included, can reach it)
    for (size_t i = 0; i < ctx->slots.size() && i < caller_stream.size(); ++i)
        if (caller_stream[i]) ctx->slots[i].stream = caller_stream[i];
    if (ctx->handover) {
        const int rc = ho_alloc(ctx);
        if (rc != WM_OK) { ctx->handover = 0; return rc; }
    }
    return WM_OK;
}

int upload_w(wm_ctx* ctx, const float* w)
{
    auto ws = std::make_shared<WShared>();
    ws->n = (size_t)ctx->rows * ctx->cols;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc((void**)&ws->d_w, ws->n * sizeof(float)));
    HIPCHK(ctx, hipMemcpy(ws->d_w, w, ws->n * sizeof(float), hipMemcpyHostToDevice));
    ctx->w = ws;
    return WM_OK;
}

// loadRandomMatrix (Watermark.cpp:62-75): raw f32 file, size must be rows*cols*4
int read_w_file(wm_ctx* ctx, const char* path, int rows, int cols, std::vector<float>& out)
{
    if (!path) return fail(ctx, WM_ERR_BAD_ARG, "null W path");
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) return fail(ctx, WM_ERR_W_OPEN, std::string("Error opening '") + path + "' file for Random noise W array");
    f.seekg(0, std::ios::end);
    const long long total = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    if ((long long)rows * cols * (long long)sizeof(float) != total)
        return fail(ctx, WM_ERR_W_SIZE,
                    "Error: W file total elements != image dimensions! W file total elements: " +
                        std::to_string(total / (long long)sizeof(float)) + ", Image width: " + std::to_string(cols) +
                        ", Image height: " + std::to_string(rows));
    out.resize((size_t)rows * cols);
    f.read(reinterpret_cast<char*>(out.data()), total);
    if (!f) return fail(ctx, WM_ERR_W_OPEN, std::string("short read on '") + path + "'");
    return WM_OK;
}

int check_params(int rows, int cols, int p, float psnr)
{
    if (p != 3 && p != 5 && p != 7 && p != 9) return WM_ERR_BAD_P;
    if (!(psnr > 0.0f)) return WM_ERR_PSNR;
    if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768) return WM_ERR_BAD_ARG;
    return WM_OK;
}

// W generated on the device from a seed (wm_create_generated; the current device is the context's)
int generate_w(wm_ctx* ctx, uint32_t seed)
{
    auto ws = std::make_shared<WShared>();
    ws->n = (size_t)ctx->rows * ctx->cols;
    if (hipMalloc((void**)&ws->d_w, ws->n * sizeof(float)) != hipSuccess) return WM_ERR_ALLOC;
    launch_gen_w(nullptr, ws->d_w, ctx->rows, ctx->cols, seed);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return WM_ERR_RUNTIME;
    ctx->w = ws;
    return WM_OK;
}

// the device a create call names becomes the current one; an invalid ordinal means the default, 0 (main.cpp:73-78)
int choose_device(int* device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return WM_ERR_NO_DEVICE;
    if (*device < 0 || *device >= ndev) *device = 0;
    return hipSetDevice(*device) == hipSuccess ? WM_OK : WM_ERR_NO_DEVICE;
}

// wm_create / wm_create_generated: they differ in how W reaches the device (generated there from the seed, or w uploaded)
int create_ctx(wm_ctx** out, int device, int rows, int cols, int p, float psnr, bool generated, const float* w, uint32_t seed)
{
    if (!out) return WM_ERR_BAD_ARG;
    *out = nullptr;
    int rc = check_params(rows, cols, p, psnr);
    if (rc != WM_OK) return rc;
    if (!generated && !w) return WM_ERR_BAD_ARG;
    if ((rc = choose_device(&device)) != WM_OK) return rc;
    std::unique_ptr<wm_ctx> ctx(new wm_ctx);
    ctx->device = device; ctx->rows = rows; ctx->cols = cols; ctx->p = p; ctx->psnr = psnr;
    ctx->sF = 255.0f / sqrtf(powf(10.0f, psnr / 10.0f));  // Watermark.cpp:22
    if ((rc = generated ? generate_w(ctx.get(), seed) : upload_w(ctx.get(), w)) != WM_OK) return rc;
    if ((rc = alloc_slots(ctx.get(), 2, 1)) != WM_OK) return rc;
    *out = ctx.release();
    return WM_OK;
}

// the aligned path addresses a plane as a buffer with 32-bit byte offsets (wm_device.hpp make_rsrc): one plane must stay
// below 4 GiB (a 32768 x 32768 f32 plane is not: it takes the generic path)
bool fits_32bit(int rows, long long pitch, int dtype)
{
    return (long long)rows * pitch * (dtype == WM_F32 ? 4 : dtype == WM_U16 ? 2 : 1) < (1LL << 32) - 4096;
}

bool vec_ok(const void* p, int rows, long long pitch, long long fstride, long long cstride, int dtype, int frames, int channels)
{
    // f32 planes: the 16-byte row loads and stores of the aligned path only need 4-byte alignment (measured on gfx950: values
    // correct, 2-5 % off the rate of naturally aligned accesses, tools/ubench/unaligned.hip), so a dense plane whose width is not
    // a multiple of 4 -- every other row 8 bytes off a 16-byte boundary -- still takes the aligned path on its full strips
    // instead of the LDS re-lay.  u8 planes keep their rule: a lane's 4 pixels are one dword
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a % 4) return false;
    if (!fits_32bit(rows, pitch, dtype)) return false;
    if (dtype == WM_F32) return true;
    if (pitch % 4) return false;
    if (frames > 1 && fstride % 4) return false;
    if (channels > 1 && cstride % 4) return false;
    return true;
}

int check_plane(wm_ctx* ctx, const wm_plane* pl, int frames_expected, bool allow_rgb, const char* what, bool allow_slot_out = false)
{
    if (!pl || (!pl->data && pl->mem != WM_MEM_SLOT_OUT)) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": null plane");
    // WM_MEM_SLOT_OUT names the slot's last grey output: an INPUT plane (wm.h).  Anywhere else it has no address behind it
    if (pl->mem == WM_MEM_SLOT_OUT && !allow_slot_out)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": WM_MEM_SLOT_OUT is valid for the grey input plane only");
    if (pl->rows != ctx->rows || pl->cols != ctx->cols)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": plane is " + std::to_string(pl->rows) + "x" + std::to_string(pl->cols) +
                                             ", engine was initialised for " + std::to_string(ctx->rows) + "x" + std::to_string(ctx->cols));
    if (pl->dtype != WM_F32 && pl->dtype != WM_U8) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": bad dtype");
    if (pl->mem != WM_MEM_DEVICE && pl->mem != WM_MEM_HOST && pl->mem != WM_MEM_SLOT_OUT) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": bad mem");
    if (pl->channels != 1 && !(allow_rgb && pl->channels == 3)) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": channels must be 1" + (allow_rgb ? " or 3" : ""));
    if (pl->pitch < pl->cols) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": pitch < cols");
    if (pl->frames < 1 || pl->frames > ctx->max_frames)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": frames=" + std::to_string(pl->frames) + " exceeds wm_configure max_frames=" + std::to_string(ctx->max_frames));
    if (frames_expected > 0 && pl->frames != frames_expected) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": frame count mismatch");
    if (pl->channels > 1 && pl->channel_stride < (int64_t)pl->rows * pl->pitch) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": channel_stride too small");
    if (pl->frames > 1 && pl->frame_stride < (int64_t)(pl->channels - 1) * (pl->channels > 1 ? pl->channel_stride : 0) + (int64_t)pl->rows * pl->pitch)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": frame_stride too small (frames overlap)");
    return WM_OK;
}

size_t elem_size(int dtype) { return dtype == WM_F32 ? 4 : dtype == WM_U16 ? 2 : 1; }

PlaneDesc desc_device(const wm_plane* pl)
{
    PlaneDesc d;
    d.p = pl->data; d.pitch = pl->pitch; d.fstride = pl->frames > 1 ? pl->frame_stride : 0;
    d.cstride = pl->channels > 1 ? pl->channel_stride : 0;
    d.dtype = pl->dtype; d.channels = pl->channels;
    // a u16 plane (the 16-bit conversions only, check_plane refuses it elsewhere): four samples of a lane are one 8-byte access when
    // the base is a multiple of 4 bytes and the pitch and the used strides are even
    if (pl->dtype == WM_U16) d.aligned = reinterpret_cast<uintptr_t>(pl->data) % 4 == 0 && d.pitch % 2 == 0 && d.fstride % 2 == 0 && d.cstride % 2 == 0 ? 1 : 0;
    else d.aligned = vec_ok(pl->data, pl->rows, d.pitch, d.fstride, d.cstride, pl->dtype, pl->frames, pl->channels) ? 1 : 0;
    return d;
}

// dense device staging layout for a host plane: pitch = cols rounded up to 4 elements
struct Staged { PlaneDesc d; size_t bytes; long long pitch; };
Staged staged_layout(const wm_plane* pl)
{
    Staged s;
    s.pitch = (pl->cols + 3) & ~3LL;
    const long long plane = s.pitch * pl->rows;
    s.d.pitch = s.pitch; s.d.cstride = plane; s.d.fstride = plane * pl->channels;
    s.d.dtype = pl->dtype; s.d.channels = pl->channels; s.d.aligned = fits_32bit(pl->rows, s.pitch, pl->dtype) ? 1 : 0; s.d.p = nullptr;
    s.bytes = (size_t)plane * pl->channels * pl->frames * elem_size(pl->dtype);
    return s;
}

// grow-on-demand device scratch.  alloc_code: what an allocation that does not fit returns (the calls whose wm.h text promises
// WM_ERR_ALLOC pass it; the others report it like any other runtime failure)
int ensure(wm_ctx* ctx, void** buf, size_t* have, size_t need, int alloc_code = WM_ERR_RUNTIME)
{
    if (*have >= need) return WM_OK;
    if (*buf) HIPCHK(ctx, hipFree(*buf));
    *buf = nullptr; *have = 0;
    const hipError_t e = hipMalloc(buf, need);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
        return fail(ctx, alloc_code, "hipMalloc(buf, need): " + std::string(hipGetErrorString(e)) + " (" + std::to_string(need) + " bytes of scratch)");
    }
    *have = need;
    return WM_OK;
}

// `bytes` of the slot's table arenas for one call (Slot::tab_host / tab_dev): the call fills *host and table_upload queues the
// copy to *dev.  The arenas are reset by wm_sync; a call that does not fit waits for the slot's stream (the queued calls still
// read their tables), then for the device (hipFree), and starts a larger pair
int table_room(wm_ctx* ctx, Slot& s, size_t bytes, void** host, void** dev)
{
    bytes = (bytes + 255) & ~(size_t)255;
    if (s.tab_used + bytes > s.tab_bytes) {
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        const size_t need = std::max(std::max(2 * s.tab_bytes, bytes), (size_t)65536);
        if (s.tab_host) HIPCHK(ctx, hipHostFree(s.tab_host));
        s.tab_host = nullptr;
        if (s.tab_dev) HIPCHK(ctx, hipFree(s.tab_dev));
        s.tab_dev = nullptr; s.tab_bytes = 0; s.tab_used = 0;
        if (hipHostMalloc(&s.tab_host, need) != hipSuccess || hipMalloc(&s.tab_dev, need) != hipSuccess) {
            (void)hipGetLastError();
            if (s.tab_host) (void)hipHostFree(s.tab_host);
            s.tab_host = nullptr; s.tab_dev = nullptr;
            return fail(ctx, WM_ERR_ALLOC, "table arenas: " + std::to_string(need) + " bytes");
        }
        s.tab_bytes = need;
    }
    *host = (char*)s.tab_host + s.tab_used; *dev = (char*)s.tab_dev + s.tab_used;
    s.tab_used += bytes;
    return WM_OK;
}
int table_upload(wm_ctx* ctx, Slot& s, const void* host, void* dev, size_t bytes)
{
    HIPCHK(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s.stream));
    return WM_OK;
}

// host plane -> staging (H2D), every (frame, channel) plane as one 2D copy (de-pitching like main.cpp:348-353)
int stage_in(wm_ctx* ctx, Slot& s, const wm_plane* pl, void* dst, const Staged& st)
{
    const size_t es = elem_size(pl->dtype);
    for (int f = 0; f < pl->frames; ++f)
        for (int ch = 0; ch < pl->channels; ++ch) {
            const char* src = (const char*)pl->data + ((size_t)f * (pl->frames > 1 ? pl->frame_stride : 0) + (size_t)ch * (pl->channels > 1 ? pl->channel_stride : 0)) * es;
            char* d = (char*)dst + ((size_t)f * st.d.fstride + (size_t)ch * st.d.cstride) * es;
            HIPCHK(ctx, hipMemcpy2DAsync(d, st.pitch * es, src, pl->pitch * es, pl->cols * es, pl->rows, hipMemcpyHostToDevice, s.stream));
        }
    return WM_OK;
}
int stage_out(wm_ctx* ctx, Slot& s, const wm_plane* pl, const void* src, const Staged& st)
{
    const size_t es = elem_size(pl->dtype);
    for (int f = 0; f < pl->frames; ++f)
        for (int ch = 0; ch < pl->channels; ++ch) {
            char* d = (char*)pl->data + ((size_t)f * (pl->frames > 1 ? pl->frame_stride : 0) + (size_t)ch * (pl->channels > 1 ? pl->channel_stride : 0)) * es;
            const char* sp = (const char*)src + ((size_t)f * st.d.fstride + (size_t)ch * st.d.cstride) * es;
            HIPCHK(ctx, hipMemcpy2DAsync(d, pl->pitch * es, sp, st.pitch * es, pl->cols * es, pl->rows, hipMemcpyDeviceToHost, s.stream));
        }
    return WM_OK;
}

// a caller's own plane as the kernels address it: a device plane described, a host plane staged into the slot's buffer *buf (grown
// on demand) and described there
int resolve_plane(wm_ctx* ctx, Slot& s, const wm_plane* pl, void** buf, size_t* have, PlaneDesc* d)
{
    if (pl->mem != WM_MEM_HOST) { *d = desc_device(pl); return WM_OK; }
    const Staged st = staged_layout(pl);
    int rc = ensure(ctx, buf, have, st.bytes);
    if (rc != WM_OK) return rc;
    if ((rc = stage_in(ctx, s, pl, *buf, st)) != WM_OK) return rc;
    *d = st.d; d->p = *buf;
    return WM_OK;
}

// bytes from the first pixel of a plane to the end of its last one (all channels and frames)
size_t plane_extent(const PlaneDesc& d, int rows, int cols, int frames)
{
    size_t n = (size_t)(rows - 1) * d.pitch + cols;
    if (d.channels > 1) n += (size_t)(d.channels - 1) * d.cstride;
    if (frames > 1) n += (size_t)(frames - 1) * d.fstride;
    return n * elem_size(d.dtype);
}
// ... as a byte range (a null plane has none and overlaps nothing)
struct ByteRange { const char* lo; const char* hi; };
ByteRange range_of(const PlaneDesc& d, int rows, int cols, int frames) { return ByteRange{(const char*)d.p, (const char*)d.p + plane_extent(d, rows, cols, frames)}; }
bool ranges_overlap(const ByteRange& a, const ByteRange& b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

// do two RESOLVED planes share a byte (what the kernels will address: a WM_MEM_SLOT_OUT input is the slot's last output, host
// planes are their staging buffers)?  frames_b > 0: `b` has that many frames (wm_embed_keys' K copies per input frame)
bool descs_overlap(const PlaneDesc& a, const PlaneDesc& b, int rows, int cols, int frames, int frames_b = 0)
{
    const char* a0 = (const char*)a.p; const char* a1 = a0 + plane_extent(a, rows, cols, frames);
    const char* b0 = (const char*)b.p; const char* b1 = b0 + plane_extent(b, rows, cols, frames_b > 0 ? frames_b : frames);
    return a0 < b1 && b0 < a1;
}

// A hand-over describes the plane a slot's last embed wrote (Slot::last_out).  Whatever the library itself writes over that
// plane afterwards -- an embed on ANOTHER slot into the same buffer, a band embed, wm_compute_mask's mask / error planes --
// ends the description; writes by the caller are the caller's contract (wm.h, WM_HANDOVER_VERIFY checks it)
void invalidate_handovers(wm_ctx* ctx, const ByteRange& written)
{
    for (auto& t : ctx->slots)
        if (t.ho.valid && t.last_out_frames != 0 && ranges_overlap(range_of(t.last_out, ctx->rows, ctx->cols, t.last_out_frames), written)) t.ho.valid = false;
}
void invalidate_handovers(wm_ctx* ctx, const PlaneDesc& written, int frames) { invalidate_handovers(ctx, range_of(written, ctx->rows, ctx->cols, frames)); }

// a profiled sweep: while the scope is set, every kernel launched through WM_KLAUNCH draws its own start / stop event pair
// (wm_kernels.hpp: the events are attached to the dispatch, so they bracket the kernel and nothing else); a sweep that is two
// launches (aligned strips + generic remainder) counts as ONE call of its kernel with the two durations added
constexpr int K_NONE = -1;  // a launch the profile leaves out (the band phases, the sweep of WM_HANDOVER_VERIFY)
struct ProfScope {
    wm_ctx* ctx; int kid; hipStream_t st;
    LaunchProf lp;
    bool on() const { return ctx->prof && kid != K_NONE; }
    ProfScope(wm_ctx* c, int k, hipStream_t s) : ctx(c), kid(k), st(s)
    {
        if (!on()) return;
        lp.get = &ProfScope::get; lp.owner = ctx;
        launch_prof_slot() = &lp;
    }
    ~ProfScope()
    {
        if (!on()) return;
        launch_prof_slot() = nullptr;
        for (int i = 0; i < lp.n; ++i) ctx->prof_recs.push_back({kid, lp.a[i], lp.b[i], i == 0});
    }
    static hipEvent_t get(void* owner)
    {
        wm_ctx* c = static_cast<wm_ctx*>(owner);
        if (!c->prof_free.empty()) { hipEvent_t e = c->prof_free.back(); c->prof_free.pop_back(); return e; }
        hipEvent_t e; (void)hipEventCreate(&e); return e;
    }
};

int prof_collect(wm_ctx* ctx)
{
    if (ctx->prof_recs.empty()) return WM_OK;
    HIPCHK(ctx, hipDeviceSynchronize());
    for (auto& r : ctx->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { ctx->prof_n[r.kid] += r.first ? 1 : 0; ctx->prof_ms[r.kid] += ms; }
        ctx->prof_free.push_back(r.a); ctx->prof_free.push_back(r.b);
    }
    ctx->prof_recs.clear();
    return WM_OK;
}

// the slot a call names: check_slot, then slot_of.  WM_SLOT_SYNC is slot 0, and the call waits for its own result
int slot_index(int slot) { return slot == WM_SLOT_SYNC ? 0 : slot; }
int check_slot(wm_ctx* ctx, int slot)
{
    if (slot_index(slot) < 0 || slot_index(slot) >= ctx->nslots) return fail(ctx, WM_ERR_BAD_ARG, "bad slot " + std::to_string(slot));
    return WM_OK;
}
Slot& slot_of(wm_ctx* ctx, int slot) { return ctx->slots[slot_index(slot)]; }

int check_mask(wm_ctx* ctx, int mask)
{
    if (mask != WM_MASK_ME && mask != WM_MASK_NVF) return fail(ctx, WM_ERR_BAD_ARG, "bad mask type");
    if (mask == WM_MASK_ME && ctx->p != 3) return fail(ctx, WM_ERR_BAD_P, "ME mask needs p == 3 (main.cpp:89)");
    return WM_OK;
}

// the calls that sweep whole images only (a band's totals are exchanged by the wm_band_* phases)
int refuse_band(wm_ctx* ctx, const char* who)
{
    return ctx->band_hi > 0 ? fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": not in band mode") : WM_OK;
}

// ---- the launch records (wm_kernels.hpp): a call fills its Sweep once, behind its geometry and its resolved input plane, and hands
// it to every launch it makes.  The mask type is the kernels' mask index, the window's pad is p / 2 (ME: p == 3, check_mask).
// detect_sweep: the detector side, which solves under either mask and reads the slot's coefficients and status.  mask_route: the
// embed side (embeds, stats, wm_compute_mask), where only ME has a solve: under NVF the record carries null for both
Sweep detect_sweep(const wm_ctx* ctx, const Slot& s, const LaunchGeom& lg, int frames, int mask, const PlaneDesc& xd)
{
    return Sweep{s.stream, lg, frames, mask, ctx->p / 2, xd, s.d_coef, s.d_status};
}
Sweep mask_route(const wm_ctx* ctx, const Slot& s, const LaunchGeom& lg, int frames, int mask, const PlaneDesc& xd)
{
    Sweep sw = detect_sweep(ctx, s, lg, frames, mask, xd);
    if (mask != WM_MASK_ME) { sw.coef = nullptr; sw.status = nullptr; }
    return sw;
}

// may the sweeps address the context's W (or a key plane of its shape) as a buffer with 32-bit offsets?  (W is a dense f32
// plane: 4-byte aligned rows suffice, vec_ok)
int aligned_w_of(const wm_ctx* ctx) { return fits_32bit(ctx->rows, ctx->cols, WM_F32) ? 1 : 0; }
// the key side of a sweep: the context's own W (a bank of one), or a bank whose planes have W's shape
KeyBank own_w(const wm_ctx* ctx) { return KeyBank{ctx->w->d_w, 0, 1, aligned_w_of(ctx)}; }
KeyBank bank_of(const wm_ctx* ctx, const wm_keys* keys) { return KeyBank{keys->d, (long long)ctx->rows * ctx->cols, keys->nkeys, aligned_w_of(ctx)}; }

// room for `records` more result records on the slot before its next wm_sync; noun: what multiplies the frames of a call with
// several records per frame ("keys", "offsets"), nullptr for one record per frame
int check_res_room(wm_ctx* ctx, const Slot& s, long long records, const char* noun = nullptr)
{
    if (s.res_used + records <= RES_CAP) return WM_OK;
    std::string msg = "too many un-synced results on this slot";
    if (noun) msg += std::string(" (frames x ") + noun + " count against " + std::to_string(RES_CAP) + ")";
    return fail(ctx, WM_ERR_BUSY, msg);
}

// after the launches of one op: a failed launch may leave the sweep's last-block tickets half counted, so clear them
// (stream-ordered) before the slot is used again
int launch_check(wm_ctx* ctx, Slot& s)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipMemsetAsync(s.d_ticket, 0, ticket_words(ctx) * sizeof(unsigned), s.stream);
        return fail(ctx, WM_ERR_RUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    }
    return WM_OK;
}

// ---- the sweeps' launches with the slot's scratch arrays filled in.  kid: the kernel the profile counts the launch as, K_NONE
// for a launch it leaves out
void sweep_gram(wm_ctx* ctx, Slot& s, int kid, const Sweep& sw, double* totals = nullptr, const int* redo = nullptr)
{
    ProfScope ps(ctx, kid, s.stream);
    launch_gram(sw, s.d_gram, s.d_gramb, s.d_ticket, s.d_coef, s.d_status, totals ? totals : s.d_gramtot, redo);
}
// the stats sweep of the context's W (sw: mask_route's; ME: behind the Gram sweep's solve); its fold tail leaves the strength records
// in `res`, the embed scalars in s.d_scal and the raw totals in s.d_raw[0 .. frames)
void sweep_stats(wm_ctx* ctx, Slot& s, bool profiled, const Sweep& sw, OpResult* res)
{
    ProfScope ps(ctx, !profiled ? K_NONE : sw.mask == WM_MASK_ME ? K_ME_STATS : K_NVF_STATS, s.stream);
    unsigned* ticket = s.d_ticket + ctx->max_frames * TKS;
    if (sw.mask == WM_MASK_ME)
        launch_me_stats(sw, own_w(ctx), s.d_pmax, s.d_pss, ticket, strip_tickets(ctx, s, 0), s.d_smax, s.d_sss, ctx->sF, sqrt_n(ctx), s.d_scal, res, s.d_raw);
    else
        launch_nvf_stats(sw, own_w(ctx), s.d_pss, ticket, strip_tickets(ctx, s, 0), s.d_sss, ctx->sF, sqrt_n(ctx), s.d_scal, res, s.d_raw);
}
// the detect sweep against the context's W (sw: detect_sweep's); its fold tail leaves the scores in `res` and the raw sums in
// s.d_raw[max_frames ..)  (dc, mode: the checking detector of the checked hand-over and its redo launch, wm_kernels.hpp)
void sweep_detect(wm_ctx* ctx, Slot& s, int kid, const Sweep& sw, OpResult* res, const DigCheck* dc = nullptr, int mode = 0)
{
    ProfScope ps(ctx, kid, s.stream);
    launch_detect(sw, own_w(ctx), s.d_pcorr, s.d_ticket + 2 * ctx->max_frames * TKS, strip_tickets(ctx, s, 1), s.d_scorr, res, s.d_raw + ctx->max_frames, dc, mode);
}

// remember where to deliver the result records of one op (the kernels write them to mapped host memory): frames * per_frame
// records from s.res_used on; keep: an unsolvable frame leaves the caller's values as they are (the embeds)
void push_pending(Slot& s, int frames, int per_frame, bool keep, float* value_out, int* status_out, float* coef_out)
{
    s.pending.push_back(Pending{frames, per_frame, keep, s.res_used, value_out, status_out, coef_out});
    s.res_used += frames * per_frame;
}

// hand the result records of everything queued on the slot to the callers' pointers (the stream has completed)
int deliver(Slot& s)
{
    int rc = WM_OK;
    for (auto& pd : s.pending) {
        // record f * per_frame + k; every record of a frame carries the frame's status.  With one record per frame this is the
        // plain loop over the frames: status, then the value unless an unsolvable embed keeps the caller's
        for (int f = 0; f < pd.frames; ++f) {
            const OpResult* r = s.h_res + pd.res_off + f * pd.per_frame;
            const int st = r[0].status;
            if (pd.status_out) pd.status_out[f] = st;
            if (st != 0) rc = WM_UNSOLVABLE;
            // unsolvable embed leaves `a` untouched (Watermark.cpp:164-165); detect delivers 0.0f (:246-247)
            if (!pd.value_out || (st != 0 && pd.keep_value_when_unsolvable)) continue;
            for (int k = 0; k < pd.per_frame; ++k) pd.value_out[f * pd.per_frame + k] = r[k].value;
        }
        // (mask-only ops, one record per frame: the coefficients lie beside the records)
        if (pd.coef_out) std::memcpy(pd.coef_out, s.h_coefres + (size_t)pd.res_off * 8, (size_t)pd.frames * 8 * sizeof(float));
    }
    s.pending.clear();
    s.res_used = 0;
    s.tab_used = 0;  // (every queued call has run: their tables are free)
    return rc;
}

int do_sync(wm_ctx* ctx, Slot& s)
{
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    return deliver(s);
}

// in front of a rebuild of the slots (wm_configure, wm_set_rows_per_segment, wm_reinit): every slot's queued results reach the
// callers' pointers as wm_sync would deliver them, before the records are freed.  An unsolvable frame is in the statuses, not in the
// return value (as with wm_set_stream); an error is returned and nothing is rebuilt
int sync_all_slots(wm_ctx* ctx)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (auto& s : ctx->slots) {
        if (!s.stream) continue;
        const int rc = do_sync(ctx, s);
        if (rc < 0) return rc;
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    return WM_OK;
}

// the back half of a call behind its launches: their check, the records queued for delivery, and the wait of a synchronous call
int finish_call(wm_ctx* ctx, Slot& s, int slot, int frames, int per_frame, bool keep, float* value_out, int* status_out, float* coef_out = nullptr)
{
    const int rc = launch_check(ctx, s);
    if (rc != WM_OK) return rc;
    push_pending(s, frames, per_frame, keep, value_out, status_out, coef_out);
    return slot == WM_SLOT_SYNC ? do_sync(ctx, s) : WM_OK;
}

}  // namespace

wm_ctx::~wm_ctx()
{
    for (auto& s : slots) free_slot(s);
    for (auto& r : prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : prof_free) (void)hipEventDestroy(e);
    if (fused_lock_fd >= 0) (void)close(fused_lock_fd);
}

extern "C" {

int wm_create(wm_ctx** out, int device, int rows, int cols, int p, float psnr, const float* w_rowmajor)
{
    return create_ctx(out, device, rows, cols, p, psnr, false, w_rowmajor, 0);
}

int wm_create_generated(wm_ctx** out, int device, int rows, int cols, int p, float psnr, uint32_t seed)
{
    return create_ctx(out, device, rows, cols, p, psnr, true, nullptr, seed);
}

int wm_create_from_file(wm_ctx** out, int device, int rows, int cols, int p, float psnr, const char* w_path)
{
    if (!out) return WM_ERR_BAD_ARG;
    *out = nullptr;
    int rc = check_params(rows, cols, p, psnr);
    if (rc != WM_OK) return rc;
    std::vector<float> w;
    rc = read_w_file(nullptr, w_path, rows, cols, w);
    if (rc != WM_OK) return rc;
    return wm_create(out, device, rows, cols, p, psnr, w.data());
}

int wm_clone(const wm_ctx* src, wm_ctx** out)
{
    if (!src || !out) return WM_ERR_BAD_ARG;
    *out = nullptr;
    std::unique_ptr<wm_ctx> ctx(new wm_ctx);
    ctx->device = src->device; ctx->rows = src->rows; ctx->cols = src->cols; ctx->p = src->p; ctx->psnr = src->psnr;
    ctx->sF = src->sF; ctx->w = src->w; ctx->rps_override = src->rps_override; ctx->fused_mode = src->fused_mode;
    ctx->handover = src->handover; ctx->checked_handover = src->checked_handover;  // (alloc_slots allocates the hand-over arrays)
    ctx->band_lo = src->band_lo; ctx->band_hi = src->band_hi; ctx->band_rows_global = src->band_rows_global;
    int rc = alloc_slots(ctx.get(), src->nslots, src->max_frames);
    if (rc != WM_OK) return rc;
    *out = ctx.release();
    return WM_OK;
}

int wm_reinit(wm_ctx* ctx, int rows, int cols, const float* w_rowmajor)
{
    if (!ctx || !w_rowmajor) return WM_ERR_BAD_ARG;
    int rc = check_params(rows, cols, ctx->p, ctx->psnr);
    if (rc != WM_OK) return fail(ctx, rc, "bad dimensions");
    if ((rc = sync_all_slots(ctx)) != WM_OK) return rc;
    // commit the new shape only once the new W is on the device; a band configuration belongs to the old shape
    const int old_rows = ctx->rows, old_cols = ctx->cols;
    ctx->rows = rows; ctx->cols = cols;
    rc = upload_w(ctx, w_rowmajor);
    if (rc != WM_OK) { ctx->rows = old_rows; ctx->cols = old_cols; return rc; }
    ctx->band_lo = ctx->band_hi = 0; ctx->band_rows_global = 0;
    return alloc_slots(ctx, ctx->nslots, ctx->max_frames);
}

int wm_reinit_from_file(wm_ctx* ctx, int rows, int cols, const char* w_path)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    std::vector<float> w;
    int rc = read_w_file(ctx, w_path, rows, cols, w);
    if (rc != WM_OK) return rc;
    return wm_reinit(ctx, rows, cols, w.data());
}

void wm_destroy(wm_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    delete ctx;
}

int wm_configure(wm_ctx* ctx, int nslots, int max_frames)
{
    if (!ctx || nslots < 1 || nslots > 64 || max_frames < 1 || max_frames > RES_CAP) return fail(ctx, WM_ERR_BAD_ARG, "wm_configure: bad arguments");
    const int rc = sync_all_slots(ctx);
    if (rc != WM_OK) return rc;
    return alloc_slots(ctx, nslots, max_frames);
}

int wm_set_fused(wm_ctx* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 1) return fail(ctx, WM_ERR_BAD_ARG, "wm_set_fused: mode must be 0 or 1");
    ctx->fused_mode = mode;
    return WM_OK;
}

int wm_set_handover(wm_ctx* ctx, int on)
{
    if (!ctx || on < 0 || on > 1) return fail(ctx, WM_ERR_BAD_ARG, "wm_set_handover: 0 or 1");
    for (auto& s : ctx->slots) s.ho.valid = false;
    if (on) {
        // switched on only when every slot has both of its arrays
        const int rc = ho_alloc(ctx);
        if (rc != WM_OK) { ctx->handover = 0; return rc; }
    }
    ctx->handover = on;
    return WM_OK;
}

int wm_set_checked_handover(wm_ctx* ctx, int on)
{
    if (!ctx || on < 0 || on > 1) return fail(ctx, WM_ERR_BAD_ARG, "wm_set_checked_handover: 0 or 1");
    for (auto& s : ctx->slots)
        if (!s.ho.promised) s.ho.valid = false;
    ctx->checked_handover = on;
    return WM_OK;
}

int wm_checked_handover_counts(wm_ctx* ctx, unsigned long long* trusted, unsigned long long* redone)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long t = 0, r = 0;
    for (auto& s : ctx->slots) {
        unsigned long long c[2] = {0, 0};
        HIPCHK(ctx, hipMemcpyAsync(c, s.d_hocnt, sizeof c, hipMemcpyDeviceToHost, s.stream));
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        t += c[0]; r += c[1];
    }
    if (trusted) *trusted = t;
    if (redone) *redone = r;
    return WM_OK;
}

int wm_fused_info(const wm_ctx* ctx, int* workgroups, int* tile_rows, unsigned long long* fallbacks)
{
    if (!ctx) return 0;
    if (workgroups) *workgroups = ctx->fg.fusable ? ctx->fg.G : 0;
    if (tile_rows) *tile_rows = ctx->fg.fusable ? ctx->fg.th : 0;
    if (fallbacks) *fallbacks = ctx->fused_fallbacks;
    return ctx->fg.fusable && ctx->fused_mode != 0 && ctx->band_hi == 0 && ctx->p == 3 ? 1 : 0;
}

unsigned long long wm_fused_lock_skips(const wm_ctx* ctx) { return ctx ? ctx->fused_lock_skips : 0; }

int wm_fused_stamps(wm_ctx* ctx, unsigned long long* out, int cap)
{
    if (!ctx || !out || ctx->slots.empty() || !ctx->slots[0].fz.stamps) return 0;
    const int n = ctx->fg.G * 16 + 16 < cap ? ctx->fg.G * 16 + 16 : cap;  // [G][16] + 16 stamps of the workgroup that folded and solved
    // synchronous fused calls return on the result record, before the kernel has retired, and the stamps are plain stores
    // (visible at the end of the kernel), the slot streams are non-blocking: wait for the slot's stream, not for the null stream
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->slots[0].stream) != hipSuccess) return 0;
    if (hipMemcpy(out, ctx->slots[0].fz.stamps, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

int wm_fused_gram(wm_ctx* ctx, double* out44)
{
    if (!ctx || !out44 || ctx->slots.empty() || !ctx->slots[0].fz.stamps) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->slots[0].stream) != hipSuccess) return 0;
    if (hipMemcpy(out44, ctx->slots[0].fz.stamps + 16 * (ctx->fg.G + 1), NGRAM * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return NGRAM;
}

int wm_set_rows_per_segment(wm_ctx* ctx, int rps)
{
    if (!ctx || rps < 0 || rps > 4096) return fail(ctx, WM_ERR_BAD_ARG, "wm_set_rows_per_segment: bad value");
    const int rc = sync_all_slots(ctx);
    if (rc != WM_OK) return rc;
    ctx->rps_override = rps;
    return alloc_slots(ctx, ctx->nslots, ctx->max_frames);
}

// does this call take the fused single-frame kernels?  Synchronous one-frame calls on whole images with the 3x3 window,
// when the shape fits the LDS tiling (fused_geometry) -- everything else takes the batched sweeps
static bool fused_call(wm_ctx* ctx, bool sync_after, int frames)
{
    if (!(sync_after && frames == 1 && ctx->fused_mode != 0 && ctx->fg.fusable && ctx->band_hi == 0 && ctx->p == 3)) return false;
    if (ctx->fused_skip > 0) { --ctx->fused_skip; return false; }  // inside a back-off window after a fallback
    return true;
}

// a fused launch ended without delivering: count it, clear the arrival counters (stream-ordered, behind the launch) and keep
// the next calls off the fused path for a window that doubles while the re-probes keep failing
static int fused_failed(wm_ctx* ctx, Slot& s)
{
    ctx->fused_fallbacks++;
    ctx->fused_backoff = ctx->fused_backoff == 0 ? 8 : (ctx->fused_backoff >= 2048 ? 4096 : 2 * ctx->fused_backoff);
    ctx->fused_skip = ctx->fused_backoff;
    HIPCHK(ctx, hipMemsetAsync(s.fz.cnt, 0, FUSED_CNT_BYTES, s.stream));
    return WM_OK;
}

// launch -> record: wait for a fused launch's result record (poll; the stream only when the output is staged to the host
// behind the kernel, or when the poll gave up).  *got holds the record as read by ONE acquire load.
static int fused_wait(wm_ctx* ctx, Slot& s, const OpResult* hres, bool need_stream, OpResult* got)
{
    got->status = FUSED_PENDING; got->value = 0.0f;
    const bool arrived = poll_record(hres, FUSED_PENDING, s.stream, got);
    if (need_stream || !arrived) {
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        *got = load_record(hres);
    }
    return WM_OK;
}

// shared front half of embed / detect / mask: stage the grey input if needed and describe it
static int prep_input(wm_ctx* ctx, Slot& s, const wm_plane* in, PlaneDesc* xd)
{
    if (in->mem == WM_MEM_SLOT_OUT) {
        // the device copy of what the last embed on this slot wrote (grey): a streamed frame is detected without
        // crossing the host link again
        if (s.last_out_frames == 0 || s.last_out.channels != 1 || in->frames != s.last_out_frames || in->dtype != s.last_out_dtype)
            return fail(ctx, WM_ERR_BAD_ARG, "WM_MEM_SLOT_OUT: no matching grey embed output on this slot (frames / dtype must equal the last wm_embed's)");
        *xd = s.last_out;
        return WM_OK;
    }
    return resolve_plane(ctx, s, in, &s.st_in, &s.st_in_bytes, xd);
}

// the front half of a call that sweeps one grey input plane: the plane's checks, room for its result records (per_frame of them
// for each frame, 0: the call queues none), the context's device, the plane staged / resolved, the launch geometry, and from
// them the call's sweep record (detect_sweep's)
static int open_input(wm_ctx* ctx, Slot& s, const wm_plane* img, const char* what, int mask, long long per_frame, const char* noun, Sweep* sw)
{
    int rc;
    PlaneDesc xd;
    LaunchGeom lg;
    if ((rc = check_plane(ctx, img, 0, false, what, true)) != WM_OK) return rc;
    if ((rc = check_res_room(ctx, s, img->frames * per_frame, noun)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = prep_input(ctx, s, img, &xd)) != WM_OK) return rc;
    if ((rc = geom_checked(ctx, img->frames, mask, &lg)) != WM_OK) return rc;
    *sw = detect_sweep(ctx, s, lg, img->frames, mask, xd);
    return WM_OK;
}

// the base plane of an embed, resolved like the input; a host base that IS the input plane (`xd`: prep_input's result) is not
// staged a second time
static int prep_base(wm_ctx* ctx, Slot& s, const wm_plane* in_gray, const wm_plane* base, const PlaneDesc& xd, PlaneDesc* bd)
{
    const bool base_is_in = base->data == in_gray->data && base->mem == in_gray->mem && base->mem != WM_MEM_SLOT_OUT && base->channels == 1 &&
                            base->dtype == in_gray->dtype && base->pitch == in_gray->pitch;
    if (base->mem == WM_MEM_HOST && base_is_in) { *bd = xd; return WM_OK; }
    return resolve_plane(ctx, s, base, &s.st_base, &s.st_base_bytes, bd);
}

// ---- the embed frame: what the embed calls share around their sweeps.  wm_embed and wm_embed_signs take all of it;
// wm_embed_keys and wm_embed_signs_multi, with K outputs per input frame, take the dtype rules and the K-output frame below
// (xd, bd, od: the RESOLVED planes, what the kernels address; st_out: the staging layout of a host output, copied out by stage_out)
struct EmbedCall { int frames; PlaneDesc xd, bd, od; Staged st_out; bool inplace; };
static int check_embed_dtypes(wm_ctx* ctx, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out)
{
    if (out->channels != base->channels || out->dtype != base->dtype) return fail(ctx, WM_ERR_BAD_ARG, "out must have the shape and dtype of base");
    if (in_gray->dtype != base->dtype) return fail(ctx, WM_ERR_BAD_ARG, "in_gray and base must have the same dtype (the reference converts whole frames, main.cpp:355-357)");
    return WM_OK;
}
static int check_embed_planes(wm_ctx* ctx, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out)
{
    int rc;
    if ((rc = check_plane(ctx, in_gray, 0, false, "in_gray", true)) != WM_OK) return rc;
    if ((rc = check_plane(ctx, base, in_gray->frames, true, "base")) != WM_OK) return rc;
    if ((rc = check_plane(ctx, out, in_gray->frames, true, "out")) != WM_OK) return rc;
    return check_embed_dtypes(ctx, in_gray, base, out);
}

// the three planes staged / resolved, the in-place judgement, and the end of every hand-over whose plane this call's output replaces
static int embed_stage(wm_ctx* ctx, Slot& s, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, EmbedCall* c)
{
    int rc;
    c->frames = in_gray->frames;
    if ((rc = prep_input(ctx, s, in_gray, &c->xd)) != WM_OK) return rc;
    if ((rc = prep_base(ctx, s, in_gray, base, c->xd, &c->bd)) != WM_OK) return rc;
    if (out->mem != WM_MEM_HOST) c->od = desc_device(out);
    else {  // (a host plane is written to the slot's staging buffer)
        c->st_out = staged_layout(out);
        if ((rc = ensure(ctx, &s.st_out, &s.st_out_bytes, c->st_out.bytes)) != WM_OK) return rc;
        c->od = c->st_out.d; c->od.p = s.st_out;
    }
    // in place = the output overlaps the plane the stencil reads, judged on the RESOLVED addresses (a WM_MEM_SLOT_OUT input is
    // the slot's last output buffer, which the caller may well pass as `out` again)
    c->inplace = descs_overlap(c->xd, c->od, ctx->rows, ctx->cols, c->frames);
    s.ho.valid = false;  // (whatever this call writes replaces the plane a hand-over described)
    invalidate_handovers(ctx, c->od, c->frames);  // (... and that of any other slot whose last output this call overwrites)
    return WM_OK;
}

// in-place embed on the sweeps (the video path hands the same frame as input, base and output, main.cpp:356,380):
// the stencil must keep reading the ORIGINAL pixels while rows of `out` are being written, so the mask
// source is snapshotted into the slot's staging buffer first: one extra device copy of the RESOLVED grey plane (a device plane,
// or the slot's last output behind WM_MEM_SLOT_OUT) into the dense staging layout of the caller's plane
static int embed_snapshot(wm_ctx* ctx, Slot& s, const wm_plane* in_gray, EmbedCall* c)
{
    if (!c->inplace) return WM_OK;
    const Staged st = staged_layout(in_gray);
    const int rc = ensure(ctx, &s.st_in, &s.st_in_bytes, st.bytes);
    if (rc != WM_OK) return rc;
    const size_t es = elem_size(in_gray->dtype);
    for (int f = 0; f < c->frames; ++f) {
        const char* src = (const char*)c->xd.p + (size_t)f * c->xd.fstride * es;
        char* d = (char*)s.st_in + (size_t)f * st.d.fstride * es;
        HIPCHK(ctx, hipMemcpy2DAsync(d, st.pitch * es, src, c->xd.pitch * es, in_gray->cols * es, in_gray->rows, hipMemcpyDeviceToDevice, s.stream));
    }
    // the base IS the input plane (video frames: input, base and output are one plane): read it from the snapshot too --
    // k_embed then takes the base from its stencil window (no base stream) and nothing reads the plane being overwritten
    const bool base_is_input = c->bd.p == c->xd.p && c->bd.pitch == c->xd.pitch && c->bd.fstride == c->xd.fstride && c->bd.dtype == c->xd.dtype && c->bd.channels == 1;
    c->xd = st.d; c->xd.p = s.st_in;
    if (base_is_input) c->bd = c->xd;
    return WM_OK;
}

// the call's result: `out` becomes the slot's last output, the strengths are queued (an unsolvable frame keeps the caller's)
static void embed_queue_result(Slot& s, const wm_plane* out, const EmbedCall& c, float* a_out, int* status_out)
{
    s.last_out = c.od; s.last_out_frames = c.frames; s.last_out_dtype = out->dtype;
    push_pending(s, c.frames, 1, true, a_out, status_out, nullptr);
}
// behind the sweeps' launches: their check, a host output copied out, the result queued, a synchronous call's wait (wm_embed_detect: the detector's covers it)
static int embed_close(wm_ctx* ctx, Slot& s, const wm_plane* out, const EmbedCall& c, float* a_out, int* status_out, int slot)
{
    int rc;
    if ((rc = launch_check(ctx, s)) != WM_OK) return rc;
    if (out->mem == WM_MEM_HOST && (rc = stage_out(ctx, s, out, s.st_out, c.st_out)) != WM_OK) return rc;
    embed_queue_result(s, out, c, a_out, status_out);
    return slot == WM_SLOT_SYNC && !ctx->pair_mode ? do_sync(ctx, s) : WM_OK;
}

// ---- the K-output frame: wm_embed_keys and wm_embed_signs_multi write K device planes per input frame (`who`: the caller's name;
// `count`: what K counts, "nkeys" / "ncopies").  They check in_gray, base and the memory kind of `out` themselves, then:
// out: frames * K planes (more than max_frames is fine: the sweeps' scratch is per input frame), each a plane check_plane admits
static int check_out_copies(wm_ctx* ctx, const char* who, const char* count, const wm_plane* out, int frames, int K)
{
    if ((long long)out->frames != (long long)frames * K)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": out->frames must be in_gray->frames * " + count + " = " + std::to_string((long long)frames * K));
    wm_plane one = *out;
    one.frames = 1;
    const int rc = check_plane(ctx, &one, 1, true, "out");
    if (rc != WM_OK) return rc;
    if (out->frames > 1 && out->frame_stride < (int64_t)(out->channels - 1) * (out->channels > 1 ? out->channel_stride : 0) + (int64_t)out->rows * out->pitch)
        return fail(ctx, WM_ERR_BAD_ARG, "out: frame_stride too small (frames overlap)");
    return WM_OK;
}
// the planes staged / resolved into c (embed_stage's part for a device `out` of K planes per frame).  K outputs of one input: an
// in-place call has no meaning (judged on the RESOLVED planes, as wm_embed judges them).  No hand-over of its own, and
// WM_MEM_SLOT_OUT keeps naming the last wm_embed output; a hand-over whose plane the copies overwrite ends here
static int copies_stage(wm_ctx* ctx, Slot& s, const char* who, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int K, EmbedCall* c)
{
    int rc;
    const int frames = c->frames = in_gray->frames;
    if ((rc = prep_input(ctx, s, in_gray, &c->xd)) != WM_OK) return rc;
    if ((rc = prep_base(ctx, s, in_gray, base, c->xd, &c->bd)) != WM_OK) return rc;
    c->od = desc_device(out);
    if (descs_overlap(c->xd, c->od, ctx->rows, ctx->cols, frames, frames * K) || descs_overlap(c->bd, c->od, ctx->rows, ctx->cols, frames, frames * K))
        return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": out overlaps in_gray or base");
    invalidate_handovers(ctx, c->od, frames * K);
    return WM_OK;
}

// a fused embed issued output stores over the call's own input or base and their completion was not observed
static int fail_partly_watermarked(wm_ctx* ctx)
{
    return fail(ctx, WM_ERR_RUNTIME, "fused embed: the completion of the output stores was not observed and the output overlaps the input "
                                     "or the base (in-place call): the frame may be partly watermarked and cannot be re-run");
}

int wm_embed(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, float* a_out,
             int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    const bool sync_after = slot == WM_SLOT_SYNC;
    if ((rc = check_embed_planes(ctx, in_gray, base, out)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    EmbedCall c;
    if ((rc = embed_stage(ctx, s, in_gray, base, out, &c)) != WM_OK) return rc;
    PlaneDesc &xd = c.xd, &bd = c.bd, &od = c.od;
    const bool inplace = c.inplace;

    // one image per synchronous call (the reference's call pattern): ONE launch with the frame's tiles resident in LDS
    // (wm_k_fused.hip).  Its y stores come after two chip-wide hand-offs behind every read of x, so an in-place call
    // needs no snapshot of the input.
    std::optional<FusedGuard> guard;
    // (a width that is not a multiple of 4: f32 planes only -- their 16-byte accesses need 4-byte alignment, a u8 lane's dword does not exist there)
    const bool width_ok = ctx->cols % 4 == 0 || (xd.dtype == WM_F32 && bd.dtype == WM_F32 && od.dtype == WM_F32);
    bool take_fused = width_ok && fused_call(ctx, sync_after, frames) && xd.aligned && bd.aligned && od.aligned;
    if (take_fused && !ctx->pair_mode) {  // (wm_embed_detect holds the lock over both launches)
        guard.emplace(ctx->device, ctx->fused_lock_fd);
        if (!guard->ok) { guard.reset(); ctx->fused_lock_skips++; take_fused = false; }
    }
    if (take_fused) {
        OpResult* hres = s.h_res + s.res_used;
        hres->status = FUSED_PENDING;
        if (++s.fz_epoch == 0) s.fz_epoch = 1;
        int lrc;
        // wm_embed_detect on device planes of one type: ONE launch for the pair (k_fused_pair) -- nothing is launched here, the
        // detector's call that follows at once launches both halves (WM_FUSED_PAIR=0: the two kernels back to back, as before)
        s.pair.deferred = ctx->pair_mode && ctx->fused_pair && out->mem != WM_MEM_HOST && od.channels == 1 && bd.channels == 1 &&
                          xd.dtype == bd.dtype && xd.dtype == od.dtype;
        if (s.pair.deferred) { s.pair.mask = mask; s.pair.epoch = s.fz_epoch; s.pair.xd = xd; s.pair.bd = bd; s.pair.od = od; lrc = 0; }
        else { ProfScope ps(ctx, K_FUSED_EMBED, s.stream); lrc = launch_fused_embed(s.stream, ctx->fg, s.fz, s.fz_epoch, mask, xd, ctx->w->d_w, bd, od, ctx->sF, sqrt_n(ctx), s.d_res + s.res_used); }
        if (lrc == 0) {
            if ((rc = launch_check(ctx, s)) != WM_OK) return rc;
            if (out->mem == WM_MEM_HOST && (rc = stage_out(ctx, s, out, s.st_out, c.st_out)) != WM_OK) return rc;
            if (ctx->pair_mode) {
                // the detector's launch follows at once on the same stream; its record completes both (wm_detect's fused branch)
                s.pair.armed = true; s.pair.res_index = s.res_used; s.pair.host_out = out->mem == WM_MEM_HOST;
                s.pair.out_overlaps_inputs = inplace || descs_overlap(bd, od, ctx->rows, ctx->cols, frames);
                embed_queue_result(s, out, c, a_out, status_out);
                return WM_OK;
            }
            // device output: the kernel writes y through to memory and reports last, so the record is the completion
            // signal; host output: the staging copy behind the kernel has to finish as well
            OpResult got;
            if ((rc = fused_wait(ctx, s, hres, out->mem == WM_MEM_HOST, &got)) != WM_OK) return rc;
            if (got.status != FUSED_PENDING && got.status != FUSED_INCOMPLETE) {
                ctx->fused_backoff = 0;
                embed_queue_result(s, out, c, a_out, status_out);
                return deliver(s);  // the record has arrived
            }
            // PENDING: a hand-off timed out before any output store (the workgroups were not all resident): nothing was
            // written, the sweeps take the call.  INCOMPLETE: output stores were issued but the end of the frame was not
            // observed -- the output plane may be partly written.  If it overlaps the input or the base, they are no longer
            // the caller's frame: re-running would watermark a watermarked frame, so the call fails instead.
            if ((rc = fused_failed(ctx, s)) != WM_OK) return rc;
            if (got.status == FUSED_INCOMPLETE) {
                HIPCHK(ctx, hipStreamSynchronize(s.stream));
                if (inplace || descs_overlap(bd, od, ctx->rows, ctx->cols, frames)) return fail_partly_watermarked(ctx);
            }
        }
    }
    guard.reset();  // (the sweeps below do not need the device to themselves)
    if ((rc = embed_snapshot(ctx, s, in_gray, &c)) != WM_OK) return rc;

    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    const Sweep sw = mask_route(ctx, s, lg, frames, mask, xd);
    OpResult* res = s.d_res + s.res_used;
    // Gram hand-over (wm_set_handover): k_embed also leaves the tile-internal lag sums of y for a detector that reads this
    // output as WM_MEM_SLOT_OUT (grey f32 planes on the aligned path; launch_embed says whether it applied)
    // (its tiles reach two rows behind their segment: not when the output overwrites the base those rows are read from)
    // ... and, with the checked hand-over on, for ANY later wm_detect of this output on this slot (ME embeds: the detector's
    // digest check decides whether the sums are used, wm.h wm_detect)
    const bool promised = ctx->handover || ctx->pair_handover;
    const bool want_ho = promised || (ctx->checked_handover && mask == WM_MASK_ME);
    if (want_ho && !ho_ready(s) && ho_alloc_slot(ctx, s) != WM_OK) { (void)hipGetLastError(); ctx->last_error.clear(); }  // (no memory: no hand-over)
    const HandOver ho = handover_of(ctx, s, lg.nstrips * lg.nsegs + handover_seam_blocks(lg));
    const HandOver* hop = want_ho && ho_ready(s) && out->channels == 1 && ho.stride <= ho_stride_max(ctx) &&
                                  !descs_overlap(bd, od, ctx->rows, ctx->cols, frames) ? &ho : nullptr;
    bool handed = false;
    if (mask == WM_MASK_ME) sweep_gram(ctx, s, K_GRAM, sw);
    sweep_stats(ctx, s, true, sw, res);
    {
        ProfScope ps(ctx, K_EMBED, s.stream);
        handed = launch_embed(sw, own_w(ctx), EmbedPlanes{bd, od, s.d_scal}, hop);
    }
    if (handed) { s.ho.valid = true; s.ho.promised = promised; s.ho.used = false; s.ho.lg = lg; s.ho.frames = frames; s.ho.stride = ho.stride; }
    return embed_close(ctx, s, out, c, a_out, status_out, slot);
}

// k_gram_ho over the sums the slot's last embed left (the border blocks are this short launch's longest: as many of them as the
// record array holds, not the batched sweep's 16)
static void gram_from_handover(wm_ctx* ctx, Slot& s, const Sweep& sw)
{
    Sweep h = sw;  // (the plane as the call resolved it, on the geometry of the embed that left the sums)
    h.lg = s.ho.lg;
    h.lg.nbb = border_blocks(ctx->rows, ctx->cols);
    launch_gram_ho(h, handover_of(ctx, s, s.ho.stride), s.d_gramb, s.d_ticket, s.d_coef, s.d_status, s.d_gramtot);
}

// does this detector input take the checked hand-over (wm.h wm_detect)?  The plane the slot's last embed wrote -- the same
// descriptor --, sums nobody has used yet, and the checking detector's path (f32, ME, overlapped aligned strips)
static bool checked_handover_applies(const wm_ctx* ctx, const Slot& s, const Sweep& sw)
{
    const PlaneDesc &o = s.last_out, &xd = sw.x;
    return ctx->checked_handover && s.ho.valid && !s.ho.used && ho_ready(s) && ctx->band_hi == 0 && s.ho.frames == sw.frames &&
           s.last_out_frames == sw.frames && xd.p == o.p && xd.pitch == o.pitch && xd.fstride == o.fstride && xd.dtype == o.dtype &&
           s.last_out_dtype == WM_F32 && xd.channels == 1 && detect_checkable(sw, aligned_w_of(ctx));
}

// the Gram sweep of a detector-side call: k_gram over the plane -- or, when the plane is the slot's last embed output and that
// embed left its tile-internal lag sums (wm_set_handover), only the seams, the border frame and the solve (k_gram_ho)
static int gram_sweep(wm_ctx* ctx, Slot& s, const Sweep& sw, const wm_plane* img)
{
    const int frames = sw.frames;
    if (img->mem == WM_MEM_SLOT_OUT && s.ho.valid && s.ho.promised && s.ho.frames == frames && ho_ready(s) && ctx->band_hi == 0) {
        s.ho.used = true;
        { ProfScope ps(ctx, K_GRAM_HO, s.stream); gram_from_handover(ctx, s, sw); }
        if (!ctx->handover_verify) return WM_OK;
        // WM_HANDOVER_VERIFY=1 (a debug mode, it synchronises): the hand-over rests on the caller's promise that the plane
        // behind WM_MEM_SLOT_OUT is still what the embed wrote.  Run the ordinary Gram sweep over the plane as it is NOW and
        // hold the 44 totals against the handed-over ones: the same exact products, so they agree to the f64 summation order
        // (<= 1e-14 relative, tests/test_gpu_handover.py) unless a single pixel changed
        std::vector<double> t_ho((size_t)frames * NGRAM), t_now((size_t)frames * NGRAM);
        HIPCHK(ctx, hipMemcpyAsync(t_ho.data(), s.d_gramtot, t_ho.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream));
        sweep_gram(ctx, s, K_NONE, sw);
        HIPCHK(ctx, hipMemcpyAsync(t_now.data(), s.d_gramtot, t_now.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        for (int f = 0; f < frames; ++f)
            for (int t = 0; t < NGRAM; ++t) {
                const double a = t_ho[(size_t)f * NGRAM + t], b = t_now[(size_t)f * NGRAM + t];
                const double scale = std::fmax(1.0, std::fmax(std::fabs(a), std::fabs(b)));
                if (!(std::fabs(a - b) <= 1e-12 * scale)) {
                    s.ho.valid = false;
                    char msg[320];
                    snprintf(msg, sizeof msg, "WM_HANDOVER_VERIFY: the plane behind WM_MEM_SLOT_OUT is not the plane the slot's last wm_embed wrote "
                             "(frame %d, Gram term %d: handed over %.17g, the plane now gives %.17g): it was modified after the embed", f, t, a, b);
                    return fail(ctx, WM_ERR_RUNTIME, msg);
                }
            }
        return WM_OK;
    }
    sweep_gram(ctx, s, K_GRAM, sw);
    return WM_OK;
}

int wm_detect(wm_ctx* ctx, int mask, const wm_plane* img, float* corr_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    const bool sync_after = slot == WM_SLOT_SYNC;
    if ((rc = check_plane(ctx, img, 0, false, "image", true)) != WM_OK) return rc;
    const int frames = img->frames;
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PlaneDesc xd;
    if ((rc = prep_input(ctx, s, img, &xd)) != WM_OK) return rc;
    const bool paired = s.pair.armed;  // a fused embed of wm_embed_detect is in flight in front of this call
    std::optional<FusedGuard> guard;
    bool take_fused = paired || ((ctx->cols % 4 == 0 || xd.dtype == WM_F32) && fused_call(ctx, sync_after, frames) && xd.aligned);
    if (take_fused && !ctx->pair_mode) {
        guard.emplace(ctx->device, ctx->fused_lock_fd);
        if (!guard->ok) { guard.reset(); ctx->fused_lock_skips++; take_fused = false; }
    }
    if (take_fused) {
        // one image per synchronous call: one launch, the frame's tiles resident in LDS (wm_k_fused.hip)
        OpResult* hres = s.h_res + s.res_used;
        hres->status = FUSED_PENDING;
        if (++s.fz_epoch == 0) s.fz_epoch = 1;
        int lrc;
        if (paired && s.pair.deferred) {
            ProfScope ps(ctx, K_FUSED_PAIR, s.stream);
            lrc = launch_fused_pair(s.stream, ctx->fg, s.fz, s.pair.epoch, s.fz_epoch, s.pair.mask, s.pair.xd, ctx->w->d_w, s.pair.bd, s.pair.od, ctx->sF,
                                    sqrt_n(ctx), s.d_res + s.pair.res_index, s.d_res + s.res_used);
        } else { ProfScope ps(ctx, K_FUSED_DETECT, s.stream); lrc = launch_fused_detect(s.stream, ctx->fg, s.fz, s.fz_epoch, mask, xd, ctx->w->d_w, s.d_res + s.res_used); }
        s.pair.deferred = false;
        OpResult got; got.status = FUSED_PENDING; got.value = 0.f;
        if (lrc == 0) {
            if ((rc = launch_check(ctx, s)) != WM_OK) { s.pair.armed = false; return rc; }
            if ((rc = fused_wait(ctx, s, hres, paired && s.pair.host_out, &got)) != WM_OK) { s.pair.armed = false; return rc; }
        }
        if (paired) {
            // the stream is in order: with the detector's record in (or the stream drained), the embed's record is final
            s.pair.armed = false;
            if (got.status == FUSED_PENDING) HIPCHK(ctx, hipStreamSynchronize(s.stream));
            const OpResult ge = load_record(s.h_res + s.pair.res_index);
            if (ge.status == FUSED_PENDING || ge.status == FUSED_INCOMPLETE) {
                // the embed did not complete: forget its queued result, back off, and let wm_embed_detect redo both on the
                // sweeps -- unless output stores went out over the call's own input (wm_embed's rule).  (A completed embed
                // with a detector that timed out is NOT re-run: the detector alone takes the sweeps below.)
                s.pending.pop_back();
                s.res_used = s.pair.res_index;
                s.last_out_frames = 0;
                if ((rc = fused_failed(ctx, s)) != WM_OK) return rc;
                if (ge.status == FUSED_INCOMPLETE && s.pair.out_overlaps_inputs) return fail_partly_watermarked(ctx);
                return PAIR_RETRY;
            }
        }
        if (lrc == 0) {
            if (got.status != FUSED_PENDING) {
                ctx->fused_backoff = 0;
                push_pending(s, frames, 1, false, corr_out, status_out, nullptr);
                return deliver(s);  // the record has arrived
            }
            if ((rc = fused_failed(ctx, s)) != WM_OK) return rc;  // (a detector writes nothing: the sweeps can always take the call)
        }
    }
    guard.reset();
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    const Sweep sw = detect_sweep(ctx, s, lg, frames, mask, xd);
    OpResult* res = s.d_res + s.res_used;
    // (a WM_MEM_SLOT_OUT plane under wm_set_handover keeps the promised hand-over of gram_sweep)
    if (!(img->mem == WM_MEM_SLOT_OUT && s.ho.promised) && checked_handover_applies(ctx, s, sw)) {
        // checked hand-over: the Gram matrix from the embed's sums, the detector checks the plane against the embed's digest, and
        // the frames it does not trust are redone by the ordinary sweeps (predicated on the device: empty launches otherwise)
        s.ho.used = true;
        const DigCheck dc{s.d_pdig, s.d_sdig, handover_of(ctx, s, s.ho.stride).fdig, s.d_redo, s.d_hocnt};
        { ProfScope ps(ctx, K_GRAM_HO_CHECKED, s.stream); gram_from_handover(ctx, s, sw); }
        sweep_detect(ctx, s, K_DETECT, sw, res, &dc, 1);
        sweep_gram(ctx, s, K_GRAM_REDO, sw, nullptr, s.d_redo);
        sweep_detect(ctx, s, K_DETECT_REDO, sw, res, &dc, 2);
    } else {
        if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
        sweep_detect(ctx, s, K_DETECT, sw, res);
    }
    return finish_call(ctx, s, slot, frames, 1, false, corr_out, status_out);
}

int wm_embed_detect(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, float* a_out,
                    float* corr_out, int* status_out, int slot)
{
    if (!ctx || !out) return WM_ERR_BAD_ARG;
    if (out->channels != 1) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_detect: grey output only (the detector reads the plane the embed wrote)");
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    const bool sync_after = slot == WM_SLOT_SYNC;
    // the detector's input: the device copy of what the embed writes (WM_MEM_SLOT_OUT) -- so on the sweeps the embed can hand
    // its output's lag sums over whether or not wm_set_handover is on (the detector's Gram sweep is not run)
    wm_plane slot_plane = *out;
    slot_plane.data = nullptr; slot_plane.mem = WM_MEM_SLOT_OUT;
    // the embed's promise is the pair's own (its detector reads the plane by construction): it ends with the pair.  Without
    // wm_set_handover the caller has promised nothing about the plane afterwards, so no later WM_MEM_SLOT_OUT detector may take the sums
    struct PairHo {
        wm_ctx* c; Slot& s;
        PairHo(wm_ctx* c_, Slot& s_) : c(c_), s(s_) { c->pair_handover = 1; }
        ~PairHo() { c->pair_handover = 0; if (!c->handover && s.ho.promised) { s.ho.promised = false; s.ho.used = true; } }
    } pair_ho(ctx, s);
    if (!sync_after) {
        // a slot in flight: the two operations queue behind each other, wm_sync delivers both
        if ((rc = wm_embed(ctx, mask, in_gray, base, out, a_out, status_out, slot)) < 0) return rc;
        return wm_detect(ctx, mask, &slot_plane, corr_out, nullptr, slot);
    }
    bool deferred;
    {
        // synchronous: when the fused kernels take the call, both launches go out back to back and the host waits ONCE, for
        // the detector's record (an in-order stream: that record completes the embed's too) -- one launch-to-poll round trip
        // and one host re-arm less than the two calls; the watermarked plane is read back from the caches
        FusedGuard guard(ctx->device, ctx->fused_lock_fd);
        // (the device's lock not obtained within the deadline: this pair runs on the sweeps)
        const int saved_mode = ctx->fused_mode;
        if (!guard.ok) { ctx->fused_lock_skips++; ctx->fused_mode = 0; }
        ctx->pair_mode = 1;
        s.pair.armed = false;
        rc = wm_embed(ctx, mask, in_gray, base, out, a_out, status_out, WM_SLOT_SYNC);
        deferred = rc == WM_OK && s.pair.armed;
        if (deferred) rc = wm_detect(ctx, mask, &slot_plane, corr_out, nullptr, WM_SLOT_SYNC);
        if (s.pair.deferred) {
            // the detector's call failed before it launched the pair: the embed it was to launch never ran -- forget its queued result
            s.pair.deferred = false;
            if (!s.pending.empty()) s.pending.pop_back();
            s.res_used = s.pair.res_index;
            s.last_out_frames = 0;
        }
        ctx->pair_mode = 0;
        ctx->fused_mode = saved_mode;
        s.pair.armed = false;
    }
    if (deferred && rc != PAIR_RETRY) return rc;
    if (deferred) {
        // the fused embed did not complete (a time-out; the context now backs off): the embed again, on the sweeps
        ctx->pair_mode = 1;
        rc = wm_embed(ctx, mask, in_gray, base, out, a_out, status_out, WM_SLOT_SYNC);
        ctx->pair_mode = 0;
    }
    // the embed went to the sweeps (queued, not waited for): the detector follows on the same stream and its wait delivers both
    if (rc < 0) return rc;
    const int rd = wm_detect(ctx, mask, &slot_plane, corr_out, nullptr, WM_SLOT_SYNC);
    if (rd < 0 && !s.pending.empty()) (void)do_sync(ctx, s);  // (never leave the embed's result queued behind a failed call)
    return rd;
}

// ---- key banks (wm_keys_*) and the multi-key detector ------------------------------------------------------------------
int wm_keys_create(wm_keys** out, int device, int rows, int cols, int nkeys)
{
    if (!out) return WM_ERR_BAD_ARG;
    *out = nullptr;
    if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768 || nkeys < 1 || nkeys > WM_KEYS_MAX) return WM_ERR_BAD_ARG;
    const int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    std::unique_ptr<wm_keys> k(new wm_keys);
    k->device = device; k->rows = rows; k->cols = cols; k->nkeys = nkeys;
    const size_t bytes = (size_t)nkeys * rows * cols * sizeof(float);
    if (hipMalloc((void**)&k->d, bytes) != hipSuccess) { (void)hipGetLastError(); k->d = nullptr; return WM_ERR_ALLOC; }
    if (hipMemset(k->d, 0, bytes) != hipSuccess) return WM_ERR_RUNTIME;
    *out = k.release();
    return WM_OK;
}

void wm_keys_destroy(wm_keys* keys) { delete keys; }

int wm_keys_count(const wm_keys* keys) { return keys ? keys->nkeys : 0; }
int wm_keys_rows(const wm_keys* keys) { return keys ? keys->rows : 0; }
int wm_keys_cols(const wm_keys* keys) { return keys ? keys->cols : 0; }
const float* wm_keys_device_ptr(const wm_keys* keys, int k)
{
    if (!keys || k < 0 || k >= keys->nkeys) return nullptr;
    return keys->d + (size_t)k * keys->rows * keys->cols;
}

int wm_keys_set(wm_keys* keys, int k, const float* w, int mem)
{
    if (!keys || !w || k < 0 || k >= keys->nkeys || (mem != WM_MEM_DEVICE && mem != WM_MEM_HOST)) return WM_ERR_BAD_ARG;
    if (hipSetDevice(keys->device) != hipSuccess) return WM_ERR_RUNTIME;
    const size_t n = (size_t)keys->rows * keys->cols;
    if (hipMemcpy(keys->d + (size_t)k * n, w, n * sizeof(float), mem == WM_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
        return WM_ERR_RUNTIME;
    return WM_OK;
}

int wm_keys_load_file(wm_keys* keys, int k, const char* path)
{
    if (!keys || !path || k < 0 || k >= keys->nkeys) return WM_ERR_BAD_ARG;
    std::vector<float> w;
    const int rc = read_w_file(nullptr, path, keys->rows, keys->cols, w);  // (loadRandomMatrix's checks: WM_ERR_W_OPEN, WM_ERR_W_SIZE)
    if (rc != WM_OK) return rc;
    return wm_keys_set(keys, k, w.data(), WM_MEM_HOST);
}

int wm_keys_generate(wm_keys* keys, int k, uint32_t seed)
{
    if (!keys || k < 0 || k >= keys->nkeys) return WM_ERR_BAD_ARG;
    if (hipSetDevice(keys->device) != hipSuccess) return WM_ERR_RUNTIME;
    // wm_create_generated's launch: the same kernel and grid, so the plane is that context's W bit for bit
    launch_gen_w(nullptr, keys->d + (size_t)k * keys->rows * keys->cols, keys->rows, keys->cols, seed);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return WM_ERR_RUNTIME;
    return WM_OK;
}

// a key bank fits a call: it lives on the engine's device and its planes have the engine's shape (exact) or are at least as
// large (wm_detect_offsets, whose windows move inside them)
static int check_bank(wm_ctx* ctx, const wm_keys* keys, const char* who, bool exact)
{
    const bool fits = exact ? keys->rows == ctx->rows && keys->cols == ctx->cols : keys->rows >= ctx->rows && keys->cols >= ctx->cols;
    if (keys->device == ctx->device && fits) return WM_OK;
    return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": the key bank is " + std::to_string(keys->rows) + "x" + std::to_string(keys->cols) + " on device " +
                                         std::to_string(keys->device) + ", the engine " + std::to_string(ctx->rows) + "x" + std::to_string(ctx->cols) +
                                         " on device " + std::to_string(ctx->device) + (exact ? "" : " (the bank must be at least as large)"));
}

// detectWatermark of every frame with `count` scores per frame (wm_detect_keys: the keys of a bank; wm_detect_offsets: the windows
// of one key): wm_detect's input, slot and Gram handling on the sweeps, the records [frames][count] delivered by wm_sync.
// launch(sw, part, rstride, res): the sweep behind the solve, != 0 when its geometry does not fit
extern "C++" {  // (a template cannot have C linkage)
template <class Launch>
static int detect_bank(wm_ctx* ctx, int mask, const wm_plane* img, long long count, const char* noun, const char* who, int kid, float* corr_out, int* status_out,
                       int slot, Launch launch)
{
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, count, noun, &sw)) != WM_OK) return rc;
    const int frames = img->frames;
    // partial records: [frames][count][rstride][2] + [frames][rstride] (one scratch for both calls: one stream, in order)
    const int rstride = std::max(ctx->max_nblk, ctx->max_nrec);
    const size_t need = (size_t)frames * (2 * (size_t)count + 1) * rstride * sizeof(double);
    if ((rc = ensure(ctx, &s.keys_part, &s.keys_part_bytes, need)) != WM_OK) return rc;
    // the image side is wm_detect's: the Gram sweep (or the hand-over of the slot's last embed) and the solve
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    {
        ProfScope ps(ctx, kid, s.stream);
        if (launch(sw, (double*)s.keys_part, rstride, s.d_res + s.res_used) != 0)
            return fail(ctx, WM_ERR_RUNTIME, std::string(who) + ": geometry exceeds the record arrays");
    }
    return finish_call(ctx, s, slot, frames, (int)count, false, corr_out, status_out);
}
}  // extern "C++"

int wm_detect_keys(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, float* corr_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!keys || !corr_out) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_keys: null keys or corr_out");
    if ((rc = check_bank(ctx, keys, "wm_detect_keys", true)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_detect_keys")) != WM_OK) return rc;
    return detect_bank(ctx, mask, img, keys->nkeys, "keys", "wm_detect_keys", K_DETECT_KEYS, corr_out, status_out, slot,
                       [&](const Sweep& sw, double* part, int rstride, OpResult* res) { return launch_detect_keys(sw, bank_of(ctx, keys), part, rstride, res); });
}

// every window of the rectangle lies inside the key plane (no device needed: wm_detect_offsets' own check)
int wm_offsets_check(int rows, int cols, int key_rows, int key_cols, int oy0, int ox0, int ny, int nx)
{
    if (rows < 1 || cols < 1 || key_rows < rows || key_cols < cols) return WM_ERR_BAD_ARG;
    if (ny < 1 || nx < 1 || oy0 < 0 || ox0 < 0) return WM_ERR_BAD_ARG;
    if ((long long)oy0 + ny - 1 + rows > key_rows || (long long)ox0 + nx - 1 + cols > key_cols) return WM_ERR_BAD_ARG;
    return WM_OK;
}

int wm_detect_offsets_group(void) { return detect_offsets_group(); }

// detectWatermark of every frame against the windows of ONE key at a rectangle of offsets: k_detect_offsets as detect_bank's sweep
int wm_detect_offsets(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k, int oy0, int ox0, int ny, int nx,
                      float* corr_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!img || !keys || !corr_out) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_offsets: null img, keys or corr_out");
    if (k < 0 || k >= keys->nkeys) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_offsets: key " + std::to_string(k) + " of a bank of " + std::to_string(keys->nkeys));
    if ((rc = check_bank(ctx, keys, "wm_detect_offsets", false)) != WM_OK) return rc;
    if (wm_offsets_check(ctx->rows, ctx->cols, keys->rows, keys->cols, oy0, ox0, ny, nx) != WM_OK)
        return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_offsets: offsets (" + std::to_string(oy0) + "," + std::to_string(ox0) + ") + " + std::to_string(ny) + "x" +
                                             std::to_string(nx) + " of " + std::to_string(ctx->rows) + "x" + std::to_string(ctx->cols) +
                                             " windows leave the " + std::to_string(keys->rows) + "x" + std::to_string(keys->cols) + " key plane");
    if ((rc = refuse_band(ctx, "wm_detect_offsets")) != WM_OK) return rc;
    // NOT aligned_w_of: the buffer descriptor of a window spans rows of the KEY plane's pitch, so that plane's extent decides the
    // 32-bit offsets
    const KeyBank key{keys->d + (size_t)k * keys->rows * keys->cols, 0, 1, fits_32bit(keys->rows, keys->cols, WM_F32) ? 1 : 0};
    return detect_bank(ctx, mask, img, (long long)ny * nx, "offsets", "wm_detect_offsets", K_DETECT_OFFSETS, corr_out, status_out, slot,
                       [&](const Sweep& sw, double* part, int rstride, OpResult* res) {
                           return launch_detect_offsets(sw, key, keys->cols, oy0, ox0, ny, nx, part, rstride, res);
                       });
}

// ---- wm_locate: the offset of a crop anywhere in its key, by FFT (wm_k_locate.hip, wm_k_fft.hip) ---------------------------------
static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
static int pow2_at_least(int n)
{
    int p = 1 << FFT_LOG_MIN;
    while (p < n) p <<= 1;
    return p;
}

int wm_locate_shape(int rows, int cols, int key_rows, int key_cols, int* ny, int* nx, int* pr, int* pc)
{
    if (!ny || !nx || !pr || !pc) return WM_ERR_BAD_ARG;
    constexpr int PMAX = 1 << FFT_LOG_MAX;
    if (rows < 1 || cols < 1 || key_rows < rows || key_cols < cols || key_rows > PMAX || key_cols > PMAX) return WM_ERR_BAD_ARG;
    *ny = key_rows - rows + 1; *nx = key_cols - cols + 1;
    *pr = pow2_at_least(key_rows); *pc = pow2_at_least(key_cols);
    return WM_OK;
}

namespace {
// what a call of the locate family asks of its scratch: the transform and offset shape, the frames' spectra it keeps (0: wm_locate,
// which finishes a frame before it starts the next), the bytes of its block records, and the bytes of the areas that only some calls
// have (0: none): the energy's per-frame records, the energy map and the per-bit maps of a wm_locate_bits call that passes none, the
// non-zero flags of wm_locate_keys
struct LocShape {
    int pr, pc, ny, nx, kept;
    size_t part, epart, energy, maps, nz;
};
// LocScratch over one allocation at `base`; returns its bytes.  base null: the areas' offsets, what loc_scratch compares
size_t loc_layout(void* base, int rows, int cols, const LocShape& sh, LocScratch* L)
{
    const size_t plane = (size_t)sh.pr * sh.pc * 2 * sizeof(float), img = round256((size_t)rows * cols * sizeof(float));
    char* p = (char*)base;
    const auto take = [&p](size_t bytes) { char* q = bytes ? p : nullptr; p += round256(bytes); return q; };
    L->pr = sh.pr; L->pc = sh.pc;
    L->plane_floats = (size_t)sh.pr * sh.pc * 2;
    L->tw_r = (float*)take((size_t)(sh.pr + sh.pc) * 2 * sizeof(float));
    L->tw_c = L->tw_r + (size_t)2 * sh.pr;
    L->hs = (float*)take(plane * sh.kept);
    L->a = (float*)take(plane);
    L->kw = (float*)take(plane);
    L->p = (float*)take(plane);
    L->e = (float*)take(img);
    L->m = (float*)take(img);
    L->energy = (float*)take(sh.energy);
    L->maps = (float*)take(sh.maps);
    L->part = take(sh.part);
    L->epart = take(sh.epart);
    L->nz = (int*)take(sh.nz);
    return (size_t)(p - (char*)base);
}

// forward 2-D transform of the [pr][pc] plane `a`; the spectrum lands TRANSPOSED ([pc][pr]) in `t`
void fft2_forward_t(hipStream_t st, const LocScratch& L, float* a, float* t)
{
    launch_fft_rows(st, a, L.pr, L.pc, L.tw_c, false);
    launch_fft_transpose(st, a, t, L.pr, L.pc);
    launch_fft_rows(st, t, L.pc, L.pr, L.tw_r, false);
}
// inverse 2-D transform of a transposed spectrum `t` ([pc][pr]); the plane lands in `a` ([pr][pc])
void fft2_inverse_t(hipStream_t st, const LocScratch& L, float* t, float* a)
{
    launch_fft_rows(st, t, L.pc, L.pr, L.tw_r, true);
    launch_fft_transpose(st, t, a, L.pc, L.pr);
    launch_fft_rows(st, a, L.pr, L.pc, L.tw_c, true);
}

// the slot's scratch of one call kind for a call's shape, its tables filled.  THE RESHAPE RULE: the calls still queued on the slot
// hold the pointers of the layout they were given and read its tables, and the tables are filled by a blocking copy.  So whenever
// the transform shape or the offset of any area differs from the layout the allocation was last filled for, or the allocation has
// to grow, the call first waits for the slot's stream, then moves the layout and fills the tables again; in every other case it
// takes the allocation as it is and waits for nothing.  (The size of the LAST area moves no pointer: a wm_locate call whose key has
// another number of offsets under the same transform does not wait)
int loc_scratch(wm_ctx* ctx, Slot& s, int kind, const LocShape& sh, LocScratch* L)
{
    int rc;
    LocAlloc& al = s.loc[kind];
    LocScratch at{};
    const size_t need = loc_layout(nullptr, ctx->rows, ctx->cols, sh, &at);
    const bool reshape = std::memcmp(&at, &al.at, sizeof at) != 0 || al.bytes < need;
    if (reshape) {
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        al.at = LocScratch{};
        if ((rc = ensure(ctx, &al.p, &al.bytes, need, WM_ERR_ALLOC)) != WM_OK) return rc;
    }
    loc_layout(al.p, ctx->rows, ctx->cols, sh, L);
    if (reshape) {
        HIPCHK(ctx, fft_twiddles_upload(L->tw_r, sh.pr, sh.pc));
        al.at = at;
    }
    return WM_OK;
}

// the call's own copy of `count` host ints in the slot's table arena (the caller's array is free when the call returns; count 0: no
// table), and behind it, where `zero` is asked for, a DEVICE int that holds 0 for the call's kernels: the status of a pooled plane,
// which has no solve of its own.  Both in ONE request, for a call takes table room once: a second request may move the arenas and
// free the block the first pointer lies in
int call_ints(wm_ctx* ctx, Slot& s, const int32_t* src, int count, const int** dev, const int** zero)
{
    int rc;
    void *th = nullptr, *td = nullptr;
    const size_t bytes = ((size_t)count + (zero ? 1 : 0)) * sizeof(int);
    if ((rc = table_room(ctx, s, bytes, &th, &td)) != WM_OK) return rc;
    if (count) std::memcpy(th, src, (size_t)count * sizeof(int));
    if (zero) { ((int*)th)[count] = 0; *zero = (const int*)td + count; }
    if ((rc = table_upload(ctx, s, th, td, bytes)) != WM_OK) return rc;
    *dev = (const int*)td;
    return WM_OK;
}

// what the six calls of the family share in front of their image side: the geometry, and the refusals from the key range on.  Keys
// k0 .. k0 + nk - 1 of the bank (`range`: the call takes a range, and says so); plane: the image plane, null for a pooled call,
// which has one frame and no plane to check; per_frame, noun: the call's records per frame, as check_res_room words them
struct LocCall { int ny, nx, pr, pc, frames; };
int locate_front(wm_ctx* ctx, const std::string& who, const wm_plane* plane, const wm_keys* keys, int k0, int nk, bool range, long long per_frame,
                 const char* noun, int slot, LocCall* c)
{
    int rc;
    if (k0 < 0 || nk < 1 || (long long)k0 + nk > keys->nkeys)
        return fail(ctx, WM_ERR_BAD_ARG, who + (range ? ": keys " + std::to_string(k0) + " .. " + std::to_string((long long)k0 + nk - 1) : ": key " + std::to_string(k0)) +
                                             " of a bank of " + std::to_string(keys->nkeys));
    if ((rc = check_bank(ctx, keys, who.c_str(), false)) != WM_OK) return rc;
    if (wm_locate_shape(ctx->rows, ctx->cols, keys->rows, keys->cols, &c->ny, &c->nx, &c->pr, &c->pc) != WM_OK)
        return fail(ctx, WM_ERR_BAD_ARG, who + ": a " + std::to_string(keys->rows) + "x" + std::to_string(keys->cols) +
                                             " key plane needs a transform above " + std::to_string(1 << FFT_LOG_MAX) + " per axis");
    if ((rc = refuse_band(ctx, who.c_str())) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    // (open_input checks the plane and the record room again: both have to be known HERE, in front of a call's own checks, of
    // per_frame narrowed to an int, and of any device work)
    if (plane && (rc = check_plane(ctx, plane, 0, false, "image", true)) != WM_OK) return rc;
    c->frames = plane ? plane->frames : 1;
    return check_res_room(ctx, slot_of(ctx, slot), c->frames * per_frame, noun);
}

// the image side of wm_locate, wm_locate_bits and wm_locate_keys: the Gram sweep and the solve (wm_detect_keys'), then the frames
// one after the other: e (and m), h laid into L.a and, in a call that keeps the spectra, its forward transform into L.hs[f];
// then(f): what the call does with frame f at once
int locate_image_side(wm_ctx* ctx, Slot& s, const Sweep& sw, const wm_plane* img, const LocScratch& L, const std::function<void(int)>& then)
{
    const int rc = gram_sweep(ctx, s, sw, img);
    if (rc != WM_OK) return rc;
    for (int f = 0; f < sw.frames; ++f) {
        launch_locate_e(sw, f, L.e, L.m);
        launch_locate_h(sw, f, L.e, L.m, L.a, L.pr, L.pc);
        if (L.hs) fft2_forward_t(s.stream, L, L.a, L.hs + f * L.plane_floats);
        then(f);
    }
    return WM_OK;
}
// the image side of the pooled calls: a caller's pooled plane (wm_clip_pool) in the place of one frame's h -- a dense real plane, as
// a key is --, and its spectrum where the call keeps one.  table (count ints; null, 0: none): the call's table; *status: the zero word
int locate_pooled_side(wm_ctx* ctx, Slot& s, int kind, const LocShape& sh, const float* pool_dev, const int32_t* table, int count, LocScratch* L,
                       const int** table_dev, const int** status)
{
    int rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = loc_scratch(ctx, s, kind, sh, L)) != WM_OK) return rc;
    if ((rc = call_ints(ctx, s, table, count, table_dev, status)) != WM_OK) return rc;
    launch_locate_lay(s.stream, pool_dev, ctx->rows, ctx->cols, L->a, L->pr, L->pc);
    if (L->hs) fft2_forward_t(s.stream, *L, L->a, L->hs);
    return WM_OK;
}

// the device benches' clock: pass p is launch(p) once untimed, then `iters` times back to back between two events on the null
// stream; us_out[p]: its mean microseconds per launch
bool bench_passes(int passes, int iters, double* us_out, const std::function<void(int)>& launch)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    for (int p = 0; ok && p < passes; ++p) {
        for (int i = -1; i < iters; ++i) {  // (one untimed launch in front)
            if (i == 0) ok = ok && hipEventRecord(e0, nullptr) == hipSuccess;
            launch(p);
        }
        float ms = 0.f;
        ok = ok && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
             hipGetLastError() == hipSuccess;
        us_out[p] = (double)ms * 1e3 / iters;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ok;
}

// wm_locate's scratch: three planes and the block records of one map
LocShape locate_shape_of(const LocCall& c) { return LocShape{c.pr, c.pc, c.ny, c.nx, 0, locate_part_bytes(c.ny, c.nx), 0, 0, 0, 0}; }
// the key's spectrum, once per call (transposed, in L.kw; L.p is the plane it is laid into)
void locate_key_spectrum(Slot& s, const LocScratch& L, const wm_keys* keys, int k)
{
    launch_locate_lay(s.stream, keys->d + (size_t)k * keys->rows * keys->cols, keys->rows, keys->cols, L.p, L.pr, L.pc);
    fft2_forward_t(s.stream, L, L.p, L.kw);
}
// wm_locate's tail of one image-side plane h laid into L.a: its spectrum, conj(H) Wf in place, back, the map and its four numbers
void locate_tail(Slot& s, const LocScratch& L, const LocCall& c, const int* status, float* map, OpResult* res)
{
    fft2_forward_t(s.stream, L, L.a, L.p);
    launch_locate_mul(s.stream, L.p, L.kw, (size_t)L.pr * L.pc);
    fft2_inverse_t(s.stream, L, L.p, L.a);
    launch_locate_map(s.stream, L.a, L.pr, L.pc, c.ny, c.nx, status, nullptr, false, map, nullptr, L.part, res);
}
}  // namespace

int wm_locate(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k, float* loc_out, float* map_dev, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!img || !keys || (!loc_out && !map_dev)) return fail(ctx, WM_ERR_BAD_ARG, "wm_locate: null img or keys, or loc_out and map_dev both null");
    LocCall c;
    if ((rc = locate_front(ctx, "wm_locate", img, keys, k, 1, false, WM_LOCATE_NVALS, "4 location records", slot, &c)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, WM_LOCATE_NVALS, "4 location records", &sw)) != WM_OK) return rc;
    LocScratch L;
    if ((rc = loc_scratch(ctx, s, LOC_PLAIN, locate_shape_of(c), &L)) != WM_OK) return rc;
    locate_key_spectrum(s, L, keys, k);
    // frame-major: a frame's tail runs before the next frame's h takes L.a
    const size_t n = (size_t)c.ny * c.nx;
    rc = locate_image_side(ctx, s, sw, img, L, [&](int f) {
        locate_tail(s, L, c, s.d_status + f, map_dev ? map_dev + f * n : nullptr, s.d_res + s.res_used + WM_LOCATE_NVALS * f);
    });
    if (rc != WM_OK) return rc;
    return finish_call(ctx, s, slot, c.frames, WM_LOCATE_NVALS, false, loc_out, status_out);
}

// wm_locate's tail on a caller's pooled image-side plane (wm_clip_pool) in the place of one frame's h
int wm_locate_pooled(wm_ctx* ctx, const float* pool_dev, const wm_keys* keys, int k, float* loc_out, float* map_dev, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc;
    if (!pool_dev || !keys || (!loc_out && !map_dev))
        return fail(ctx, WM_ERR_BAD_ARG, "wm_locate_pooled: null pool_dev or keys, or loc_out and map_dev both null");
    LocCall c;
    if ((rc = locate_front(ctx, "wm_locate_pooled", nullptr, keys, k, 1, false, WM_LOCATE_NVALS, "4 location records", slot, &c)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    LocScratch L;
    const int *none = nullptr, *status = nullptr;
    if ((rc = locate_pooled_side(ctx, s, LOC_PLAIN, locate_shape_of(c), pool_dev, nullptr, 0, &L, &none, &status)) != WM_OK) return rc;
    locate_key_spectrum(s, L, keys, k);
    locate_tail(s, L, c, status, map_dev, s.d_res + s.res_used);
    return finish_call(ctx, s, slot, 1, WM_LOCATE_NVALS, false, loc_out, nullptr);
}


// the frames of a clip pooled on the image side: wm_locate's Gram sweep and solve, then ONE launch of k_clip_pool
int wm_clip_pool(wm_ctx* ctx, int mask, const wm_plane* img, const float* weights, float* pool_dev, int accumulate, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!img || !pool_dev) return fail(ctx, WM_ERR_BAD_ARG, "wm_clip_pool: null img or pool_dev");
    if ((rc = refuse_band(ctx, "wm_clip_pool")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    // (open_input checks the plane and the record room again: the frame count has to be known HERE, in front of the weights' check)
    if ((rc = check_plane(ctx, img, 0, false, "image", true)) != WM_OK) return rc;
    const int frames = img->frames;
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    for (int f = 0; weights && f < frames; ++f)
        if (!std::isfinite(weights[f])) return fail(ctx, WM_ERR_BAD_ARG, "wm_clip_pool: weights[" + std::to_string(f) + "] is not finite");
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, 1, nullptr, &sw)) != WM_OK) return rc;
    // the call's own copy of the weights (the caller's array is free when this function returns)
    void *th = nullptr, *td = nullptr;
    if ((rc = table_room(ctx, s, (size_t)frames * sizeof(float), &th, &td)) != WM_OK) return rc;
    for (int f = 0; f < frames; ++f) ((float*)th)[f] = weights ? weights[f] : 1.0f;
    if ((rc = table_upload(ctx, s, th, td, (size_t)frames * sizeof(float))) != WM_OK) return rc;
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    launch_clip_pool(sw, (const float*)td, pool_dev, accumulate != 0, s.d_res + s.res_used);
    return finish_call(ctx, s, slot, frames, 1, false, nullptr, status_out);
}

// k_clip_pool (x and e tiles in LDS) and k_clip_pool_gather (a direct gather from cache), each launched `iters` times back to back
// between two events on the null stream over `frames` dense f32 frames of rows x cols: mean microseconds per launch, and whether the
// two pools have equal bits (tools/locate_clip_bench.py holds them against wm_membench's copy)
int wm_clip_pool_bench(int device, int rows, int cols, int frames, int mask, int p, int iters, double* us_out, int* equal_out)
{
    if (!us_out || !equal_out || iters < 1 || rows < 1 || cols < 1 || rows > 32768 || cols > 32768 || frames < 1 || frames > 1024 ||
        (mask != WM_MASK_ME && mask != WM_MASK_NVF) || p < 3 || p > 9 || p % 2 == 0 || (mask == WM_MASK_ME && p != 3))
        return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    const size_t n = (size_t)rows * cols, img = round256(n * sizeof(float)), small = round256((size_t)frames * 8 * sizeof(float));
    const size_t total = (size_t)frames * img + 2 * img + 4 * small;
    char* scr = nullptr;
    if (hipMalloc((void**)&scr, total) != hipSuccess) { (void)hipGetLastError(); return WM_ERR_ALLOC; }
    float* pool[2] = {(float*)(scr + (size_t)frames * img), (float*)(scr + (size_t)frames * img + img)};
    char* tail = scr + (size_t)frames * img + 2 * img;
    float* coef = (float*)tail; int* status = (int*)(tail + small); float* weights = (float*)(tail + 2 * small); OpResult* res = (OpResult*)(tail + 3 * small);
    // frames that differ: a hash of the index in 0 .. 255, as 8-bit pixels; coefficients 1/8 (a plain mean of the neighbours)
    std::vector<float> hx((size_t)frames * (img / sizeof(float)), 0.0f), hc((size_t)frames * 8, 0.125f), hw((size_t)frames, 1.0f);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = (float)(((i * 2654435761ull) >> 13) & 255);
    bool ok = hipMemset(scr, 0, total) == hipSuccess && hipMemcpy(scr, hx.data(), hx.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(coef, hc.data(), hc.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(weights, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    Sweep sw{};
    sw.s = nullptr; sw.lg.rows = rows; sw.lg.cols = cols; sw.frames = frames; sw.mask = mask; sw.pad = p / 2;
    sw.x = PlaneDesc{scr, cols, (long long)(img / sizeof(float)), 0, WM_F32, 1, 0};
    sw.coef = coef; sw.status = status;
    ok = ok && bench_passes(WM_CLIP_POOL_BENCH_ROUTES, iters, us_out, [&](int route) {
             if (route == 0) launch_clip_pool(sw, weights, pool[0], false, res);
             else launch_clip_pool_gather(sw, weights, pool[1], false, res);
         });
    if (ok) {
        std::vector<float> a(n), b(n);
        ok = hipMemcpy(a.data(), pool[0], n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(b.data(), pool[1], n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
        *equal_out = ok && std::memcmp(a.data(), b.data(), n * sizeof(float)) == 0 ? 1 : 0;
    }
    (void)hipFree(scr);
    return ok ? WM_OK : WM_ERR_RUNTIME;
}

int wm_fft2(int device, float* data_dev, int pr, int pc, int inverse)
{
    if (!data_dev || fft_log2(pr) < 0 || fft_log2(pc) < 0) return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    const size_t plane = (size_t)pr * pc * 2 * sizeof(float);
    float* scr = nullptr;
    if (hipMalloc((void**)&scr, plane + (size_t)(pr + pc) * 2 * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return WM_ERR_ALLOC; }
    float* tw_r = scr + (size_t)pr * pc * 2;
    float* tw_c = tw_r + (size_t)pr * 2;
    bool ok = fft_twiddles_upload(tw_r, pr, pc) == hipSuccess;
    if (ok) {
        // rows, transpose, rows (the columns), transpose back
        launch_fft_rows(nullptr, data_dev, pr, pc, tw_c, inverse != 0);
        launch_fft_transpose(nullptr, data_dev, scr, pr, pc);
        launch_fft_rows(nullptr, scr, pc, pr, tw_r, inverse != 0);
        launch_fft_transpose(nullptr, scr, data_dev, pc, pr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    (void)hipFree(scr);
    return ok ? WM_OK : WM_ERR_RUNTIME;
}

// the seven passes of one forward + product + inverse transform of wm_locate, each launched `iters` times back to back between two
// events on the null stream: mean microseconds per launch (tools/locate_bench.py holds them against wm_membench's copy)
int wm_fft_bench(int device, int pr, int pc, int iters, double* us_out)
{
    if (!us_out || iters < 1 || fft_log2(pr) < 0 || fft_log2(pc) < 0) return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    const size_t plane = (size_t)pr * pc * 2 * sizeof(float);
    float* scr = nullptr;
    if (hipMalloc((void**)&scr, 2 * plane + (size_t)(pr + pc) * 2 * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return WM_ERR_ALLOC; }
    float* a = scr;
    float* b = scr + (size_t)pr * pc * 2;
    float* tw_r = b + (size_t)pr * pc * 2;
    float* tw_c = tw_r + (size_t)pr * 2;
    const bool ok = hipMemset(scr, 0, 2 * plane) == hipSuccess && fft_twiddles_upload(tw_r, pr, pc) == hipSuccess &&
                    bench_passes(WM_FFT_BENCH_PASSES, iters, us_out, [&](int pass) {
                        switch (pass) {
                        case 0: launch_fft_rows(nullptr, a, pr, pc, tw_c, false); break;
                        case 1: launch_fft_transpose(nullptr, a, b, pr, pc); break;
                        case 2: launch_fft_rows(nullptr, b, pc, pr, tw_r, false); break;
                        case 3: launch_locate_mul(nullptr, b, a, (size_t)pr * pc); break;
                        case 4: launch_fft_rows(nullptr, b, pc, pr, tw_r, true); break;
                        case 5: launch_fft_transpose(nullptr, b, a, pc, pr); break;
                        default: launch_fft_rows(nullptr, a, pr, pc, tw_c, true); break;
                        }
                    });
    (void)hipFree(scr);
    return ok ? WM_OK : WM_ERR_RUNTIME;
}

// tiles per axis of wm_detect_tiles: the last tile of each axis takes the remainder (pure host arithmetic)
int wm_tiles_shape(int rows, int cols, int tile_rows, int tile_cols, int* ny, int* nx)
{
    if (!ny || !nx) return WM_ERR_BAD_ARG;
    if (rows < 1 || cols < 1 || rows > 32768 || cols > 32768) return WM_ERR_BAD_ARG;
    if (tile_rows < 32 || tile_rows % 8 != 0 || tile_cols < 32 || tile_cols % 4 != 0) return WM_ERR_BAD_ARG;
    *ny = std::max(1, rows / tile_rows);
    *nx = std::max(1, cols / tile_cols);
    return WM_OK;
}

// ---- the tile calls' front: the tile grid of the engine's plane, and a payload's table over it
static int tiles_checked(wm_ctx* ctx, const char* who, int tile_rows, int tile_cols, TileShape* ts)
{
    ts->th = tile_rows; ts->tw = tile_cols;
    if (wm_tiles_shape(ctx->rows, ctx->cols, tile_rows, tile_cols, &ts->ny, &ts->nx) == WM_OK) return WM_OK;
    return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": tile shape " + std::to_string(tile_rows) + "x" + std::to_string(tile_cols) +
                                         " (rows: a multiple of 8, >= 32; columns: a multiple of 4, >= 32)");
}

// nbits and tile_bit [T] of wm_embed_bits / wm_detect_bits: every entry in -1 .. nbits - 1
static int tile_bits_checked(wm_ctx* ctx, const char* who, const int32_t* tile_bit, long long T, int nbits)
{
    bool ok = nbits >= 1 && nbits <= 4096;
    for (long long t = 0; ok && t < T; ++t) ok = tile_bit[t] >= -1 && tile_bit[t] < nbits;
    return ok ? WM_OK : fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": nbits must be 1 .. 4096 and every tile_bit entry -1 .. nbits - 1");
}

// detectWatermark of every frame against the context's W with the three sums kept per tile: wm_detect's input and slot
// handling on the sweeps, k_detect_tiles + k_tiles_fold in k_detect's place; the map stays on the device
int wm_detect_tiles(wm_ctx* ctx, int mask, const wm_plane* img, int tile_rows, int tile_cols, float* map_dev, double* sums_dev,
                    int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!img || !map_dev) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_tiles: null img or map_dev");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_detect_tiles", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_detect_tiles")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, 1, nullptr, &sw)) != WM_OK) return rc;
    const int frames = img->frames;
    const TilesPlan pl = tiles_plan(sw, aligned_w_of(ctx), ts);
    if ((rc = ensure(ctx, &s.tiles_rec, &s.tiles_rec_bytes, pl.rec_bytes)) != WM_OK) return rc;
    OpResult* res = s.d_res + s.res_used;
    // the image side is wm_detect's: the Gram sweep (or the hand-over of the slot's last embed) and the solve
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    { ProfScope ps(ctx, K_DETECT_TILES, s.stream); launch_detect_tiles(sw, pl, own_w(ctx), (float*)s.tiles_rec); }
    { ProfScope ps(ctx, K_TILES_FOLD, s.stream); launch_tiles_fold(s.stream, pl, frames, (const float*)s.tiles_rec, s.d_status, map_dev, sums_dev, res); }
    return finish_call(ctx, s, slot, frames, 1, false, nullptr, status_out);
}

// wm_detect_tiles with every key of the bank in the place of the context's W: wm_detect_keys' image side (one Gram sweep or
// hand-over and one solve per frame), k_detect_keys_tiles + k_keys_tiles_fold behind it; map and sums stay on the device.  The two
// kernels are launched outside any ProfScope: the list of profiling names is not extended for them
int wm_detect_keys_tiles(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int tile_rows, int tile_cols, float* map_dev,
                         double* sums_dev, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!img || !keys || !map_dev) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_keys_tiles: null img, keys or map_dev");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_detect_keys_tiles", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = check_bank(ctx, keys, "wm_detect_keys_tiles", true)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_detect_keys_tiles")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    // (open_input checks the plane again: img->frames has to be known to be sane HERE, for the grid check in front of any device work)
    if ((rc = check_plane(ctx, img, 0, false, "image", true)) != WM_OK) return rc;
    const int frames = img->frames, nkeys = keys->nkeys;
    if (!keys_tiles_grids_fit(ctx->rows, ctx->cols, tile_rows, frames, nkeys, ts.ny, ts.nx))
        return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_keys_tiles: " + std::to_string(frames) + " frames x " + std::to_string(nkeys) + " keys x " +
                                             std::to_string(ts.ny) + "x" + std::to_string(ts.nx) + " tiles exceed a launch grid of 31 bits");
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, 1, nullptr, &sw)) != WM_OK) return rc;
    const TilesPlan pl = tiles_plan(sw, aligned_w_of(ctx), ts);
    if ((rc = ensure(ctx, &s.keys_tiles_rec, &s.keys_tiles_rec_bytes, keys_tiles_rec_bytes(pl, frames, nkeys), WM_ERR_ALLOC)) != WM_OK) return rc;
    OpResult* res = s.d_res + s.res_used;
    // the image side is wm_detect's: the Gram sweep (or the hand-over of the slot's last embed) and the solve
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    launch_detect_keys_tiles(sw, pl, bank_of(ctx, keys), (float*)s.keys_tiles_rec);
    launch_keys_tiles_fold(s.stream, pl, frames, nkeys, (const float*)s.keys_tiles_rec, s.d_status, map_dev, sums_dev, res);
    return finish_call(ctx, s, slot, frames, 1, false, nullptr, status_out);
}

// ---- a payload in the mark: wm_bits_layout, wm_embed_signs, wm_embed_bits, wm_detect_bits --------------------------------------
// which bit does tile t carry?  A Fisher-Yates shuffle of 0 .. T - 1 driven by splitmix64(seed), then mod nbits: every bit owns
// floor(T / nbits) or ceil(T / nbits) tiles, spread over the frame (pure host arithmetic)
int wm_bits_layout(int ny, int nx, int nbits, uint64_t seed, int32_t* tile_bit)
{
    if (!tile_bit || ny < 1 || nx < 1) return WM_ERR_BAD_ARG;
    const long long T = (long long)ny * nx;
    if (nbits < 1 || nbits > 4096 || nbits > T || T > (1LL << 30)) return WM_ERR_BAD_ARG;
    std::vector<int32_t> perm((size_t)T);
    for (long long t = 0; t < T; ++t) perm[(size_t)t] = (int32_t)t;
    uint64_t state = seed;
    for (long long i = T - 1; i >= 1; --i) {
        state += 0x9E3779B97F4A7C15ULL;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        std::swap(perm[(size_t)i], perm[(size_t)(z % (uint64_t)(i + 1))]);
    }
    for (long long t = 0; t < T; ++t) tile_bit[t] = perm[(size_t)t] % nbits;
    return WM_OK;
}

// makeWatermark with the watermark term of every pixel multiplied by the sign of its tile: wm_embed's input, base and output
// handling and its Gram, solve and stats sweeps (||u|| does not see the signs); k_embed_signs in k_embed's place.  Never the fused
// kernels, no Gram hand-over.  k_embed_signs is launched outside any ProfScope: the list of profiling names is not extended for it
int wm_embed_signs(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows, int tile_cols,
                   const int8_t* signs, float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!in_gray || !base || !out || !signs) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs: null in_gray, base, out or signs");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_embed_signs", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_embed_signs")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_embed_planes(ctx, in_gray, base, out)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    const size_t nsigns = (size_t)frames * ts.ny * ts.nx;
    for (size_t i = 0; i < nsigns; ++i)
        if (signs[i] < -1 || signs[i] > 1)
            return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs: sign " + std::to_string((int)signs[i]) + " at index " + std::to_string(i) + " (must be -1, 0 or +1)");
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));

    // the call's own copy of the table: the caller's array is free when this function returns (uploaded in front of the planes' staging copies)
    void *th = nullptr, *td = nullptr;
    if ((rc = table_room(ctx, s, nsigns, &th, &td)) != WM_OK) return rc;
    std::memcpy(th, signs, nsigns);
    if ((rc = table_upload(ctx, s, th, td, nsigns)) != WM_OK) return rc;

    EmbedCall c;  // (no hand-over of its own)
    if ((rc = embed_stage(ctx, s, in_gray, base, out, &c)) != WM_OK) return rc;
    if ((rc = embed_snapshot(ctx, s, in_gray, &c)) != WM_OK) return rc;
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    const Sweep sw = mask_route(ctx, s, lg, frames, mask, c.xd);
    if (mask == WM_MASK_ME) sweep_gram(ctx, s, K_GRAM, sw);
    sweep_stats(ctx, s, true, sw, s.d_res + s.res_used);
    launch_embed_signs(sw, own_w(ctx), EmbedPlanes{c.bd, c.od, s.d_scal}, (const signed char*)td, ts);
    return embed_close(ctx, s, out, c, a_out, status_out, slot);
}

// a host layer over wm_embed_signs: tile t carries payload bit tile_bit[t] as +1 (bit set) or -1, or nothing (tile_bit[t] = -1)
int wm_embed_bits(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows, int tile_cols,
                  const int32_t* tile_bit, int nbits, const uint8_t* payload, float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!in_gray || !tile_bit || !payload) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_bits: null in_gray, tile_bit or payload");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_embed_bits", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    const long long T = (long long)ts.ny * ts.nx;
    if ((rc = tile_bits_checked(ctx, "wm_embed_bits", tile_bit, T, nbits)) != WM_OK) return rc;
    if (in_gray->frames < 1 || in_gray->frames > ctx->max_frames)
        return fail(ctx, WM_ERR_BAD_ARG, "in_gray: frames=" + std::to_string(in_gray->frames) + " exceeds wm_configure max_frames=" + std::to_string(ctx->max_frames));
    const int frames = in_gray->frames, pbytes = (nbits + 7) / 8;
    std::vector<int8_t> signs((size_t)frames * T);
    for (int f = 0; f < frames; ++f)
        for (long long t = 0; t < T; ++t) {
            const int b = tile_bit[t];
            signs[(size_t)f * T + t] = b < 0 ? 0 : (((payload[(size_t)f * pbytes + b / 8] >> (b % 8)) & 1) ? 1 : -1);
        }
    return wm_embed_signs(ctx, mask, in_gray, base, out, tile_rows, tile_cols, signs.data(), a_out, status_out, slot);
}

// wm_detect_tiles with one more fold: the tile sums land in slot-owned scratch and k_bits_fold adds each bit's tiles in ascending
// tile index into one result record per (frame, bit).  k_bits_fold is launched outside any ProfScope
int wm_detect_bits(wm_ctx* ctx, int mask, const wm_plane* img, int tile_rows, int tile_cols, const int32_t* tile_bit, int nbits, float* soft_out,
                   int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!img || !tile_bit || !soft_out) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_bits: null img, tile_bit or soft_out");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_detect_bits", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    const int T = ts.ny * ts.nx;
    if ((rc = tile_bits_checked(ctx, "wm_detect_bits", tile_bit, T, nbits)) != WM_OK) return rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_detect_bits")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, nbits, "bits", &sw)) != WM_OK) return rc;
    const int frames = img->frames;
    const TilesPlan pl = tiles_plan(sw, aligned_w_of(ctx), ts);
    if ((rc = ensure(ctx, &s.tiles_rec, &s.tiles_rec_bytes, pl.rec_bytes)) != WM_OK) return rc;
    // the tile fold's output: sums [frames][T][3] f64, its status records [frames], map [frames][T] f32
    const size_t nt = (size_t)frames * T;
    if ((rc = ensure(ctx, &s.bits_scr, &s.bits_scr_bytes, nt * 3 * sizeof(double) + (size_t)frames * sizeof(OpResult) + nt * sizeof(float))) != WM_OK) return rc;
    double* sums = (double*)s.bits_scr;
    OpResult* tres = (OpResult*)(sums + nt * 3);
    float* map = (float*)(tres + frames);
    // the tiles of every bit in ascending index: start [nbits + 1], idx [tiles that carry a bit] (a counting sort, stable)
    void *th = nullptr, *td = nullptr;
    const size_t tab = ((size_t)nbits + 1 + T) * sizeof(int);
    if ((rc = table_room(ctx, s, tab, &th, &td)) != WM_OK) return rc;
    int* start = (int*)th;
    int* idx = start + nbits + 1;
    std::fill(start, start + nbits + 1, 0);
    for (int t = 0; t < T; ++t)
        if (tile_bit[t] >= 0) start[tile_bit[t] + 1]++;
    for (int b = 0; b < nbits; ++b) start[b + 1] += start[b];
    {
        std::vector<int> fill(start, start + nbits);
        for (int t = 0; t < T; ++t)
            if (tile_bit[t] >= 0) idx[fill[tile_bit[t]]++] = t;
    }
    if ((rc = table_upload(ctx, s, th, td, tab)) != WM_OK) return rc;
    // the image side is wm_detect's: the Gram sweep (or the hand-over of the slot's last embed) and the solve
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    { ProfScope ps(ctx, K_DETECT_TILES, s.stream); launch_detect_tiles(sw, pl, own_w(ctx), (float*)s.tiles_rec); }
    { ProfScope ps(ctx, K_TILES_FOLD, s.stream); launch_tiles_fold(s.stream, pl, frames, (const float*)s.tiles_rec, s.d_status, map, sums, tres); }
    launch_bits_fold(s.stream, frames, nbits, T, sums, (const int*)td, (const int*)td + nbits + 1, s.d_status, s.d_res + s.res_used);
    return finish_call(ctx, s, slot, frames, nbits, false, soft_out, status_out);
}

// ---- wm_locate_bits: a payload-marked crop found and read without a hint ---------------------------------
int wm_locate_bits_cover(int rows, int cols, int key_rows, int key_cols, int tile_rows, int tile_cols, const int32_t* tile_bit, int nbits, int oy,
                         int ox, int64_t* pixels_out)
{
    int ny, nx, pr, pc, tny, tnx;
    if (!tile_bit || !pixels_out || nbits < 1 || nbits > 4096) return WM_ERR_BAD_ARG;
    if (wm_locate_shape(rows, cols, key_rows, key_cols, &ny, &nx, &pr, &pc) != WM_OK) return WM_ERR_BAD_ARG;
    if (wm_tiles_shape(key_rows, key_cols, tile_rows, tile_cols, &tny, &tnx) != WM_OK) return WM_ERR_BAD_ARG;
    if (oy < 0 || oy >= ny || ox < 0 || ox >= nx) return WM_ERR_BAD_ARG;
    for (int t = 0; t < tny * tnx; ++t)
        if (tile_bit[t] < -1 || tile_bit[t] >= nbits) return WM_ERR_BAD_ARG;
    std::fill(pixels_out, pixels_out + nbits, (int64_t)0);
    for (int ty = 0; ty < tny; ++ty) {
        // the tile's rows [r0, r1) of the key plane (the last tile takes the remainder) cut with the window's [oy, oy + rows)
        const int r0 = ty * tile_rows, r1 = ty == tny - 1 ? key_rows : r0 + tile_rows;
        const int64_t hr = std::min(r1, oy + rows) - std::max(r0, oy);
        if (hr <= 0) continue;
        for (int tx = 0; tx < tnx; ++tx) {
            const int c0 = tx * tile_cols, c1 = tx == tnx - 1 ? key_cols : c0 + tile_cols;
            const int64_t wc = std::min(c1, ox + cols) - std::max(c0, ox);
            const int b = tile_bit[ty * tnx + tx];
            if (wc > 0 && b >= 0) pixels_out[b] += hr * wc;
        }
    }
    return WM_OK;
}

namespace {
// what wm_locate_bits and wm_locate_bits_pooled check behind the family's front: the tile grid of the KEY plane and the table over
// it; has: which bits have a tile at all
struct LocBitsCall { LocCall c; TileShape ts; std::vector<char> has; };
int locate_bits_checks(wm_ctx* ctx, const std::string& who, const wm_plane* plane, const wm_keys* keys, int k, int tile_rows, int tile_cols,
                       const int32_t* tile_bit, int nbits, int slot, LocBitsCall* b)
{
    int rc = locate_front(ctx, who, plane, keys, k, 1, false, WM_LOCATE_BITS_NVALS + (long long)std::max(nbits, 0), "(4 + bits)", slot, &b->c);
    if (rc != WM_OK) return rc;
    b->ts.th = tile_rows; b->ts.tw = tile_cols;
    if (wm_tiles_shape(keys->rows, keys->cols, tile_rows, tile_cols, &b->ts.ny, &b->ts.nx) != WM_OK)
        return fail(ctx, WM_ERR_BAD_ARG, who + ": tile shape " + std::to_string(tile_rows) + "x" + std::to_string(tile_cols) +
                                             " (rows: a multiple of 8, >= 32; columns: a multiple of 4, >= 32)");
    const int T = b->ts.ny * b->ts.nx;
    if ((rc = tile_bits_checked(ctx, who.c_str(), tile_bit, T, nbits)) != WM_OK) return rc;
    b->has.assign((size_t)nbits + 1, 0);
    for (int t = 0; t < T; ++t)
        if (tile_bit[t] >= 0) b->has[(size_t)tile_bit[t]] = 1;
    return WM_OK;
}
// wm_locate_bits' scratch: the frames' spectra and three planes, the bits' block records [frames][pairs][blocks], the energy's
// [frames][blocks], and the energy map and the per-bit maps where the caller passes none
LocShape locate_bits_shape(const LocCall& c, int nbits, bool own_energy, bool own_maps)
{
    const size_t n = (size_t)c.ny * c.nx, F = (size_t)c.frames;
    return LocShape{c.pr, c.pc, c.ny, c.nx, c.frames, locate_bits_part_bytes(c.ny, c.nx) * (size_t)((nbits + 1) / 2) * F, locate_part_bytes(c.ny, c.nx) * F,
                    own_energy ? n * F * sizeof(float) : 0, own_maps ? n * F * nbits * sizeof(float) : 0, 0};
}

// wm_locate_bits' tail behind the frames' spectra in L.hs.  Pair-major: the pair's key plane and its spectrum once per call, then
// per frame the product, the way back and the accumulate pass; behind the last pair the folds and the records: [frames][4] of the
// energy map, then [frames][nbits] soft values.  status: the frames' DEVICE status words
int locate_bits_tail(wm_ctx* ctx, Slot& s, int slot, const LocBitsCall& b, const LocScratch& L, const wm_keys* keys, int k, const int* table_dev, int nbits,
                     const int* status, float* energy_dev, float* maps_dev, float* loc_out, float* soft_out, int* status_out)
{
    int rc;
    const int pr = L.pr, pc = L.pc, ny = b.c.ny, nx = b.c.nx, frames = b.c.frames;
    const size_t n = (size_t)ny * nx, npl = (size_t)pr * pc;
    float* energy = energy_dev ? energy_dev : L.energy;
    float* maps = maps_dev ? maps_dev : L.maps;
    OpResult* res = s.d_res + s.res_used;
    const float* key = keys->d + (size_t)k * keys->rows * keys->cols;
    const int npairs = (nbits + 1) / 2;
    const size_t blk_bytes = locate_bits_part_bytes(ny, nx), part_stride = blk_bytes * npairs, epart_stride = locate_part_bytes(ny, nx);
    for (int pi = 0; pi < npairs; ++pi) {
        const int b0 = 2 * pi, b1 = b0 + 1 < nbits ? b0 + 1 : -2;
        launch_locate_lay_bits(s.stream, key, keys->rows, keys->cols, table_dev, b.ts, b0, b1, L.a, pr, pc);
        fft2_forward_t(s.stream, L, L.a, L.kw);
        for (int f = 0; f < frames; ++f) {
            launch_locate_mul3(s.stream, L.hs + f * L.plane_floats, L.kw, L.p, npl);
            fft2_inverse_t(s.stream, L, L.p, L.a);
            float* mf = maps + (size_t)f * nbits * n;
            launch_locate_bits_acc(s.stream, L.a, pr, pc, ny, nx, status + f, pi == 0, b.has[(size_t)b0] != 0, b1 >= 0 && b.has[(size_t)b1] != 0,
                                   mf + (size_t)b0 * n, b1 >= 0 ? mf + (size_t)b1 * n : nullptr, energy + (size_t)f * n,
                                   L.part + (size_t)f * part_stride + (size_t)pi * blk_bytes, pi == npairs - 1 ? L.epart + (size_t)f * epart_stride : nullptr);
        }
    }
    for (int f = 0; f < frames; ++f)
        launch_locate_bits_fold(s.stream, L.epart + (size_t)f * epart_stride, L.part + (size_t)f * part_stride, ny, nx, nbits, energy + (size_t)f * n,
                                maps + (size_t)f * nbits * n, status + f, res + WM_LOCATE_BITS_NVALS * f,
                                res + WM_LOCATE_BITS_NVALS * frames + (size_t)f * nbits);
    if ((rc = launch_check(ctx, s)) != WM_OK) return rc;
    push_pending(s, frames, WM_LOCATE_BITS_NVALS, false, loc_out, status_out, nullptr);
    return finish_call(ctx, s, slot, frames, nbits, false, soft_out, nullptr);
}
}  // namespace

// wm_locate with the key masked to the tiles of one payload bit at a time, two bits per complex transform: the frames' spectra are
// kept, every pair's key plane is transformed once per call, and per (pair, frame) there are a product, an inverse transform and the
// accumulate pass; behind the last pair the folds.  None of its kernels runs inside a ProfScope
int wm_locate_bits(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k, int tile_rows, int tile_cols, const int32_t* tile_bit,
                   int nbits, float* loc_out, float* soft_out, float* energy_dev, float* maps_dev, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!img || !keys || !tile_bit || !loc_out || !soft_out)
        return fail(ctx, WM_ERR_BAD_ARG, "wm_locate_bits: null img, keys, tile_bit, loc_out or soft_out");
    LocBitsCall b;
    if ((rc = locate_bits_checks(ctx, "wm_locate_bits", img, keys, k, tile_rows, tile_cols, tile_bit, nbits, slot, &b)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, WM_LOCATE_BITS_NVALS + nbits, "(4 + bits)", &sw)) != WM_OK) return rc;
    LocScratch L;
    if ((rc = loc_scratch(ctx, s, LOC_BITS, locate_bits_shape(b.c, nbits, !energy_dev, !maps_dev), &L)) != WM_OK) return rc;
    const int* table_dev = nullptr;
    if ((rc = call_ints(ctx, s, tile_bit, b.ts.ny * b.ts.nx, &table_dev, nullptr)) != WM_OK) return rc;
    if ((rc = locate_image_side(ctx, s, sw, img, L, [](int) {})) != WM_OK) return rc;
    return locate_bits_tail(ctx, s, slot, b, L, keys, k, table_dev, nbits, s.d_status, energy_dev, maps_dev, loc_out, soft_out, status_out);
}

// wm_locate_bits' tail on a caller's pooled image-side plane (wm_clip_pool) in the place of one frame's h
int wm_locate_bits_pooled(wm_ctx* ctx, const float* pool_dev, const wm_keys* keys, int k, int tile_rows, int tile_cols, const int32_t* tile_bit,
                          int nbits, float* loc_out, float* soft_out, float* energy_dev, float* maps_dev, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc;
    if (!pool_dev || !keys || !tile_bit || !loc_out || !soft_out)
        return fail(ctx, WM_ERR_BAD_ARG, "wm_locate_bits_pooled: null pool_dev, keys, tile_bit, loc_out or soft_out");
    LocBitsCall b;
    if ((rc = locate_bits_checks(ctx, "wm_locate_bits_pooled", nullptr, keys, k, tile_rows, tile_cols, tile_bit, nbits, slot, &b)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    LocScratch L;
    const int *table_dev = nullptr, *status = nullptr;
    if ((rc = locate_pooled_side(ctx, s, LOC_BITS, locate_bits_shape(b.c, nbits, !energy_dev, !maps_dev), pool_dev, tile_bit, b.ts.ny * b.ts.nx, &L, &table_dev,
                                 &status)) != WM_OK)
        return rc;
    return locate_bits_tail(ctx, s, slot, b, L, keys, k, table_dev, nbits, status, energy_dev, maps_dev, loc_out, soft_out, nullptr);
}


// the three passes wm_locate_bits adds to wm_fft_bench's seven, timed the same way: the key-pair plane (128 x 128 tiles over a key
// of the transform's size), the three-operand product, and the accumulate pass of a later pair over ny x nx offsets
int wm_locate_bits_bench(int device, int pr, int pc, int ny, int nx, int iters, double* us_out)
{
    if (!us_out || iters < 1 || fft_log2(pr) < 0 || fft_log2(pc) < 0 || pr < 128 || pc < 128 || ny < 1 || ny > pr || nx < 1 || nx > pc) return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    const size_t plane = (size_t)pr * pc * 2 * sizeof(float), n = round256((size_t)ny * nx * sizeof(float));
    const TileShape ts{128, 128, pr / 128, pc / 128};
    const size_t tab = round256((size_t)ts.ny * ts.nx * sizeof(int)), part = round256(locate_bits_part_bytes(ny, nx));
    char* scr = nullptr;
    const size_t total = 3 * plane + 3 * n + 2 * part + tab + 256;
    if (hipMalloc((void**)&scr, total) != hipSuccess) { (void)hipGetLastError(); return WM_ERR_ALLOC; }
    float *a = (float*)scr, *b = (float*)(scr + plane), *c = (float*)(scr + 2 * plane);
    float *m0 = (float*)(scr + 3 * plane), *m1 = (float*)(scr + 3 * plane + n), *en = (float*)(scr + 3 * plane + 2 * n);
    char* p0 = scr + 3 * plane + 3 * n;
    int* table = (int*)(p0 + 2 * part);
    int* status = (int*)(p0 + 2 * part + tab);
    const bool ok = hipMemset(scr, 0, total) == hipSuccess && bench_passes(WM_LOCATE_BITS_BENCH_PASSES, iters, us_out, [&](int pass) {
        switch (pass) {
        case 0: launch_locate_lay_bits(nullptr, a, pr, pc, table, ts, 0, 1, b, pr, pc); break;
        case 1: launch_locate_mul3(nullptr, a, b, c, (size_t)pr * pc); break;
        default: launch_locate_bits_acc(nullptr, c, pr, pc, ny, nx, status, false, true, true, m0, m1, en, p0, p0 + part); break;
        }
    });
    (void)hipFree(scr);
    return ok ? WM_OK : WM_ERR_RUNTIME;
}

// ---- wm_locate_keys: whose key is in a crop, and where ----------------------------------------------------
namespace {
constexpr int LOCK_MAX_KEYS = RES_CAP / WM_LOCATE_KEYS_NVALS;  // (more keys than this never pass the record-room check)
// wm_locate_keys' scratch: the frames' spectra and three planes, the block records of the two halves of one (pair, frame), and the
// per-key non-zero flags (+ 1: the flag of the odd last key's missing partner)
LocShape locate_keys_shape(const LocCall& c)
{
    return LocShape{c.pr, c.pc, c.ny, c.nx, c.frames, 2 * locate_part_bytes(c.ny, c.nx), 0, 0, 0, (size_t)(LOCK_MAX_KEYS + 1) * sizeof(int)};
}

// wm_locate_keys' tail behind the frames' spectra in L.hs.  Pair-major: the pair's plane and its spectrum once per call, then per
// frame the product, the way back, the maps and the records.  status: the frames' DEVICE status words
int locate_keys_tail(wm_ctx* ctx, Slot& s, int slot, const LocCall& c, const LocScratch& L, const wm_keys* keys, int k0, int nk, const int* status,
                     float* loc_out, float* maps_dev, int* status_out)
{
    const int pr = L.pr, pc = L.pc, frames = c.frames;
    const size_t n = (size_t)c.ny * c.nx, npl = (size_t)pr * pc, key_elems = (size_t)keys->rows * keys->cols;
    OpResult* res = s.d_res + s.res_used;
    HIPCHK(ctx, hipMemsetAsync(L.nz, 0, (size_t)(nk + 1) * sizeof(int), s.stream));
    for (int j = 0; j < nk; j += 2) {
        const bool pair = j + 1 < nk;
        const float* ka = keys->d + (size_t)(k0 + j) * key_elems;
        launch_locate_lay_keys(s.stream, ka, pair ? ka + key_elems : nullptr, keys->rows, keys->cols, L.a, pr, pc, L.nz + j);
        fft2_forward_t(s.stream, L, L.a, L.kw);
        for (int f = 0; f < frames; ++f) {
            launch_locate_mul3(s.stream, L.hs + f * L.plane_floats, L.kw, L.p, npl);
            fft2_inverse_t(s.stream, L, L.p, L.a);
            float* mf = maps_dev ? maps_dev + ((size_t)f * nk + j) * n : nullptr;
            launch_locate_map(s.stream, L.a, pr, pc, c.ny, c.nx, status + f, L.nz + j, pair, mf, mf && pair ? mf + n : nullptr, L.part,
                              res + ((size_t)f * nk + j) * WM_LOCATE_KEYS_NVALS);
        }
    }
    return finish_call(ctx, s, slot, frames, WM_LOCATE_KEYS_NVALS * nk, false, loc_out, status_out);
}
}  // namespace

// wm_locate of every frame against keys k0 .. k0 + nk - 1, two keys per complex transform: the frames' spectra are kept, every
// pair's plane is transformed once per call, and per (pair, frame) there are a product, an inverse transform, the map pass and the
// fold of its records.  None of its kernels runs inside a ProfScope
int wm_locate_keys(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k0, int nk, float* loc_out, float* maps_dev, int* status_out,
                   int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!img || !keys || (!loc_out && !maps_dev)) return fail(ctx, WM_ERR_BAD_ARG, "wm_locate_keys: null img or keys, or loc_out and maps_dev both null");
    LocCall c;
    if ((rc = locate_front(ctx, "wm_locate_keys", img, keys, k0, nk, true, (long long)WM_LOCATE_KEYS_NVALS * nk, "(4 x keys)", slot, &c)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, WM_LOCATE_KEYS_NVALS * nk, "(4 x keys)", &sw)) != WM_OK) return rc;
    LocScratch L;
    if ((rc = loc_scratch(ctx, s, LOC_KEYS, locate_keys_shape(c), &L)) != WM_OK) return rc;
    if ((rc = locate_image_side(ctx, s, sw, img, L, [](int) {})) != WM_OK) return rc;
    return locate_keys_tail(ctx, s, slot, c, L, keys, k0, nk, s.d_status, loc_out, maps_dev, status_out);
}

// wm_locate_keys' tail on a caller's pooled image-side plane (wm_clip_pool) in the place of one frame's h
int wm_locate_keys_pooled(wm_ctx* ctx, const float* pool_dev, const wm_keys* keys, int k0, int nk, float* loc_out, float* maps_dev, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc;
    if (!pool_dev || !keys || (!loc_out && !maps_dev))
        return fail(ctx, WM_ERR_BAD_ARG, "wm_locate_keys_pooled: null pool_dev or keys, or loc_out and maps_dev both null");
    LocCall c;
    if ((rc = locate_front(ctx, "wm_locate_keys_pooled", nullptr, keys, k0, nk, true, (long long)WM_LOCATE_KEYS_NVALS * nk, "(4 x keys)", slot, &c)) != WM_OK)
        return rc;
    Slot& s = slot_of(ctx, slot);
    LocScratch L;
    const int *none = nullptr, *status = nullptr;
    if ((rc = locate_pooled_side(ctx, s, LOC_KEYS, locate_keys_shape(c), pool_dev, nullptr, 0, &L, &none, &status)) != WM_OK) return rc;
    return locate_keys_tail(ctx, s, slot, c, L, keys, k0, nk, status, loc_out, maps_dev, nullptr);
}


int wm_locate_keys_rank(const float* loc, int nk, int* best, float* z_best, float* z_next)
{
    if (!loc || !best || !z_best || !z_next || nk < 1) return WM_ERR_BAD_ARG;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    int b = -1;
    for (int j = 0; j < nk; ++j) {
        const float z = loc[(size_t)j * WM_LOCATE_KEYS_NVALS + 3];
        if (z == z && (b < 0 || z > loc[(size_t)b * WM_LOCATE_KEYS_NVALS + 3])) b = j;  // (NaN is ignored; ties: the smallest index)
    }
    float next = nan;
    for (int j = 0; j < nk; ++j) {
        const float z = loc[(size_t)j * WM_LOCATE_KEYS_NVALS + 3];
        if (j != b && z == z && !(next >= z)) next = z;
    }
    *best = b;
    *z_best = b < 0 ? nan : loc[(size_t)b * WM_LOCATE_KEYS_NVALS + 3];
    *z_next = next;
    return WM_OK;
}

// the two passes wm_locate_keys adds to wm_fft_bench's seven and wm_locate_bits_bench's product, timed the same way: the key-pair
// plane (two keys of the transform's size) and the map pass of a pair over ny x nx offsets, both maps stored
int wm_locate_keys_bench(int device, int pr, int pc, int ny, int nx, int iters, double* us_out)
{
    if (!us_out || iters < 1 || fft_log2(pr) < 0 || fft_log2(pc) < 0 || pr < 128 || pc < 128 || ny < 1 || ny > pr || nx < 1 || nx > pc) return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    const size_t plane = (size_t)pr * pc * 2 * sizeof(float), n = round256((size_t)ny * nx * sizeof(float));
    const size_t part = round256(2 * locate_part_bytes(ny, nx));
    char* scr = nullptr;
    const size_t total = 2 * plane + 2 * n + part + 256;
    if (hipMalloc((void**)&scr, total) != hipSuccess) { (void)hipGetLastError(); return WM_ERR_ALLOC; }
    // (plane a doubles as the two keys, pr x pc f32 each; its zeros leave the flags clear, which costs the map pass nothing less)
    float *a = (float*)scr, *b = (float*)(scr + plane);
    float *m0 = (float*)(scr + 2 * plane), *m1 = (float*)(scr + 2 * plane + n);
    char* p0 = scr + 2 * plane + 2 * n;
    int* nz = (int*)(p0 + part);
    int* status = nz + 2;
    const bool ok = hipMemset(scr, 0, total) == hipSuccess && bench_passes(WM_LOCATE_KEYS_BENCH_PASSES, iters, us_out, [&](int pass) {
        if (pass == 0) launch_locate_lay_keys(nullptr, a, a + (size_t)pr * pc, pr, pc, b, pr, pc, nz);
        else launch_locate_map(nullptr, b, pr, pc, ny, nx, status, nz, true, m0, m1, p0, nullptr);
    });
    (void)hipFree(scr);
    return ok ? WM_OK : WM_ERR_RUNTIME;
}

// makeWatermark of every frame with every key of the bank: wm_embed's input and base handling, one record per (frame, key)
int wm_embed_keys(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_keys* keys, const wm_plane* out,
                  float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if (!keys || !out) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_keys: null keys or out");
    if ((rc = check_bank(ctx, keys, "wm_embed_keys", true)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_embed_keys")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_plane(ctx, in_gray, 0, false, "in_gray", true)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    const int nkeys = keys->nkeys;
    if ((rc = check_plane(ctx, base, frames, true, "base")) != WM_OK) return rc;
    if (out->mem != WM_MEM_DEVICE) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_keys: out must be a WM_MEM_DEVICE plane");
    if ((rc = check_out_copies(ctx, "wm_embed_keys", "nkeys", out, frames, nkeys)) != WM_OK) return rc;
    if ((rc = check_embed_dtypes(ctx, in_gray, base, out)) != WM_OK) return rc;
    if ((rc = check_res_room(ctx, s, (long long)frames * nkeys, "keys")) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));

    EmbedCall c;
    if ((rc = copies_stage(ctx, s, "wm_embed_keys", in_gray, base, out, nkeys, &c)) != WM_OK) return rc;
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    const int rstride = std::max(ctx->max_nblk, ctx->max_nrec);
    if ((rc = ensure(ctx, &s.ekeys_part, &s.ekeys_part_bytes, embed_keys_scratch_bytes(frames, nkeys, rstride))) != WM_OK) return rc;
    const Sweep sw = mask_route(ctx, s, lg, frames, mask, c.xd);
    const KeyBank bank = bank_of(ctx, keys);
    OpResult* res = s.d_res + s.res_used;
    // the image side is wm_embed's: the Gram sweep and solve (ME)
    if (mask == WM_MASK_ME) sweep_gram(ctx, s, K_GRAM, sw);
    {
        ProfScope ps(ctx, K_STATS_KEYS, s.stream);
        if (launch_stats_keys(sw, bank, s.ekeys_part, rstride) != 0) return fail(ctx, WM_ERR_RUNTIME, "wm_embed_keys: geometry exceeds the record arrays");
    }
    { ProfScope ps(ctx, K_EMBED_KEYS_FOLD, s.stream); launch_embed_keys_fold(sw, nkeys, s.ekeys_part, rstride, ctx->sF, sqrt_n(ctx), res); }
    { ProfScope ps(ctx, K_EMBED_KEYS, s.stream); launch_embed_keys(sw, bank, EmbedPlanes{c.bd, c.od, nullptr}, s.ekeys_part, rstride); }
    return finish_call(ctx, s, slot, frames, nkeys, true, a_out, status_out);  // (wm_embed's rule: an unsolvable frame leaves its K strengths untouched)
}

// ---- a key per frame of a batch: wm_key_schedule, wm_embed_select, wm_detect_select ------------------------------------------------
// key_of_frame[i] = z(first_frame + i) mod nkeys, z(n) the (n + 1)-th value of wm_bits_layout's splitmix64 started at `seed`, formed
// directly from n (pure host arithmetic)
int wm_key_schedule(int nkeys, uint64_t seed, uint64_t first_frame, int frames, int32_t* key_of_frame)
{
    if (!key_of_frame || nkeys < 1 || nkeys > WM_KEYS_MAX || frames < 1) return WM_ERR_BAD_ARG;
    for (int i = 0; i < frames; ++i) {
        uint64_t z = seed + (first_frame + (uint64_t)i + 1) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        key_of_frame[i] = (int32_t)(z % (uint64_t)nkeys);
    }
    return WM_OK;
}

// every entry of a call's key table names a key of the bank
static int key_table_checked(wm_ctx* ctx, const char* who, const wm_keys* keys, const int32_t* key_of_frame, int frames)
{
    for (int f = 0; f < frames; ++f)
        if (key_of_frame[f] < 0 || key_of_frame[f] >= keys->nkeys)
            return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": key_of_frame[" + std::to_string(f) + "] = " + std::to_string(key_of_frame[f]) + " for frame " +
                                                 std::to_string(f) + " (the bank has keys 0 .. " + std::to_string(keys->nkeys - 1) + ")");
    return WM_OK;
}
// the call's own copy of the table, kept like wm_embed_signs': the caller's array is free when the call returns
static int key_table_upload(wm_ctx* ctx, Slot& s, const int32_t* key_of_frame, int frames, const int** kidx)
{
    void *th = nullptr, *td = nullptr;
    const size_t bytes = (size_t)frames * sizeof(int32_t);
    int rc;
    if ((rc = table_room(ctx, s, bytes, &th, &td)) != WM_OK) return rc;
    std::memcpy(th, key_of_frame, bytes);
    if ((rc = table_upload(ctx, s, th, td, bytes)) != WM_OK) return rc;
    *kidx = (const int*)td;
    return WM_OK;
}

// makeWatermark of frame f with key key_of_frame[f] of the bank as W: wm_embed's input, base and output handling and its Gram sweep and
// solve on the sweeps; then the stats and embed sweeps with W resolved per frame (k_me_stats_sel / k_nvf_stats_sel, k_embed_sel), each
// launched once for the batch.  Never the fused kernels, no Gram hand-over.  The *_sel kernels are launched outside any ProfScope: the
// list of profiling names is not extended for them
int wm_embed_select(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, const wm_keys* keys,
                    const int32_t* key_of_frame, float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!in_gray || !base || !out || !keys || !key_of_frame) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_select: null in_gray, base, out, keys or key_of_frame");
    int rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_embed_select")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_embed_planes(ctx, in_gray, base, out)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    if ((rc = check_bank(ctx, keys, "wm_embed_select", true)) != WM_OK) return rc;
    if ((rc = key_table_checked(ctx, "wm_embed_select", keys, key_of_frame, frames)) != WM_OK) return rc;
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));

    const int* kidx = nullptr;
    if ((rc = key_table_upload(ctx, s, key_of_frame, frames, &kidx)) != WM_OK) return rc;
    EmbedCall c;  // (no hand-over of its own)
    if ((rc = embed_stage(ctx, s, in_gray, base, out, &c)) != WM_OK) return rc;
    if ((rc = embed_snapshot(ctx, s, in_gray, &c)) != WM_OK) return rc;
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    const Sweep sw = mask_route(ctx, s, lg, frames, mask, c.xd);
    const KeyBank bank = bank_of(ctx, keys);
    OpResult* res = s.d_res + s.res_used;
    // the image side is wm_embed's: the Gram sweep and solve (ME); the scratch arrays are sweep_stats'
    if (mask == WM_MASK_ME) sweep_gram(ctx, s, K_GRAM, sw);
    unsigned* ticket = s.d_ticket + ctx->max_frames * TKS;
    if (mask == WM_MASK_ME)
        launch_me_stats_sel(sw, bank, kidx, s.d_pmax, s.d_pss, ticket, strip_tickets(ctx, s, 0), s.d_smax, s.d_sss, ctx->sF, sqrt_n(ctx), s.d_scal, res, s.d_raw);
    else
        launch_nvf_stats_sel(sw, bank, kidx, s.d_pss, ticket, strip_tickets(ctx, s, 0), s.d_sss, ctx->sF, sqrt_n(ctx), s.d_scal, res, s.d_raw);
    launch_embed_sel(sw, bank, EmbedPlanes{c.bd, c.od, s.d_scal}, kidx);
    return embed_close(ctx, s, out, c, a_out, status_out, slot);
}

// detectWatermark of frame f against key key_of_frame[f]: detect_bank's image side (wm_detect's input handling on the sweeps, the Gram
// sweep -- a promised hand-over of a WM_MEM_SLOT_OUT plane included, never the checked one -- and the solve), then k_detect_sel on
// sweep_detect's scratch arrays, one record per frame
int wm_detect_select(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, const int32_t* key_of_frame, float* corr_out,
                     int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!img || !keys || !key_of_frame || !corr_out) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect_select: null img, keys, key_of_frame or corr_out");
    int rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_detect_select")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_plane(ctx, img, 0, false, "image", true)) != WM_OK) return rc;
    const int frames = img->frames;
    if ((rc = check_bank(ctx, keys, "wm_detect_select", true)) != WM_OK) return rc;
    if ((rc = key_table_checked(ctx, "wm_detect_select", keys, key_of_frame, frames)) != WM_OK) return rc;
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, 1, nullptr, &sw)) != WM_OK) return rc;  // (record room, device, the plane resolved)
    const int* kidx = nullptr;
    if ((rc = key_table_upload(ctx, s, key_of_frame, frames, &kidx)) != WM_OK) return rc;
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    launch_detect_sel(sw, bank_of(ctx, keys), kidx, s.d_pcorr, s.d_ticket + 2 * ctx->max_frames * TKS, strip_tickets(ctx, s, 1), s.d_scorr,
                      s.d_res + s.res_used, s.d_raw + ctx->max_frames);
    return finish_call(ctx, s, slot, frames, 1, false, corr_out, status_out);
}

int wm_embed_signs_group(void) { return embed_signs_group(); }

// wm_embed_signs of every frame once per table of signs [frames][ncopies][ny][nx]: wm_embed_signs' table handling, Gram, solve and
// single-W stats sweeps (one strength per frame), wm_embed_keys' planes (K device outputs per frame, no overlap, no last_out, no
// hand-over), k_embed_signs_multi in k_embed_signs' place -- launched outside any ProfScope, like it
int wm_embed_signs_multi(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows, int tile_cols,
                         int ncopies, const int8_t* signs, float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!in_gray || !base || !out || !signs) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs_multi: null in_gray, base, out or signs");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_embed_signs_multi", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_embed_signs_multi")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_plane(ctx, in_gray, 0, false, "in_gray", true)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    if ((rc = check_plane(ctx, base, frames, true, "base")) != WM_OK) return rc;
    if (out->mem != WM_MEM_DEVICE) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs_multi: out must be a WM_MEM_DEVICE plane");
    if (ncopies < 1 || ncopies > 4096) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs_multi: ncopies must be 1 .. 4096");
    if ((rc = check_out_copies(ctx, "wm_embed_signs_multi", "ncopies", out, frames, ncopies)) != WM_OK) return rc;
    if ((rc = check_embed_dtypes(ctx, in_gray, base, out)) != WM_OK) return rc;
    const LaunchGeom lg0 = make_geom(ctx, frames, mask);
    if (!embed_signs_multi_grid_fits(lg0, frames, ncopies))
        return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs_multi: the sweep's grid times the copy groups exceeds a launch grid of 31 bits");
    const size_t nsigns = (size_t)frames * ncopies * ts.ny * ts.nx;
    for (size_t i = 0; i < nsigns; ++i)
        if (signs[i] < -1 || signs[i] > 1)
            return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_signs_multi: sign " + std::to_string((int)signs[i]) + " at index " + std::to_string(i) + " (must be -1, 0 or +1)");
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));

    // the call's own copy of the tables, as wm_embed_signs keeps its one
    void *th = nullptr, *td = nullptr;
    if ((rc = table_room(ctx, s, nsigns, &th, &td)) != WM_OK) return rc;
    std::memcpy(th, signs, nsigns);
    if ((rc = table_upload(ctx, s, th, td, nsigns)) != WM_OK) return rc;

    EmbedCall c;
    if ((rc = copies_stage(ctx, s, "wm_embed_signs_multi", in_gray, base, out, ncopies, &c)) != WM_OK) return rc;
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    const Sweep sw = mask_route(ctx, s, lg, frames, mask, c.xd);
    if (mask == WM_MASK_ME) sweep_gram(ctx, s, K_GRAM, sw);
    sweep_stats(ctx, s, true, sw, s.d_res + s.res_used);
    launch_embed_signs_multi(sw, own_w(ctx), EmbedPlanes{c.bd, c.od, s.d_scal}, (const signed char*)td, ncopies, ts);
    return finish_call(ctx, s, slot, frames, 1, true, a_out, status_out);
}

// a host layer over wm_embed_signs_multi: the table of copy (f, k) is wm_embed_bits' table for payloads[f][k]
int wm_embed_bits_multi(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows, int tile_cols,
                        const int32_t* tile_bit, int nbits, int ncopies, const uint8_t* payloads, float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!in_gray || !tile_bit || !payloads) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_bits_multi: null in_gray, tile_bit or payloads");
    TileShape ts;
    int rc;
    if ((rc = tiles_checked(ctx, "wm_embed_bits_multi", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    const long long T = (long long)ts.ny * ts.nx;
    if ((rc = tile_bits_checked(ctx, "wm_embed_bits_multi", tile_bit, T, nbits)) != WM_OK) return rc;
    if (in_gray->frames < 1 || in_gray->frames > ctx->max_frames)
        return fail(ctx, WM_ERR_BAD_ARG, "in_gray: frames=" + std::to_string(in_gray->frames) + " exceeds wm_configure max_frames=" + std::to_string(ctx->max_frames));
    if (ncopies < 1 || ncopies > 4096) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed_bits_multi: ncopies must be 1 .. 4096");
    const long long copies = (long long)in_gray->frames * ncopies;
    const int pbytes = (nbits + 7) / 8;
    std::vector<int8_t> signs((size_t)(copies * T));
    for (long long fk = 0; fk < copies; ++fk)
        for (long long t = 0; t < T; ++t) {
            const int b = tile_bit[t];
            signs[(size_t)(fk * T + t)] = b < 0 ? 0 : (((payloads[(size_t)fk * pbytes + b / 8] >> (b % 8)) & 1) ? 1 : -1);
        }
    return wm_embed_signs_multi(ctx, mask, in_gray, base, out, tile_rows, tile_cols, ncopies, signs.data(), a_out, status_out, slot);
}

int wm_compute_mask(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* mask_out, const wm_plane* e_out,
                    float* coef_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = check_mask(ctx, mask);
    if (rc != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_plane(ctx, in_gray, 0, false, "in_gray", true)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    if ((rc = check_plane(ctx, mask_out, frames, false, "mask_out")) != WM_OK) return rc;
    if (mask_out->dtype != WM_F32 || mask_out->mem != WM_MEM_DEVICE) return fail(ctx, WM_ERR_BAD_ARG, "mask_out must be a device f32 plane");
    if (e_out) {
        if ((rc = check_plane(ctx, e_out, frames, false, "e_out")) != WM_OK) return rc;
        if (e_out->dtype != WM_F32 || e_out->mem != WM_MEM_DEVICE) return fail(ctx, WM_ERR_BAD_ARG, "e_out must be a device f32 plane");
    }
    if ((rc = check_res_room(ctx, s, frames)) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PlaneDesc xd;
    if ((rc = prep_input(ctx, s, in_gray, &xd)) != WM_OK) return rc;
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    PlaneDesc mo = desc_device(mask_out), eo;
    if (e_out) eo = desc_device(e_out); else { eo = mo; eo.p = nullptr; }
    invalidate_handovers(ctx, mo, frames);
    invalidate_handovers(ctx, eo, frames);
    OpResult* res = s.d_res + s.res_used;
    float* coefres = s.d_coefres + (size_t)s.res_used * 8;
    const Sweep sw = mask_route(ctx, s, lg, frames, mask, xd);
    // (ME: the prediction error scaled by the stats sweep's maximum, behind the Gram and stats sweeps; NVF needs neither, nor scalars)
    if (mask == WM_MASK_ME) {
        sweep_gram(ctx, s, K_GRAM, sw);
        sweep_stats(ctx, s, true, sw, res);
    }
    { ProfScope ps(ctx, K_MASK, s.stream); launch_mask(sw, mask == WM_MASK_ME ? s.d_scal : nullptr, mo, eo); }
    launch_mask_result(s.stream, frames, sw.status, sw.coef, res, coefres);
    return finish_call(ctx, s, slot, frames, 1, false, nullptr, status_out, coef_out);
}

// ---- the conversion calls (wm.h): the pixel-format front wm_rgb2gray, wm_unpack_rgb8, wm_pack_rgb8 (kernels in wm_k_convert.hip) and
// the samples of 9 to 16 bits, wm_unpack16 and wm_pack16 (wm_k_convert16.hip), with their host layers wm_embed16 and wm_detect16.
// One frame, convert_call below, runs all five conversions: an entry point tests its pointers, lists its operands with their rules
// and hands over its scalar check and its launch.  First this family's rules for one operand and one scalar argument
static bool plane_null(const wm_plane* pl) { return !pl || (!pl->data && pl->mem != WM_MEM_SLOT_OUT); }
static int check_shape(wm_ctx* ctx, int rows, int cols, const char* what)
{
    if (rows == ctx->rows && cols == ctx->cols) return WM_OK;
    return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": plane is " + std::to_string(rows) + "x" + std::to_string(cols) + ", engine was initialised for " +
                                         std::to_string(ctx->rows) + "x" + std::to_string(ctx->cols));
}
static int check_packed(wm_ctx* ctx, const wm_packed* pk, const char* what)
{
    if (pk->mem != WM_MEM_DEVICE && pk->mem != WM_MEM_HOST) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": bad mem (device or host)");
    if (pk->pitch_bytes < 3 * (int64_t)pk->cols) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": pitch_bytes < 3 * cols");
    if (pk->frames < 1 || pk->frames > ctx->max_frames)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": frames=" + std::to_string(pk->frames) + " exceeds wm_configure max_frames=" + std::to_string(ctx->max_frames));
    if (pk->frames > 1 && pk->frame_stride_bytes < (int64_t)pk->rows * pk->pitch_bytes)
        return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": frame_stride_bytes too small (frames overlap)");
    return WM_OK;
}
static int check_rgb_plane(wm_ctx* ctx, const wm_plane* pl, const char* what, bool allow_slot_out)
{
    const int rc = check_plane(ctx, pl, 0, true, what, allow_slot_out);
    if (rc != WM_OK) return rc;
    return pl->channels == 3 ? WM_OK : fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": channels must be 3 (planar RGB)");
}
static int check_gray_f32(wm_ctx* ctx, const wm_plane* pl, const char* what)
{
    const int rc = check_plane(ctx, pl, 0, false, what);
    if (rc != WM_OK) return rc;
    return pl->dtype == WM_F32 ? WM_OK : fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": must be a 1-channel f32 plane");
}
static int check_weights(wm_ctx* ctx, const float* weights, float* w)
{
    w[0] = 0.299f; w[1] = 0.587f; w[2] = 0.114f;  // af::rgb2gray's defaults (main.cpp:153-154)
    if (!weights) return WM_OK;
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(weights[i])) return fail(ctx, WM_ERR_BAD_ARG, "weights: not finite");
        w[i] = weights[i];
    }
    return WM_OK;
}
// what the slot's last output must be for a WM_MEM_SLOT_OUT input: a 3-channel embed output of the operand's frames and dtype ...
static int slot_out_rgb(wm_ctx* ctx, const Slot& s, const wm_plane* rgb)
{
    if (s.last_out_frames == 0 || s.last_out.channels != 3 || rgb->frames != s.last_out_frames || rgb->dtype != s.last_out_dtype)
        return fail(ctx, WM_ERR_BAD_ARG, "WM_MEM_SLOT_OUT: no matching 3-channel embed output on this slot (frames / dtype must equal the last wm_embed's)");
    return WM_OK;
}
// ... or an f32 embed output of the operand's channels and frames
static int slot_out_f32(wm_ctx* ctx, const Slot& s, const wm_plane* src)
{
    if (s.last_out_frames == 0 || s.last_out.channels != src->channels || src->frames != s.last_out_frames || s.last_out_dtype != WM_F32)
        return fail(ctx, WM_ERR_BAD_ARG, "WM_MEM_SLOT_OUT: no matching f32 embed output on this slot (channels / frames must equal the last wm_embed's)");
    return WM_OK;
}
int wm_depth_scale(int bits, float* to255, float* from255)
{
    if (bits < 9 || bits > 16 || !to255 || !from255) return WM_ERR_BAD_ARG;
    const double maxv = (double)((1u << bits) - 1u);
    *to255 = (float)(255.0 / maxv);
    *from255 = (float)(maxv / 255.0);
    return WM_OK;
}
// what a u16 plane must satisfy on its own: check_plane's rules for 2-byte elements (check_plane itself keeps refusing the dtype
// for every other entry point) and a 2-byte aligned base
static int check_plane16(wm_ctx* ctx, const wm_plane* pl, const char* what)
{
    if (pl->dtype != WM_U16) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": must be a WM_U16 plane");
    wm_plane t = *pl;
    t.dtype = WM_U8;  // (the rules below do not depend on the element size)
    const int rc = check_plane(ctx, &t, 0, true, what);
    if (rc != WM_OK) return rc;
    return reinterpret_cast<uintptr_t>(pl->data) % 2 == 0 ? WM_OK : fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": data must be 2-byte aligned");
}
static int check_plane_f32(wm_ctx* ctx, const wm_plane* pl, const char* what, bool allow_slot_out)
{
    if (pl->dtype != WM_F32) return fail(ctx, WM_ERR_BAD_ARG, std::string(what) + ": must be a WM_F32 plane");
    return check_plane(ctx, pl, 0, true, what, allow_slot_out);
}
static int check_depth(wm_ctx* ctx, int bits, int msb_aligned)
{
    if (bits < 9 || bits > 16) return fail(ctx, WM_ERR_BAD_ARG, "bits=" + std::to_string(bits) + ": must be 9..16");
    return msb_aligned == 0 || msb_aligned == 1 ? WM_OK : fail(ctx, WM_ERR_BAD_ARG, "msb_aligned must be 0 or 1");
}

// ---- one operand of a conversion call.  The input comes first in a call's list, its outputs follow (at most two).  A packed buffer
// is carried as the plane its bytes are -- u8, 1 channel, 3 * cols wide, pitch and frame stride in bytes -- so that extents, staging
// and the copies both ways are the planes' (staged_layout then gives rows of 3 * cols bytes at a pitch rounded up to 4)
enum ConvKind { OP_RGB, OP_GRAY_F32, OP_U16, OP_F32, OP_PACKED };  // the operand's own rule: conv_check_operand
typedef int (*SlotOutRule)(wm_ctx*, const Slot&, const wm_plane*);
struct ConvOp {
    const char* name;      // the argument's name in messages
    ConvKind kind;
    const wm_plane* pl;    // as passed: a planar operand, or
    const wm_packed* pk;   // a packed one; both null: an output the call leaves out
    SlotOutRule match;     // an input that may be WM_MEM_SLOT_OUT: what the slot's last output must be (null: a caller's plane only)
    wm_plane v;            // the operand as a plane
    PlaneDesc d;           // resolved: what the kernel addresses -- the device plane, the slot's last output, or its place in a staging buffer
    Staged st;             // a host output's staging layout ...
    size_t off;            // ... and its offset in Slot::st_base
    bool present() const { return pl || pk; }
    bool in(int mem) const { return present() && v.mem == mem; }
    ByteRange range() const { return range_of(d, v.rows, v.cols, v.frames); }  // (nothing before the operand is resolved)
};
static ConvOp conv_plane(const char* name, ConvKind kind, const wm_plane* pl, SlotOutRule match = nullptr)
{
    ConvOp o{};
    o.name = name; o.kind = kind; o.pl = pl; o.match = match;
    if (pl) o.v = *pl;
    return o;
}
static ConvOp conv_packed(const char* name, const wm_packed* pk)
{
    ConvOp o{};
    o.name = name; o.kind = OP_PACKED; o.pk = pk;
    o.v.data = pk->data; o.v.rows = pk->rows; o.v.cols = (int32_t)(3 * (int64_t)pk->cols); o.v.channels = 1; o.v.dtype = WM_U8; o.v.mem = pk->mem;
    o.v.frames = pk->frames; o.v.pitch = pk->pitch_bytes; o.v.frame_stride = pk->frame_stride_bytes;
    return o;
}
// the descriptor the packed kernels take: a lane's four pixels are three dwords when base, pitch and frame stride are multiples of 4
static PackedDesc packed_desc(const ConvOp& o)
{
    PackedDesc d;
    d.p = o.d.p; d.pitch = o.d.pitch; d.fstride = o.d.fstride;
    d.aligned = reinterpret_cast<uintptr_t>(d.p) % 4 == 0 && d.pitch % 4 == 0 && d.fstride % 4 == 0;
    return d;
}
static int conv_check_operand(wm_ctx* ctx, const ConvOp& o)
{
    switch (o.kind) {
    case OP_RGB: return check_rgb_plane(ctx, o.pl, o.name, o.match != nullptr);
    case OP_GRAY_F32: return check_gray_f32(ctx, o.pl, o.name);
    case OP_U16: return check_plane16(ctx, o.pl, o.name);
    case OP_F32: return check_plane_f32(ctx, o.pl, o.name, o.match != nullptr);
    default: return check_packed(ctx, o.pk, o.name);
    }
}
static int fail_overlap(wm_ctx* ctx, const char* who, const ConvOp* op, int n, const char* where)
{
    if (n == 3) return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": " + op[0].name + ", " + op[1].name + " and " + op[2].name + " must not overlap" + where);
    return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": " + op[1].name + " overlaps " + op[0].name + where);
}

// ---- the conversions' frame.  The arguments are looked at in wm.h's order: shapes, each operand's own rules, frames between the
// operands (per_channel, the 16-bit calls: channels too, and the grid's z is frames x channels), the launch grid, overlap of device
// operands, slot, the scalar argument (scalar_check: weights, or bits / msb_aligned), and last what needs the slot -- a
// WM_MEM_SLOT_OUT input's matching rule and its overlap with the outputs.  Nothing is staged or launched before all of them have
// passed.  A host input is staged in Slot::st_in, host outputs side by side in Slot::st_base at multiples of 256 bytes -- never in
// st_out, which may hold the plane WM_MEM_SLOT_OUT names (the conversions neither read their input from the buffer they write nor
// change what the name means).  Every output ends the hand-overs whose plane it overwrites.  launch(stream, frames) reads the
// resolved operands; the calls are plain enqueues and queue no result records
extern "C++" {  // (a template cannot have C linkage)
template <class Scalar, class Launch>
static int convert_call(wm_ctx* ctx, const char* who, bool per_channel, ConvOp* op, int n, int slot, Scalar scalar_check, Launch launch)
{
    int rc;
    for (int i = 0; i < n; ++i)
        if (op[i].present() && (rc = check_shape(ctx, op[i].v.rows, op[i].pk ? op[i].pk->cols : op[i].v.cols, op[i].name)) != WM_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (op[i].present() && (rc = conv_check_operand(ctx, op[i])) != WM_OK) return rc;
    const int frames = op[0].v.frames, channels = op[0].v.channels;
    for (int i = 1; i < n && per_channel; ++i)
        if (op[i].present() && op[i].v.channels != channels) return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": channel count mismatch");
    for (int i = 1; i < n; ++i)
        if (op[i].present() && op[i].v.frames != frames) return fail(ctx, WM_ERR_BAD_ARG, std::string(per_channel ? who : op[i].name) + ": frame count mismatch");
    if (!convert_grid_fits(ctx->rows, per_channel ? frames * channels : frames)) return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": rows or frames beyond the launch grid");
    // overlap, on the resolved operands: host operands resolve to staging buffers of their own, a WM_MEM_SLOT_OUT input below
    for (int i = 0; i < n; ++i)
        if (op[i].in(WM_MEM_DEVICE)) op[i].d = desc_device(&op[i].v);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (ranges_overlap(op[i].range(), op[j].range())) return fail_overlap(ctx, who, op, n, "");
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = scalar_check()) != WM_OK) return rc;
    if (op[0].in(WM_MEM_SLOT_OUT)) {
        if ((rc = op[0].match(ctx, s, op[0].pl)) != WM_OK) return rc;
        op[0].d = s.last_out;
        for (int j = 1; j < n; ++j)
            if (ranges_overlap(op[0].range(), op[j].range())) return fail_overlap(ctx, who, op, n, " (the slot's last output)");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!op[0].in(WM_MEM_SLOT_OUT) && (rc = resolve_plane(ctx, s, &op[0].v, &s.st_in, &s.st_in_bytes, &op[0].d)) != WM_OK) return rc;
    size_t need = 0;
    for (int j = 1; j < n; ++j)
        if (op[j].in(WM_MEM_HOST)) { op[j].st = staged_layout(&op[j].v); op[j].off = round256(need); need = op[j].off + op[j].st.bytes; }
    if (need && (rc = ensure(ctx, &s.st_base, &s.st_base_bytes, need)) != WM_OK) return rc;
    for (int j = 1; j < n; ++j) {
        if (op[j].in(WM_MEM_HOST)) { op[j].d = op[j].st.d; op[j].d.p = (char*)s.st_base + op[j].off; }
        if (op[j].present()) invalidate_handovers(ctx, op[j].range());
    }
    launch(s.stream, frames);
    if ((rc = launch_check(ctx, s)) != WM_OK) return rc;
    for (int j = 1; j < n; ++j)
        if (op[j].in(WM_MEM_HOST) && (rc = stage_out(ctx, s, &op[j].v, op[j].d.p, op[j].st)) != WM_OK) return rc;
    return finish_call(ctx, s, slot, 0, 0, false, nullptr, nullptr);
}
}  // extern "C++"

int wm_rgb2gray(wm_ctx* ctx, const wm_plane* rgb, const wm_plane* gray_out, const float* weights, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (plane_null(rgb) || plane_null(gray_out)) return fail(ctx, WM_ERR_BAD_ARG, "wm_rgb2gray: null plane");
    ConvOp op[] = {conv_plane("rgb", OP_RGB, rgb, slot_out_rgb), conv_plane("gray_out", OP_GRAY_F32, gray_out)};
    float w[3];
    return convert_call(ctx, "wm_rgb2gray", false, op, 2, slot, [&] { return check_weights(ctx, weights, w); },
                        [&](hipStream_t st, int frames) { launch_rgb2gray(st, ctx->rows, ctx->cols, frames, op[0].d, op[1].d, w); });
}

int wm_unpack_rgb8(wm_ctx* ctx, const wm_packed* packed, const wm_plane* rgb_out, const wm_plane* gray_out, const float* weights, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!packed || !packed->data) return fail(ctx, WM_ERR_BAD_ARG, "wm_unpack_rgb8: null packed buffer");
    if (!rgb_out && !gray_out) return fail(ctx, WM_ERR_BAD_ARG, "wm_unpack_rgb8: rgb_out and gray_out are both null");
    if ((rgb_out && !rgb_out->data) || (gray_out && !gray_out->data)) return fail(ctx, WM_ERR_BAD_ARG, "wm_unpack_rgb8: null plane");
    ConvOp op[] = {conv_packed("packed", packed), conv_plane("rgb_out", OP_RGB, rgb_out), conv_plane("gray_out", OP_GRAY_F32, gray_out)};
    float w[3];
    return convert_call(ctx, "wm_unpack_rgb8", false, op, 3, slot, [&] { return check_weights(ctx, weights, w); },
                        [&](hipStream_t st, int frames) { launch_unpack_rgb8(st, ctx->rows, ctx->cols, frames, packed_desc(op[0]), op[1].d, op[2].d, w); });
}

int wm_pack_rgb8(wm_ctx* ctx, const wm_plane* rgb, const wm_packed* packed_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (plane_null(rgb) || !packed_out || !packed_out->data) return fail(ctx, WM_ERR_BAD_ARG, "wm_pack_rgb8: null plane or packed buffer");
    ConvOp op[] = {conv_plane("rgb", OP_RGB, rgb, slot_out_rgb), conv_packed("packed_out", packed_out)};
    return convert_call(ctx, "wm_pack_rgb8", false, op, 2, slot, [] { return WM_OK; },
                        [&](hipStream_t st, int frames) { launch_pack_rgb8(st, ctx->rows, ctx->cols, frames, op[0].d, packed_desc(op[1])); });
}

int wm_unpack16(wm_ctx* ctx, const wm_plane* src16, int bits, int msb_aligned, const wm_plane* out_f32, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!src16 || !src16->data || !out_f32 || !out_f32->data) return fail(ctx, WM_ERR_BAD_ARG, "wm_unpack16: null plane");
    ConvOp op[] = {conv_plane("src16", OP_U16, src16), conv_plane("out_f32", OP_F32, out_f32)};
    return convert_call(ctx, "wm_unpack16", true, op, 2, slot, [&] { return check_depth(ctx, bits, msb_aligned); }, [&](hipStream_t st, int frames) {
        float k_in, k_out;
        (void)wm_depth_scale(bits, &k_in, &k_out);
        launch_unpack16(st, ctx->rows, ctx->cols, frames, op[0].d, op[1].d, bits, msb_aligned, k_in);
    });
}

int wm_pack16(wm_ctx* ctx, const wm_plane* src_f32, const wm_plane* out16, int bits, int msb_aligned, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (plane_null(src_f32) || !out16 || !out16->data) return fail(ctx, WM_ERR_BAD_ARG, "wm_pack16: null plane");
    ConvOp op[] = {conv_plane("src_f32", OP_F32, src_f32, slot_out_f32), conv_plane("out16", OP_U16, out16)};
    return convert_call(ctx, "wm_pack16", true, op, 2, slot, [&] { return check_depth(ctx, bits, msb_aligned); }, [&](hipStream_t st, int frames) {
        float k_in, k_out;
        (void)wm_depth_scale(bits, &k_in, &k_out);
        launch_pack16(st, ctx->rows, ctx->cols, frames, op[0].d, op[1].d, bits, msb_aligned, k_out);  // (the u16 output is judged by the bytes it spans)
    });
}

// the front of the two host layers: everything they refuse themselves, before anything is queued; then the slot's f32 plane(s),
// dense in staged_layout's form, described as device planes for the calls below
static int open16(wm_ctx* ctx, const char* who, int mask, const wm_plane* p16, const char* what, int bits, int msb_aligned, int slot)
{
    int rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK || (rc = refuse_band(ctx, who)) != WM_OK) return rc;
    if ((rc = check_shape(ctx, p16->rows, p16->cols, what)) != WM_OK || (rc = check_plane16(ctx, p16, what)) != WM_OK) return rc;
    if (p16->channels != 1) return fail(ctx, WM_ERR_BAD_ARG, std::string(who) + ": grey planes only");
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    if ((rc = check_depth(ctx, bits, msb_aligned)) != WM_OK) return rc;
    return check_res_room(ctx, slot_of(ctx, slot), p16->frames);
}
static int slot_plane16(wm_ctx* ctx, void** buf, size_t* have, const wm_plane* like, wm_plane* pl)
{
    *pl = *like;
    pl->dtype = WM_F32; pl->mem = WM_MEM_DEVICE; pl->channels = 1; pl->channel_stride = 0;
    const Staged st = staged_layout(pl);
    pl->pitch = st.pitch; pl->frame_stride = st.d.fstride;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = ensure(ctx, buf, have, st.bytes, WM_ERR_ALLOC);
    pl->data = *buf;
    return rc;
}

int wm_embed16(wm_ctx* ctx, int mask, const wm_plane* in16, const wm_plane* out16, int bits, int msb_aligned, float* a_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!in16 || !in16->data || !out16 || !out16->data) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed16: null plane");
    int rc;
    if ((rc = check_shape(ctx, out16->rows, out16->cols, "out16")) != WM_OK) return rc;
    if ((rc = open16(ctx, "wm_embed16", mask, in16, "in16", bits, msb_aligned, slot)) != WM_OK) return rc;
    if ((rc = check_plane16(ctx, out16, "out16")) != WM_OK) return rc;
    if (out16->channels != 1 || out16->frames != in16->frames) return fail(ctx, WM_ERR_BAD_ARG, "wm_embed16: out16 must be a grey plane with in16's frame count");
    Slot& s = slot_of(ctx, slot);
    wm_plane X, Y;
    if ((rc = slot_plane16(ctx, &s.x16, &s.x16_bytes, in16, &X)) != WM_OK) return rc;
    // (a Y that moves takes the plane WM_MEM_SLOT_OUT named with it)
    if (s.y16_bytes < (size_t)X.frame_stride * X.frames * sizeof(float) && s.last_out.p == s.y16) { s.last_out_frames = 0; s.ho.valid = false; }
    if ((rc = slot_plane16(ctx, &s.y16, &s.y16_bytes, in16, &Y)) != WM_OK) return rc;
    // three enqueues; the embed as a batched call (never the fused kernels), one wait at the end of a synchronous call.
    // in16 is read completely before out16 is written (stream order): out16 may be in16
    const int q = slot_index(slot);
    if ((rc = wm_unpack16(ctx, in16, bits, msb_aligned, &X, q)) != WM_OK) return rc;
    if ((rc = wm_embed(ctx, mask, &X, &X, &Y, a_out, status_out, q)) != WM_OK) return rc;
    if ((rc = wm_pack16(ctx, &Y, out16, bits, msb_aligned, q)) != WM_OK) return rc;
    return slot == WM_SLOT_SYNC ? do_sync(ctx, s) : WM_OK;
}

int wm_detect16(wm_ctx* ctx, int mask, const wm_plane* img16, int bits, int msb_aligned, float* corr_out, int* status_out, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!img16 || !img16->data) return fail(ctx, WM_ERR_BAD_ARG, "wm_detect16: null plane");
    int rc;
    if ((rc = open16(ctx, "wm_detect16", mask, img16, "img16", bits, msb_aligned, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    wm_plane X;
    if ((rc = slot_plane16(ctx, &s.x16, &s.x16_bytes, img16, &X)) != WM_OK) return rc;
    const int q = slot_index(slot);
    if ((rc = wm_unpack16(ctx, img16, bits, msb_aligned, &X, q)) != WM_OK) return rc;
    if ((rc = wm_detect(ctx, mask, &X, corr_out, status_out, q)) != WM_OK) return rc;
    return slot == WM_SLOT_SYNC ? do_sync(ctx, s) : WM_OK;
}

// ---- wm_quality: PSNR and SSIM of a marked copy against its base (wm_k_quality.hip).  Both planes are only read: nothing of the slot
// changes but its staging buffers (a host ref is staged in st_in, a host test in st_base -- never in st_out, which may hold the plane
// WM_MEM_SLOT_OUT names), its quality scratch and, with q_out, its result records.  The kernels are launched outside any ProfScope
double wm_psnr_from_mse(double mse, double peak)
{
    if (!(mse >= 0.0) || !(peak > 0.0)) return std::numeric_limits<double>::quiet_NaN();
    if (mse == 0.0) return std::numeric_limits<double>::infinity();
    return 10.0 * std::log10(peak * peak / mse);
}

// what the slot's last output must be for a WM_MEM_SLOT_OUT test plane: an embed output of the operand's channels, frames and dtype
static int slot_out_any(wm_ctx* ctx, const Slot& s, const wm_plane* pl)
{
    if (s.last_out_frames == 0 || s.last_out.channels != pl->channels || pl->frames != s.last_out_frames || pl->dtype != s.last_out_dtype)
        return fail(ctx, WM_ERR_BAD_ARG, "WM_MEM_SLOT_OUT: no matching embed output on this slot (channels / frames / dtype must equal the last wm_embed's)");
    return WM_OK;
}

int wm_quality(wm_ctx* ctx, const wm_plane* ref, const wm_plane* test, int tile_rows, int tile_cols, float* q_out, double* sums_dev, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!ref || !ref->data || plane_null(test)) return fail(ctx, WM_ERR_BAD_ARG, "wm_quality: null plane");
    if (!q_out && !sums_dev) return fail(ctx, WM_ERR_BAD_ARG, "wm_quality: q_out and sums_dev are both null");
    int rc;
    if ((rc = check_shape(ctx, ref->rows, ref->cols, "ref")) != WM_OK || (rc = check_shape(ctx, test->rows, test->cols, "test")) != WM_OK) return rc;
    if ((rc = check_plane(ctx, ref, 0, true, "ref")) != WM_OK || (rc = check_plane(ctx, test, 0, true, "test", true)) != WM_OK) return rc;
    if (ref->channels != test->channels) return fail(ctx, WM_ERR_BAD_ARG, "wm_quality: channel count mismatch");
    if (ref->frames != test->frames) return fail(ctx, WM_ERR_BAD_ARG, "wm_quality: frame count mismatch");
    const int frames = ref->frames, channels = ref->channels, planes = frames * channels;
    if (!quality_grid_fits(planes)) return fail(ctx, WM_ERR_BAD_ARG, "wm_quality: frames x channels beyond the launch grid");
    TileShape ts{0, 0, 1, 1};  // tile_rows == tile_cols == 0: one tile per plane
    if ((tile_rows != 0 || tile_cols != 0) && (rc = tiles_checked(ctx, "wm_quality", tile_rows, tile_cols, &ts)) != WM_OK) return rc;
    if ((rc = refuse_band(ctx, "wm_quality")) != WM_OK) return rc;
    if ((rc = check_slot(ctx, slot)) != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if (test->mem == WM_MEM_SLOT_OUT && (rc = slot_out_any(ctx, s, test)) != WM_OK) return rc;
    if (q_out && (rc = check_res_room(ctx, s, (long long)planes * WM_QUALITY_NVALS, "channels x 3")) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PlaneDesc xd, yd;
    if ((rc = resolve_plane(ctx, s, ref, &s.st_in, &s.st_in_bytes, &xd)) != WM_OK) return rc;
    if (test->mem == WM_MEM_SLOT_OUT) yd = s.last_out;
    else if ((rc = resolve_plane(ctx, s, test, &s.st_base, &s.st_base_bytes, &yd)) != WM_OK) return rc;
    const QualityGeom q = quality_geom(ctx->rows, ctx->cols, channels, ts.th);
    const size_t rec_bytes = round256(quality_rec_bytes(q, ts, planes));
    const size_t sums_bytes = sums_dev ? 0 : (size_t)planes * ts.ny * ts.nx * WM_QUALITY_NSUMS * sizeof(double);
    if ((rc = ensure(ctx, &s.qual_scr, &s.qual_scr_bytes, rec_bytes + sums_bytes, WM_ERR_ALLOC)) != WM_OK) return rc;
    double* sums = sums_dev ? sums_dev : (double*)((char*)s.qual_scr + rec_bytes);
    // the Gaussian of Wang et al.: g[i] = exp(-(i - 5)^2 / 4.5) over the sum of the eleven values, f64, formed here once per call
    double g[11], gsum = 0.0;
    for (int i = 0; i < 11; ++i) { g[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5); gsum += g[i]; }
    QualityWeights w;
    for (int i = 0; i < 6; ++i) w.g[i] = g[i] / gsum;
    launch_quality(s.stream, q, w, ts, planes, xd, yd, (double*)s.qual_scr, sums, q_out ? s.d_res + s.res_used : nullptr);
    return finish_call(ctx, s, slot, q_out ? frames : 0, q_out ? channels * WM_QUALITY_NVALS : 0, false, q_out, nullptr);
}

int wm_gram(wm_ctx* ctx, const wm_plane* img, double* gram_out, int slot)
{
    if (!ctx || !gram_out) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", WM_MASK_ME, 0, nullptr, &sw)) != WM_OK) return rc;
    const int frames = img->frames;
    if ((rc = gram_sweep(ctx, s, sw, img)) != WM_OK) return rc;
    if ((rc = launch_check(ctx, s)) != WM_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    HIPCHK(ctx, hipMemcpy(gram_out, s.d_gramtot, (size_t)frames * NGRAM * sizeof(double), hipMemcpyDeviceToHost));
    return WM_OK;
}

// ---- intra-frame sharding: the context works on a row band of a larger image (wm.h) ----------------------------
int wm_band_configure(wm_ctx* ctx, int own_lo, int own_hi, long long rows_global)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    for (auto& t : ctx->slots) t.ho.valid = false;  // (a hand-over holds whole-image lag sums: not what a band's Gram sweep adds up)
    if (own_hi == 0) { ctx->band_lo = ctx->band_hi = 0; ctx->band_rows_global = 0; return WM_OK; }
    if (own_lo < 0 || own_hi > ctx->rows || own_lo >= own_hi) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_configure: bad row range");
    // a side that is not an image border needs p/2 + 1 halo rows of image data: k_detect scores e_u = u - c.nbrs(u), i.e. it
    // reads the mask one row away from the pixel, and the mask reads x another p/2 rows away (2 rows for p = 3)
    const int need = ctx->p / 2 + 1 > 2 ? ctx->p / 2 + 1 : 2;
    if ((own_lo > 0 && own_lo < need) || (own_hi < ctx->rows && ctx->rows - own_hi < need))
        return fail(ctx, WM_ERR_BAD_ARG, "wm_band_configure: an interior side needs " + std::to_string(need) + " halo rows (p/2 + 1)");
    if (rows_global < own_hi - own_lo) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_configure: rows_global smaller than the band");
    if (ctx->rows < 4 || ctx->cols < 5) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_configure: band too small");
    ctx->band_lo = own_lo; ctx->band_hi = own_hi; ctx->band_rows_global = rows_global;
    return WM_OK;
}

int wm_band_solve(wm_ctx* ctx, const double* totals, int frames, int* status_out, int slot)
{
    if (!ctx || !totals || frames < 1 || frames > ctx->max_frames) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_solve: bad arguments");
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(s.d_totals, totals, (size_t)frames * NGRAM * sizeof(double), hipMemcpyHostToDevice, s.stream));
    launch_solve_totals(s.stream, frames, s.d_totals, s.d_coef, s.d_status);
    if ((rc = launch_check(ctx, s)) != WM_OK) return rc;
    std::vector<int> st((size_t)frames);
    HIPCHK(ctx, hipMemcpyAsync(st.data(), s.d_status, (size_t)frames * sizeof(int), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    rc = WM_OK;
    for (int f = 0; f < frames; ++f) {
        if (status_out) status_out[f] = st[f];
        if (st[f] != 0) rc = WM_UNSOLVABLE;
    }
    return rc;
}

// ---- the launches of the band phases, shared by the host-exchange calls (totals copied to the caller's host arrays) and the
// device-resident ones (wm_band_*_dev: totals handed over in device memory, nothing synchronises); the profile leaves them out
// stats sweep of the owned rows; the fold tail leaves {max|e| (or 1), sum} per frame in s.d_raw[0 .. frames)
static int band_stats_launch(wm_ctx* ctx, Slot& s, int mask, const wm_plane* in_gray, int* frames_out)
{
    int rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    Sweep sw;
    if ((rc = open_input(ctx, s, in_gray, "inputImage", mask, 1, nullptr, &sw)) != WM_OK) return rc;
    const int frames = in_gray->frames;
    sweep_stats(ctx, s, false, mask_route(ctx, s, sw.lg, frames, mask, sw.x), s.d_res + s.res_used);  // (records written by the tail, not delivered: no pending entry)
    *frames_out = frames;
    return launch_check(ctx, s);
}

// embed sweep of the owned rows with the scalars in s.d_scal (device planes, out must not overlap the input)
static int band_embed_launch(wm_ctx* ctx, Slot& s, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out)
{
    int rc;
    const int frames = in_gray->frames;
    if ((rc = check_plane(ctx, base, frames, true, "outputImage")) != WM_OK) return rc;
    if ((rc = check_plane(ctx, out, frames, true, "out")) != WM_OK) return rc;
    if (out->channels != base->channels || out->dtype != base->dtype) return fail(ctx, WM_ERR_BAD_ARG, "out must match outputImage in channels and dtype");
    if (in_gray->mem != WM_MEM_DEVICE || base->mem != WM_MEM_DEVICE || out->mem != WM_MEM_DEVICE)
        return fail(ctx, WM_ERR_BAD_ARG, "wm_band_embed: device planes only");
    const PlaneDesc xd = desc_device(in_gray), bd = desc_device(base), od = desc_device(out);
    if (descs_overlap(xd, od, ctx->rows, ctx->cols, frames)) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_embed: out must not overlap the input (halo rows are shared)");
    invalidate_handovers(ctx, od, frames);
    LaunchGeom lg;
    if ((rc = geom_checked(ctx, frames, mask, &lg)) != WM_OK) return rc;
    launch_embed(mask_route(ctx, s, lg, frames, mask, xd), own_w(ctx), EmbedPlanes{bd, od, s.d_scal});
    return launch_check(ctx, s);
}

// detect sweep of the owned rows; the fold tail leaves {<e_u,e_w>, |e_u|^2, |e_w|^2} per frame in s.d_raw[max_frames ..)
static int band_detect_launch(wm_ctx* ctx, Slot& s, int mask, const wm_plane* img, int* frames_out)
{
    int rc;
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", mask, 1, nullptr, &sw)) != WM_OK) return rc;
    const int frames = img->frames;
    sweep_detect(ctx, s, K_NONE, sw, s.d_res + s.res_used);
    *frames_out = frames;
    return launch_check(ctx, s);
}

int wm_band_stats(wm_ctx* ctx, int mask, const wm_plane* in_gray, double* out, int slot)
{
    if (!ctx || !out) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    int frames = 0;
    if ((rc = band_stats_launch(ctx, s, mask, in_gray, &frames)) != WM_OK) return rc;
    std::vector<RawSums> raw((size_t)frames);
    HIPCHK(ctx, hipMemcpyAsync(raw.data(), s.d_raw, (size_t)frames * sizeof(RawSums), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    for (int f = 0; f < frames; ++f) { out[2 * f] = raw[f].v[0]; out[2 * f + 1] = raw[f].v[1]; }
    return WM_OK;
}

int wm_band_embed(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out,
                  const double* max_sum, float* a_out, int slot)
{
    if (!ctx || !max_sum) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = check_plane(ctx, in_gray, 0, false, "inputImage")) != WM_OK) return rc;
    const int frames = in_gray->frames;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the strength from the all-reduced totals, as embed_scalars_frame computes it (Watermark.cpp:170)
    std::vector<EmbedScalars> sc((size_t)frames);
    for (int f = 0; f < frames; ++f) {
        const double mx = max_sum[2 * f], ss = max_sum[2 * f + 1];
        sc[f].maxe = mask == WM_MASK_ME ? (float)mx : 1.0f;
        const double nrm = mask == WM_MASK_ME ? sqrt(ss) / (double)sc[f].maxe : sqrt(ss);
        sc[f].a = ctx->sF / (float)(nrm / sqrt_n(ctx));
        if (a_out) a_out[f] = sc[f].a;
    }
    HIPCHK(ctx, hipMemcpyAsync(s.d_scal, sc.data(), (size_t)frames * sizeof(EmbedScalars), hipMemcpyHostToDevice, s.stream));
    rc = band_embed_launch(ctx, s, mask, in_gray, base, out);
    HIPCHK(ctx, hipStreamSynchronize(s.stream));  // sc must outlive the copy
    return rc;
}

int wm_band_detect_sums(wm_ctx* ctx, int mask, const wm_plane* img, double* out, int slot)
{
    if (!ctx || !out) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    int frames = 0;
    if ((rc = band_detect_launch(ctx, s, mask, img, &frames)) != WM_OK) return rc;
    std::vector<RawSums> raw((size_t)frames);
    HIPCHK(ctx, hipMemcpyAsync(raw.data(), s.d_raw + ctx->max_frames, (size_t)frames * sizeof(RawSums), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(ctx, hipStreamSynchronize(s.stream));
    for (int f = 0; f < frames; ++f) { out[3 * f] = raw[f].v[0]; out[3 * f + 1] = raw[f].v[1]; out[3 * f + 2] = raw[f].v[2]; }
    return WM_OK;
}

// ---- the same phases with the exchange resident in device memory: every call only ENQUEUES on the slot's stream (give the
// slot the stream the caller's collectives are ordered on: wm_set_stream), every total is handed over in device memory the
// caller owns, so the collectives (RCCL all-reduce / all-gather on that stream) run between them without the host in the chain
int wm_band_gram_dev(wm_ctx* ctx, const wm_plane* img, double* totals_dev, int slot)
{
    if (!ctx || !totals_dev) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    Sweep sw;
    if ((rc = open_input(ctx, s, img, "image", WM_MASK_ME, 0, nullptr, &sw)) != WM_OK) return rc;
    // (the sweep's solve tail also solves from the band's own partial totals into the slot: overwritten by wm_band_solve_dev)
    sweep_gram(ctx, s, K_NONE, sw, totals_dev);
    return launch_check(ctx, s);
}

int wm_band_solve_dev(wm_ctx* ctx, const double* totals_dev, int frames, int slot)
{
    if (!ctx || !totals_dev || frames < 1 || frames > ctx->max_frames) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_solve_dev: bad arguments");
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    launch_solve_totals(s.stream, frames, totals_dev, s.d_coef, s.d_status);
    return launch_check(ctx, s);
}

int wm_band_stats_dev(wm_ctx* ctx, int mask, const wm_plane* in_gray, double* max_sum_dev, int slot)
{
    if (!ctx || !max_sum_dev) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    int frames = 0;
    if ((rc = band_stats_launch(ctx, s, mask, in_gray, &frames)) != WM_OK) return rc;
    launch_band_pick(s.stream, frames, s.d_raw, 2, max_sum_dev);
    return launch_check(ctx, s);
}

int wm_band_embed_dev(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out,
                      const double* gathered_max_sum_dev, int nparts, float* a_dev, int slot)
{
    if (!ctx || !gathered_max_sum_dev || nparts < 1) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    if ((rc = check_mask(ctx, mask)) != WM_OK) return rc;
    if ((rc = check_plane(ctx, in_gray, 0, false, "inputImage")) != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    launch_band_scalars(s.stream, in_gray->frames, gathered_max_sum_dev, nparts, mask, ctx->sF, sqrt_n(ctx), mask == WM_MASK_ME ? s.d_status : nullptr, s.d_scal, a_dev);
    return band_embed_launch(ctx, s, mask, in_gray, base, out);
}

int wm_band_detect_sums_dev(wm_ctx* ctx, int mask, const wm_plane* img, double* sums_dev, int slot)
{
    if (!ctx || !sums_dev) return WM_ERR_BAD_ARG;
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    int frames = 0;
    if ((rc = band_detect_launch(ctx, s, mask, img, &frames)) != WM_OK) return rc;
    launch_band_pick(s.stream, frames, s.d_raw + ctx->max_frames, 3, sums_dev);
    return launch_check(ctx, s);
}

int wm_band_corr_dev(wm_ctx* ctx, const double* sums_dev, int frames, float* corr_dev, int slot)
{
    if (!ctx || !sums_dev || !corr_dev || frames < 1 || frames > ctx->max_frames) return fail(ctx, WM_ERR_BAD_ARG, "wm_band_corr_dev: bad arguments");
    int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    Slot& s = slot_of(ctx, slot);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    launch_band_corr(s.stream, frames, sums_dev, s.d_status, corr_dev);
    return launch_check(ctx, s);
}

int wm_sync(wm_ctx* ctx, int slot)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    const int rc = check_slot(ctx, slot);
    if (rc != WM_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return do_sync(ctx, slot_of(ctx, slot));
}

int wm_set_stream(wm_ctx* ctx, int slot, void* hip_stream)
{
    if (!ctx || slot < 0 || slot >= ctx->nslots) return fail(ctx, WM_ERR_BAD_ARG, "bad slot");
    Slot& s = ctx->slots[slot];
    if (!s.pending.empty()) { int rc = do_sync(ctx, s); if (rc < 0) return rc; }
    const hipStream_t next = hip_stream ? (hipStream_t)hip_stream : s.own;
    if (next != s.stream) {
        // the slot's scratch (coefficients, status words, raw totals, tickets) may still be in use by work enqueued on the old
        // stream that nobody waits for (the wm_band_*_dev phases only enqueue): the new stream starts behind it
        HIPCHK(ctx, hipSetDevice(ctx->device));
        hipEvent_t ev;
        HIPCHK(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, s.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(next, ev, 0);
        (void)hipEventDestroy(ev);  // (released once the recorded work has completed)
        if (e != hipSuccess) return fail(ctx, WM_ERR_RUNTIME, std::string("wm_set_stream: ") + hipGetErrorString(e));
        s.stream = next;
    }
    return WM_OK;
}

void* wm_get_stream(wm_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= ctx->nslots) return nullptr;
    return (void*)ctx->slots[slot].stream;
}

void* wm_dev_alloc(int device, size_t bytes)
{
    void* p = nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
    return p;
}
void wm_dev_free(void* p) { if (p) (void)hipFree(p); }
int wm_memcpy_h2d(void* dst, const void* src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? WM_OK : WM_ERR_RUNTIME;
}
int wm_memcpy_d2h(void* dst, const void* src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? WM_OK : WM_ERR_RUNTIME;
}
int wm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void* wm_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void wm_host_free(void* p) { if (p) (void)hipHostFree(p); }

int wm_selftest_nvf_quotient(int device, int variant, uint32_t bits_lo, uint32_t bits_hi, unsigned long long* mismatches, uint32_t* first_bad)
{
    if (variant < 0 || variant > 3 || bits_lo > bits_hi) return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    unsigned long long* d = nullptr;
    if (hipMalloc((void**)&d, 16) != hipSuccess) return WM_ERR_ALLOC;
    const unsigned long long init[2] = {0ull, ~0ull};
    unsigned long long got[2] = {0ull, ~0ull};
    if (hipMemcpy(d, init, 16, hipMemcpyHostToDevice) != hipSuccess) rc = WM_ERR_RUNTIME;
    if (rc == WM_OK) {
        launch_selftest_quot(nullptr, variant, bits_lo, bits_hi, d);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(got, d, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = WM_ERR_RUNTIME;
    }
    (void)hipFree(d);
    if (mismatches) *mismatches = got[0];
    if (first_bad) *first_bad = (uint32_t)got[1];
    return rc;
}

int wm_membench(int device, int kind, size_t bytes, double seconds, double* mean_us, int* launches)
{
    if (kind < 0 || kind > 5 || bytes < 4096 || !(seconds >= 0.0) || seconds > 30.0) return WM_ERR_BAD_ARG;
    int rc = choose_device(&device);
    if (rc != WM_OK) return rc;
    const size_t n16 = bytes / 16;
    void *src = nullptr, *dst = nullptr;
    unsigned long long* sink = nullptr;
    hipStream_t st = nullptr;
    constexpr int NEV = 32;   // launches in flight between two waits
    hipEvent_t ea[NEV], eb[NEV];
    int nev = 0;
    double total_ms = 0.0;
    int count = 0;
    do {
        if (kind % 3 != 0 && hipMalloc(&src, n16 * 16) != hipSuccess) { rc = WM_ERR_ALLOC; break; }
        if (kind % 3 != 2 && hipMalloc(&dst, n16 * 16) != hipSuccess) { rc = WM_ERR_ALLOC; break; }
        if (hipMalloc((void**)&sink, 8) != hipSuccess) { rc = WM_ERR_ALLOC; break; }
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { rc = WM_ERR_RUNTIME; break; }
        if (src && hipMemsetAsync(src, 0x3c, n16 * 16, st) != hipSuccess) { rc = WM_ERR_RUNTIME; break; }
        if (hipMemsetAsync(sink, 0, 8, st) != hipSuccess) { rc = WM_ERR_RUNTIME; break; }
        for (; nev < NEV; ++nev)
            if (hipEventCreate(&ea[nev]) != hipSuccess || hipEventCreate(&eb[nev]) != hipSuccess) { rc = WM_ERR_RUNTIME; break; }
        if (rc != WM_OK) break;
        for (int w = 0; w < 3; ++w) launch_membench(st, kind, src, dst, n16, sink, ea[0], eb[0]);  // warm-up
        if (hipStreamSynchronize(st) != hipSuccess) { rc = WM_ERR_RUNTIME; break; }
        const auto t0 = std::chrono::steady_clock::now();
        do {
            for (int k = 0; k < NEV; ++k) launch_membench(st, kind, src, dst, n16, sink, ea[k], eb[k]);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { rc = WM_ERR_RUNTIME; break; }
            for (int k = 0; k < NEV; ++k) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ea[k], eb[k]) == hipSuccess) { total_ms += ms; ++count; }
            }
        } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);
    } while (false);
    for (int k = 0; k < nev; ++k) { (void)hipEventDestroy(ea[k]); (void)hipEventDestroy(eb[k]); }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(src); (void)hipFree(dst); (void)hipFree(sink);
    if (rc != WM_OK) { (void)hipGetLastError(); return rc; }
    if (mean_us) *mean_us = count ? 1e3 * total_ms / count : 0.0;
    if (launches) *launches = count;
    return WM_OK;
}

int wm_rows(const wm_ctx* ctx) { return ctx ? ctx->rows : 0; }
int wm_cols(const wm_ctx* ctx) { return ctx ? ctx->cols : 0; }
int wm_p(const wm_ctx* ctx) { return ctx ? ctx->p : 0; }
float wm_strength_factor(const wm_ctx* ctx) { return ctx ? ctx->sF : 0.0f; }
int wm_device(const wm_ctx* ctx) { return ctx ? ctx->device : -1; }
const float* wm_w_device(const wm_ctx* ctx) { return ctx && ctx->w ? ctx->w->d_w : nullptr; }

int wm_prof_enable(wm_ctx* ctx, int on)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    if (!on) { int rc = prof_collect(ctx); if (rc != WM_OK) return rc; }
    ctx->prof = on != 0;
    return WM_OK;
}
int wm_prof_reset(wm_ctx* ctx)
{
    if (!ctx) return WM_ERR_BAD_ARG;
    int rc = prof_collect(ctx);
    for (int k = 0; k < K_COUNT; ++k) { ctx->prof_n[k] = 0; ctx->prof_ms[k] = 0.0; }
    return rc;
}
int wm_prof_kernel_count(void) { return K_COUNT; }
const char* wm_prof_kernel_name(int k) { return k >= 0 && k < K_COUNT ? kKernelNames[k] : ""; }
int wm_prof_get(wm_ctx* ctx, int k, uint64_t* launches, double* total_ms)
{
    if (!ctx || k < 0 || k >= K_COUNT) return WM_ERR_BAD_ARG;
    int rc = prof_collect(ctx);
    if (launches) *launches = ctx->prof_n[k];
    if (total_ms) *total_ms = ctx->prof_ms[k];
    return rc;
}

const char* wm_strerror(int code)
{
    switch (code) {
        case WM_OK: return "ok";
        case WM_UNSOLVABLE: return "prediction system not solvable (image passed through / correlation 0)";
        case WM_ERR_BAD_P: return "Wrong p parameter";
        case WM_ERR_W_OPEN: return "Error opening file for Random noise W array";
        case WM_ERR_W_SIZE: return "Error: W file total elements != image dimensions!";
        case WM_ERR_RUNTIME: return "HIP runtime or kernel failure";
        case WM_ERR_BAD_ARG: return "bad argument";
        case WM_ERR_NO_DEVICE: return "no usable HIP device (the engine has no CPU fallback)";
        case WM_ERR_ALLOC: return "allocation failed";
        case WM_ERR_PSNR: return "PSNR must be a positive number";
        case WM_ERR_BUSY: return "too many un-synced operations on this slot";
        default: return "unknown error";
    }
}
const char* wm_last_error(const wm_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }
const char* wm_version(void) { return "wm-hip 0.1 (gfx950)"; }

}  // extern "C"
