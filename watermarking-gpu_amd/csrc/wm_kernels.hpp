// wm_kernels.hpp -- host-visible launch interface of the HIP kernels (internal to libwm_hip.so)
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

namespace wmk {

// Per-kernel timing (wm_prof_*): the events of a profiled launch are attached to the dispatch itself (hipExtLaunchKernelGGL's
// start / stop events = the begin and end time stamps of that dispatch, what rocprofv3's kernel trace reports).  Events
// recorded around a launch (hipEventRecord before / after) also time the marker packets and the dispatch gap between two
// dependent kernels: 5-25 us on top of a ~110 us kernel, different for every kernel.  The launcher functions do not know
// about profiling: wm_api.hip's ProfScope parks itself in a thread-local slot, every launch made through WM_KLAUNCH while it
// is set draws a pair of events from it.
struct LaunchProf {
    static constexpr int MAX = 4;          // launches of one sweep at most (aligned part + generic remainder, march + border ...)
    hipEvent_t a[MAX], b[MAX];
    int n = 0;
    hipEvent_t (*get)(void*) = nullptr;    // hands out an event (the context's pool)
    void* owner = nullptr;
};
LaunchProf*& launch_prof_slot();  // (thread-local; defined in wm_api.hip)
// every launch made while a scope is set gets its own start / stop pair (a sweep may be two launches: the aligned strips and
// the generic remainder; their durations are summed into one call of that kernel)
#define WM_KLAUNCH(KERNEL, GRID, BLOCKDIM, SHMEM, STREAM, ...)                                                         \
    do {                                                                                                               \
        ::wmk::LaunchProf* lp_ = ::wmk::launch_prof_slot();                                                            \
        if (lp_ && lp_->n < ::wmk::LaunchProf::MAX) {                                                                  \
            const int i_ = lp_->n++;                                                                                   \
            lp_->a[i_] = lp_->get(lp_->owner); lp_->b[i_] = lp_->get(lp_->owner);                                      \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCKDIM, SHMEM, STREAM, lp_->a[i_], lp_->b[i_], 0, __VA_ARGS__);      \
        } else {                                                                                                       \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCKDIM, SHMEM, STREAM, __VA_ARGS__);                                    \
        }                                                                                                              \
    } while (0)

constexpr int NGRAM = 44;  // 36 unique Rx entries + 8 rx entries (me_p3.hpp:8-21)
// Ticket counters of the fold tails ("the last block / wave finishes") sit one per 128-byte line: TKS words apart.  Packed,
// the 16 frame counters of a launch shared ONE line and the 256 strip counters eight: every arrival of a launch (2 880 blocks
// in k_gram, 11 520 waves in k_detect, each a returning atomic the wave waits for before it may leave) queued on the same
// few lines, and how long that queue was depended on where the allocation happened to land.
constexpr int TKS = 32;

struct PlaneDesc {
    const void* p;
    long long pitch;    // elements
    long long fstride;  // elements between frames
    long long cstride;  // elements between channels
    int dtype;          // 0 f32, 1 u8 (2 u16: wm_k_convert16.hip only)
    int channels;
    int aligned;        // base/pitch/strides allow 4-pixel vector access
};

struct LaunchGeom {
    int rows, cols;
    int nstrips, nfull, nsegs, rps;  // nfull = strips lying fully inside the image (cols / 256)
    int nblk;  // strip-march blocks per frame (all strips)
    int nbb;   // blocks per frame of k_gram_border
    // rows whose pixels this launch owns: sums and stores cover [row_lo, row_hi) only.  The whole image unless the
    // context works on a row band of a larger image (intra-frame sharding, wm_band_*): then the plane is the band plus
    // its halo rows, row_lo == 0 / row_hi == rows mark the sides that are true image borders
    int row_lo, row_hi;
};

// Which strips a detector sweep runs on (detect_plan, wm_march.hpp): the records, the strip tickets and the folds follow ld
struct DetectPlan {
    LaunchGeom ld;        // the sweep's geometry
    bool overlap, split;  // overlapped strips / overlapped strips + one generic strip; neither: the plain strips
};

struct EmbedScalars {
    float a;     // watermark strength (Watermark.cpp:170)
    float maxe;  // max|e| (ME) or 1
};

// ---- the launch records: what the sweep launchers below share, filled once per call (wm_api.hip) and described here only ----
// What every launcher of a call is told about it.  coef / status: the Gram sweep's solve per frame as the sweeps behind it read
// it; null where the call's route has no solve (the embed side under NVF)
struct Sweep {
    hipStream_t s;
    LaunchGeom lg;
    int frames;
    int mask, pad;       // the kernels' mask index (0 ME, 1 NVF) and the half width of the window (ME: 1)
    PlaneDesc x;         // the grey input plane
    const float* coef;   // [frames][8]
    const int* status;   // [frames]
};
// The key side of a sweep: one W plane (the context's own: a bank of one) or a bank of nkeys planes kstride elements apart.
// aligned_w: the planes may be addressed as buffers with 32-bit offsets
struct KeyBank {
    const float* W;
    long long kstride;
    int nkeys;
    int aligned_w;
};
// the groups of `per` that n keys / copies / offsets make (the last one may be short): the grid blocks per tile of the group kernels
inline int group_count(int n, int per) { return (n + per - 1) / per; }
// The planes an embed sweep reads and writes beside x, and the frames' scalars of the stats sweep (null: the launcher has its own)
struct EmbedPlanes {
    PlaneDesc base, out;
    const EmbedScalars* scal;
};
// Tile shape and tiles per axis (wm_tiles_shape): pixel (r, c) belongs to tile (min(r / th, ny - 1), min(c / tw, nx - 1))
struct TileShape {
    int th, tw, ny, nx;
};

// raw totals of the stats and detect sweeps, written by the fold tails beside the finished scalars: what a row band of a
// sharded image contributes to the all-reduce (wm_band_*)
struct RawSums {
    double v[4];  // stats: {max|e| (or 1), sum (m W)^2, -, -}; detect: {<e_u,e_w>, ||e_u||^2, ||e_w||^2, -}
};

struct alignas(8) OpResult {  // (8 bytes, naturally aligned: the fused kernels deliver it with one store)
    int status;   // 0 OK, 1 unsolvable
    float value;  // a (embed) or correlation (detect)
};

// Fold tails ("the last block finishes", wm_device.hpp): what the block that arrives last does with the partials.
struct SolveTail {       // k_gram: fold Gram partials, solve the 8x8 system (Watermark.cpp:203)
    unsigned* ticket;    // [frames] zero between ops
    int expected;        // blocks per frame over all launches of the sweep (march blocks + border blocks)
    int nbb_total;       // border partial records per frame
    float* coef;         // [frames][8]
    int* status;         // [frames]
    double* gram_tot;    // [frames][44]
};
struct ScalarsTail {     // k_me_stats / k_nvf_stats: a = sF / (float)(||u|| / sqrt(N))   (Watermark.cpp:170)
    unsigned* ticket;        // [frames] frame-level tickets: blocks of the frame, or (Geom::quad) its strips
    unsigned* ticket_strip;  // quad: [frames][nstrips] strip-level tickets (count the waves = segments of a strip)
    int expected;            // blocks per frame over all launches of the sweep (block-level fold)
    int nsegs, nstrips;
    float* smax;             // [frames][nstrips] strip records: max|e| ...
    double* sss;             // ... and sum
    float sF;
    double sqrt_n;
    EmbedScalars* scal;
    OpResult* res;
    RawSums* raw;        // [frames]
};
struct CorrTail {        // k_detect: corr = (float)dot / (float)(||e_w|| ||e_u||)   (Watermark.cpp:230)
    unsigned* ticket;
    unsigned* ticket_strip;
    int expected;
    int nsegs, nstrips;
    double* scorr;           // [frames][nstrips][3] strip records
    OpResult* res;
    RawSums* raw;        // [frames]
};

// ---- fused single-frame path (wm_k_fused.hip): one launch per operation, the frame's tiles stay in LDS ----------------
struct FusedGeom {
    int rows, cols;
    int nstrips, nbands, th;  // tiles of 256 columns x th rows; grid = nstrips * nbands workgroups (<= CU count)
    int rpw;                  // rows per wavefront: 4 (th <= 64) or 8 (th <= 128) with 16 wavefronts; 16 with 8 (experiments)
    int G;
    int nbw;                  // workgroups that take the Gram matrix's border chunks
    int folder;               // workgroup that folds the statistics of an embed
    int bx0, bx1, bn0;        // ... those of XCDs bx0, bx1 (bn0 = workgroups on bx0), or bx0 < 0: the first nbw
    int fusable;              // 0: shape not supported by the fused kernels (the caller takes the streaming kernels)
};
struct FusedScratch {        // per slot, device memory (one allocation; layout in wm_api.hip)
    double* pmain;            // 2 x ([13][G] + [44][nbw])  workgroup records of the Gram phase (term-major); second half: k_fused_pair's detector
    unsigned long long* gstat;  // [G][4]  statistics of an embed as {epoch, 32 bits} granules
    unsigned long long* gcorr;  // [G][8]  the detector's sums as {epoch, half} granule pairs
    unsigned long long* gdone;  // [G]     end-of-embed flags
    unsigned long long* gran; // 2 x [32] published {epoch, value} granules (second half: k_fused_pair's detector)
    unsigned* cnt;            // [27][32] arrival counters, one per 128-byte line (zero between calls)
    unsigned long long* stamps;  // [G][16] phase time stamps (development aid) or null
    int dbg;                     // development switches of the fused kernels (timing experiments; 0 in production)
};
constexpr size_t FUSED_CNT_BYTES = 27 * 128;
constexpr int FUSED_MAX_WG = 256;        // workgroups of a fused grid at most: what the folding wavefronts cover (4 per lane)
constexpr int FUSED_INCOMPLETE = -98;    // result-record status: output stores were issued but the end of the frame was not observed
FusedGeom fused_geometry(int rows, int cols, int ncu);
// return 0 when the launch was issued (errors of the launch itself surface through hipGetLastError)
// embed + detect of its output in one launch (grey planes of one type): -2 = planes the pair kernel does not take
int launch_fused_pair(hipStream_t s, const FusedGeom& fg, const FusedScratch& sc, unsigned epoch_embed, unsigned epoch_detect, int mask,
                      const PlaneDesc& x, const float* W, const PlaneDesc& base, const PlaneDesc& out, float sF, double sqrt_n,
                      OpResult* res_embed, OpResult* res_detect);
int launch_fused_embed(hipStream_t s, const FusedGeom& fg, const FusedScratch& sc, unsigned epoch, int mask, const PlaneDesc& x,
                       const float* W, const PlaneDesc& base, const PlaneDesc& out, float sF, double sqrt_n, OpResult* res);
int launch_fused_detect(hipStream_t s, const FusedGeom& fg, const FusedScratch& sc, unsigned epoch, int mask, const PlaneDesc& x,
                        const float* W, OpResult* res);

// redo: frames with redo[f] == 0 are skipped (k_gram_redo, the fallback of a checked hand-over), null: every frame (k_gram)
// coef / status (here and in launch_gram_ho): where the solve tail writes what the later sweeps read as sw.coef / sw.status
void launch_gram(const Sweep& sw, double* pmain, double* pborder, unsigned* ticket, float* coef, int* status, double* gram_tot,
                 const int* redo = nullptr);
void launch_me_stats(const Sweep& sw, const KeyBank& w, float* pmax, double* pss, unsigned* ticket, unsigned* ticket_strip, float* smax,
                     double* sss, float sF, double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw);
void launch_nvf_stats(const Sweep& sw, const KeyBank& w, double* pss, unsigned* ticket, unsigned* ticket_strip, double* sss, float sF,
                      double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw);
// Gram hand-over from an embed to the detector that reads its output (wm_set_handover, WM_MEM_SLOT_OUT): k_embed holds every
// row of y in registers, so it also accumulates y's 13 lag sums over the products that stay inside a wave's tile (its strip's
// columns x its segment's rows and the two rows behind them) and leaves one record per wave, plus a compact copy of the two
// columns on either side of every strip boundary; k_gram_ho adds the products across strip boundaries from that copy, the
// border frame and the solve -- the detector's Gram sweep over y is not run.
//   rec:  [frames][stride][13]            wave records at [0, nstrips * nsegs), k_gram_ho's seam-block records behind them
//   seam: [frames][nstrips - 1][rows][4]  y at columns S-2, S-1, S, S+1 of the boundary S in front of strip k (k = 1 ..)
//   dig:  [frames][stride]                digest records of y (dig_add, wm_device.hpp): one per wave of k_embed, k_gram_ho's
//                                         seam-block shares of them behind
//   fdig: [frames]                        the digest of each frame of y, folded by k_gram_ho's last block
struct HandOver {
    double* rec;
    int stride;
    float* seam;
    unsigned long long* dig;
    unsigned long long* fdig;
};
// Checked hand-over (wm_detect on the plane a slot's last embed wrote): k_detect's checking instance sums the digest of the
// plane it reads and holds it against HandOver::fdig -- equal: the score stands; different: nothing is published, redo[f] = 1,
// and the predicated k_gram_redo / k_detect_redo that follow redo that frame from the plane as it is (their blocks of frames
// with redo[f] = 0 leave at once, before any ticket)
struct DigCheck {
    unsigned long long* pdig;        // [frames][records] digest records of this sweep
    unsigned long long* sdig;        // [frames][nstrips] strip records (Geom::quad)
    const unsigned long long* want;  // [frames] HandOver::fdig
    int* redo;                       // [frames] written by the checking instance, read by the redo launches
    unsigned long long* count;       // [2] frames trusted / redone (cumulative)
};
int handover_seam_blocks(const LaunchGeom& lg);   // seam blocks per frame of k_gram_ho for this geometry
// returns true when the hand-over instantiation ran (f32 grey planes on the aligned path, p = 3, segments of >= 2 rows)
bool launch_embed(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const HandOver* ho = nullptr);
// sw.x: y, the plane the embed wrote; sw.lg: the geometry of the embed that left the wave records
void launch_gram_ho(const Sweep& sw, const HandOver& ho, double* pborder, unsigned* ticket, float* coef, int* status, double* gram_tot);
void launch_mask(const Sweep& sw, const EmbedScalars* scal, const PlaneDesc& mo, const PlaneDesc& eo);
// dc / mode: 0 = the ordinary sweep (dc unused); 1 = the checking instance (f32 planes on the overlapped aligned 3x3 path:
// detect_checkable); 2 = k_detect_redo, the frames with dc->redo[f] != 0 only
void launch_detect(const Sweep& sw, const KeyBank& w, double* pcorr, unsigned* ticket, unsigned* ticket_strip, double* scorr, OpResult* res,
                   RawSums* raw, const DigCheck* dc = nullptr, int mode = 0);
bool detect_checkable(const Sweep& sw, int aligned_w);
// one image against a bank of keys (wm_detect_keys, wm_k_detect_keys.hip): k_detect's sweep for every key of the bank, key
// groups as a grid axis, then one fold block per (frame, key) into res[frame * nkeys + key].  part: [frames][2 nkeys + 1][rstride]
// doubles of scratch.  Returns -1 when the sweep's records exceed rstride (nothing is launched)
int launch_detect_keys(const Sweep& sw, const KeyBank& bank, double* part, int rstride, OpResult* res);
int detect_keys_group(void);  // keys per group of k_detect_keys (compile-time KG)
// k_keys_fold: one block per (frame, key) folds the records part [frames][nkeys][rstride][2] / partw [frames][rstride] of a
// sweep in k_detect's order into res[frame * nkeys + key]; a strip-level fold (quad) covers KEYS_MAX_STRIPS strips
constexpr int KEYS_MAX_STRIPS = 256;
void launch_keys_fold(hipStream_t s, const double* part, const double* partw, int rstride, int frames, int nkeys, int quad, int nblk,
                      int nsegs, int nstrips, const int* status, OpResult* res);
// one image against a rectangle of window offsets into ONE key plane of pitch key_cols that is larger than the image
// (wm_detect_offsets, wm_k_detect_offsets.hip): offset (oy0 + i, ox0 + j), i < ny, j < nx, scores the image against the window
// key[oy : oy + rows, ox : ox + cols] -- k_detect_keys' sweep with groups of horizontally adjacent offsets as a grid axis, then
// k_keys_fold into res[frame * ny * nx + i * nx + j].  The caller has checked that every window lies inside the plane.
// key: the one plane (nkeys 1, kstride unused), aligned_w: the KEY plane's extent allows 32-bit offsets.  part: [frames][2 ny nx + 1][rstride]
// doubles of scratch.  Returns -1 when the sweep's records exceed rstride (nothing is launched)
int launch_detect_offsets(const Sweep& sw, const KeyBank& key, int key_cols, int oy0, int ox0, int ny, int nx, double* part, int rstride,
                          OpResult* res);
int detect_offsets_group(void);  // offsets per group of k_detect_offsets' shared-row instances (compile-time OG)
// the detector's three sums per tile of the frame (wm_detect_tiles, wm_k_detect_tiles.hip).  k_detect_tiles is k_detect's sweep
// with segments whose height divides tile_rows; every lane leaves its f32 partials in rec [frames][nsegs][nstrips][3][64], and
// k_tiles_fold adds each tile's records in a fixed order in f64 into map [frames][ny][nx] (and sums [frames][ny][nx][3], may be
// null) on the device and res[frame] = {status, 0}
struct TileGeom {
    int th, tw, ny, nx;        // the call's TileShape
    int rps, nsegs, nstrips;   // the sweep's record geometry: segments of rps rows (rps divides th), strips
    int layout;                // who owns a column group of 4: 0 = strips of 256, 1 = overlapped strips, 2 = overlapped + one generic strip
    int nown;                  // layouts 1, 2: column groups the overlapped strips own
    int ngroups;               // column groups in all (layout 2: the generic strip's 64 lanes count as the last 64)
};
struct TilesPlan : DetectPlan {  // the sweep's geometry: strips as every detector takes them for this plane
    TileGeom tg;
    size_t rec_bytes;          // size of rec for this call
    int fold_threads;          // threads per tile of k_tiles_fold: 64 or 256
};
int tiles_segment_rows(int tile_rows);  // the largest divisor of tile_rows in 8 .. 48 (tile_rows is a multiple of 8)
// sw.lg: make_geom's geometry of the call (the plan replaces its segments; the launchers that take a plan sweep on pl.ld)
TilesPlan tiles_plan(const Sweep& sw, int aligned_w, const TileShape& ts);
void launch_detect_tiles(const Sweep& sw, const TilesPlan& pl, const KeyBank& w, float* rec);
void launch_tiles_fold(hipStream_t s, const TilesPlan& pl, int frames, const float* rec, const int* status, float* map, double* sums,
                       OpResult* res);
// the detector's three sums per tile of the frame AND per key of a bank (wm_detect_keys_tiles, wm_k_detect_keys_tiles.hip):
// k_detect_keys' sweep (key groups of detect_keys_group() keys as a grid axis) on the geometry of tiles_plan; every lane leaves its
// f32 partials in rec [frames][ngroups][nsegs][nstrips][2 G + 1][64] (keys_tiles_rec_bytes), and k_keys_tiles_fold adds each
// (frame, key, tile)'s records in k_tiles_fold's order into map [frames][nkeys][ny][nx] (and sums [...][3], may be null) on the
// device and res[frame] = {status, 0}.  keys_tiles_grids_fit: both grids of such a call fit 31 bits (from the shapes alone)
size_t keys_tiles_rec_bytes(const TilesPlan& pl, int frames, int nkeys);
bool keys_tiles_grids_fit(int rows, int cols, int tile_rows, int frames, int nkeys, int ny, int nx);
void launch_detect_keys_tiles(const Sweep& sw, const TilesPlan& pl, const KeyBank& bank, float* rec);
void launch_keys_tiles_fold(hipStream_t s, const TilesPlan& pl, int frames, int nkeys, const float* rec, const int* status, float* map,
                            double* sums, OpResult* res);
// one image embedded with every key of a bank (wm_embed_keys, wm_k_embed_keys.hip).  The image side is wm_embed's (launch_gram:
// coef / status); then k_stats_keys (k_me_stats' / k_nvf_stats' sweep for every key, key groups as a grid axis), one fold block
// per (frame, key) into res[frame * nkeys + key] and the scalars k_embed_keys reads, and k_embed_keys (k_embed's sweep for every
// key: copy (frame, key) is frame frame * nkeys + key of `out`).  scratch: embed_keys_scratch_bytes of device memory, the same
// for the three launches.  launch_stats_keys returns -1 when the sweep's records exceed rstride (nothing is launched)
size_t embed_keys_scratch_bytes(int frames, int nkeys, int rstride);
int launch_stats_keys(const Sweep& sw, const KeyBank& bank, void* scratch, int rstride);
void launch_embed_keys_fold(const Sweep& sw, int nkeys, void* scratch, int rstride, float sF, double sqrt_n, OpResult* res);
void launch_embed_keys(const Sweep& sw, const KeyBank& bank, const EmbedPlanes& ep, void* scratch, int rstride);  // (ep.scal: null, the scalars lie in scratch)
int embed_keys_group(void);  // keys per group of k_stats_keys / k_embed_keys (compile-time EKG)
// a payload in the mark (wm_embed_signs / wm_detect_bits, wm_k_bits.hip).  k_embed_signs is k_embed's sweep (the same body, march
// and launch loop, wm_embed_march.hpp; never the hand-over) with u = m W multiplied by the sign of the pixel's tile: signs [frames][ny][nx]
// int8 in {-1, 0, +1} on the device.  k_bits_fold: one wave per (frame, bit) adds the rows of sums [frames][ntiles][3] (k_tiles_fold's)
// named by idx [start[bit], start[bit + 1]) one after the other and writes res[frame * nbits + bit] = {status, soft}
void launch_embed_signs(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const signed char* signs, const TileShape& ts);
void launch_bits_fold(hipStream_t s, int frames, int nbits, int ntiles, const double* sums, const int* start, const int* idx,
                      const int* status, OpResult* res);
// one frame, many payload copies (wm_embed_signs_multi, wm_k_embed_signs_multi.hip): k_embed_signs' sweep with the image side formed
// once per row and the sign, fmaf, clamp and store repeated for a compile-time group of copies; copy groups are a grid axis
// (k_embed_keys' block order).  signs [frames][ncopies][ny][nx] on the device; copy (frame, k) is frame frame * ncopies + k of ep.out;
// ep.scal: the frame's scalars of the single-W stats sweep.  embed_signs_multi_grid_fits: every grid of the sweep times the copy groups
// fits 31 bits -- from the shapes alone, asked before the call has resolved a plane, so from the geometry and not from a Sweep
bool embed_signs_multi_grid_fits(const LaunchGeom& lg, int frames, int ncopies);
void launch_embed_signs_multi(const Sweep& sw, const KeyBank& w, const EmbedPlanes& ep, const signed char* signs, int ncopies, const TileShape& ts);
int embed_signs_group(void);  // copies per group of k_embed_signs_multi (compile-time SMG)
// a key per frame of a batch (wm_embed_select / wm_detect_select, wm_k_select.hip): the single-key sweeps above -- their bodies, launch
// plans and scratch arrays -- with W resolved per frame, W_f = bank.W + kidx[frame] * bank.kstride.  kidx [frames] on the device, every
// entry in 0 .. bank.nkeys - 1 (checked by the caller); bank.aligned_w: every plane of the bank may be addressed with 32-bit offsets.
// launch_embed_sel never hands over; launch_detect_sel is launch_detect's ordinary sweep (mode 0)
void launch_me_stats_sel(const Sweep& sw, const KeyBank& bank, const int* kidx, float* pmax, double* pss, unsigned* ticket,
                         unsigned* ticket_strip, float* smax, double* sss, float sF, double sqrt_n, EmbedScalars* scal, OpResult* res,
                         RawSums* raw);
void launch_nvf_stats_sel(const Sweep& sw, const KeyBank& bank, const int* kidx, double* pss, unsigned* ticket, unsigned* ticket_strip,
                          double* sss, float sF, double sqrt_n, EmbedScalars* scal, OpResult* res, RawSums* raw);
void launch_embed_sel(const Sweep& sw, const KeyBank& bank, const EmbedPlanes& ep, const int* kidx);
void launch_detect_sel(const Sweep& sw, const KeyBank& bank, const int* kidx, double* pcorr, unsigned* ticket, unsigned* ticket_strip,
                       double* scorr, OpResult* res, RawSums* raw);
// the pixel-format front (wm_rgb2gray / wm_unpack_rgb8 / wm_pack_rgb8, wm_k_convert.hip): element-wise kernels, a lane per four
// consecutive pixels of a row, grid (column chunks, rows, frames) -- convert_grid_fits: rows and frames fit the grid's y and z.
// PackedDesc: interleaved 8-bit R, G, B (wm_packed) in BYTES; aligned: base, pitch and frame stride are multiples of 4, so a
// lane's four pixels are three dwords.  PlaneDesc::aligned says the same of a planar plane (vec_ok's rule); a null PlaneDesc::p
// is an output the call leaves out.  w: the three grey weights; grey = (w[0] * R + w[1] * G) + w[2] * B in f32
struct PackedDesc {
    const void* p;
    long long pitch, fstride;  // bytes
    int aligned;
};
bool convert_grid_fits(int rows, int frames);
void launch_rgb2gray(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& rgb, const PlaneDesc& gray, const float* w);
void launch_unpack_rgb8(hipStream_t s, int rows, int cols, int frames, const PackedDesc& pk, const PlaneDesc& rgb, const PlaneDesc& gray, const float* w);
void launch_pack_rgb8(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& rgb, const PackedDesc& pk);
// samples of 9 to 16 bits (wm_unpack16 / wm_pack16, wm_k_convert16.hip): the same lane mapping with frames x channels as the grid's
// z (convert_grid_fits(rows, frames * channels)).  One plane has dtype 2 (u16: 2-byte elements; aligned: base a multiple of 4 bytes,
// pitch and used strides even, so a lane's four samples are one 8-byte access), the other is f32; both have the same channels.
// k_in / k_out: wm_depth_scale's constants of `bits`
void launch_unpack16(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& src, const PlaneDesc& out, int bits, int msb_aligned, float k_in);
void launch_pack16(hipStream_t s, int rows, int cols, int frames, const PlaneDesc& src, const PlaneDesc& out, int bits, int msb_aligned, float k_out);
// PSNR and SSIM of one plane against another (wm_quality, wm_k_quality.hip).  A plane is one (frame, channel) pair, `planes` =
// frames x channels of them (the grid's z: quality_grid_fits).  k_quality marches strips of 64 columns in segments of rps rows and
// leaves rec [planes][nsegs][ngroups][3] f64 = {sse, ssim_sum, max|d|} per column group of 4; k_quality_fold_cols and k_quality_fold add
// each tile's records in a fixed order (per segment and tile column into part [planes][nsegs][nx][3] behind rec, then per tile) into
// sums [planes][ny][nx][5] = {sse, npix, ssim_sum, nwin, max|d|}; k_quality_total (res non-null) adds a plane's tiles in ascending
// index and writes res[plane * 3 ..] = {mse, ssim, max|d|}, status 0.  rec: quality_rec_bytes of scratch.  ts: the tile grid,
// th = tw = 0 with ny = nx = 1 for one tile per plane.  w: the six distinct weights of the 11-tap Gaussian, g[i] = g[10 - i], formed
// on the host
struct QualityGeom {
    int rows, cols, channels;
    int rps, nsegs, nstrips;  // segments of rps rows (rps divides the tile height), strips of 64 columns
    int ngroups;              // column groups of 4
};
struct QualityWeights {
    double g[6];
};
QualityGeom quality_geom(int rows, int cols, int channels, int tile_rows);
size_t quality_rec_bytes(const QualityGeom& q, const TileShape& ts, int planes);
bool quality_grid_fits(int planes);
void launch_quality(hipStream_t s, const QualityGeom& q, const QualityWeights& w, const TileShape& ts, int planes, const PlaneDesc& x,
                    const PlaneDesc& y, double* rec, double* sums, OpResult* res);
// the 2-D complex f32 transform (wm_fft2 / wm_locate, wm_k_fft.hip).  launch_fft_rows: every row of a dense [nrows][P] interleaved
// complex plane in place, P = 2^6 .. 2^13, nrows a multiple of 64, exp(-2 pi i ..) forward and exp(+2 pi i ..) inverse, neither
// normalised; tw: [P] complex, fft_twiddles' table of that length on the device.  launch_fft_transpose: dst [ncols][nrows] =
// src^T, both sides multiples of 64, out of place.  launch_locate_mul: a = conj(a) * b over n complex elements (n even)
constexpr int FFT_LOG_MIN = 6, FFT_LOG_MAX = 13;
int fft_log2(int n);                   // log2 of a length the row transform takes, -1 for any other n
void fft_twiddles(int P, float* out);  // [P][2] = exp(-2 pi i t / P), formed in f64 (host)
// the tables of a [pr][pc] transform on the device (a blocking copy): tw_dev [pr] complex for the columns, then [pc] complex for the rows
hipError_t fft_twiddles_upload(float* tw_dev, int pr, int pc);
void launch_fft_rows(hipStream_t s, float* data, int nrows, int P, const float* tw, bool inverse);
void launch_fft_transpose(hipStream_t s, const float* src, float* dst, int nrows, int ncols);
void launch_locate_mul(hipStream_t s, float* a, const float* b, size_t n);
// where a crop sits in its key (the locate family, wm_k_locate.hip), one frame per launch.  launch_locate_e: the frame's prediction
// error e (and, under NVF, mask m) as dense [rows][cols] f32 planes, from sw.x with the solve sw.coef / sw.status of that frame.
// launch_locate_h: h = m * (adjoint of the stencil) e as the real part of the zeroed [pr][pc] complex plane.
// The key side, a source laid into a zeroed [pr][pc] complex plane: launch_locate_lay, one dense real [rows][cols] plane (a key, or a
// pooled image side in the place of h) as the real part; launch_locate_lay_bits, the key masked to the tiles of bit b0 (real part) and
// of bit b1 (imaginary part; -2: none), tile_bit: the DEVICE table over the tiles ts of the KEY plane; launch_locate_lay_keys, key_a
// (real part) and key_b (imaginary part; null: none), and nz[0] / nz[1], DEVICE ints cleared on the stream beforehand, set to 1 when
// key_a / key_b holds a value other than 0.
// launch_locate_map: the admissible ny x nx values of the inverse plane times 1 / (pr pc) into map_a (real parts) and, with pair,
// map_b (imaginary parts; either may be null), a half whose nz is clear as exact zero (nz null: no flags, key A in use), and the
// frame's four records {oy, ox, peak, z} of key A into res[0 .. 4), of key B into res[4 .. 8) (res null: the map pass alone); part:
// locate_part_bytes of scratch per half; status: the frame's
size_t locate_part_bytes(int ny, int nx);
void launch_locate_e(const Sweep& sw, int frame, float* e, float* m);
void launch_locate_h(const Sweep& sw, int frame, const float* e, const float* m, float* plane, int pr, int pc);
void launch_locate_lay(hipStream_t s, const float* src, int rows, int cols, float* plane, int pr, int pc);
void launch_locate_lay_bits(hipStream_t s, const float* key, int key_rows, int key_cols, const int* tile_bit, const TileShape& ts, int b0, int b1,
                            float* plane, int pr, int pc);
void launch_locate_lay_keys(hipStream_t s, const float* key_a, const float* key_b, int key_rows, int key_cols, float* plane, int pr, int pc, int* nz);
void launch_locate_map(hipStream_t s, const float* plane, int pr, int pc, int ny, int nx, const int* status, const int* nz, bool pair, float* map_a,
                       float* map_b, void* part, OpResult* res);
// a payload-marked crop (wm_locate_bits): two bits per transform.  launch_locate_mul3: out = conj(h) * k over n complex elements (n
// even), h and k kept.  launch_locate_bits_acc: the pair's inverse plane into the two maps (map1 null: no second bit; use0 / use1
// false: a bit without a tile, whose map is exactly zero) and into energy (first: stored, else added); part: one frame's and pair's
// block records (locate_bits_part_bytes), epart: the frame's fold of the finished energy map (locate_part_bytes; the last pair only,
// else null).  launch_locate_bits_fold: the frame's four records of the energy map into loc[0 .. 4) and its soft values into
// soft[0 .. nbits); part: [pairs][blocks], maps: [nbits][ny nx]
size_t locate_bits_part_bytes(int ny, int nx);
void launch_locate_mul3(hipStream_t s, const float* h, const float* k, float* out, size_t n);
void launch_locate_bits_acc(hipStream_t s, const float* plane, int pr, int pc, int ny, int nx, const int* status, bool first, bool use0, bool use1,
                            float* map0, float* map1, float* energy, void* part, void* epart);
void launch_locate_bits_fold(hipStream_t s, const void* epart, const void* part, int ny, int nx, int nbits, const float* energy, const float* maps,
                             const int* status, OpResult* loc, OpResult* soft);
// the frames of a clip pooled on the image side (wm_clip_pool), one launch per call: pool = fmaf(w_f, h_f, pool) over the solvable
// frames of sw in ascending order, h_f being launch_locate_e's and launch_locate_h's bit for bit; pool: a dense DEVICE
// [rows][cols] f32 plane, started from 0.0f unless accumulate; weights: DEVICE [frames]; res[0 .. frames): the frames' status records
void launch_clip_pool(const Sweep& sw, const float* weights, float* pool, bool accumulate, OpResult* res);
// ... the same result by a direct gather from cache, one pixel per lane and no LDS: wm_clip_pool_bench's yardstick, taken by no call
void launch_clip_pool_gather(const Sweep& sw, const float* weights, float* pool, bool accumulate, OpResult* res);
// band mode: solve the 8x8 system from all-reduced Gram totals [frames][44]; writes coef / status like k_gram's tail
void launch_solve_totals(hipStream_t s, int frames, const double* totals, float* coef, int* status);
// band mode, device-resident exchange (wm_band_*_dev): glue kernels between the sweeps and the caller's collectives
void launch_band_pick(hipStream_t s, int frames, const RawSums* raw, int n, double* out);
void launch_band_scalars(hipStream_t s, int frames, const double* parts, int nparts, int mask, float sF, double sqrt_n, const int* status,
                         EmbedScalars* scal, float* a_dev);
void launch_band_corr(hipStream_t s, int frames, const double* sums, const int* status, float* corr);
// W generated on the device (wm_create_generated): same values as csrc/app/wm_genw.cpp writes
void launch_gen_w(hipStream_t s, float* w, int rows, int cols, uint32_t seed);
// exhaustive check of the NVF quotient sequence against the IEEE division (wm_selftest_nvf_quotient)
void launch_selftest_quot(hipStream_t s, int variant, uint32_t bits_lo, uint32_t bits_hi, unsigned long long* out2);
// memory-system yardstick (wm_membench): kind 0 store, 1 copy, 2 read; n16 = 16-byte elements
void launch_membench(hipStream_t s, int kind, const void* src, void* dst, size_t n16, unsigned long long* sink, hipEvent_t a, hipEvent_t b);
void launch_mask_result(hipStream_t s, int frames, const int* status, const float* coef, OpResult* res, float* coef_out);

}  // namespace wmk
