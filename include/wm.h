/*
 * wm.h -- C ABI of the MI355X-native watermark engine (libwm_hip.so).
 *
 * This is the drop-in boundary for the reference's `Watermark` class hot path
 * (kar-dim/Watermarking-GPU, Watermark_GPU/Watermark.hpp:26-72, Watermark.cpp:21-258):
 * NVF mask, 3x3 prediction-error (ME) mask, PSNR-scaled embed, correlation detector.
 * The reference has no FFI of its own (its L3 class calls ArrayFire/OpenCL directly);
 * each entry point below names the reference member it replaces.  The C++ surface that keeps
 * the reference's class/method names lives in include/Watermark.hpp and is a thin wrapper
 * over exactly these functions.
 *
 * Conventions
 *  - planes are row-major: x(r,c) = data[r*pitch + c]  (reference frames: main.cpp:355,379,405;
 *    W file: Watermark.cpp:62-75, W(r,c) = file[r*cols + c]); borders replicate (clamp-to-edge,
 *    nvf.hpp:9, me_p3.hpp:45, scaled_neighbors_p3.hpp:14).
 *  - all plane pointers are DEVICE pointers unless mem == WM_MEM_HOST (then the library
 *    stages through its own device buffers with hipMemcpy2DAsync on the slot's stream;
 *    pinned host memory from wm_host_alloc() makes those copies truly asynchronous).
 *  - a plane may describe a batch: `frames` planes `frame_stride` elements apart; one call
 *    then processes all frames with one launch per kernel (frames are independent units,
 *    main.cpp:326-331).
 *  - every call is an ENQUEUE on the slot's HIP stream; scalar results (a, correlation, status)
 *    are delivered to the caller's pointers by wm_sync(ctx, slot).  Passing slot = WM_SLOT_SYNC
 *    runs on slot 0 and synchronises before returning.
 *  - status codes: 0 OK; 1 WM_UNSOLVABLE (not an error: embed leaves out == base bit-exact and
 *    `a` untouched, detect yields 0.0f -- Watermark.cpp:164-165,246-247); < 0 errors, which the
 *    C++ wrapper turns into std::runtime_error like the reference (Watermark.cpp:24-25,65-66,70-71,
 *    111-113).
 *  - a ctx is thread-compatible, not thread-safe (the reference object is not re-entrant either:
 *    its const methods mutate the shared texture, Watermark.cpp:88-93,223).  Concurrency is by
 *    slot: each slot owns a stream and private scratch.
 */
#ifndef WM_H_
#define WM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM_OK 0
#define WM_UNSOLVABLE 1
#define WM_ERR_BAD_P (-1)      /* p not in {3,5,7,9} (Watermark.cpp:24-25); ME needs p == 3 (main.cpp:89) */
#define WM_ERR_W_OPEN (-2)     /* W file cannot be opened (Watermark.cpp:65-66) */
#define WM_ERR_W_SIZE (-3)     /* W file size != rows*cols*4 (Watermark.cpp:70-71) */
#define WM_ERR_RUNTIME (-4)    /* HIP runtime / kernel failure (Watermark.cpp:111-113,133-135,194-196) */
#define WM_ERR_BAD_ARG (-5)    /* null pointer, shape mismatch, bad slot, unsupported layout */
#define WM_ERR_NO_DEVICE (-6)  /* no usable HIP device: the product path has no CPU fallback */
#define WM_ERR_ALLOC (-7)
#define WM_ERR_PSNR (-8)       /* psnr <= 0 (main.cpp:96) */
#define WM_ERR_BUSY (-9)       /* too many un-synced operations queued on one slot */

#define WM_SLOT_SYNC (-1)

typedef struct wm_ctx wm_ctx;

/* enum MASK_TYPE { ME, NVF }  (Watermark.hpp:10-14) -- same order and values */
typedef enum wm_mask_type { WM_MASK_ME = 0, WM_MASK_NVF = 1 } wm_mask_type;
/* WM_U16: 2-byte samples of 9 to 16 bits (10-bit video).  Only wm_unpack16, wm_pack16, wm_embed16 and wm_detect16 take it; every
 * other entry point refuses it as a bad dtype. */
typedef enum wm_dtype { WM_F32 = 0, WM_U8 = 1, WM_U16 = 2 } wm_dtype;
/* WM_MEM_SLOT_OUT (input planes only, `data` ignored): the device copy of what the last wm_embed on the same slot wrote
 * (grey output; same frames / dtype).  A streamed frame staged from host memory is then detected without crossing the host
 * link a second time: wm_embed(host in, host out, slot) ; wm_detect(SLOT_OUT plane, slot).  Valid until the slot's next embed.
 * wm_rgb2gray and wm_pack_rgb8 take the slot's last 3-CHANNEL output under the same name. */
typedef enum wm_mem { WM_MEM_DEVICE = 0, WM_MEM_HOST = 1, WM_MEM_SLOT_OUT = 2 } wm_mem;

/* Stand-in for the af::array arguments of makeWatermark/detectWatermark (Watermark.hpp:69-70):
 * a non-owning view.  channels == 1 (grey) or 3 (planar RGB: [3][rows][pitch], main.cpp:169-190).
 * Any base address, pitch and width is accepted.  Speed: device planes of f32 elements whose base is 4-byte aligned, and of
 * u8 elements whose base, pitch and strides are multiples of 4 bytes, take the kernels' vector path (planes below 4 GiB);
 * a width that is not a multiple of 4 costs 10-17 % (one generic strip at the right edge), anything else re-lays every row
 * through LDS (~25 % slower).  WM_MEM_HOST planes are de-pitched into an aligned staging buffer. */
typedef struct wm_plane {
    void* data;
    int32_t rows, cols;
    int32_t channels;
    int32_t dtype;           /* wm_dtype: f32 in [0,255], or u8 (video Y plane, main.cpp:355-357); u16 for the four *16 calls only */
    int32_t mem;             /* wm_mem */
    int32_t frames;          /* >= 1 */
    int64_t pitch;           /* elements between rows (>= cols) */
    int64_t channel_stride;  /* elements between channel planes (ignored when channels == 1) */
    int64_t frame_stride;    /* elements between frames (ignored when frames == 1) */
} wm_plane;

/* Watermark::Watermark(rows, cols, randomMatrixPath, p, psnr, programs)  (Watermark.hpp:63, Watermark.cpp:21-27).
 * `w_rowmajor` is the host copy of the W file contents (rows*cols f32).  `device` replaces
 * settings.ini's opencl_device (main.cpp:73) as a HIP device ordinal. */
int wm_create(wm_ctx** out, int device, int rows, int cols, int p, float psnr, const float* w_rowmajor);
/* same, reading the raw f32 file itself: loadRandomMatrix (Watermark.cpp:62-75) */
int wm_create_from_file(wm_ctx** out, int device, int rows, int cols, int p, float psnr, const char* w_path);
/* same, with W generated ON the device from a seed: the counter-based N(0,1) generator of csrc/app/wm_genw.cpp (this build's
 * CommonRandomMatrix, CommonRandomMatrix/main.cpp:16-68) -- element (r,c) depends on (seed, r, c) only, so the matrix equals
 * the file `wm_genw rows cols seed file` writes (to the last ulp of the device's f64 log / cos) and every GPU of a node
 * fills its own copy without a file, an upload or a broadcast.  wm_w_device() + wm_memcpy_d2h() read it back. */
int wm_create_generated(wm_ctx** out, int device, int rows, int cols, int p, float psnr, uint32_t seed);
/* Watermark(const Watermark&) / operator= (Watermark.cpp:30-51): shares W, owns new scratch.  The clone takes EVERY setting of the
 * source: shape, p, psnr, slots and max_frames, rows per segment, fused mode, wm_set_handover, wm_set_checked_handover and the band.
 * It does not take the caller's streams (every slot of the clone runs on a stream of its own), queued results, what
 * WM_MEM_SLOT_OUT names, pending hand-overs, the checked hand-over's counts or profile numbers (profiling starts switched off).
 * Source and clone are independent afterwards: either may be reinitialised or destroyed without the other noticing. */
int wm_clone(const wm_ctx* src, wm_ctx** out);
/* ---- Reconfiguring a context: wm_reinit, wm_reinit_from_file, wm_configure, wm_set_rows_per_segment ------------------------------
 * All four rebuild every slot, and behave alike.  After the arguments have been checked (a refused call changes nothing) they
 *   1. wait for all slots and DELIVER what is queued on them, as wm_sync would: strengths, scores, statuses and coefficients reach
 *      the callers' pointers.  An unsolvable frame is in its status; the call itself still returns WM_OK (as wm_set_stream does),
 *      and a wm_sync afterwards has nothing left to deliver.  An error (< 0) of the wait is returned and nothing is rebuilt;
 *   2. start every slot afresh: WM_MEM_SLOT_OUT names nothing until the slot's next embed (WM_ERR_BAD_ARG), no hand-over is pending,
 *      promised or checked, wm_checked_handover_counts reads (0, 0), and the scratch that grows on demand (staging buffers, key and
 *      tile records, table arenas, the 16-bit planes) is gone and grows again with the first call that needs it.
 * KEPT by all four: p, psnr, the number of slots and max_frames (wm_configure: as given), rows per segment (wm_set_rows_per_segment:
 * as given), fused mode, wm_set_handover, wm_set_checked_handover, profiling (switched on or off, and the numbers recorded so far),
 * and the caller's stream of every slot that still exists: a slot given a stream with wm_set_stream still runs on it, ordered with
 * the caller's collectives as before; a slot index beyond a smaller nslots is gone, and its stream with it (WM_ERR_BAD_ARG).
 * The BAND (wm_band_configure) is kept by wm_configure and wm_set_rows_per_segment and cleared by the two reinits: it describes rows
 * of the old planes.  After a reinit planes and key banks of the old shape are WM_ERR_BAD_ARG.
 * Results do not depend on how a context reached its configuration: the same shape, W, p, psnr, slots, max_frames, rows per segment,
 * fused mode, hand-over settings and band give the same bits (tests/test_gpu_lifecycle.py). */
/* Watermark::reinitialize(path, rows, cols)  (Watermark.cpp:78-85) */
int wm_reinit(wm_ctx* ctx, int rows, int cols, const float* w_rowmajor);
int wm_reinit_from_file(wm_ctx* ctx, int rows, int cols, const char* w_path);
void wm_destroy(wm_ctx* ctx);

/* number of slots (streams + scratch) and the largest `frames` a call may carry; default 2 x 1.  A reconfiguring call (above) */
int wm_configure(wm_ctx* ctx, int nslots, int max_frames);
/* One image per synchronous call (slot = WM_SLOT_SYNC, frames == 1: what makeWatermark / detectWatermark are in the
 * reference, Watermark.cpp:156-172,234-250) runs as ONE launch whose tiles stay in LDS when the shape allows it (p = 3,
 * cols >= 256 -- any width for f32 planes, a multiple of 4 for u8 planes --, rows/cols small enough for one 256 x <=128 tile
 * per CU: up to 3840x2160 on MI355X; aligned planes); everything else, and every batched / asynchronous call, takes the batched sweeps.  mode 0 switches
 * the fused kernels off, 1 (default; environment WM_FUSED=0 changes the default) on.  Results of the two paths agree to
 * the rounding of the partial sums' grouping (tests/test_gpu_fused.py). */
int wm_set_fused(wm_ctx* ctx, int mode);
/* Gram hand-over from wm_embed to a detector that reads its output (opt-in; default off).  The detector's first sweep --
 * the Gram matrix of the watermarked plane, Watermark.cpp:234-250 through computePredictionErrorMask -- reads a plane that
 * k_embed has just produced in registers.  With the hand-over on, a batched wm_embed (two frames or more) of grey f32 planes on the
 * aligned path (p = 3) also accumulates the lag sums of its output that stay inside each wavefront's tile, and wm_detect /
 * wm_gram on a WM_MEM_SLOT_OUT plane (the slot's last embed output, by contract unmodified since) then only adds the
 * products across tile seams, the border frame and the solve: one of the five sweeps of an embed + detect pair is not run.
 * The 44 sums are the same exact products in another f64 summation order (agreement ~1e-16 relative, tests/test_gpu_handover.py);
 * any other detector input, dtype or shape takes the ordinary Gram sweep.  Costs ~19 MB of device memory per slot at 4K.
 * The sums describe the plane, not a detector: every detector-side call that names the plane as WM_MEM_SLOT_OUT with the embed's
 * frame count (wm_detect, wm_detect_keys, wm_detect_offsets, wm_detect_tiles, wm_detect_keys_tiles, wm_detect_bits, wm_gram, under
 * either mask) takes them, a second one after the first as well, until a library write ends the hand-over.  An in-place embed
 * (out overlaps in_gray) hands over like any other, the stencil reads the snapshot; an embed whose out overlaps a base that is not
 * its input leaves no hand-over, and neither does a one-frame embed.
 *
 * HAZARD.  The hand-over is only as good as the caller's promise that the output plane is UNMODIFIED between the embed and the
 * detector that names it as WM_MEM_SLOT_OUT.  The library ends a hand-over whenever it writes that plane itself (the slot's
 * next embed, an embed on another slot into the same buffer, wm_band_embed, wm_compute_mask outputs, wm_band_configure), but
 * it cannot see a write by the caller -- a kernel on another stream, a copy, the host through mapped memory.  After such a
 * write the detector would use the Gram matrix of the OLD plane with the pixels of the NEW one: a wrong correlation, no
 * error.  Environment WM_HANDOVER_VERIFY=1 (read when the context is created; a debug mode, it synchronises every call)
 * makes every handed-over wm_detect / wm_gram also run the ordinary Gram sweep over the plane as it is and compare the 44
 * totals to 1e-12 relative: a mismatch fails the call with WM_ERR_RUNTIME and a message naming frame and term. */
int wm_set_handover(wm_ctx* ctx, int on);
/* returns 1 if synchronous one-frame calls of this context take the fused kernels; workgroups / tile_rows describe the
 * tiling, fallbacks counts fused launches that timed out in a hand-off and were re-run on the sweeps (any may be NULL) */
int wm_fused_info(const wm_ctx* ctx, int* workgroups, int* tile_rows, unsigned long long* fallbacks);
/* Fused launches need the device to themselves; processes that share a device serialise them with an advisory lock on a
 * per-device file (named after the PCI address, in $WM_FUSED_LOCK_DIR, else /run/lock, else $TMPDIR or /tmp; opened
 * read-only and never through a symbolic link).  The lock is tried for 5 ms; a call that does not get it (a holder that is
 * stopped in a debugger must not hang everybody else) runs on the sweeps.  Returns how often that happened. */
unsigned long long wm_fused_lock_skips(const wm_ctx* ctx);
/* development aid: with WM_FUSED_STAMPS set in the environment when the context is created, every workgroup of a fused
 * launch records up to 16 time stamps (100 MHz clock) at its phase boundaries; copies up to `cap` of the last call's
 * [workgroups + 1][16] values of slot 0 to `out`, returns the count (0 when stamps are off) */
int wm_fused_stamps(wm_ctx* ctx, unsigned long long* out, int cap);
/* Self-test of the NVF quotient (nvf.hpp:50, `variance / (1 + variance)`): the kernels form it as reciprocal, product and one
 * residual correction (4 operations) instead of the IEEE division sequence.  The divisor is a function of the dividend, so
 * the inputs are a one-parameter family, and this entry checks it exhaustively: `variant` 2 (what the kernels use; 0 and 1 =
 * the 8- and 6-operation sequences with a refined reciprocal, 3 = product alone, which is NOT exact and shows the test can
 * fail) against the compiler's correctly rounded division for every f32 whose bit pattern lies in [bits_lo, bits_hi),
 * counting the values whose results differ in any bit.  The mask can only produce variances in [-0.5, 2^17): bits
 * [0, 0x48000000) and (0x80000000, 0xBF000000) -- 2.2e9 values, well under a second on the device.
 * Returns WM_OK; *mismatches = differing values, *first_bad = the smallest differing bit pattern (if any). */
int wm_selftest_nvf_quotient(int device, int variant, uint32_t bits_lo, uint32_t bits_hi, unsigned long long* mismatches, uint32_t* first_bad);
/* with WM_FUSED_STAMPS set: the 44 Gram sums (wm_gram's order) the last fused ME call of slot 0 folded; returns 44 or 0 */
int wm_fused_gram(wm_ctx* ctx, double* out44);
/* rows each wavefront marches per segment (tuning knob; 0 = automatic) */
int wm_set_rows_per_segment(wm_ctx* ctx, int rows_per_segment);

/* Watermark::makeWatermark(inputImage, outputImage, watermarkStrength, maskType)  (Watermark.cpp:156-172).
 * in_gray: the mask source ([rows,cols], 1 channel); base: what the watermark is added to (1 or 3
 * channels, same rows/cols/dtype family); out: same shape as base, may alias base.  If out also overlaps
 * in_gray (in-place video frames, main.cpp:356,380) the library snapshots in_gray first (one extra copy).
 * a_out[frames], status_out[frames] (either may be NULL) are written by wm_sync.
 * Zero-energy frames: when u = m W vanishes (an integer-flat frame under NVF, a zero W), ||u|| = 0 and the strength is
 * a = sF / 0 = +inf, reported as such with status WM_OK; the watermark term is then taken as 0, so out == base bit for bit
 * (the reference's result is undefined there: af::clamp of NaN, Watermark.cpp:170-171).  wm_detect with a zero W scores
 * 0 / 0 = NaN with status WM_OK. */
int wm_embed(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, float* a_out,
             int* status_out, int slot);
/* Watermark::detectWatermark(watermarkedImage, maskType)  (Watermark.cpp:234-250).
 * The caller promises nothing about `img`.  When it is the device plane the same slot's last wm_embed wrote (same pointer,
 * pitch, frame stride, frames and dtype), that embed handed its Gram sums over (ME mask, grey f32 planes on the aligned path,
 * p = 3, two frames or more, no band) and no detector has used them yet, the call takes the CHECKED hand-over: the Gram
 * matrix comes from the embed's sums (k_gram_ho, no Gram sweep over img), and the detector's own sweep sums a 64-bit digest
 * of the pixels it reads that any change of a single pixel alters.  A frame whose digest equals the one the embed left
 * keeps its score; any other frame is redone on the device from the plane as it is (k_gram_redo + k_detect_redo, launched
 * after every checked detect, empty when nothing changed) -- the result is then the ordinary path's.  Scores agree with the
 * ordinary path to the rounding of the Gram sums' grouping (<= 1.2e-7).  wm_set_checked_handover switches this off.
 * The checked hand-over is taken under the ME mask of the DETECTOR; the embed handed its sums over if it ran under the ME mask or,
 * under either mask, under wm_set_handover.  Naming the plane as WM_MEM_SLOT_OUT counts as naming its pointer -- unless the embed ran
 * under wm_set_handover: then WM_MEM_SLOT_OUT takes the promised hand-over, unchecked, and only the pointer takes the checked one.  A
 * promised hand-over that a detector has taken is used up for the checked one too. */
int wm_detect(wm_ctx* ctx, int mask, const wm_plane* img, float* corr_out, int* status_out, int slot);
/* the checked hand-over of wm_detect: 1 (default; environment WM_CHECKED_HANDOVER=0 changes the default) on, 0 off -- every
 * wm_detect then takes the ordinary Gram sweep and wm_embed leaves sums behind only under wm_set_handover, as before */
int wm_set_checked_handover(wm_ctx* ctx, int on);
/* frames the checked hand-over trusted (digest equal) and redid (digest different) since the context was configured, over
 * all slots; waits for every slot's queued work.  Either pointer may be NULL */
int wm_checked_handover_counts(wm_ctx* ctx, unsigned long long* trusted, unsigned long long* redone);

/* makeWatermark followed by detectWatermark on its result -- the pair the reference's sample protocol runs per image
 * (testForImage, main.cpp:165-220) -- as ONE call: the results of wm_embed(...) then wm_detect(out, ...), delivered
 * together (on the fused kernels bit for bit; on the sweeps the embed hands the lag sums of its output to the detector as
 * under wm_set_handover, so y and the strength are bit-identical and the score agrees to the rounding of the Gram sums'
 * grouping, <= 2e-7).  Grey output only (out->channels == 1); the detector reads the device copy of the plane the embed wrote
 * (WM_MEM_SLOT_OUT), so a host-staged frame crosses the host link once each way.  Synchronous one-image calls on the fused
 * kernels launch both operations back to back and wait once (one launch-to-completion round trip less than two calls;
 * environment WM_FUSED_PAIR=1: both halves in ONE launch, the same bits, measured 1.5-2 us slower at 4K -- DESIGN.md section 8);
 * everything else queues the two operations on the slot.  status_out[frames] (may be NULL): the embed's status.
 * The hand-over inside the pair is the pair's own: without wm_set_handover it ends with the pair's detector, and a later detector of
 * the slot's WM_MEM_SLOT_OUT (or of the plane's pointer) takes the ordinary Gram sweep over the plane as it then is. */
int wm_embed_detect(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, float* a_out,
                    float* corr_out, int* status_out, int slot);

/* ---- Key identification: one image against a bank of watermark keys ------------------------------------------------------
 * A bank holds K watermark planes (the W of wm_create) of one rows x cols shape on one device, stacked as ONE device allocation
 * [K][rows][cols] f32, row-major (each plane in the W file's layout, Watermark.cpp:62-75).  The bank always owns a copy of its
 * planes; every fill call completes before it returns.  Argument errors (nkeys < 1 or > WM_KEYS_MAX, k out of range, rows or
 * cols outside 1..32768, null pointers) return WM_ERR_BAD_ARG before any device is touched; WM_ERR_ALLOC when the bank does
 * not fit.  A new bank's planes are zero. */
#define WM_KEYS_MAX 4096
typedef struct wm_keys wm_keys;
int wm_keys_create(wm_keys** out, int device, int rows, int cols, int nkeys);
void wm_keys_destroy(wm_keys* keys);
int wm_keys_count(const wm_keys* keys);
int wm_keys_rows(const wm_keys* keys);
int wm_keys_cols(const wm_keys* keys);
const float* wm_keys_device_ptr(const wm_keys* keys, int k);  /* device plane of key k (NULL if out of range) */
/* key k := rows*cols floats at `w`, a host (WM_MEM_HOST) or device (WM_MEM_DEVICE) array */
int wm_keys_set(wm_keys* keys, int k, const float* w, int mem);
/* key k := a W file (loadRandomMatrix, Watermark.cpp:62-75): WM_ERR_W_OPEN / WM_ERR_W_SIZE as wm_create_from_file */
int wm_keys_load_file(wm_keys* keys, int k, const char* path);
/* key k := the W of wm_create_generated(..., seed), bit for bit (the same device generator) */
int wm_keys_generate(wm_keys* keys, int k, uint32_t seed);

/* detectWatermark (Watermark.cpp:234-250) of every frame of `img` against EVERY key of the bank: whose key is in this copy?
 * corr_out[frames][nkeys] (row-major), status_out[frames] (may be NULL).  Takes every input wm_detect takes (f32 / u8, any
 * pitch and width, WM_MEM_HOST, WM_MEM_SLOT_OUT, batches up to max_frames, ME with p = 3, NVF with p = 3..9); the context
 * supplies shape, p and device -- its own W is not used -- and a bank of another shape or device is WM_ERR_BAD_ARG.  The image
 * side runs once for all keys (wm_detect's Gram sweep, hand-over included, and solve); one sweep then reads the image once per
 * group of keys and every key plane once (k_detect_keys).  Key k's score is wm_detect's with key k as W on the batched sweeps, bit
 * for bit.  An unsolvable frame has status WM_UNSOLVABLE and 0.0f for every key (Watermark.cpp:246-247).
 * An ENQUEUE on the slot like wm_detect (WM_SLOT_SYNC: slot 0, waits); it may share a slot with embeds and detects in any order.
 * frames * nkeys results count against the slot's capacity of 4096 un-synced results (shared with the other calls' one result per
 * frame); beyond it the call returns WM_ERR_BUSY.  Never takes the fused single-launch kernels.
 *
 * HAZARD.  The kernels read the bank when the stream reaches them: the bank must stay ALIVE and UNMODIFIED (no wm_keys_set /
 * _load_file / _generate / _destroy on it) until wm_sync of this slot has returned.  The library does not check this. */
int wm_detect_keys(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, float* corr_out, int* status_out, int slot);

/* ---- Crop search: one image against a rectangle of window offsets into one key ---------------------------------------------
 * A copy that was CROPPED after it was marked no longer lines up with its key: W is white noise, so one pixel of misalignment
 * takes the score from ~0.54 to ~0.22 (ME) and two pixels to ~0.04.  The detector is local, though: a frame marked at KR x KC and
 * cropped to rows x cols at (oy, ox) scores against the WINDOW key[oy : oy + rows, ox : ox + cols] almost what the full frame
 * scores against the key.  wm_detect_offsets runs that search: detectWatermark (Watermark.cpp:234-250) of every frame of `img`
 * against the windows of key `k` of the bank at the offsets (oy0 + i, ox0 + j), i < ny, j < nx.
 * The context supplies the image shape rows x cols, p and the device -- its own W is not used.  `keys` is a bank on the same
 * device whose planes are KR x KC with KR >= rows and KC >= cols.  Every window must lie inside the key plane: oy0 >= 0,
 * ox0 >= 0, ny >= 1, nx >= 1, oy0 + ny - 1 + rows <= KR, ox0 + nx - 1 + cols <= KC (wm_offsets_check is that test on its own,
 * WM_OK or WM_ERR_BAD_ARG).  WM_ERR_BAD_ARG, before any device work is queued, for a window outside the key plane, a null ctx /
 * img / keys / corr_out, k out of range, a bank on another device or smaller than the image, and in band mode.
 * corr_out[frames][ny][nx] (row-major), status_out[frames] (may be NULL), both written by wm_sync.  Takes every input
 * wm_detect_keys takes (f32 / u8, any pitch and width, WM_MEM_HOST, WM_MEM_SLOT_OUT, batches up to max_frames, ME with p = 3 --
 * WM_ERR_BAD_P otherwise --, NVF with p = 3..9).
 * Score (i, j) is wm_detect's on the batched sweeps with W = the window copied out -- equivalently wm_detect_keys' on a rows x cols
 * bank that holds the window -- BIT FOR BIT: the replicate border of u = m W is taken at the window's edge (key values outside
 * an offset's window never enter its score), and the sweep geometry is chosen from the image plane alone.  The image side runs
 * once (wm_detect's Gram sweep, hand-over included, and solve); one sweep (k_detect_offsets) then scores groups of horizontally
 * adjacent offsets that share one stream of key rows, so no bank of candidate windows is built or read.  An unsolvable frame
 * has status WM_UNSOLVABLE and 0.0f at every offset; a key that is all zero scores NaN, as in wm_detect_keys.
 * The peak is not one pixel wide: the prediction filter smears it over the 3x3 neighbourhood, so the 8 offsets around the true
 * one score 0.1-0.25 where offsets two or more pixels away score < 0.05.
 * An ENQUEUE on the slot like wm_detect_keys (WM_SLOT_SYNC: slot 0, waits); it may share a slot with any other call in any order.
 * frames * ny * nx results count against the slot's capacity of 4096 un-synced results; beyond it the call returns WM_ERR_BUSY.
 * Never takes the fused single-launch kernels.
 *
 * HAZARD.  As for wm_detect_keys: the kernels read the bank when the stream reaches them: the bank must stay ALIVE and UNMODIFIED
 * (no wm_keys_set / _load_file / _generate / _destroy on it) until wm_sync of this slot has returned.  The library does not
 * check this. */
int wm_offsets_check(int rows, int cols, int key_rows, int key_cols, int oy0, int ox0, int ny, int nx);
int wm_detect_offsets_group(void);  /* G: horizontally adjacent offsets that share one stream of key rows (nx < G: one each) */
int wm_detect_offsets(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k, int oy0, int ox0, int ny, int nx,
                      float* corr_out, int* status_out, int slot);

/* ---- Crop search without a hint: every admissible offset at once, by FFT -----------------------------------------------------
 * wm_detect_offsets searches a rectangle of offsets the caller suspects, at most 4096 per call.  wm_locate names the offset among
 * ALL of them.  With the frame's coefficients c solved, the detector's numerator is linear in W:
 *     <e_u, e_w>(oy, ox) = sum_q h(q) key[q + (oy, ox)],     h = m * F^T e_w,
 * e_w the frame's prediction error, m its mask (ME: |e_w|, without the 1 / max|e| -- the scale of wm_detect_tiles' sums_dev[0]; NVF:
 * the mask of window p) and F^T the exact adjoint of the replicate-border prediction-error stencil.  That is ONE 2-D cross-correlation
 * of the image-side plane h with key plane k: three 2-D transforms (the key's once per call) give it for every offset.
 * wm_locate_shape (pure host arithmetic): ny = key_rows - rows + 1, nx = key_cols - cols + 1 admissible offsets per axis; pr, pc: the
 * padded transform, the smallest powers of two >= max(key_rows, 64) and >= max(key_cols, 64).  WM_ERR_BAD_ARG for a null pointer,
 * rows or cols < 1, a key smaller than the image, pr or pc above 8192 (a row of 8192 complex f32 fills the 64 KiB of LDS a
 * workgroup transforms it in).  No wrap-around of the circular correlation reaches an admissible offset: q + o < key_rows <= pr.
 * wm_locate takes wm_detect_offsets' inputs (the context supplies the image shape, p and the device, not its W; f32 / u8, any pitch
 * and width, WM_MEM_HOST, batches up to max_frames, ME with p = 3 -- WM_ERR_BAD_P otherwise --, NVF with p = 3..9) and refuses in
 * its order: null ctx, mask, null img / keys or loc_out and map_dev both NULL, k, the bank (device, at least as large),
 * wm_locate_shape, band mode, slot, plane, record room.  The image side is wm_detect_keys' (Gram sweep and solve); per frame it
 * then forms h, correlates, writes map[i][j] = sum_q h(q) key[q + (i, j)] for the ny x nx offsets into map_dev [frames][ny][nx]
 * (DEVICE f32, may be NULL) and folds the map into loc_out[frame][4] (HOST, may be NULL, delivered by wm_sync):
 *     oy, ox   the argmax (ties: the smallest i * nx + j), as floats (exact below 2^24)
 *     peak     map[oy][ox]: the detector's <e_u, e_w> against the window at (oy, ox), to the f32 transform's rounding
 *     z        (float)((peak - mu) / sigma), mu and sigma the f64 mean and population standard deviation of the map over the
 *              offsets OUTSIDE the 3 x 3 block around the argmax (the prediction filter smears the peak over its neighbours);
 *              NaN when fewer than two offsets lie outside that block or sigma = 0 (a zero key, key == image)
 * status_out[frames] (may be NULL).  An unsolvable frame -- a flat frame is one -- has status WM_UNSOLVABLE, {0, 0, 0, 0} (z = 0, not
 * NaN) and a zero map.  A marked crop
 * reaches z of 20-60, an unmarked one stays below 5; wm_detect_offsets with ny = nx = 1 at (oy, ox) then gives
 * the score.  A payload-marked copy (wm_embed_bits) has tiles of both signs whose contributions cancel in a whole-frame map:
 * wm_locate_bits below finds and reads such a copy.
 * An ENQUEUE on the slot like wm_detect_offsets; frames * 4 records count against the slot's 4096 (WM_ERR_BUSY).  Never takes the
 * fused kernels, leaves no hand-over, ends none, does not change what WM_MEM_SLOT_OUT names; its kernels are not in the wm_prof_*
 * list.  A frame's map and numbers do not depend on the batch or on repetition.  Scratch per slot: three pr x pc complex f32 planes
 * and the frame's e (and m) planes -- 384 MB for a 4K key, 1.5 GB at 8192 x 8192 -- grown on demand (WM_ERR_ALLOC when it does not
 * fit; the first growing call waits for the device) and released by the reconfiguring calls.
 * HAZARD: the bank stays alive and unmodified until wm_sync of this slot, as for wm_detect_keys.
 * wm_fft2: the transform on its own, a synchronous building block for parity tests.  In place over data_dev [pr][pc] interleaved
 * complex f32 on `device`, exp(-2 pi i ..) forward and exp(+2 pi i ..) inverse, neither normalised (inverse(forward(x)) = pr pc x);
 * pr and pc powers of two in 64 .. 8192, anything else WM_ERR_BAD_ARG. */
#define WM_LOCATE_NVALS 4   /* per frame, HOST f32, delivered by wm_sync: {oy, ox, peak, z} */
int wm_locate_shape(int rows, int cols, int key_rows, int key_cols, int* ny, int* nx, int* pr, int* pc);
int wm_locate(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k,
              float* loc_out /* HOST [frames][4], by wm_sync */, float* map_dev /* DEVICE [frames][ny][nx] f32, may be NULL */,
              int* status_out, int slot);
int wm_fft2(int device, float* data_dev /* [pr][pc] interleaved complex f32, in place */, int pr, int pc, int inverse);
/* Yardstick of the transform (tools/locate_bench.py): the seven passes one frame of wm_locate makes over a pr x pc plane -- rows of pc,
 * transpose, rows of pr, the spectrum product, rows of pr (inverse), transpose, rows of pc (inverse) -- each launched `iters` times
 * back to back between two events; us_out[7]: mean microseconds per launch.  A row or transpose pass reads and writes the plane once
 * (pr pc 8 bytes each way: wm_membench kind 4 on that many bytes is the copy to hold it against), the product reads two planes. */
#define WM_FFT_BENCH_PASSES 7
int wm_fft_bench(int device, int pr, int pc, int iters, double* us_out /* [WM_FFT_BENCH_PASSES] */);

/* ---- A payload-marked crop: found without a hint, and read ---------------------------------------------------------------------
 * wm_embed_bits marks tile t with +W or -W by the bit it carries, so in wm_locate's whole-key map the tiles cancel.  Tile signs are a
 * property of KEY coordinates: with key_b = key * [tile_bit[tile(p)] == b], the key masked to the tiles of bit b, the marked crop's
 * numerator at offset o is sum_b s_b map_b(o), map_b(o) = sum_q h(q) key_b[q + o] -- wm_locate's correlation with another key plane.
 * The energy E(o) = sum_b map_b(o)^2 does not see the signs s_b; the sign of map_b at E's argmax is bit b.  h is real, so two bits
 * ride in one complex transform: correlating h with key_b + i key_b' gives map_b + i map_b' (for an odd nbits the last bit rides alone).
 * Geometry: the tiles are wm_tiles_shape(key_rows, key_cols, tile_rows, tile_cols) over the KEY plane, where wm_embed_bits put them on a
 * context of the key's shape; tile_bit [ty * tx] is wm_bits_layout's table or the caller's own, -1: the tile belongs to no bit.  Offsets
 * and the transform are wm_locate_shape's; h is wm_locate's (the same Gram sweep, solve and kernels).
 * wm_locate_bits takes wm_locate's inputs and refuses in its order -- null ctx, mask, a null img / keys / tile_bit / loc_out / soft_out,
 * k, the bank, wm_locate_shape, band mode, slot, plane, record room (frames * (4 + nbits) records against the slot's 4096,
 * WM_ERR_BUSY) --, then a tile shape wm_tiles_shape refuses on the key's shape, nbits outside 1 .. 4096 and a tile_bit entry outside
 * -1 .. nbits - 1; all of it before any device work.  tile_bit is read before the call returns.  Outputs, valid after wm_sync:
 *     loc_out[frame][4]       wm_locate's {oy, ox, peak, z} taken on E: the argmax o* (ties: the smallest index), E there, and z against
 *                             the offsets outside the 3 x 3 block around o* (f64), NaN by wm_locate's rule
 *     soft_out[frame][nbits]  (float)((map_b(o*) - mu_b) / sigma_b), mu_b and sigma_b the f64 mean and population standard deviation
 *                             of map_b over the offsets outside that same block: the bit is soft > 0, |soft| is in standard deviations
 *                             of the bit's own unmarked level.  NaN where sigma_b = 0 (a bit without a tile, a zero key) or fewer
 *                             than two offsets lie outside the block.  A bit without a pixel in the window reads about 0:
 *                             wm_locate_bits_cover names those bits
 *     energy_dev              DEVICE [frames][ny][nx] f32, may be NULL: E, added in f32 in ascending pair order (the first pair stores)
 *     maps_dev                DEVICE [frames][nbits][ny][nx] f32, may be NULL: the maps; peak == energy_dev[oy][ox] bit for bit
 * An unsolvable frame: status WM_UNSOLVABLE, {0, 0, 0, 0}, soft zero, zero maps and a zero E.  A frame's numbers, E and maps do not
 * depend on the batch or on repetition.  A marked crop reaches z of 140-680 on E and an unmarked one stays below 10 (DESIGN.md section
 * 25); a plainly marked copy (all signs +1) is found as well.
 * An ENQUEUE on the slot; never takes the fused kernels, leaves no hand-over, ends none, does not change what WM_MEM_SLOT_OUT names; its
 * kernels are not in the wm_prof_* list.  Scratch per slot, grown on demand (WM_ERR_ALLOC when it does not fit; a call whose shapes
 * differ from the one before waits for the slot's stream) and released by the reconfiguring calls:
 *     bytes = (frames + 3) * pr * pc * 8  +  2 * rows * cols * 4  +  [energy_dev NULL] frames * ny * nx * 4
 *             +  [maps_dev NULL] frames * nbits * ny * nx * 4  +  frames * (ceil(nbits / 2) + 1) * ceil(ny * nx / 4096) * 32  +  tables
 * -- about 700 MB for a 4K key (4096 x 4096 transform), a 1600 x 3000 crop, 64 bits and one frame.
 * HAZARD: the bank stays alive and unmodified until wm_sync of this slot, as for wm_locate.
 * wm_locate_bits_cover (pure host arithmetic): pixels_out[b] = the pixels of the rows x cols window at (oy, ox) whose key tile carries
 * bit b.  WM_ERR_BAD_ARG for what wm_locate_shape or wm_tiles_shape refuse, an offset outside 0 .. ny - 1, 0 .. nx - 1, a null
 * pointer, nbits outside 1 .. 4096 or a tile_bit entry outside -1 .. nbits - 1. */
#define WM_LOCATE_BITS_NVALS 4   /* {oy, ox, peak, z} of the energy map, then nbits soft values */
int wm_locate_bits(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k,
                   int tile_rows, int tile_cols, const int32_t* tile_bit /* HOST [ty*tx] over the KEY plane, -1 .. nbits-1 */, int nbits,
                   float* loc_out  /* HOST [frames][4], by wm_sync */,
                   float* soft_out /* HOST [frames][nbits], by wm_sync */,
                   float* energy_dev /* DEVICE [frames][ny][nx] f32, may be NULL */,
                   float* maps_dev   /* DEVICE [frames][nbits][ny][nx] f32, may be NULL */,
                   int* status_out, int slot);
int wm_locate_bits_cover(int rows, int cols, int key_rows, int key_cols, int tile_rows, int tile_cols,
                         const int32_t* tile_bit, int nbits, int oy, int ox, int64_t* pixels_out /* [nbits] */);
/* Yardstick (tools/locate_bits_bench.py), beside wm_fft_bench and timed the same way: the three passes wm_locate_bits adds to the
 * seven of a transform -- the key-pair plane (128 x 128 tiles over a pr x pc key: one plane written), the three-operand product (two
 * planes read, one written), the accumulate pass of a later pair over ny x nx offsets (8 bytes read, 4 read and 12 written per
 * offset).  pr, pc: powers of two in 128 .. 8192, ny <= pr, nx <= pc; anything else WM_ERR_BAD_ARG. */
#define WM_LOCATE_BITS_BENCH_PASSES 3
int wm_locate_bits_bench(int device, int pr, int pc, int ny, int nx, int iters, double* us_out /* [WM_LOCATE_BITS_BENCH_PASSES] */);

/* ---- A crop against a bank of keys: whose key, and where -------------------------------------------------------------------------
 * wm_embed_keys hands every recipient a copy marked with their own key; such a copy comes back cropped.  wm_locate_keys is wm_locate of
 * every frame against keys k0 .. k0 + nk - 1 of the bank in one call.  Nothing on the image side depends on the key: the Gram sweep,
 * the solve, h and its spectrum are formed once per frame.  h and the keys are real, so two keys ride in one complex transform:
 * correlating h with key_a + i key_b gives map_a + i map_b.  Keys k0 + 2i and k0 + 2i + 1 form pair i; for an odd nk the last key rides
 * alone with a zero imaginary half.  Per frame that is one forward transform, and per pair of keys and frame one forward (shared by
 * the frames) and one inverse transform.
 * Inputs and geometry are wm_locate's: the context supplies the image shape, p and the device, not its W; planes of f32 or u8, any
 * pitch and width, WM_MEM_HOST included, in batches up to max_frames; ME needs p = 3 (WM_ERR_BAD_P), NVF takes p = 3 .. 9;
 * wm_locate_shape gives ny, nx, pr and pc.  It refuses in wm_locate's order -- null ctx, mask, a null img or keys or loc_out and
 * maps_dev both NULL, the key range (k0 < 0, nk < 1, k0 + nk > nkeys), the bank, wm_locate_shape, band mode, slot, plane, record room
 * (frames * nk * 4 records against the slot's 4096, WM_ERR_BUSY) --, all of it before any device work.  Outputs, valid after wm_sync:
 *     loc_out[frame][j][4]    wm_locate's {oy, ox, peak, z} of key k0 + j, by its rule: the argmax (ties: the smallest index), the map
 *                             value there, z in f64 against the offsets outside the 3 x 3 block around it, NaN by wm_locate's
 *                             conditions.  The nine values are formed again as the map pass formed them: they are the map's bits
 *     maps_dev                DEVICE [frames][nk][ny][nx] f32, may be NULL: the maps; maps_dev[f][j][oy][ox] == peak bit for bit
 *     status_out[frames]      may be NULL
 * An unsolvable frame: status WM_UNSOLVABLE, {0, 0, 0, 0} for every key and zero maps.  A key plane that is all zero (a new bank's
 * planes are) gives an exact zero map and {0, 0, 0, NaN}, as wm_locate gives for it: the device notes per key whether its plane holds
 * a value other than 0, and a half of a pair without one is written as zero, not as the f32 residue of its partner.
 * A (frame, key)'s map and numbers do not depend on the batch or on repetition.  They DO depend, in the last bits, on the key's
 * partner in the pair and hence on k0 and nk, and they agree with wm_locate's for that key to the transform's rounding (1e-4 sigma_W
 * is the tested bound of either against the f64 model), not bit for bit.  wm_locate_keys_rank names the owner; the owner's key
 * reaches z of 20-80 at the true offset and every other key stays below 6.
 * An ENQUEUE on the slot (WM_SLOT_SYNC: slot 0, and waits); never takes the fused kernels, leaves no hand-over, ends none, does not
 * change what WM_MEM_SLOT_OUT names; its kernels are not in the wm_prof_* list.  Scratch per slot, an allocation of its own beside
 * wm_locate's and wm_locate_bits', grown on demand (WM_ERR_ALLOC when it does not fit; a call whose shapes or frame count differ from
 * the one before waits for the slot's stream) and released by the reconfiguring calls:
 *     bytes = (frames + 3) * pr * pc * 8  +  2 * rows * cols * 4  +  2 * ceil(ny * nx / 4096) * 32  +  1025 * 4  +  tables
 * -- about 575 MB for a 4K key (4096 x 4096 transform), a 1600 x 3000 crop and one frame, whatever nk.  There is no map storage when
 * maps_dev is NULL: the records of a pair are folded from the inverse plane before the next pair overwrites it.
 * HAZARD: the bank stays alive and unmodified until wm_sync of this slot, as for wm_locate.
 * wm_locate_keys_rank (pure host arithmetic) reads one frame's [nk][4] records: best = the index of the largest z (NaN is ignored,
 * ties: the smallest index), z_best that z, z_next the largest z among the other keys (NaN when there is none); best = -1 and both
 * NaN when every z is NaN.  WM_ERR_BAD_ARG for a null pointer or nk < 1. */
#define WM_LOCATE_KEYS_NVALS 4   /* per (frame, key), HOST f32, by wm_sync: {oy, ox, peak, z} */
int wm_locate_keys(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int k0, int nk,
                   float* loc_out  /* HOST [frames][nk][4], by wm_sync */,
                   float* maps_dev /* DEVICE [frames][nk][ny][nx] f32, may be NULL */,
                   int* status_out /* [frames], may be NULL */, int slot);
int wm_locate_keys_rank(const float* loc /* [nk][4] of one frame */, int nk, int* best, float* z_best, float* z_next);
/* Yardstick (tools/locate_keys_bench.py), beside wm_fft_bench and wm_locate_bits_bench and timed the same way: the two passes
 * wm_locate_keys adds to them -- the key-pair plane (two pr x pc keys read, one plane written) and the map pass of a pair over
 * ny x nx offsets (8 bytes read and 8 written per offset).  pr, pc: powers of two in 128 .. 8192, ny <= pr, nx <= pc; anything else
 * WM_ERR_BAD_ARG. */
#define WM_LOCATE_KEYS_BENCH_PASSES 2
int wm_locate_keys_bench(int device, int pr, int pc, int ny, int nx, int iters, double* us_out /* [WM_LOCATE_KEYS_BENCH_PASSES] */);

/* ---- A clip's frames pooled into one crop search ----------------------------------------------------------------------------------
 * What is traced in practice is a clip: many frames, one crop rectangle, one key, one payload.  The map is linear in the image-side
 * plane, map(o) = sum_q h(q) key[q + o], so the pooled map of a clip is the map of the pooled h:
 *     sum_f w_f map_f = correlate(sum_f w_f h_f, key),
 * and the same holds per payload bit and per key of a bank.  A clip of F frames costs F image-sized passes and ONE transform tail.  On
 * small crops and weak marks, where no single frame reaches a decision, the pooled clip does.
 * The pooled plane belongs to the CALLER: a dense DEVICE f32 [rows][cols] plane of the context's shape and on its device.  The slot
 * keeps no state of a clip, so a clip longer than max_frames is pooled in several calls.
 * wm_clip_pool takes wm_locate's image side (f32 / u8, any pitch and width, WM_MEM_HOST, batches up to max_frames, ME with p = 3 --
 * WM_ERR_BAD_P otherwise --, NVF with p = 3..9) and refuses in its order, all before any device work: null ctx, mask, null img or
 * pool_dev, band mode, slot, plane, record room (frames records, WM_ERR_BUSY), then a weight that is not finite (WM_ERR_BAD_ARG).
 * It runs the Gram sweep and the solve as wm_locate does and then ONE kernel over the batch:
 *     pool(q) = fmaf(w_f, h_f(q), pool(q))   for f ascending,
 * from 0.0f when accumulate == 0 and from the plane's content otherwise; h_f is wm_locate's h of that frame bit for bit.  weights:
 * HOST [frames], read before the call returns, NULL: all 1.  A frame whose status is not 0 (WM_UNSOLVABLE) is skipped: it makes no
 * fmaf and changes nothing; status_out[frames] (may be NULL) is delivered by wm_sync.  The pool's bits depend only on the frames,
 * their order and the weights: not on how the clip was cut into calls, on the batch size, on pitch or memory kind, or on repetition.
 * pool_dev must not overlap the image or any plane a queued call still uses.
 * An ENQUEUE on the slot with wm_locate's side-effect rules: never takes the fused kernels, leaves no hand-over, ends none, does not
 * change what WM_MEM_SLOT_OUT names; its kernel is not in the wm_prof_* list.  No scratch beyond the frames' weights in the slot's
 * table arena.
 * wm_locate_pooled, wm_locate_bits_pooled and wm_locate_keys_pooled are the tails of wm_locate, wm_locate_bits and wm_locate_keys with
 * ONE frame and pool_dev in the place of h: the same launches on the same scratch.  The context supplies the shape, the device and
 * the slots; neither its p nor a mask matters to them.  Refusal order (without mask and plane), record room (4, 4 + nbits, 4 * nk
 * records), records, scratch rules (a pooled call is a call of one frame), the zero-key rule and the bank HAZARD are those of the
 * call each is the tail of; there is no status_out: a pool has no solve.  A pool that is all zero (no solvable frame) gives a zero
 * map and {0, 0, 0, NaN}.  For a clip of ONE frame with weights NULL and accumulate == 0 the pooled calls' maps and numbers equal the
 * per-frame calls' as floats (a -0 of h becomes +0).  A pooled clip of 8 frames at PSNR 52 on a 64 x 256 crop reaches z of 20-23
 * where its frames reach 5-10, and an unmarked clip stays below 5. */
int wm_clip_pool(wm_ctx* ctx, int mask, const wm_plane* img,
                 const float* weights /* HOST [frames], NULL: all 1; read before return */,
                 float* pool_dev /* DEVICE [rows][cols] f32 */, int accumulate,
                 int* status_out /* [frames], may be NULL */, int slot);
int wm_locate_pooled(wm_ctx* ctx, const float* pool_dev, const wm_keys* keys, int k,
                     float* loc_out /* HOST [4], by wm_sync */, float* map_dev /* DEVICE [ny][nx] f32, may be NULL */, int slot);
int wm_locate_bits_pooled(wm_ctx* ctx, const float* pool_dev, const wm_keys* keys, int k,
                          int tile_rows, int tile_cols, const int32_t* tile_bit /* HOST [ty*tx] over the KEY plane */, int nbits,
                          float* loc_out /* HOST [4], by wm_sync */, float* soft_out /* HOST [nbits], by wm_sync */,
                          float* energy_dev /* DEVICE [ny][nx] f32, may be NULL */,
                          float* maps_dev /* DEVICE [nbits][ny][nx] f32, may be NULL */, int slot);
int wm_locate_keys_pooled(wm_ctx* ctx, const float* pool_dev, const wm_keys* keys, int k0, int nk,
                          float* loc_out /* HOST [nk][4], by wm_sync */, float* maps_dev /* DEVICE [nk][ny][nx] f32, may be NULL */,
                          int slot);
/* Yardstick (tools/locate_clip_bench.py), timed as wm_fft_bench is: the pool kernel of wm_clip_pool over `frames` dense f32 frames of
 * rows x cols made up on the spot (mask and p as for wm_clip_pool), by its two routes -- us_out[0]: x and e tiles in LDS, the route
 * wm_clip_pool takes; us_out[1]: a direct gather of the 5 x 5 window from cache, one pixel per lane, taken by no call.  equal_out: 1
 * when the two pools have equal bits.  frames 1 .. 1024; anything else WM_ERR_BAD_ARG. */
#define WM_CLIP_POOL_BENCH_ROUTES 2
int wm_clip_pool_bench(int device, int rows, int cols, int frames, int mask, int p, int iters,
                       double* us_out /* [WM_CLIP_POOL_BENCH_ROUTES] */, int* equal_out);

/* ---- Tile map: where in the frame is the mark? -------------------------------------------------------------------------------
 * wm_detect answers with one correlation for the whole plane.  A copy with a logo pasted over it, a picture-in-picture or a
 * spliced region only lets that score sag.  The detector is local, though: after the one solve per frame, e_w, u = m W and e_u
 * are 3x3 stencils, so the three sums of computeCorrelation can be kept PER TILE of the frame.
 * wm_detect_tiles is detectWatermark (Watermark.cpp:234-250) of every frame of `img` against the context's own W -- one
 * Gram sweep (the hand-over of the slot's last embed included, exactly as wm_detect_keys takes it) and one solve per frame, so
 * ONE coefficient vector and ONE mask per frame -- with the sums <e_u,e_w>, ||e_u||^2, ||e_w||^2 kept per tile.
 *
 * wm_tiles_shape: tiles per axis: ny = max(1, rows / tile_rows), nx = max(1, cols / tile_cols) (integer division); pixel (r, c)
 * belongs to tile (min(r / tile_rows, ny - 1), min(c / tile_cols, nx - 1)): the LAST tile of each axis takes the remainder, so no
 * tile is smaller than tile_rows x tile_cols and there are no sliver tiles.  WM_OK, or WM_ERR_BAD_ARG unless tile_rows is a
 * multiple of 8 and >= 32, tile_cols a multiple of 4 and >= 32, rows, cols in 1..32768 and ny, nx non-null.  Pure host arithmetic.
 * (Tiles below 32 x 32 hold too few pixels for the 1e-5 agreement with the CPU oracle that every detector here keeps.)
 *
 * map_dev [frames][ny][nx] is a DEVICE f32 array on the context's device: (float)dot / (float)(sqrt(nw) * sqrt(nu)) of the tile's
 * sums.  sums_dev [frames][ny][nx][3] is a DEVICE f64 array and may be NULL: {<e_u,e_w>, ||e_u||^2, ||e_w||^2}, the quantities
 * wm_band_detect_sums reports; under ME they are taken with m = |e_w| (the 1 / max|e| cancels in every score and is not applied).
 * Tile sums ADD: the score of any union of tiles is formed on the host from the sums of its tiles, and the sums added over all
 * tiles give wm_detect's score of the frame on the sweeps to <= 2e-7 (a regrouping of the same products).
 * Behind a Gram hand-over (a WM_MEM_SLOT_OUT plane under a promise) the f32 coefficients may differ from the Gram sweep's by one ulp:
 * a tile's score then agrees with the ordinary path's to <= 2e-7 and each of its sums to <= 1e-5 relative (wm_detect_keys_tiles
 * likewise); statuses and everything else are the ordinary path's bits.
 * Both arrays are written on the slot's stream and are valid once wm_sync(ctx, slot) has returned; they must stay allocated
 * until then.  The map does not pass through the slot's result records (a 4K frame in 32 x 32 tiles is 8040 scores).
 * status_out[frames] may be NULL; it is delivered by wm_sync like wm_detect's, and `frames` results count against the slot's
 * capacity of 4096 un-synced results (WM_ERR_BUSY beyond it).
 *   - An unsolvable frame has status WM_UNSOLVABLE, 0.0f in every tile and zero sums.
 *   - A tile whose ||e_u||^2 or ||e_w||^2 is zero (a flat patch, a zero W) scores 0/0 = NaN with status WM_OK: wm_detect's
 *     zero-W rule, per tile.
 *   - Takes every input wm_detect takes on the sweeps: f32 / u8, any pitch and width, WM_MEM_HOST, WM_MEM_SLOT_OUT, batches up to
 *     max_frames, ME with p = 3 (WM_ERR_BAD_P otherwise), NVF with p = 3..9.
 *   - An ENQUEUE on the slot (WM_SLOT_SYNC: slot 0, waits); it may share a slot with any other call in any order.  The sweep's
 *     record scratch is kept per slot and grown on demand (its size follows from the tile shape): the FIRST call on a slot that
 *     needs more of it than any call before -- more frames, or a tile_rows with shorter segments -- reallocates it, which waits
 *     for the whole device, the other slots' streams included.  Later calls only enqueue.
 *   - Never takes the fused single-launch kernels.  Refused in band mode (WM_ERR_BAD_ARG).
 *   - WM_ERR_BAD_ARG, before any device work, for a null ctx, img or map_dev and for a tile shape wm_tiles_shape refuses.
 * Bits: a frame's map and sums do not depend on the batch it arrives in or on repetition (the sweep's segments follow from
 * tile_rows alone; the fold adds in a fixed order, no atomics).  A WM_MEM_HOST plane gives the bits of the same plane on the
 * device whenever both take the same strips: always for f32 planes and for widths that are multiples of 4. */
int wm_tiles_shape(int rows, int cols, int tile_rows, int tile_cols, int* ny, int* nx);
int wm_detect_tiles(wm_ctx* ctx, int mask, const wm_plane* img, int tile_rows, int tile_cols, float* map_dev, double* sums_dev,
                    int* status_out, int slot);

/* ---- Tile map per key: whose mark is where? ----------------------------------------------------------------------------------
 * Collusion by mosaic: several recipients of per-key copies (wm_embed_keys) splice their copies together region by region.  The
 * copies share one base image, so the seams are invisible; every colluder's whole-frame score falls by the number of colluders
 * and wm_detect_keys shows a few weak keys it cannot tell from noise.  The per-tile, per-key map separates them: the argmax over
 * keys names the source of every tile.
 * wm_detect_keys_tiles is wm_detect_tiles with EVERY key of the bank in the place of the context's W: one Gram sweep (the
 * hand-over of the slot's last embed included, exactly as wm_detect_keys takes it) and one solve per frame, then ONE sweep that
 * reads the image once per group of keys and every key plane once (k_detect_keys_tiles), the three sums kept per
 * (frame, key, tile).  The context supplies shape, p and device -- its own W is not used.
 *
 * map_dev [frames][nkeys][ny][nx] is a DEVICE f32 array on the context's device, sums_dev [frames][nkeys][ny][nx][3] a DEVICE f64
 * array {<e_u,e_w>, ||e_u||^2, ||e_w||^2} that may be NULL; tile geometry (wm_tiles_shape) and the score expression are
 * wm_detect_tiles', unchanged.  Key k's map and sums equal, BIT FOR BIT, what wm_detect_tiles gives on a context created with key
 * k as W.  The sums ADD, in f64, per frame, key and tile: the caller may pool the tiles of a region or the frames of a clip on the
 * host and score the total with the same expression; ||e_w||^2 does not depend on the key.
 * Both arrays are written on the slot's stream and are valid once wm_sync(ctx, slot) has returned; they must stay allocated
 * until then.  status_out[frames] may be NULL; it is delivered by wm_sync, and `frames` results count against the slot's capacity
 * of 4096 un-synced results (WM_ERR_BUSY beyond it).
 *   - Takes everything wm_detect_keys and wm_detect_tiles both take: f32 / u8, any pitch and width, WM_MEM_HOST, WM_MEM_SLOT_OUT,
 *     batches up to max_frames, ME with p = 3 (WM_ERR_BAD_P otherwise), NVF with p = 3..9.
 *   - An unsolvable frame has status WM_UNSOLVABLE, 0.0f in every tile of every key and zero sums.
 *   - A zero key (a bank's planes start at zero) scores NaN in every tile with status WM_OK; a flat tile under NVF is NaN for
 *     every key.  Other keys and other tiles are unaffected by either.
 *   - An ENQUEUE on the slot (WM_SLOT_SYNC: slot 0, waits); it may share a slot with any other call in any order.  Never takes the
 *     fused single-launch kernels.  Its two kernels are not in the wm_prof_* list.
 *   - The sweep's record scratch is kept per slot and grown on demand:
 *     frames * ceil(nkeys / G) * nsegs * nstrips * (2 G + 1) * 64 * 4 bytes, G = 2 keys per group, nsegs segments of the largest
 *     divisor of tile_rows in 8..48 rows, nstrips strips of 248 columns -- about 11 MB for one 4K frame, 16 keys and tile_rows
 *     128.  WM_ERR_ALLOC when it does not fit.  As for wm_detect_tiles, the FIRST call on a slot that needs more of it than any
 *     call before -- more frames, more keys, or a tile_rows with shorter segments -- reallocates it, which waits for the whole
 *     device, the other slots' streams included.  Later calls only enqueue.
 *   - WM_ERR_BAD_ARG, before any device work, for a null ctx, img, keys or map_dev, a tile shape wm_tiles_shape refuses, a bank of
 *     another shape or device, a bad slot, band mode, and frames * nkeys * ny * nx (or the sweep's blocks) beyond a launch grid of
 *     31 bits.  Index arithmetic is 64-bit throughout.
 * Bits: a (frame, key)'s map and sums do not depend on the batch the frame arrives in, on the key's position in the bank or on
 * the other keys, or on repetition (segments follow from tile_rows alone; the fold adds in a fixed order, no atomics).  A
 * WM_MEM_HOST plane gives the bits of the same plane on the device for f32 planes and for widths that are multiples of 4.
 *
 * HAZARD.  As for wm_detect_keys: the kernels read the bank when the stream reaches them: the bank must stay ALIVE and UNMODIFIED
 * (no wm_keys_set / _load_file / _generate / _destroy on it) until wm_sync of this slot has returned.  The library does not
 * check this. */
int wm_detect_keys_tiles(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, int tile_rows, int tile_cols,
                         float* map_dev, double* sums_dev, int* status_out, int slot);

/* ---- A payload in the mark: one bit per tile -------------------------------------------------------------------------------------
 * A frame is marked with a key or it is not: the mark carries no bits, and naming a recipient costs one key plane each.  But the
 * detector is local and its score is SIGNED, wm_detect_tiles keeps <e_u,e_w>, ||e_u||^2 and ||e_w||^2 per tile and those sums add,
 * and the strength a = sF / (||m W|| / sqrt(N)) does not change when W changes sign anywhere.  A frame whose tile (ty, tx) is marked
 * with s W, s = +-1, therefore carries one bit per tile, read back from the sign of the tile's <e_u,e_w>; several tiles that carry
 * the same bit pool their sums.  One ID of up to a few hundred bits costs one key and one wm_detect_tiles-sized call.
 * Tile geometry is wm_tiles_shape's throughout, unchanged: tile_rows a multiple of 8 and >= 32, tile_cols a multiple of 4 and
 * >= 32, the last tile of each axis takes the remainder; tables are row-major over (ty, tx), T = ny * nx entries.
 * How many tiles per bit?  At psnr 40, p = 3, u8 output, the weakest bit of a marked frame scores |soft| 0.42 (ME) and 0.16 (NVF)
 * with ONE 32 x 32 tile per bit, where an unmarked frame reaches 0.13 / 0.12: NVF with one 32 x 32 tile per bit is close to the
 * unmarked level -- use two tiles per bit or more there (0.25 against 0.09 at 270 x 480 with 48 bits).
 *
 * wm_bits_layout: which bit does tile t carry?  perm = 0 .. T - 1; for i = T - 1 down to 1: j = next() mod (i + 1), swap perm[i] and
 * perm[j]; tile_bit[t] = perm[t] mod nbits, where next() is splitmix64 started at state = seed (state += 0x9E3779B97F4A7C15;
 * z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31; modulo 2^64).
 * Every bit gets floor(T / nbits) or ceil(T / nbits) tiles, spread over the frame.  WM_OK, or WM_ERR_BAD_ARG unless
 * 1 <= nbits <= min(T, 4096), ny, nx >= 1 and tile_bit is non-null.  Pure host arithmetic; it touches no device.
 *
 * wm_embed_signs: makeWatermark (Watermark.cpp:156-172) with the watermark term of every pixel multiplied by the sign of its tile:
 *     y = clamp(base + a * s(ty, tx) * m * W, 0, 255)
 * signs is a HOST array [frames][ny][nx] of -1, 0 or +1.  The Gram sweep, the solve and the stats sweep are wm_embed's own (||u||
 * does not see the signs); only the last sweep is new (k_embed_signs).  Bit for bit against wm_embed on the batched sweeps
 * (wm_set_fused(0)): `a` is wm_embed's with the context's W; a pixel in a +1 tile is wm_embed's pixel; a pixel in a -1 tile is
 * wm_embed's pixel on a context whose W is -W; a pixel in a 0 tile is clamp(base, 0, 255) -- for planes in the documented range base
 * itself, which wm_embed with a zero W returns.  An unsolvable frame and a zero-energy frame follow wm_embed's rules unchanged.
 *   - Takes every input wm_embed takes on the sweeps: f32 / u8, a grey or planar-RGB base (all channels take the tile's sign), a
 *     base that is in_gray, in place (with the snapshot), any pitch and width, WM_MEM_HOST in and out, WM_MEM_SLOT_OUT for in_gray,
 *     batches up to max_frames, ME with p = 3 (WM_ERR_BAD_P otherwise), NVF with p = 3..9.
 *   - Never takes the fused single-launch kernels.  Refused in band mode (WM_ERR_BAD_ARG).
 *   - An ENQUEUE on the slot like wm_embed (WM_SLOT_SYNC: slot 0, waits); `frames` results count against the slot's capacity of
 *     4096 un-synced results.  Its output becomes what WM_MEM_SLOT_OUT names, as wm_embed's does.  Unlike wm_embed it leaves NO Gram
 *     hand-over behind, checked or promised, and like every library write it ends a hand-over whose plane it overwrites.
 *   - `signs` is read before the call returns: the caller may change or free it at once, and several un-synced calls on one slot
 *     each keep their own table.  The copies live in a pinned host arena and a device arena per slot, reset by wm_sync and grown
 *     on demand: the FIRST call on a slot that needs more of them than are left -- larger tables, or more un-synced calls than
 *     before -- waits for the slot's stream and reallocates them, which waits for the whole device, the other slots' streams
 *     included.  Later calls only enqueue.  k_embed_signs is not in the wm_prof_* list.
 *   - WM_ERR_BAD_ARG, before any device work, for a null ctx, plane or signs, a tile shape wm_tiles_shape refuses and a sign
 *     outside {-1, 0, +1}.
 *
 * wm_embed_bits: a host layer over wm_embed_signs.  tile_bit is a HOST array [ny * nx] (wm_bits_layout's, or the caller's own): a
 * tile with tile_bit[t] = b >= 0 gets +1 where payload bit b is 1 and -1 where it is 0, a tile with tile_bit[t] = -1 gets 0 (left
 * unmarked).  payload is a HOST array [frames][(nbits + 7) / 8], bit b = payload[b / 8] >> (b % 8) & 1.  WM_ERR_BAD_ARG unless
 * 1 <= nbits <= 4096 and every entry lies in -1 .. nbits - 1; everything else is wm_embed_signs'.
 *
 * wm_detect_bits: wm_detect_tiles' call with one more fold.  Inputs, the Gram sweep with the hand-over, the solve, k_detect_tiles
 * and k_tiles_fold (into slot-owned scratch) are wm_detect_tiles'; then for bit b the three f64 sums of the tiles with
 * tile_bit == b are added IN ASCENDING TILE INDEX, one after the other (k_bits_fold), and
 *     soft[f][b] = (float)dot / (float)(sqrt(nw) * sqrt(nu)),
 * the expression every detector here uses.  The decoded bit is soft > 0.  soft_out is a HOST array [frames][nbits] written by
 * wm_sync, status_out[frames] may be NULL.
 *   - A bit with no tile scores NaN (the zero-W rule).  An unsolvable frame gives 0.0f for every bit and status WM_UNSOLVABLE.
 *   - Delivery is through the slot's result records, as for wm_detect_keys: frames * nbits results count against the capacity of
 *     4096 un-synced results; beyond it the call returns WM_ERR_BUSY.
 *   - Bits: soft[f][b] equals, bit for bit, that expression over wm_detect_tiles' sums_dev of the same plane added sequentially
 *     in that order; it does not depend on the batch or on repetition.
 *   - tile_bit is read before the call returns (kept like wm_embed_signs' table, with the same caveat for the first call that
 *     grows the arenas; the tile sums' scratch is grown on demand like wm_detect_tiles' record scratch).  Never takes the fused
 *     kernels; refused in band mode; k_bits_fold is not in the wm_prof_* list.
 *   - WM_ERR_BAD_ARG, before any device work, for a null ctx, img, tile_bit or soft_out, a tile shape wm_tiles_shape refuses,
 *     nbits outside 1 .. 4096 and a tile_bit entry outside -1 .. nbits - 1. */
int wm_bits_layout(int ny, int nx, int nbits, uint64_t seed, int32_t* tile_bit /* [ny*nx] */);
int wm_embed_signs(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows, int tile_cols,
                   const int8_t* signs /* HOST [frames][ny][nx], -1 | 0 | +1 */, float* a_out, int* status_out, int slot);
int wm_embed_bits(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows, int tile_cols,
                  const int32_t* tile_bit /* HOST [ny*nx], -1 .. nbits-1 */, int nbits,
                  const uint8_t* payload /* HOST [frames][(nbits+7)/8], bit b = payload[b/8] >> (b%8) & 1 */, float* a_out,
                  int* status_out, int slot);
int wm_detect_bits(wm_ctx* ctx, int mask, const wm_plane* img, int tile_rows, int tile_cols, const int32_t* tile_bit, int nbits,
                   float* soft_out /* HOST [frames][nbits], by wm_sync */, int* status_out, int slot);

/* ---- One frame, many payload copies: K recipients, one key, one call ---------------------------------------------------------------
 * A distributor marks one frame for K recipients, each copy with its own ID and all of them with the context's W.  Nothing on the
 * image side depends on the payload: the Gram sums, the coefficients, the mask and max|e| are the frame's, and so is the strength,
 * since ||m W|| does not see the signs.  wm_embed_signs_multi runs ONE Gram sweep, ONE solve and ONE stats sweep per frame (wm_embed's
 * own, with the context's W -- not wm_embed_keys' per-key statistics) and ONE embed sweep (k_embed_signs_multi) that forms m, the W
 * row, u = m W and the base row once per row for a group of wm_embed_signs_group() copies and then, per copy, multiplies by the tile's
 * sign and stores: K stores of y, and x, W and base read once per group.
 *
 * signs is a HOST array [frames][ncopies][ny][nx] of -1, 0 or +1.  Copy (f, k) is frame f * ncopies + k of `out` and equals, bit for
 * bit, what wm_embed_signs on the batched sweeps writes for frame f with the table signs[f][k]; a_out[frames] is wm_embed_signs'
 * strength, which is wm_embed's: ONE strength per frame, not per copy.  status_out[frames]; either may be NULL; both are written by
 * wm_sync.
 *   - in_gray and base take everything wm_embed_keys takes: f32 / u8, a grey or planar-RGB base (run once per channel), a base that is
 *     in_gray itself, any pitch and width, WM_MEM_HOST, WM_MEM_SLOT_OUT for in_gray, batches up to max_frames, ME with p = 3
 *     (WM_ERR_BAD_P otherwise), NVF with p = 3..9.
 *   - `out` follows wm_embed_keys' rules: a WM_MEM_DEVICE plane with the channels and dtype of `base`, out->frames ==
 *     in_gray->frames * ncopies (it may exceed max_frames), any pitch and frame stride; its frames must not overlap each other,
 *     in_gray or base (WM_ERR_BAD_ARG, judged on the resolved planes).
 *   - 1 <= ncopies <= 4096, and the sweep's grid times the copy groups must fit a launch grid of 31 bits: WM_ERR_BAD_ARG before any
 *     device work otherwise.
 *   - An unsolvable frame has status WM_UNSOLVABLE: all its copies equal base bit for bit and a_out[f] is left untouched.  A
 *     zero-energy frame follows wm_embed's rule: a = +inf, copies equal base.
 *   - An ENQUEUE on the slot (WM_SLOT_SYNC: slot 0, waits); `frames` results count against the slot's capacity of 4096 un-synced
 *     results.  Like wm_embed_keys it leaves no Gram hand-over behind, does not change what WM_MEM_SLOT_OUT names, and ends a
 *     hand-over whose plane its copies overwrite.  Never takes the fused kernels; refused in band mode (WM_ERR_BAD_ARG).
 *     k_embed_signs_multi is not in the wm_prof_* list.
 *   - `signs` is read before the call returns and kept like wm_embed_signs' table, frames * ncopies * ny * nx bytes in the slot's
 *     pinned host arena and device arena: the FIRST call on a slot that needs more of them than are left waits for the slot's stream
 *     and reallocates them, which waits for the whole device, the other slots' streams included.  Later calls only enqueue.
 *   - WM_ERR_BAD_ARG, before any device work, for a null ctx, plane or signs, a tile shape wm_tiles_shape refuses and a sign outside
 *     {-1, 0, +1} (its index is in the message).  Arguments are looked at in wm_embed_signs' order: null pointers, tile shape, mask,
 *     band mode, slot, planes, ncopies, signs, record room.
 *
 * wm_embed_bits_multi: a host layer over it.  payloads is a HOST array [frames][ncopies][(nbits + 7) / 8]; the table of copy (f, k)
 * is built exactly as wm_embed_bits builds its table from payloads[f][k].  tile_bit and nbits as for wm_embed_bits.
 *
 * wm_embed_signs_group: G, the copies whose stores share one march (a compile-time constant of the library). */
int wm_embed_signs_group(void);
int wm_embed_signs_multi(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows,
                         int tile_cols, int ncopies, const int8_t* signs /* HOST [frames][ncopies][ny][nx], -1 | 0 | +1 */,
                         float* a_out /* [frames] */, int* status_out /* [frames] */, int slot);
int wm_embed_bits_multi(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, int tile_rows,
                        int tile_cols, const int32_t* tile_bit /* HOST [ny*nx] */, int nbits, int ncopies,
                        const uint8_t* payloads /* HOST [frames][ncopies][(nbits+7)/8] */, float* a_out, int* status_out, int slot);

/* makeWatermark (Watermark.cpp:156-172) of every frame of `in_gray` once with EVERY key of the bank as W: one marked copy per
 * recipient.  Copy (f, k) -- frame f marked with key k -- is frame f * nkeys + k of `out`, so out->frames must be
 * in_gray->frames * nkeys; `out` is a WM_MEM_DEVICE plane with the channels and dtype of `base` (any pitch and frame stride; it
 * may hold more frames than max_frames).  a_out[frames][nkeys] (row-major) and status_out[frames] (either may be NULL) are
 * written by wm_sync.  in_gray and base take everything wm_embed takes (f32 / u8, grey or planar RGB base, a base that is
 * in_gray itself, any pitch and width, WM_MEM_HOST, WM_MEM_SLOT_OUT for in_gray, batches up to max_frames, ME with p = 3 --
 * WM_ERR_BAD_P otherwise, as wm_embed --, NVF with p = 3..9); the context supplies shape, p, psnr and device -- its own W is not
 * used.  WM_ERR_BAD_ARG for a host `out`, an `out` that overlaps in_gray or base, a wrong out->frames, a bank of another shape
 * or device, and in band mode.  Copy (f, k) and a[f][k] equal, bit for bit, what wm_embed on the batched sweeps
 * (wm_set_fused(0)) gives with key k as W.  The image side -- the Gram sweep, the solve, the mask and max|e| -- runs once for all
 * keys; one sweep (k_stats_keys) then sums every key's ||u|| reading the image once per group of keys and every key plane once,
 * and one more (k_embed_keys) writes the copies.  For a grey base it also reads the image once per group and every key plane
 * once; for a planar-RGB base it runs once per channel, so the image is read three times per group and every key plane three
 * times.  An unsolvable frame has status WM_UNSOLVABLE: all its copies equal
 * base bit for bit and its K strengths are left untouched (Watermark.cpp:164-165).  A zero key (a bank's planes start at
 * zero) follows wm_embed's zero-energy rule on its own: its copies equal base bit for bit, its strength is +inf, and the
 * other keys' copies are unaffected; wm_detect_keys scores it NaN.
 * An ENQUEUE on the slot like wm_embed (WM_SLOT_SYNC: slot 0, waits); never takes the fused single-launch kernels.  frames * nkeys
 * results count against the slot's capacity of 4096 un-synced results; beyond it the call returns WM_ERR_BUSY.  It leaves no
 * Gram hand-over behind and does not change what WM_MEM_SLOT_OUT names (still the slot's last wm_embed output); like every
 * library write it ends a hand-over whose plane its copies overwrite.
 *
 * HAZARD.  As for wm_detect_keys: the bank must stay ALIVE and UNMODIFIED until wm_sync of this slot has returned. */
int wm_embed_keys(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_keys* keys, const wm_plane* out,
                  float* a_out, int* status_out, int slot);

/* ---- A key per frame of a batch: frame f is marked, or scored, with key key_of_frame[f] of a bank --------------------------------
 * A batch is what makes the engine fast, and a batch of wm_embed / wm_detect has one watermark: the context's W.  wm_embed_keys and
 * wm_detect_keys pair every frame with EVERY key.  These two calls pair frame f with ONE key, key_of_frame[f]: a clip whose key
 * rotates by a secret schedule (the same additive pattern on every frame is what a frame-averaging estimate recovers), or a batch
 * filled with frames of several customers' streams.  Everything on the image side is independent of the key -- the Gram sweep, the
 * solve, the mask, max|e| -- and the sweeps that read W take it as one pointer, so a W per frame is a pointer per frame
 * (wm_k_select.hip).
 *
 * wm_key_schedule: a schedule from a seed.  key_of_frame[i] = z(first_frame + i) mod nkeys, i < frames, where z(n) is the (n + 1)-th
 * value of the splitmix64 of wm_bits_layout started at `seed`, formed directly from n:
 *     state = seed + (n + 1) * 0x9E3779B97F4A7C15;  z = state;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB;  z(n) = z ^ z >> 31                                              (all modulo 2^64)
 * so a clip cut from the middle of a video gets its schedule from the number of its first frame alone.  WM_OK, or WM_ERR_BAD_ARG
 * unless 1 <= nkeys <= WM_KEYS_MAX, frames >= 1 and key_of_frame is non-null.  Pure host arithmetic; it touches no device.
 *
 * wm_embed_select: makeWatermark (Watermark.cpp:156-172) of frame f with key key_of_frame[f] of the bank as W.  The context supplies
 * shape, p, psnr and device; its own W is not used.  Frame f of `out` and a_out[f] equal, bit for bit, what wm_embed on the batched
 * sweeps (wm_set_fused(0)) gives for frame f of the SAME batch on a context whose W is that key.  The Gram sweep and the solve are
 * wm_embed's own; then one stats sweep and one embed sweep, each launched once for the whole batch.
 *   - Takes every input wm_embed takes on the sweeps: f32 / u8, a grey or planar-RGB base, a base that is in_gray, in place (with the
 *     snapshot), any pitch and width, WM_MEM_HOST in and out, WM_MEM_SLOT_OUT for in_gray, batches up to max_frames, ME with p = 3
 *     (WM_ERR_BAD_P otherwise), NVF with p = 3..9.
 *   - An unsolvable frame follows wm_embed's rule, independent of the other frames: status WM_UNSOLVABLE, out = base bit for bit,
 *     a_out[f] untouched.  A zero-energy frame -- one whose key is an all-zero plane included -- follows wm_embed's rule too:
 *     a = +inf, out = base.
 *   - Like wm_embed_signs: an ENQUEUE on the slot (WM_SLOT_SYNC: slot 0, waits); `frames` results count against the slot's capacity
 *     of 4096 un-synced results; its output becomes what WM_MEM_SLOT_OUT names; it leaves NO Gram hand-over behind, checked or
 *     promised, and ends a hand-over whose plane it overwrites; it never takes the fused kernels and is refused in band mode.
 *
 * wm_detect_select: detectWatermark (Watermark.cpp:234-250) of frame f against key key_of_frame[f].  corr_out[f] equals, bit for
 * bit, wm_detect's on the batched sweeps for frame f of the same batch on a context whose W is that key.  The image side is
 * wm_detect_keys': every input it takes, the Gram sweep and the solve exactly as it takes them, a promised hand-over of a
 * WM_MEM_SLOT_OUT plane (wm_set_handover) included.  Never the checked hand-over, never the fused kernels; refused in band mode.
 * One result per frame.  A zero key scores NaN with status WM_OK; an unsolvable frame gives 0.0f and WM_UNSOLVABLE.
 *
 * Both calls:
 *   - key_of_frame is a HOST array [frames], read before the call returns: the caller may change or free it at once, and several
 *     un-synced calls on one slot each keep their own table.  The copies live in the slot's pinned host arena and device arena, like
 *     wm_embed_signs' table, with its caveat: the FIRST call on a slot that needs more of them than are left waits for the slot's
 *     stream and reallocates them, which waits for the whole device.  Later calls only enqueue.
 *   - WM_ERR_BAD_ARG before any device work, looked at in wm_embed_signs' order: null pointers, mask, band mode, slot, planes, a bank
 *     of another shape or device, an index outside 0 .. nkeys - 1 (wm_last_error names the frame); then record room (WM_ERR_BUSY).
 *   - What a table costs: in a single-key batch the frames of a launch share one W plane -- the four waves of a block read the same
 *     W rows, and all but the first frame's reads are cache hits.  With distinct keys every frame streams its own plane from memory
 *     in each of the three sweeps that read W (stats, embed, detect).  Runs of equal keys in the table get the sharing back by
 *     themselves: with an all-equal table every sweep runs at its single-key twin's speed, and the call adds the copy of the table
 *     in front of them.  Measured at 4K, F = 16: 16 distinct keys cost 1.16 (u8 NVF) to 1.68 (u8 ME) times the single-key embed +
 *     detect pair, f32 ME 1.36, and 0.31-0.82 of 16 queued one-frame calls on 16 contexts.
 *   - The new kernels are not in the wm_prof_* list.
 *
 * HAZARD.  As for wm_detect_keys: the kernels read the bank when the stream reaches them: the bank must stay ALIVE and UNMODIFIED (no
 * wm_keys_set / _load_file / _generate / _destroy on it) until wm_sync of this slot has returned.  The library does not check this. */
int wm_key_schedule(int nkeys, uint64_t seed, uint64_t first_frame, int frames, int32_t* key_of_frame /* [frames] */);
int wm_embed_select(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out, const wm_keys* keys,
                    const int32_t* key_of_frame /* HOST [frames] */, float* a_out, int* status_out, int slot);
int wm_detect_select(wm_ctx* ctx, int mask, const wm_plane* img, const wm_keys* keys, const int32_t* key_of_frame /* HOST [frames] */,
                     float* corr_out, int* status_out, int slot);

/* ---- Pixel formats: RGB to grey, interleaved 8-bit pixels to planes and back ----------------------------------------------------
 * The reference's image mode converts on the device around its two calls: af::rgb2gray of the RGB input for the mask source,
 * af::rgb2gray of every watermarked RGB result for the detector, .as(u8) in front of af::saveImageNative (main.cpp:153-154,196-197,
 * 235-237).  These three calls are that front: element-wise kernels, one lane per four consecutive pixels of a row (DESIGN.md
 * section 18).  Speed follows wm_plane's rule per plane: f32 planes with a 4-byte aligned base and u8 planes whose base, pitch and
 * strides are multiples of 4 move as 16-byte / dword accesses, packed pixels whose `data`, pitch_bytes and frame_stride_bytes are
 * multiples of 4 as 12-byte accesses; a width that is not a multiple of 4 costs a per-pixel tail at the right edge, any other layout
 * is moved pixel by pixel.  All of it is correct for any base address, pitch and stride.
 * All three are ENQUEUES on the slot like every other call (WM_SLOT_SYNC: slot 0, waits).  They deliver no scalar results and take
 * none of the slot's 4096 result records; they may share a slot with any other call in any order; their kernels are not in the
 * wm_prof_* list.  They do not change what WM_MEM_SLOT_OUT names and leave no hand-over; like every library write they end a
 * hand-over whose plane an output overlaps.  WM_MEM_HOST planes and packed buffers are staged through the slot's staging buffers
 * with hipMemcpy2DAsync on the slot's stream (a packed buffer as rows of 3 * cols bytes).
 * Arguments are looked at in this order, and the first failure is WM_ERR_BAD_ARG before any device work: null pointers (ctx, a
 * plane or packed buffer or its data); shapes (rows x cols of every plane must be the context's); channels, dtype and what else one
 * plane must satisfy on its own (pitch, strides, mem, frames within max_frames; pitch_bytes >= 3 * cols); frame counts that differ
 * between the planes; overlap of two device planes of the call; the slot; a weight that is not finite; a WM_MEM_SLOT_OUT input that
 * does not match the slot's last wm_embed output, or that the output overlaps (overlap is judged on the resolved planes: host planes
 * resolve to staging buffers of their own and overlap nothing).
 *
 * wm_packed: interleaved 8-bit pixels, three bytes per pixel in R, G, B order, as image files and most decoders hold them.
 * pixel (r, c) of frame f starts at data + f * frame_stride_bytes + r * pitch_bytes + 3 * c. */
typedef struct wm_packed {
    void* data;
    int32_t rows, cols;
    int32_t mem;                 /* WM_MEM_DEVICE or WM_MEM_HOST */
    int32_t frames;              /* >= 1 */
    int64_t pitch_bytes;         /* bytes between rows (>= 3 * cols, any value) */
    int64_t frame_stride_bytes;  /* bytes between frames (>= rows * pitch_bytes; ignored when frames == 1) */
} wm_packed;

/* af::rgb2gray(img, r, g, b)  (main.cpp:153-154,196-197).  rgb: a 3-channel planar plane, f32 or u8, device, host, or
 * WM_MEM_SLOT_OUT when the slot's last wm_embed wrote a 3-channel output with the same frames and dtype (a host-staged RGB image is
 * then converted without crossing the host link again); batches up to max_frames.  gray_out: a 1-channel f32 plane, device or host,
 * with the same frame count, that does not overlap rgb.  weights[3] = {r, g, b}; NULL means 0.299, 0.587, 0.114.
 * grey = (r * R + g * G) + b * B in f32, each product and sum rounded on its own (no fused multiply-add); u8 samples are converted
 * to f32 first, which is exact.  Bit for bit the oracle's wmo_rgb2gray. */
int wm_rgb2gray(wm_ctx* ctx, const wm_plane* rgb, const wm_plane* gray_out, const float* weights /* [3] or NULL */, int slot);
/* Interleaved 8-bit pixels -> the engine's planar layout and, in the same pass, the grey: one kernel that reads every source byte
 * once.  packed: device or host.  rgb_out: 3-channel planar, f32 or u8, device or host, may be NULL; gray_out: 1-channel f32, device
 * or host, may be NULL; not both NULL; same frame count as packed; none of the three may overlap another.  The planar samples are the
 * source bytes exactly; the grey equals wm_rgb2gray(rgb_out, weights) bit for bit. */
int wm_unpack_rgb8(wm_ctx* ctx, const wm_packed* packed, const wm_plane* rgb_out /* or NULL */, const wm_plane* gray_out /* or NULL */,
                   const float* weights /* [3] or NULL */, int slot);
/* The .as(u8) in front of af::saveImageNative (main.cpp:235-237): a planar 3-channel plane (f32 or u8; device, host, or the slot's
 * 3-channel WM_MEM_SLOT_OUT) -> interleaved 8-bit pixels, device or host.  f32 samples are clamped to [0, 255] and truncated toward
 * zero, NaN gives 0 (for the in-range values wm_embed produces: the C cast to uint8_t).  Bytes of a padded packed row beyond
 * 3 * cols are left untouched. */
int wm_pack_rgb8(wm_ctx* ctx, const wm_plane* rgb, const wm_packed* packed_out, int slot);

/* ---- Samples of 9 to 16 bits: 10-bit video (yuv420p10le, P010, y4m C420p10) and its kin ------------------------------------------
 * The engine's arithmetic takes any f32 value in [0, 255]; a d-bit sample is brought onto that scale and back (DESIGN.md section
 * 19).  bits = d in 9..16, maxv = 2^d - 1, and two constants, each the double quotient rounded once to f32:
 *     k_in = (float)(255.0 / maxv)        k_out = (float)(maxv / 255.0)
 * Unpack of a sample v (uint16):  s = msb_aligned ? v >> (16 - d) : min(v, maxv);  g = (float)s * k_in  (one f32 multiply).
 * Pack of a value g (f32):        t = g * k_out  (one f32 multiply);  t = fmin(fmax(t, 0), maxv), NaN gives 0 as in wm_pack_rgb8;
 *                                 q = rint(t), ties to even -- NOT truncation;  v = msb_aligned ? q << (16 - d) : q.
 * With these constants pack(unpack(v)) == v for every v <= maxv and every d, and maxv maps to exactly 255.0f: a pixel the embed
 * leaves alone survives the round trip bit for bit (truncation would not give that).  A PSNR against peak 255 on the scaled plane
 * is the PSNR against peak maxv on the samples.  msb_aligned = 1: the sample sits in the high bits of its 16 (the Y plane of P010,
 * P012, P016; on unpack the low 16 - d bits are ignored, on pack they are written as zero); msb_aligned = 0: in the low bits
 * (yuv420p10le / p12le, y4m C420pNN; on unpack a code above maxv is clamped to maxv).  Samples are in the host's byte order.
 *
 * A WM_U16 plane has 2-byte elements; pitch and strides are in elements and `data` must be 2-byte aligned.  Speed: a plane whose
 * base is a multiple of 4 bytes and whose pitch and used strides are even moves as one 8-byte access per four pixels, any other
 * pixel by pixel; the f32 side follows wm_plane's rule; a width that is not a multiple of 4 costs a per-pixel tail at the right edge.
 *
 * wm_unpack16 and wm_pack16 behave like the pixel-format front above: ENQUEUES on the slot (WM_SLOT_SYNC: slot 0, waits), no result
 * records, kernels outside the wm_prof_* list, no change of what WM_MEM_SLOT_OUT names, no hand-over left, and the end of a
 * hand-over whose plane an output overlaps.  WM_MEM_HOST planes are staged with hipMemcpy2DAsync on the slot's stream.  Arguments are
 * looked at in that front's order, and the first failure is WM_ERR_BAD_ARG before any device work: null pointers; shapes; channels
 * (1 or 3, planar), dtype and what else one plane must satisfy on its own (2-byte alignment of a u16 plane among it); channel
 * counts, then frame counts, that differ between the two planes; overlap of two device planes; the slot; `bits` outside 9..16 or
 * msb_aligned outside {0, 1}; a WM_MEM_SLOT_OUT input that does not match the slot's last wm_embed output or that the output
 * overlaps. */

/* The two scale constants of `bits` (pure host arithmetic, touches no device).  WM_OK, or WM_ERR_BAD_ARG for bits outside 9..16 or
 * a null pointer. */
int wm_depth_scale(int bits, float* to255, float* from255);
/* src16: WM_U16, device or host.  out_f32: WM_F32, device or host.  Both with 1 or 3 planar channels, the same channel and frame
 * count (batches up to max_frames) and the context's shape; they must not overlap. */
int wm_unpack16(wm_ctx* ctx, const wm_plane* src16, int bits, int msb_aligned, const wm_plane* out_f32, int slot);
/* src_f32: WM_F32; device, host, or WM_MEM_SLOT_OUT: the slot's last wm_embed output when that is an f32 plane of the same channels
 * (1 or 3) and frames.  out16: WM_U16, device or host, not overlapping src_f32.  Elements of a padded row beyond cols are left
 * untouched. */
int wm_pack16(wm_ctx* ctx, const wm_plane* src_f32, const wm_plane* out16, int bits, int msb_aligned, int slot);
/* The video call: watermark d-bit grey frames.  out16 may be in16 itself (in place): in16 is read completely before out16 is written.
 * A host layer over three enqueues on the slot: wm_unpack16(in16) into a slot-owned f32 plane X, wm_embed(X, X, Y) into a second
 * slot-owned f32 plane Y (not in place: no snapshot; queued as a batched call, so it never takes the fused kernels, whatever the
 * slot), wm_pack16(Y) into out16.  With WM_SLOT_SYNC it waits once at the end.  The bytes and the strength are those of the three
 * calls made one by one.  Everything wm_embed documents holds for Y: the strength, WM_UNSOLVABLE and zero-energy frames (such a frame
 * comes back as pack(unpack(in16))), hand-overs, and afterwards the slot's WM_MEM_SLOT_OUT names Y, an f32 grey plane wm_detect
 * accepts.  `frames` results count against the slot's 4096.  ME with p = 3 (WM_ERR_BAD_P otherwise), NVF with p = 3..9; refused in
 * band mode.  X and Y are kept per slot and grown on demand: the FIRST call on a slot that needs more of them than any call before
 * reallocates them, which waits for the whole device, the other slots' streams included.  Later calls only enqueue. */
int wm_embed16(wm_ctx* ctx, int mask, const wm_plane* in16, const wm_plane* out16, int bits, int msb_aligned, float* a_out,
               int* status_out, int slot);
/* wm_unpack16(img16) into the slot's X, then wm_detect(X) on the sweeps (never the fused kernels): the score of
 * wm_detect(wm_unpack16(img16)) bit for bit.  Grey only; masks, band mode, result records and X as for wm_embed16. */
int wm_detect16(wm_ctx* ctx, int mask, const wm_plane* img16, int bits, int msb_aligned, float* corr_out, int* status_out, int slot);

/* ---- Quality of a marked copy: PSNR and SSIM against its base, measured on the device ---------------------------------------------
 * The one quality knob is psnr, and wm_embed scales `a` so that the UNCLAMPED float term a m W has exactly that PSNR.  What a
 * recipient gets has also been through the clamp to [0, 255], truncation to u8 (wm_pack_rgb8, u8 planes) or rounding to d bits
 * (wm_pack16), tiles with sign 0 (wm_embed_signs) and K keys with K strengths (wm_embed_keys).  wm_quality measures what a call
 * actually achieved: the mean squared error, the SSIM index of Wang et al. (2004) and the largest difference of `test` against
 * `ref`, per (frame, channel) and, in sums_dev, per tile.  Every difference, square, product and sum below is f64.
 *
 * d = (double)ref - (double)test per sample (u8 samples convert exactly).
 * Sums over a tile's pixels: sse = sum d^2;  max|d|;  npix = the tile's pixel count.
 * SSIM: an 11 x 11 window with weights g[i] g[j], g[i] = exp(-(i - 5)^2 / 4.5) divided by the sum of the eleven values (f64, formed
 * on the host).  L = 255 (the engine's scale is [0, 255] everywhere), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.  Only windows that lie
 * wholly inside the plane are evaluated -- no padding --, so the window centres are rows 5 .. rows - 6 and columns 5 .. cols - 6.
 * Per window, with E[.] the weighted mean over the window, x = ref and y = test:
 *     mx = E[x], my = E[y];  vx = E[x^2] - mx^2, vy = E[y^2] - my^2, cxy = E[x y] - mx my;
 *     s = ((2 mx my + C1) (2 cxy + C2)) / ((mx^2 + my^2 + C1) (vx + vy + C2))
 * evaluated separably (rows, then columns) with the taps i and 10 - i added before they are weighted.  A window belongs to the tile
 * that holds its centre pixel: ssim_sum = sum s, nwin = the tile's window count.
 * Tile geometry is wm_tiles_shape's, unchanged; tile_rows == tile_cols == 0 means ONE tile per plane (ny = nx = 1); any other tile
 * shape must pass wm_tiles_shape.
 *
 * sums_dev [frames][channels][ny][nx][WM_QUALITY_NSUMS] is a DEVICE f64 array on the context's device and may be NULL:
 * {sse, npix, ssim_sum, nwin, max|d|} per tile, written on the slot's stream and valid once wm_sync(ctx, slot) has returned.  The
 * sums ADD over tiles (max for the fifth).  q_out [frames][channels][WM_QUALITY_NVALS] is a HOST f32 array written by wm_sync and may
 * be NULL (not both): {(float)(sse / npix), (float)(ssim_sum / nwin), (float)max|d|} over the whole plane, the tile sums added in
 * ascending tile index (max for the third).  PSNR = wm_psnr_from_mse(mse, 255).
 *   - A plane with rows < 11 or cols < 11 has no window: nwin = 0 and its ssim is 0 / 0 = NaN, the zero rule of this header; its mse
 *     and max|d| are unaffected.  Planes that hold non-finite samples give unspecified values; the call completes.
 *   - ref and test are f32 or u8, independently (all four combinations), 1 or 3 planar channels, equal between the two, equal frame
 *     counts within max_frames, any base address, pitch and strides, WM_MEM_DEVICE or WM_MEM_HOST.  test (only) may be
 *     WM_MEM_SLOT_OUT: the slot's last embed output, 1 or 3 channels, when its channels, frames and dtype are the plane's (the rule of
 *     wm_pack_rgb8 and wm_pack16).  The planes may overlap or be the same plane: both are only read.  The context supplies shape,
 *     device and slots; its W, p and psnr are not used.
 *   - An ENQUEUE on the slot (WM_SLOT_SYNC: slot 0, waits); it may share a slot with any other call in any order.  It writes no plane
 *     and changes nothing about the slot: not what WM_MEM_SLOT_OUT names, and it neither leaves nor ends a hand-over, checked or
 *     promised.  Never takes the fused kernels; refused in band mode.  Its kernels are not in the wm_prof_* list.
 *   - frames * channels * 3 result records count against the slot's 4096 (WM_ERR_BUSY) when q_out is non-null; none otherwise.
 *   - Scratch (frames * channels * ceil(rows / rps) * ceil(cols / 4) * 24 bytes of records, rps = the largest divisor of tile_rows in
 *     8 .. 48, 48 for one tile per plane -- 1.0 to 1.6 MB per 4K plane --, a few per cent more for the folds, and the tile sums when sums_dev
 *     is NULL) is kept per slot and grown on demand (WM_ERR_ALLOC when it does not fit): the FIRST call on a slot that needs more of
 *     it than any call before reallocates it, which waits for the whole device, the other slots' streams included.  Later calls only
 *     enqueue.
 *   - WM_ERR_BAD_ARG, before any device work, looked at in this order: a null ctx or plane, or q_out and sums_dev both NULL; shapes
 *     (rows x cols of both planes must be the context's); each plane's own rules; channel counts that differ; frame counts that differ
 *     (and frames * channels beyond 65535, the launch grid); the tile shape; band mode; the slot; a WM_MEM_SLOT_OUT test plane that
 *     does not match the slot's last embed output.  Record room is looked at after these.
 * Bits: a (frame, channel)'s sums do not depend on the batch it arrives in or on repetition (segments follow from tile_rows alone;
 * every fold adds in a fixed order, no atomics).
 *
 * wm_psnr_from_mse: 10 log10(peak^2 / mse).  +inf for mse == 0; NaN for a negative or NaN mse and for peak <= 0 (or NaN).  Pure host
 * arithmetic; it touches no device. */
#define WM_QUALITY_NVALS 3  /* per (frame, channel), HOST f32, delivered by wm_sync: {mse, ssim, max|d|} */
#define WM_QUALITY_NSUMS 5  /* per (frame, channel, tile), DEVICE f64: {sse, npix, ssim_sum, nwin, max|d|} */
int wm_quality(wm_ctx* ctx, const wm_plane* ref, const wm_plane* test, int tile_rows, int tile_cols,
               float* q_out /* HOST [frames][channels][3], may be NULL */,
               double* sums_dev /* DEVICE [frames][channels][ny][nx][5], may be NULL */, int slot);
double wm_psnr_from_mse(double mse, double peak);

/* Building blocks exposed for parity tests (the reference keeps them private):
 * computeCustomMask / computePredictionErrorMask (Watermark.cpp:96-114,176-218).
 * mask_out / e_out: f32 device planes [rows,cols] (e_out may be NULL; ignored for NVF).
 * coef_out[8*frames] (may be NULL) receives the prediction coefficients at wm_sync. */
int wm_compute_mask(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* mask_out, const wm_plane* e_out,
                    float* coef_out, int* status_out, int slot);

/* Gram sums of the 3x3 neighbourhood (me kernel + af::sum folding, me_p3.hpp:8-21,61-82, Watermark.cpp:140-151):
 * gram_out[44*frames] doubles = the 36 upper-triangle Rx entries (i <= j, row-major) then the 8 rx entries.
 * Synchronous (parity-test building block). */
int wm_gram(wm_ctx* ctx, const wm_plane* img, double* gram_out, int slot);

/* ---- Intra-frame sharding: one image split into row bands over several GPUs -----------------
 * No counterpart in the reference (one image = one device there); for single images too large or too urgent for one
 * GPU.  A context created for `rows` x `cols` then holds a BAND: its owned rows plus p/2 + 1 halo rows (2 for p = 3) of real image data on
 * every side that is not an image border (W likewise: the band's rows of the watermark file).  wm_band_configure names
 * the owned rows [own_lo, own_hi) in plane coordinates and the row count of the whole image; own_lo == 0 /
 * own_hi == rows mark true image borders (replicate padding applies there only).  Sweeps then sum and store the
 * owned rows only, and the caller all-reduces the partial totals between the phases (one process per GPU,
 * torch.distributed / RCCL; watermarking-gpu_amd/bands.py):
 *   embed : wm_gram (44 sums) -> SUM -> wm_band_solve -> wm_band_stats ({max|e|, sum}) -> MAX, SUM -> wm_band_embed
 *   detect: halo rows of y from the neighbour bands -> wm_gram -> SUM -> wm_band_solve
 *           -> wm_band_detect_sums ({<e_u,e_w>, |e_u|^2, |e_w|^2}) -> SUM -> corr = (float)dot / (float)(sqrt(nw) * sqrt(nu))
 * The halo rule bounds the split as well: the rows below a band's owned rows are its lower neighbours' owned rows, so the band
 * that holds the image's bottom border owns at least p/2 + 1 >= 2 rows (the top band likewise).  The Gram sweep relies on it: it
 * sums the window rows R-2, R-1 and R of the image in the band with own_hi == rows, and every band above stops at R-3.  A split
 * whose last band is the image's last row alone is therefore refused -- at the band above, which would hold one row below its own
 * ("an interior side needs 2 halo rows").
 * All five calls are synchronous.  own_hi == 0 switches band mode off.  In band mode wm_embed / wm_detect see only the
 * band and are not meaningful. */
int wm_band_configure(wm_ctx* ctx, int own_lo, int own_hi, long long rows_global);
/* totals[44*frames]: the all-reduced wm_gram sums; solves c (Watermark.cpp:203) into the slot; status_out[frames] may be NULL */
int wm_band_solve(wm_ctx* ctx, const double* totals, int frames, int* status_out, int slot);
/* out[2*frames]: {max|e| (1 for NVF), sum (m W)^2 without the 1/max^2} over the owned rows; needs wm_band_solve first (ME) */
int wm_band_stats(wm_ctx* ctx, int mask, const wm_plane* in_gray, double* out, int slot);
/* max_sum[2*frames]: the all-reduced wm_band_stats values; writes the owned rows of `out` (device planes, out must not
 * overlap in_gray); a_out[frames] (may be NULL) receives the strength (Watermark.cpp:170) */
int wm_band_embed(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out,
                  const double* max_sum, float* a_out, int slot);
/* out[3*frames]: {<e_u,e_w>, ||e_u||^2, ||e_w||^2} over the owned rows; needs wm_band_solve first */
int wm_band_detect_sums(wm_ctx* ctx, int mask, const wm_plane* img, double* out, int slot);

/* The same phases with the exchange RESIDENT IN DEVICE MEMORY ("one RCCL all-reduce of 44 doubles per sweep"):
 * every call only enqueues on the slot's stream -- give the slot the stream the caller's collectives are ordered on with
 * wm_set_stream -- and hands its totals over in device memory the caller owns; the caller all-reduces / all-gathers them in
 * place with RCCL on that stream (watermarking-gpu_amd/bands.py with backend "nccl"; ncclAllReduce / ncclAllGather from C++).
 * Nothing synchronises with the host until the caller reads a result.
 *   embed : wm_band_gram_dev -> all-reduce SUM [44] -> wm_band_solve_dev -> wm_band_stats_dev -> all-gather [2] per rank
 *           -> wm_band_embed_dev (folds the gathered parts in rank order: the same bits on every rank)
 *   detect: halo rows of y (ncclSend / ncclRecv) -> wm_band_gram_dev -> all-reduce -> wm_band_solve_dev
 *           -> wm_band_detect_sums_dev -> all-reduce SUM [3] -> wm_band_corr_dev
 * totals_dev[44*frames], max_sum_dev[2*frames], gathered_max_sum_dev[nparts][2*frames], sums_dev[3*frames] doubles;
 * a_dev[frames] (may be NULL; NaN for an unsolvable frame, whose output is the base: Watermark.cpp:164-165), corr_dev[frames]
 * (0.0f when unsolvable: Watermark.cpp:246-247) floats -- all device pointers. */
int wm_band_gram_dev(wm_ctx* ctx, const wm_plane* img, double* totals_dev, int slot);
int wm_band_solve_dev(wm_ctx* ctx, const double* totals_dev, int frames, int slot);
int wm_band_stats_dev(wm_ctx* ctx, int mask, const wm_plane* in_gray, double* max_sum_dev, int slot);
int wm_band_embed_dev(wm_ctx* ctx, int mask, const wm_plane* in_gray, const wm_plane* base, const wm_plane* out,
                      const double* gathered_max_sum_dev, int nparts, float* a_dev, int slot);
int wm_band_detect_sums_dev(wm_ctx* ctx, int mask, const wm_plane* img, double* sums_dev, int slot);
int wm_band_corr_dev(wm_ctx* ctx, const double* sums_dev, int frames, float* corr_dev, int slot);

/* waits for everything queued on `slot`, then delivers the scalar results; returns WM_OK,
 * WM_UNSOLVABLE if any delivered frame was unsolvable, or < 0 */
int wm_sync(wm_ctx* ctx, int slot);

/* stream plumbing: run a slot on the caller's hipStream_t (NULL restores the slot's own stream; the legacy default stream
 * is named by HIP's handle for it, hipStreamLegacy) */
int wm_set_stream(wm_ctx* ctx, int slot, void* hip_stream);
void* wm_get_stream(wm_ctx* ctx, int slot);

/* device memory helpers so that host code above this ABI needs no HIP headers (include/Watermark.hpp is plain C++) */
void* wm_dev_alloc(int device, size_t bytes);
void wm_dev_free(void* p);
int wm_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes);
int wm_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes);
int wm_device_count(void);

/* pinned host memory for WM_MEM_HOST planes (the reference's CL_MEM_ALLOC_HOST_PTR buffer, main.cpp:273-275) */
void* wm_host_alloc(size_t bytes);
void wm_host_free(void* p);

/* properties */
int wm_rows(const wm_ctx* ctx);
int wm_cols(const wm_ctx* ctx);
int wm_p(const wm_ctx* ctx);
float wm_strength_factor(const wm_ctx* ctx); /* Watermark.cpp:22 */
int wm_device(const wm_ctx* ctx);
const float* wm_w_device(const wm_ctx* ctx); /* device copy of W, row-major */

/* Memory-system yardstick of the box, independent of the engine's sweeps (bench.py's `membench` leg): one kernel per launch over
 * `bytes` of device memory this call allocates -- kind 0: pure store (16 B per lane, non-temporal, the store form k_embed
 * uses), 1: pure copy (16 B loads + the same stores; `bytes` read and `bytes` written), 2: pure read (16 B loads folded into a
 * checksum); kinds 3, 4, 5: the same three in the grid shape that streams fastest on MI355X (65536 blocks of 256 threads, one
 * element per thread; kinds 0-2 use 2048 blocks with four elements in flight per thread, a grid like the sweeps' own) --
 * launched back to back for at least `seconds`, every launch timed by events attached to the dispatch.  Writes the
 * mean launch duration in microseconds and the launch count; GB/s = bytes moved per launch / that.  Two boxes that run
 * k_embed at different speeds with equal clocks and power either differ here too (a slow-writing memory system) or do not
 * (then the difference is the kernel's). */
int wm_membench(int device, int kind, size_t bytes, double seconds, double* mean_us, int* launches);

/* per-kernel timing with hipEvents recorded on the launch stream (bench.py's roofline leg) */
int wm_prof_enable(wm_ctx* ctx, int on);
int wm_prof_reset(wm_ctx* ctx);
int wm_prof_kernel_count(void);
const char* wm_prof_kernel_name(int kernel_id);
/* launches and total milliseconds recorded for one kernel since the last reset (syncs the device) */
int wm_prof_get(wm_ctx* ctx, int kernel_id, uint64_t* launches, double* total_ms);

const char* wm_strerror(int code);
const char* wm_last_error(const wm_ctx* ctx); /* detail of the last failing call ("" if none) */
const char* wm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WM_H_ */
