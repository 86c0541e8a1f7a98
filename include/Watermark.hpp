// Watermark.hpp -- drop-in C++ surface for the reference's `Watermark` class
// (kar-dim/Watermarking-GPU, Watermark_GPU/Watermark.hpp:26-72) on top of the C ABI of wm.h.
//
// Same class name, method names, enum and argument order as the reference.  Differences forced by the target:
//   * af::array does not exist on MI355X boxes: images are wm::Image (a ref-counted device buffer, planar
//     [channels][rows][cols], f32 or u8).  Like af::array it is cheap to copy (shared buffer).
//   * the `programs` constructor argument (pre-built OpenCL programs, Watermark.hpp:63) is gone: the kernels are
//     compiled into libwm_hip.so.  An optional trailing `device` replaces main.cpp:73's af::setDevice().
//   * makeWatermark returns a finished image (the reference returns a lazy ArrayFire expression, Watermark.cpp:171).
// Error behaviour is the reference's: std::runtime_error with the same messages (Watermark.cpp:24-25,65-66,70-71);
// an unsolvable prediction system is NOT an error: makeWatermark returns `outputImage` itself and leaves
// `watermarkStrength` untouched, detectWatermark returns 0.0f (Watermark.cpp:164-165,246-247).
// This header is plain C++17: it needs no HIP headers, only wm.h and libwm_hip.so at link time.
#pragma once
#include "wm.h"

#include <cstdint>
#include <fstream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

using dim_t = long long;  // ArrayFire's dim_t

enum MASK_TYPE  // Watermark.hpp:10-14
{
    ME,
    NVF
};

struct dim2  // Watermark.hpp:16-20
{
    dim_t rows;
    dim_t cols;
};

namespace wm {

enum class dtype { f32 = WM_F32, u8 = WM_U8 };

// Stand-in for af::array on this path: planar [channels][rows][cols] device image.
class Image {
public:
    Image() = default;
    Image(dim_t rows, dim_t cols, int channels = 1, dtype t = dtype::f32, int device = 0)
        : rows_(rows), cols_(cols), channels_(channels), type_(t), device_(device)
    {
        // device buffers are recycled through a small per-process pool (like ArrayFire's memory manager): a
        // hipMalloc/hipFree pair per makeWatermark call would dominate a single-image call
        const size_t nb = bytes();
        void* p = pool_take(device, nb);
        if (!p) p = wm_dev_alloc(device, nb);
        if (!p) throw std::runtime_error("wm::Image: device allocation failed (no usable HIP device?)\n");
        buf_ = std::shared_ptr<void>(p, [device, nb](void* q) { pool_give(device, nb, q); });
    }
    // n images of one shape in ONE device buffer, image i at i * elements() (each shares the buffer; what a batched plane
    // with frame stride elements() addresses)
    static std::vector<Image> stack(int n, dim_t rows, dim_t cols, int channels = 1, dtype t = dtype::f32, int device = 0)
    {
        Image all(rows * n, cols, channels, t, device);
        const size_t each = all.bytes() / (size_t)n;
        std::vector<Image> v((size_t)n);
        for (int i = 0; i < n; ++i) {
            Image& im = v[(size_t)i];
            im.rows_ = rows; im.cols_ = cols; im.channels_ = channels; im.type_ = t; im.device_ = device;
            im.buf_ = std::shared_ptr<void>(all.buf_, static_cast<char*>(all.buf_.get()) + (size_t)i * each);
        }
        return v;
    }
    static Image fromHost(const float* data, dim_t rows, dim_t cols, int channels = 1, int device = 0)
    {
        Image im(rows, cols, channels, dtype::f32, device);
        if (wm_memcpy_h2d(im.buf_.get(), data, im.bytes()) != WM_OK) throw std::runtime_error("wm::Image: upload failed\n");
        return im;
    }
    static Image fromHost(const uint8_t* data, dim_t rows, dim_t cols, int channels = 1, int device = 0)
    {
        Image im(rows, cols, channels, dtype::u8, device);
        if (wm_memcpy_h2d(im.buf_.get(), data, im.bytes()) != WM_OK) throw std::runtime_error("wm::Image: upload failed\n");
        return im;
    }
    void host(void* dst) const  // af::array::host()
    {
        if (wm_memcpy_d2h(dst, buf_.get(), bytes()) != WM_OK) throw std::runtime_error("wm::Image: download failed\n");
    }
    dim_t rows() const { return rows_; }
    dim_t cols() const { return cols_; }
    dim_t dims(int i) const { return i == 0 ? rows_ : (i == 1 ? cols_ : (i == 2 ? channels_ : 1)); }
    int channels() const { return channels_; }
    dim_t elements() const { return rows_ * cols_ * channels_; }
    dtype type() const { return type_; }
    bool isempty() const { return !buf_; }
    void* device_ptr() const { return buf_.get(); }
    size_t bytes() const { return (size_t)elements() * (type_ == dtype::f32 ? 4 : 1); }
    bool same_buffer(const Image& o) const { return buf_.get() == o.buf_.get(); }
    wm_plane plane() const
    {
        wm_plane p{};
        p.data = buf_.get(); p.rows = (int32_t)rows_; p.cols = (int32_t)cols_; p.channels = channels_;
        p.dtype = (int32_t)type_; p.mem = WM_MEM_DEVICE; p.frames = 1; p.pitch = cols_;
        p.channel_stride = rows_ * cols_; p.frame_stride = 0;
        return p;
    }

private:
    struct PoolEntry { int device; size_t bytes; void* p; };
    static std::vector<PoolEntry>& pool() { static std::vector<PoolEntry> v; return v; }
    static std::mutex& pool_mu() { static std::mutex m; return m; }  // Images are created / destroyed from several host threads
    static void* pool_take(int device, size_t nb)
    {
        std::lock_guard<std::mutex> lk(pool_mu());
        auto& v = pool();
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].device == device && v[i].bytes == nb) { void* p = v[i].p; v.erase(v.begin() + (long)i); return p; }
        return nullptr;
    }
    static void pool_give(int device, size_t nb, void* p)
    {
        std::lock_guard<std::mutex> lk(pool_mu());
        auto& v = pool();
        if (v.size() >= 16) { wm_dev_free(v.front().p); v.erase(v.begin()); }
        v.push_back({device, nb, p});
    }
    std::shared_ptr<void> buf_;
    dim_t rows_ = 0, cols_ = 0;
    int channels_ = 1;
    dtype type_ = dtype::f32;
    int device_ = 0;
};

// What Watermark::quality measures per channel (wm.h wm_quality): the mean squared error, its PSNR against peak 255, the mean SSIM
// index over the whole windows (NaN below 11 x 11) and the largest absolute difference
struct Quality { float mse, psnr, ssim, maxAbs; };

}  // namespace wm

// What Watermark::locate finds per frame (wm.h wm_locate): the offset of the crop in its key, the map value there (the detector's
// <e_u, e_w> against that window) and its distance from the rest of the map in standard deviations (NaN: no such measure)
struct WmLocation { int oy, ox; float peak, z; };

// A bank of watermark keys on one device (wm.h wm_keys_*): what Watermark::detectWatermarkKeys scores one image against.
// Owns its device planes; movable, not copyable.  Errors throw std::runtime_error like the Watermark methods.
class WatermarkKeys {
public:
    WatermarkKeys(const dim_t rows, const dim_t cols, const int nkeys, const int device = 0)
    {
        wm_keys* k = nullptr;
        check(wm_keys_create(&k, device, (int)rows, (int)cols, nkeys), "WatermarkKeys");
        keys = k;
    }
    WatermarkKeys(const WatermarkKeys&) = delete;
    WatermarkKeys& operator=(const WatermarkKeys&) = delete;
    WatermarkKeys(WatermarkKeys&& other) noexcept : keys(other.keys) { other.keys = nullptr; }
    WatermarkKeys& operator=(WatermarkKeys&& other) noexcept
    {
        if (this != &other) { wm_keys_destroy(keys); keys = other.keys; other.keys = nullptr; }
        return *this;
    }
    ~WatermarkKeys() { wm_keys_destroy(keys); }

    // key k := host floats [rows * cols], a W file (loadRandomMatrix's checks), or the W generated from a seed
    void set(int k, const float* host_w) { check(wm_keys_set(keys, k, host_w, WM_MEM_HOST), "WatermarkKeys::set"); }
    void load(int k, const std::string& randomMatrixPath) { check(wm_keys_load_file(keys, k, randomMatrixPath.c_str()), "WatermarkKeys::load"); }
    void generate(int k, uint32_t seed) { check(wm_keys_generate(keys, k, seed), "WatermarkKeys::generate"); }
    int count() const { return wm_keys_count(keys); }
    dim2 size() const { return {wm_keys_rows(keys), wm_keys_cols(keys)}; }
    const wm_keys* handle() const { return keys; }

private:
    wm_keys* keys = nullptr;
    static void check(int rc, const char* where)
    {
        if (rc != WM_OK) throw std::runtime_error(std::string("ERROR in ") + where + ": " + wm_strerror(rc) + " Error code: " + std::to_string(rc) + "\n");
    }
};

/*!
 *  \brief  Functions for watermark computation and detection (MI355X-native engine behind the reference's surface)
 */
class Watermark {
public:
    Watermark(const dim_t rows, const dim_t cols, const std::string& randomMatrixPath, const int p, const float psnr, const int device = 0)
        : dims({rows, cols}), p(p), psnr(psnr), device(device)
    {
        if (p != 3 && p != 5 && p != 7 && p != 9)
            throw std::runtime_error(std::string("Wrong p parameter: ") + std::to_string(p) + "!\n");  // Watermark.cpp:24-25
        wm_ctx* c = nullptr;
        check_w(wm_create_from_file(&c, device, (int)rows, (int)cols, p, psnr, randomMatrixPath.c_str()), randomMatrixPath, rows, cols);
        ctx = c;
    }
    Watermark(const Watermark& other) : dims(other.dims), p(other.p), psnr(other.psnr), device(other.device)  // Watermark.cpp:30-37
    {
        wm_ctx* c = nullptr;
        check(wm_clone(other.ctx, &c), "Watermark copy");
        ctx = c;
    }
    Watermark(Watermark&& other) noexcept = delete;
    Watermark& operator=(Watermark&& other) noexcept = delete;
    Watermark& operator=(const Watermark& other)  // Watermark.cpp:40-51
    {
        if (this != &other) {
            wm_ctx* c = nullptr;
            check(wm_clone(other.ctx, &c), "Watermark copy assignment");
            wm_destroy(ctx);
            ctx = c; dims = other.dims; p = other.p; psnr = other.psnr; device = other.device;
        }
        return *this;
    }
    ~Watermark() { wm_destroy(ctx); }

    void reinitialize(const std::string& randomMatrixPath, const dim_t rows, const dim_t cols)  // Watermark.cpp:78-85
    {
        check_w(wm_reinit_from_file(ctx, (int)rows, (int)cols, randomMatrixPath.c_str()), randomMatrixPath, rows, cols);
        dims = {rows, cols};
    }

    // Watermark.cpp:156-172
    wm::Image makeWatermark(const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, MASK_TYPE maskType) const
    {
        wm::Image out(outputImage.rows(), outputImage.cols(), outputImage.channels(), outputImage.type(), device);
        const wm_plane pin = inputImage.plane(), pbase = outputImage.plane(), pout = out.plane();
        float a = 0.0f;
        int st = 0;
        const int rc = wm_embed(ctx, (int)maskType, &pin, &pbase, &pout, &a, &st, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeWatermark");
        if (st != 0) return outputImage;  // not solvable: output image without modification, strength untouched
        // ||m W|| = 0 (integer-flat image under NVF, zero W): strength +inf, out == outputImage bit for bit (wm.h wm_embed)
        watermarkStrength = a;
        return out;
    }
    // Watermark.cpp:234-250
    float detectWatermark(const wm::Image& watermarkedImage, MASK_TYPE maskType) const
    {
        const wm_plane pimg = watermarkedImage.plane();
        float corr = 0.0f;
        const int rc = wm_detect(ctx, (int)maskType, &pimg, &corr, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "detectWatermark");
        return corr;
    }
    // af::rgb2gray(img, r, g, b) (main.cpp:153-154,196-197) on the device (wm.h wm_rgb2gray): the f32 grey of a planar RGB image,
    // f32 or u8, (r R + g G) + b B in f32
    wm::Image rgb2gray(const wm::Image& rgb, float r = 0.299f, float g = 0.587f, float b = 0.114f) const
    {
        wm::Image gray(rgb.rows(), rgb.cols(), 1, wm::dtype::f32, device);
        const wm_plane prgb = rgb.plane(), pg = gray.plane();
        const float w[3] = {r, g, b};
        const int rc = wm_rgb2gray(ctx, &prgb, &pg, w, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "rgb2gray");
        return gray;
    }
    // interleaved 8-bit pixels on the host (rows * cols * 3 bytes, R G B) -> {planar f32 RGB, f32 grey (empty unless wantGray)} on
    // the device: the image crosses the host link once, as bytes (wm.h wm_unpack_rgb8)
    std::pair<wm::Image, wm::Image> unpackRgb8(const uint8_t* interleavedHost, bool wantGray) const
    {
        wm::Image rgb(dims.rows, dims.cols, 3, wm::dtype::f32, device), gray;
        if (wantGray) gray = wm::Image(dims.rows, dims.cols, 1, wm::dtype::f32, device);
        const wm_packed pk = packed(const_cast<uint8_t*>(interleavedHost));
        const wm_plane prgb = rgb.plane(), pg = wantGray ? gray.plane() : wm_plane{};
        const int rc = wm_unpack_rgb8(ctx, &pk, &prgb, wantGray ? &pg : nullptr, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "unpackRgb8");
        return {rgb, gray};
    }
    // the .as(u8) in front of af::saveImageNative (main.cpp:235-237): a planar RGB image -> interleaved 8-bit pixels on the host,
    // packed on the device and downloaded as 3 bytes per pixel (wm.h wm_pack_rgb8)
    void packRgb8(const wm::Image& rgb, uint8_t* interleavedHost) const
    {
        const wm_plane prgb = rgb.plane();
        const wm_packed pk = packed(interleavedHost);
        const int rc = wm_pack_rgb8(ctx, &prgb, &pk, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "packRgb8");
    }
    // Samples of 9 to 16 bits (10-bit video; wm.h wm_unpack16 ...): dense host planes of the engine's shape, `channels` planar
    // planes of uint16 in the host's byte order, in the low bits of their 16 or, msbAligned, in the high bits (P010's Y plane).
    // unpack16: the f32 image on [0, 255] on the device, min(v, 2^bits - 1) * (float)(255.0 / (2^bits - 1))
    wm::Image unpack16(const uint16_t* host, int channels, int bits, bool msbAligned = false) const
    {
        wm::Image out(dims.rows, dims.cols, channels, wm::dtype::f32, device);
        const wm_plane src = plane16(const_cast<uint16_t*>(host), channels), po = out.plane();
        const int rc = wm_unpack16(ctx, &src, bits, msbAligned ? 1 : 0, &po, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "unpack16");
        return out;
    }
    // pack16: an f32 image -> samples on the host, clamped and rounded to nearest (ties to even); unpack16's inverse on every code
    void pack16(const wm::Image& image, uint16_t* host, int bits, bool msbAligned = false) const
    {
        const wm_plane src = image.plane(), po = plane16(host, image.channels());
        const int rc = wm_pack16(ctx, &src, &po, bits, msbAligned ? 1 : 0, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "pack16");
    }
    // makeWatermark of a grey `bits`-bit frame IN PLACE (wm.h wm_embed16: unpack, embed onto the frame itself, pack, one wait).
    // Returns the strength; a frame whose system is not solvable comes back unchanged and the strength is 0
    float makeWatermark16(uint16_t* hostY, int bits, MASK_TYPE maskType, bool msbAligned = false) const
    {
        const wm_plane py = plane16(hostY, 1);
        float a = 0.0f;
        int st = 0;
        const int rc = wm_embed16(ctx, (int)maskType, &py, &py, bits, msbAligned ? 1 : 0, &a, &st, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeWatermark16");
        return st != 0 ? 0.0f : a;
    }
    // detectWatermark of a grey `bits`-bit frame (wm.h wm_detect16); 0.0f when the prediction system is not solvable
    float detectWatermark16(const uint16_t* hostY, int bits, MASK_TYPE maskType, bool msbAligned = false) const
    {
        const wm_plane py = plane16(const_cast<uint16_t*>(hostY), 1);
        float corr = 0.0f;
        const int rc = wm_detect16(ctx, (int)maskType, &py, bits, msbAligned ? 1 : 0, &corr, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "detectWatermark16");
        return corr;
    }
    // PSNR and SSIM of `test` (a marked copy) against `ref` (its base), measured on the device (wm.h wm_quality): one entry per
    // channel.  The images are f32 or u8, independently, with the engine's shape and the same channel count (1 or 3)
    std::vector<wm::Quality> quality(const wm::Image& ref, const wm::Image& test) const
    {
        const wm_plane pr = ref.plane(), pt = test.plane();
        const size_t ch = (size_t)(ref.channels() > 0 ? ref.channels() : 0);
        std::vector<float> q(ch * WM_QUALITY_NVALS, 0.0f);
        const int rc = wm_quality(ctx, &pr, &pt, 0, 0, q.data(), nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "quality");
        std::vector<wm::Quality> out(ch);
        for (size_t c = 0; c < ch; ++c)
            out[c] = wm::Quality{q[3 * c], (float)wm_psnr_from_mse((double)q[3 * c], 255.0), q[3 * c + 1], q[3 * c + 2]};
        return out;
    }
    // detectWatermark of one grey image against every key of `keys` in one call (wm.h wm_detect_keys): score k is what
    // detectWatermark returns with key k as W (0.0f for every key when the prediction system is not solvable)
    std::vector<float> detectWatermarkKeys(const wm::Image& watermarkedImage, const WatermarkKeys& keys, MASK_TYPE maskType) const
    {
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> corr((size_t)keys.count(), 0.0f);
        const int rc = wm_detect_keys(ctx, (int)maskType, &pimg, keys.handle(), corr.data(), nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "detectWatermarkKeys");
        return corr;
    }
    // where does a cropped copy lie in its key?  detectWatermark of one grey image against the windows of key `k` of `keys` (planes
    // at least as large as the image) at the offsets (oy0 + i, ox0 + j), i < ny, j < nx, in one call (wm.h wm_detect_offsets):
    // score [i * nx + j] is what detectWatermark returns with that window as W.  The prediction filter smears the peak over the
    // 3x3 neighbourhood of the true offset: take the argmax
    std::vector<float> detectOffsets(const wm::Image& watermarkedImage, const WatermarkKeys& keys, int k, int oy0, int ox0, int ny, int nx,
                                     MASK_TYPE maskType) const
    {
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> corr((size_t)(ny > 0 ? ny : 0) * (size_t)(nx > 0 ? nx : 0), 0.0f);
        const int rc = wm_detect_offsets(ctx, (int)maskType, &pimg, keys.handle(), k, oy0, ox0, ny, nx, corr.data(), nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "detectOffsets");
        return corr;
    }
    // where does a cropped copy lie in its key, without a hint?  One grey image (or a batch: one entry per frame) cross-correlated
    // with key k of `keys` over EVERY admissible offset by FFT (wm.h wm_locate).  An unsolvable frame gives {0, 0, 0, 0};
    // detectOffsets with ny = nx = 1 at the offset found gives the score
    std::vector<WmLocation> locate(const wm::Image& watermarkedImage, const WatermarkKeys& keys, int k, MASK_TYPE maskType) const
    {
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> v((size_t)pimg.frames * WM_LOCATE_NVALS, 0.0f);
        const int rc = wm_locate(ctx, (int)maskType, &pimg, keys.handle(), k, v.data(), nullptr, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "locate");
        std::vector<WmLocation> out((size_t)pimg.frames);
        for (size_t f = 0; f < out.size(); ++f) out[f] = WmLocation{(int)v[4 * f], (int)v[4 * f + 1], v[4 * f + 2], v[4 * f + 3]};
        return out;
    }
    // whose key is in a cropped copy, and where?  locate of every frame against keys k0 .. k0 + nk - 1 of `keys` in one call, two keys
    // per transform (wm.h wm_locate_keys).  Frame-major: entry [frame * nk + j] is key k0 + j's; wm_locate_keys_rank names the owner
    // of a frame from the z of its nk entries.  A key plane that is all zero gives {0, 0, 0, NaN}, an unsolvable frame {0, 0, 0, 0}
    std::vector<WmLocation> locateKeys(const wm::Image& watermarkedImage, const WatermarkKeys& keys, int k0, int nk, MASK_TYPE maskType) const
    {
        const wm_plane pimg = watermarkedImage.plane();
        const size_t n = (size_t)pimg.frames * (size_t)(nk > 0 ? nk : 0);
        std::vector<float> v(n * WM_LOCATE_KEYS_NVALS + 1, 0.0f);  // (never an empty buffer: nk < 1 is the library's to refuse)
        const int rc = wm_locate_keys(ctx, (int)maskType, &pimg, keys.handle(), k0, nk, v.data(), nullptr, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "locateKeys");
        std::vector<WmLocation> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = WmLocation{(int)v[4 * i], (int)v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
        return out;
    }
    // locate for a cropped copy that carries a PAYLOAD (wm.h wm_locate_bits): tileBit holds one entry per tileRows x tileCols tile of
    // the KEY plane (-1: no bit).  Returns per frame the location on the energy map; soft [frame * nbits + b] > 0 reads bit b as set
    // (NaN: a bit without a tile)
    std::vector<WmLocation> locateBits(const wm::Image& watermarkedImage, const WatermarkKeys& keys, int k, int tileRows, int tileCols,
                                       const std::vector<int32_t>& tileBit, int nbits, MASK_TYPE maskType, std::vector<float>& soft) const
    {
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> v((size_t)pimg.frames * WM_LOCATE_BITS_NVALS, 0.0f);
        soft.assign((size_t)pimg.frames * (size_t)(nbits > 0 ? nbits : 0), 0.0f);
        int ty = 0, tx = 0;  // (a table shorter than the key plane's tile grid must not reach the library)
        if (wm_tiles_shape(wm_keys_rows(keys.handle()), wm_keys_cols(keys.handle()), tileRows, tileCols, &ty, &tx) == WM_OK &&
            tileBit.size() != (size_t)ty * (size_t)tx)
            fail(WM_ERR_BAD_ARG, "locateBits: tileBit must hold one entry per tile of the key plane");
        const int rc = wm_locate_bits(ctx, (int)maskType, &pimg, keys.handle(), k, tileRows, tileCols, tileBit.data(), nbits, v.data(), soft.data(),
                                      nullptr, nullptr, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "locateBits");
        std::vector<WmLocation> out((size_t)pimg.frames);
        for (size_t f = 0; f < out.size(); ++f) out[f] = WmLocation{(int)v[4 * f], (int)v[4 * f + 1], v[4 * f + 2], v[4 * f + 3]};
        return out;
    }
    // a clip's frames pooled on the image side (wm.h wm_clip_pool): poolDev, a dense DEVICE f32 [rows][cols] plane of the caller's,
    // becomes fmaf(w_f, h_f, pool) over the solvable frames of `clip` in ascending order, from zero unless `accumulate`; weights:
    // empty (all 1) or one per frame.  Returns the frames' statuses; a clip longer than max_frames is pooled in several calls
    std::vector<int> poolClip(const wm::Image& clip, MASK_TYPE maskType, float* poolDev, bool accumulate = false,
                              const std::vector<float>& weights = {}) const
    {
        const wm_plane pimg = clip.plane();
        if (!weights.empty() && weights.size() != (size_t)pimg.frames) fail(WM_ERR_BAD_ARG, "poolClip: weights must hold one entry per frame");
        std::vector<int> status((size_t)pimg.frames, 0);
        const int rc = wm_clip_pool(ctx, (int)maskType, &pimg, weights.empty() ? nullptr : weights.data(), poolDev, accumulate ? 1 : 0, status.data(),
                                    WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "poolClip");
        return status;
    }
    // locate, locateKeys and locateBits of a pooled clip (wm.h wm_locate_pooled, wm_locate_keys_pooled, wm_locate_bits_pooled): one
    // transform tail for the whole clip.  A pool without a solvable frame gives {0, 0, 0, NaN}
    WmLocation locatePooled(const float* poolDev, const WatermarkKeys& keys, int k) const
    {
        float v[WM_LOCATE_NVALS] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int rc = wm_locate_pooled(ctx, poolDev, keys.handle(), k, v, nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "locatePooled");
        return WmLocation{(int)v[0], (int)v[1], v[2], v[3]};
    }
    std::vector<WmLocation> locateKeysPooled(const float* poolDev, const WatermarkKeys& keys, int k0, int nk) const
    {
        const size_t n = (size_t)(nk > 0 ? nk : 0);
        std::vector<float> v(n * WM_LOCATE_KEYS_NVALS + 1, 0.0f);  // (never an empty buffer: nk < 1 is the library's to refuse)
        const int rc = wm_locate_keys_pooled(ctx, poolDev, keys.handle(), k0, nk, v.data(), nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "locateKeysPooled");
        std::vector<WmLocation> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = WmLocation{(int)v[4 * i], (int)v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
        return out;
    }
    WmLocation locateBitsPooled(const float* poolDev, const WatermarkKeys& keys, int k, int tileRows, int tileCols, const std::vector<int32_t>& tileBit,
                                int nbits, std::vector<float>& soft) const
    {
        float v[WM_LOCATE_BITS_NVALS] = {0.0f, 0.0f, 0.0f, 0.0f};
        soft.assign((size_t)(nbits > 0 ? nbits : 0), 0.0f);
        int ty = 0, tx = 0;  // (a table shorter than the key plane's tile grid must not reach the library)
        if (wm_tiles_shape(wm_keys_rows(keys.handle()), wm_keys_cols(keys.handle()), tileRows, tileCols, &ty, &tx) == WM_OK &&
            tileBit.size() != (size_t)ty * (size_t)tx)
            fail(WM_ERR_BAD_ARG, "locateBitsPooled: tileBit must hold one entry per tile of the key plane");
        const int rc = wm_locate_bits_pooled(ctx, poolDev, keys.handle(), k, tileRows, tileCols, tileBit.data(), nbits, v, soft.data(), nullptr, nullptr,
                                             WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "locateBitsPooled");
        return WmLocation{(int)v[0], (int)v[1], v[2], v[3]};
    }
    // where in the frame is the mark?  detectWatermark of one grey image against this engine's W with the correlation's three sums
    // kept per tile of tileRows x tileCols pixels (wm.h wm_detect_tiles; the last tile of each axis takes the remainder): score
    // [i * nx + j] is tile (i, j)'s, NaN for a tile without energy, 0 everywhere when the system is not solvable.  ny / nx, if
    // given, receive the tiles per axis (wm_tiles_shape)
    std::vector<float> detectTiles(const wm::Image& watermarkedImage, int tileRows, int tileCols, MASK_TYPE maskType, int* ny = nullptr,
                                   int* nx = nullptr) const
    {
        int ty = 0, tx = 0;
        int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        if (rc < 0) fail(rc, "detectTiles");
        if (ny) *ny = ty;
        if (nx) *nx = tx;
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> map((size_t)ty * (size_t)tx, 0.0f);
        float* dmap = static_cast<float*>(wm_dev_alloc(wm_device(ctx), map.size() * sizeof(float)));
        if (!dmap) fail(WM_ERR_ALLOC, "detectTiles");
        rc = wm_detect_tiles(ctx, (int)maskType, &pimg, tileRows, tileCols, dmap, nullptr, nullptr, WM_SLOT_SYNC);
        const int rd = rc < 0 ? WM_OK : wm_memcpy_d2h(map.data(), dmap, map.size() * sizeof(float));
        wm_dev_free(dmap);
        if (rc < 0) fail(rc, "detectTiles");
        if (rd < 0) fail(rd, "detectTiles");
        return map;
    }
    // whose mark is where?  detectTiles of one grey image with every key of `keys` in the place of this engine's W, in one call
    // (wm.h wm_detect_keys_tiles): score [(k * ny + i) * nx + j] is what detectTiles returns for tile (i, j) with key k as W.  The
    // argmax over k names the key a tile was marked with.  ny / nx, if given, receive the tiles per axis (wm_tiles_shape)
    std::vector<float> detectKeysTiles(const wm::Image& watermarkedImage, const WatermarkKeys& keys, int tileRows, int tileCols,
                                       MASK_TYPE maskType, int* ny = nullptr, int* nx = nullptr) const
    {
        int ty = 0, tx = 0;
        int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        if (rc < 0) fail(rc, "detectKeysTiles");
        if (ny) *ny = ty;
        if (nx) *nx = tx;
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> map((size_t)keys.count() * (size_t)ty * (size_t)tx, 0.0f);
        float* dmap = static_cast<float*>(wm_dev_alloc(wm_device(ctx), map.size() * sizeof(float)));
        if (!dmap) fail(WM_ERR_ALLOC, "detectKeysTiles");
        rc = wm_detect_keys_tiles(ctx, (int)maskType, &pimg, keys.handle(), tileRows, tileCols, dmap, nullptr, nullptr, WM_SLOT_SYNC);
        const int rd = rc < 0 ? WM_OK : wm_memcpy_d2h(map.data(), dmap, map.size() * sizeof(float));
        wm_dev_free(dmap);
        if (rc < 0) fail(rc, "detectKeysTiles");
        if (rd < 0) fail(rd, "detectKeysTiles");
        return map;
    }
    // a payload in the mark, one bit per tile (wm.h wm_bits_layout): the bit every tile of an ny x nx grid carries, 0 .. nbits - 1,
    // every bit on floor(T / nbits) or ceil(T / nbits) tiles spread over the frame by a shuffle seeded with `seed`
    static std::vector<int32_t> bitsLayout(int ny, int nx, int nbits, uint64_t seed)
    {
        std::vector<int32_t> tileBit((size_t)(ny > 0 ? ny : 0) * (size_t)(nx > 0 ? nx : 0));
        const int rc = wm_bits_layout(ny, nx, nbits, seed, tileBit.empty() ? nullptr : tileBit.data());
        if (rc < 0) throw std::runtime_error(std::string("bitsLayout: ") + wm_strerror(rc));
        return tileBit;
    }
    // makeWatermark with the watermark term of every pixel multiplied by the sign of its tile (wm.h wm_embed_signs): signs
    // [i * nx + j] in {-1, 0, +1} for tile (i, j) of wm_tiles_shape's grid.  Never the fused kernels; otherwise makeWatermark's rules
    wm::Image makeWatermarkSigns(const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, int tileRows, int tileCols,
                                 const std::vector<int8_t>& signs, MASK_TYPE maskType) const
    {
        int ty = 0, tx = 0;
        int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        if (rc < 0 || signs.size() != (size_t)ty * (size_t)tx) fail(WM_ERR_BAD_ARG, "makeWatermarkSigns");
        wm::Image out(outputImage.rows(), outputImage.cols(), outputImage.channels(), outputImage.type(), device);
        const wm_plane pin = inputImage.plane(), pbase = outputImage.plane(), pout = out.plane();
        float a = 0.0f;
        int st = 0;
        rc = wm_embed_signs(ctx, (int)maskType, &pin, &pbase, &pout, tileRows, tileCols, signs.data(), &a, &st, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeWatermarkSigns");
        if (st != 0) return outputImage;  // not solvable: output image without modification, strength untouched
        watermarkStrength = a;
        return out;
    }
    // makeWatermark that carries `payload` (wm.h wm_embed_bits): (nbits + 7) / 8 bytes, bit b = payload[b / 8] >> (b % 8) & 1; tile
    // t is marked with +W where bit tileBit[t] is set, with -W where it is not, and left unmarked where tileBit[t] = -1
    wm::Image makeWatermarkBits(const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, int tileRows, int tileCols,
                                const std::vector<int32_t>& tileBit, int nbits, const std::vector<uint8_t>& payload, MASK_TYPE maskType) const
    {
        int ty = 0, tx = 0;
        int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        if (rc < 0 || tileBit.size() != (size_t)ty * (size_t)tx || nbits < 1 || payload.size() != (size_t)(nbits + 7) / 8) fail(WM_ERR_BAD_ARG, "makeWatermarkBits");
        wm::Image out(outputImage.rows(), outputImage.cols(), outputImage.channels(), outputImage.type(), device);
        const wm_plane pin = inputImage.plane(), pbase = outputImage.plane(), pout = out.plane();
        float a = 0.0f;
        int st = 0;
        rc = wm_embed_bits(ctx, (int)maskType, &pin, &pbase, &pout, tileRows, tileCols, tileBit.data(), nbits, payload.data(), &a, &st, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeWatermarkBits");
        if (st != 0) return outputImage;
        watermarkStrength = a;
        return out;
    }
    // reads the payload back (wm.h wm_detect_bits): soft[b] is the score of the pooled tiles of bit b (0 when the system is not
    // solvable, NaN for a bit without a tile), the decoded bit is soft[b] > 0; `payload`, if given, receives the bits packed as
    // makeWatermarkBits takes them
    std::vector<float> detectBits(const wm::Image& watermarkedImage, int tileRows, int tileCols, const std::vector<int32_t>& tileBit, int nbits,
                                  MASK_TYPE maskType, std::vector<uint8_t>* payload = nullptr) const
    {
        int ty = 0, tx = 0;
        int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        if (rc < 0 || tileBit.size() != (size_t)ty * (size_t)tx || nbits < 1) fail(WM_ERR_BAD_ARG, "detectBits");
        const wm_plane pimg = watermarkedImage.plane();
        std::vector<float> soft((size_t)nbits, 0.0f);
        rc = wm_detect_bits(ctx, (int)maskType, &pimg, tileRows, tileCols, tileBit.data(), nbits, soft.data(), nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "detectBits");
        if (payload) {
            payload->assign((size_t)(nbits + 7) / 8, 0);
            for (int b = 0; b < nbits; ++b)
                if (soft[(size_t)b] > 0.0f) (*payload)[(size_t)b / 8] |= (uint8_t)(1u << (b % 8));
        }
        return soft;
    }
    // makeWatermark of one grey image with every key of `keys` as W in one call (wm.h wm_embed_keys): copy k is what
    // makeWatermark returns with key k as W, strengths[k] its strength.  Not solvable: every copy is `outputImage` itself and
    // `strengths` is left untouched (Watermark.cpp:164-165)
    std::vector<wm::Image> makeWatermarkKeys(const wm::Image& inputImage, const wm::Image& outputImage, const WatermarkKeys& keys,
                                             std::vector<float>& strengths, MASK_TYPE maskType) const
    {
        const int K = keys.count();
        std::vector<wm::Image> copies = wm::Image::stack(K, outputImage.rows(), outputImage.cols(), outputImage.channels(), outputImage.type(), device);
        const wm_plane pin = inputImage.plane(), pbase = outputImage.plane();
        wm_plane pout = copies[0].plane();
        pout.frames = K;
        pout.frame_stride = (int64_t)outputImage.elements();
        std::vector<float> a((size_t)K, 0.0f);
        int st = 0;
        const int rc = wm_embed_keys(ctx, (int)maskType, &pin, &pbase, keys.handle(), &pout, a.data(), &st, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeWatermarkKeys");
        if (st != 0) return std::vector<wm::Image>((size_t)K, outputImage);
        strengths = a;
        return copies;
    }
    // ---- a key per frame of a batch (wm.h wm_key_schedule, wm_embed_select, wm_detect_select).  A batch is a stack of images
    // (wm::Image::stack: one buffer, image i at i * elements()); the engine must have been configured for that many frames
    // (configure(nslots, maxFrames)).
    // which key does frame n of a video take?  Entry i is a function of (seed, firstFrame + i) alone, in 0 .. nkeys - 1
    static std::vector<int32_t> keySchedule(int nkeys, uint64_t seed, uint64_t firstFrame, int frames)
    {
        std::vector<int32_t> keyOfFrame((size_t)(frames > 0 ? frames : 0));
        const int rc = wm_key_schedule(nkeys, seed, firstFrame, frames, keyOfFrame.empty() ? nullptr : keyOfFrame.data());
        if (rc < 0) throw std::runtime_error(std::string("keySchedule: ") + wm_strerror(rc));
        return keyOfFrame;
    }
    void configure(int nslots, int maxFrames) const
    {
        const int rc = wm_configure(ctx, nslots, maxFrames);
        if (rc < 0) fail(rc, "configure");
    }
    // makeWatermark of image f of the stack with key keyOfFrame[f] of `keys` as W in one call: image f of the result is what
    // makeWatermark returns with that key as W, strengths[f] its strength.  An image that is not solvable comes back as its base,
    // bit for bit, and its strength is left as it was (Watermark.cpp:164-165); the context's own W is not used
    std::vector<wm::Image> makeWatermarkSelect(const std::vector<wm::Image>& inputStack, const std::vector<wm::Image>& outputStack,
                                               const WatermarkKeys& keys, const std::vector<int32_t>& keyOfFrame, std::vector<float>& strengths,
                                               MASK_TYPE maskType) const
    {
        const wm_plane pin = stackPlane(inputStack, "makeWatermarkSelect"), pbase = stackPlane(outputStack, "makeWatermarkSelect");
        const size_t F = inputStack.size();
        if (keyOfFrame.size() != F || outputStack.size() != F) fail(WM_ERR_BAD_ARG, "makeWatermarkSelect");
        const wm::Image& b0 = outputStack[0];
        std::vector<wm::Image> out = wm::Image::stack((int)F, b0.rows(), b0.cols(), b0.channels(), b0.type(), device);
        const wm_plane pout = stackPlane(out, "makeWatermarkSelect");
        std::vector<float> a(F, 0.0f);
        std::vector<int> st(F, 0);
        const int rc = wm_embed_select(ctx, (int)maskType, &pin, &pbase, &pout, keys.handle(), keyOfFrame.data(), a.data(), st.data(), WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeWatermarkSelect");
        strengths.resize(F, 0.0f);
        for (size_t f = 0; f < F; ++f)
            if (st[f] == 0) strengths[f] = a[f];
        return out;
    }
    // detectWatermark of image f of the stack against key keyOfFrame[f] of `keys` in one call: score f is what detectWatermark
    // returns with that key as W (0.0f where the prediction system is not solvable)
    std::vector<float> detectWatermarkSelect(const std::vector<wm::Image>& watermarkedStack, const WatermarkKeys& keys,
                                             const std::vector<int32_t>& keyOfFrame, MASK_TYPE maskType) const
    {
        const wm_plane pimg = stackPlane(watermarkedStack, "detectWatermarkSelect");
        if (keyOfFrame.size() != watermarkedStack.size()) fail(WM_ERR_BAD_ARG, "detectWatermarkSelect");
        std::vector<float> corr(keyOfFrame.size(), 0.0f);
        const int rc = wm_detect_select(ctx, (int)maskType, &pimg, keys.handle(), keyOfFrame.data(), corr.data(), nullptr, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "detectWatermarkSelect");
        return corr;
    }
    // the same two enqueued on `slot` (wm.h: planes of any memory kind, WM_MEM_SLOT_OUT included; keyOfFrame is copied before the
    // call returns; strengths / correlations [frames] and status [frames], may be null, are written by sync(slot); `keys` must stay
    // alive and unmodified until then)
    void makeWatermarkSelectAsync(const wm_plane& input, const wm_plane& base, const wm_plane& out, const WatermarkKeys& keys,
                                  const int32_t* keyOfFrame, float* strengths, int* status, MASK_TYPE maskType, int slot) const
    {
        const int rc = wm_embed_select(ctx, (int)maskType, &input, &base, &out, keys.handle(), keyOfFrame, strengths, status, slot);
        if (rc < 0) fail(rc, "makeWatermarkSelectAsync");
    }
    void detectWatermarkSelectAsync(const wm_plane& image, const WatermarkKeys& keys, const int32_t* keyOfFrame, float* correlations, int* status,
                                    MASK_TYPE maskType, int slot) const
    {
        const int rc = wm_detect_select(ctx, (int)maskType, &image, keys.handle(), keyOfFrame, correlations, status, slot);
        if (rc < 0) fail(rc, "detectWatermarkSelectAsync");
    }
    // waits for everything enqueued on `slot` and delivers its results: WM_OK, or WM_UNSOLVABLE when a frame's system was not solvable
    int sync(int slot) const
    {
        const int rc = wm_sync(ctx, slot);
        if (rc < 0) fail(rc, "sync");
        return rc;
    }
    // one image, K payload copies in one call (wm.h wm_embed_signs_multi): signs[k] is makeWatermarkSigns' table of copy k, copy k what
    // makeWatermarkSigns returns with it; ONE strength for all copies.  Not solvable: every copy is `outputImage` itself and
    // `watermarkStrength` is left untouched
    std::vector<wm::Image> makeWatermarkSignsMulti(const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, int tileRows,
                                                   int tileCols, const std::vector<std::vector<int8_t>>& signs, MASK_TYPE maskType) const
    {
        int ty = 0, tx = 0;
        const int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        const size_t T = (size_t)ty * (size_t)tx;
        if (rc < 0 || signs.empty()) fail(WM_ERR_BAD_ARG, "makeWatermarkSignsMulti");
        std::vector<int8_t> flat;
        for (const auto& s : signs) {
            if (s.size() != T) fail(WM_ERR_BAD_ARG, "makeWatermarkSignsMulti");
            flat.insert(flat.end(), s.begin(), s.end());
        }
        return embedMulti("makeWatermarkSignsMulti", inputImage, outputImage, watermarkStrength, (int)signs.size(), [&](const wm_plane* pin, const wm_plane* pbase, const wm_plane* pout, float* a, int* st) {
            return wm_embed_signs_multi(ctx, (int)maskType, pin, pbase, pout, tileRows, tileCols, (int)signs.size(), flat.data(), a, st, WM_SLOT_SYNC);
        });
    }
    // one image, K payloads in one call (wm.h wm_embed_bits_multi): payloads[k] is makeWatermarkBits' payload of copy k
    std::vector<wm::Image> makeWatermarkBitsMulti(const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, int tileRows,
                                                  int tileCols, const std::vector<int32_t>& tileBit, int nbits,
                                                  const std::vector<std::vector<uint8_t>>& payloads, MASK_TYPE maskType) const
    {
        int ty = 0, tx = 0;
        const int rc = wm_tiles_shape(wm_rows(ctx), wm_cols(ctx), tileRows, tileCols, &ty, &tx);
        if (rc < 0 || tileBit.size() != (size_t)ty * (size_t)tx || nbits < 1 || payloads.empty()) fail(WM_ERR_BAD_ARG, "makeWatermarkBitsMulti");
        std::vector<uint8_t> flat;
        for (const auto& p : payloads) {
            if (p.size() != (size_t)(nbits + 7) / 8) fail(WM_ERR_BAD_ARG, "makeWatermarkBitsMulti");
            flat.insert(flat.end(), p.begin(), p.end());
        }
        return embedMulti("makeWatermarkBitsMulti", inputImage, outputImage, watermarkStrength, (int)payloads.size(), [&](const wm_plane* pin, const wm_plane* pbase, const wm_plane* pout, float* a, int* st) {
            return wm_embed_bits_multi(ctx, (int)maskType, pin, pbase, pout, tileRows, tileCols, tileBit.data(), nbits, (int)payloads.size(), flat.data(), a, st,
                                       WM_SLOT_SYNC);
        });
    }
    // makeWatermark, then detectWatermark on its result (the pair testForImage runs per image, main.cpp:165-220), as ONE call:
    // same results, one wait (wm.h wm_embed_detect; grey output images)
    wm::Image makeAndDetectWatermark(const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, float& correlation,
                                     MASK_TYPE maskType) const
    {
        wm::Image out(outputImage.rows(), outputImage.cols(), outputImage.channels(), outputImage.type(), device);
        const wm_plane pin = inputImage.plane(), pbase = outputImage.plane(), pout = out.plane();
        float a = 0.0f, corr = 0.0f;
        int st = 0;
        const int rc = wm_embed_detect(ctx, (int)maskType, &pin, &pbase, &pout, &a, &corr, &st, WM_SLOT_SYNC);
        if (rc < 0) fail(rc, "makeAndDetectWatermark");
        correlation = corr;
        if (st != 0) return outputImage;
        watermarkStrength = a;
        return out;
    }
    // names used by BASELINE.json's north_star
    wm::Image embed(const wm::Image& in, const wm::Image& out, float& a, MASK_TYPE m) const { return makeWatermark(in, out, a, m); }
    float detect(const wm::Image& img, MASK_TYPE m) const { return detectWatermark(img, m); }

    // opt-in: batched embeds of grey f32 images leave the lag sums of their output for a detector that reads it as
    // WM_MEM_SLOT_OUT through the slot interface of wm.h (wm_set_handover); no effect on the synchronous methods above
    void setHandover(bool on) const
    {
        const int rc = wm_set_handover(ctx, on ? 1 : 0);
        if (rc < 0) fail(rc, "setHandover");
    }
    wm_ctx* handle() const { return ctx; }  // for callers that want the asynchronous slot interface of wm.h
    dim2 size() const { return dims; }

private:
    dim2 dims;
    int p;
    float psnr;
    int device;
    wm_ctx* ctx = nullptr;

    void fail(int rc, const char* where) const
    {
        throw std::runtime_error(std::string("ERROR in ") + where + ": " + wm_strerror(rc) + " " + (ctx ? wm_last_error(ctx) : "") +
                                 " Error code: " + std::to_string(rc) + "\n");
    }
    // a dense host buffer of `channels` planar uint16 planes of the engine's shape as wm_plane
    wm_plane plane16(uint16_t* host, int channels) const
    {
        wm_plane pl{};
        pl.data = host; pl.rows = (int32_t)dims.rows; pl.cols = (int32_t)dims.cols; pl.channels = channels; pl.dtype = WM_U16; pl.mem = WM_MEM_HOST;
        pl.frames = 1; pl.pitch = dims.cols; pl.channel_stride = dims.rows * dims.cols; pl.frame_stride = 0;
        return pl;
    }
    // a stack of images (wm::Image::stack) as one batched plane: every image of the first one's shape, image i at i * elements()
    wm_plane stackPlane(const std::vector<wm::Image>& v, const char* where) const
    {
        if (v.empty() || v[0].isempty()) fail(WM_ERR_BAD_ARG, where);
        wm_plane pl = v[0].plane();
        for (size_t i = 0; i < v.size(); ++i) {
            const wm::Image& im = v[i];
            if (im.rows() != v[0].rows() || im.cols() != v[0].cols() || im.channels() != v[0].channels() || im.type() != v[0].type() ||
                static_cast<const char*>(im.device_ptr()) != static_cast<const char*>(v[0].device_ptr()) + i * v[0].bytes())
                fail(WM_ERR_BAD_ARG, where);
        }
        pl.frames = (int32_t)v.size();
        pl.frame_stride = (int64_t)v[0].elements();
        return pl;
    }
    // a dense interleaved host buffer of the engine's shape as wm_packed
    wm_packed packed(uint8_t* interleavedHost) const
    {
        wm_packed pk{};
        pk.data = interleavedHost; pk.rows = (int32_t)dims.rows; pk.cols = (int32_t)dims.cols; pk.mem = WM_MEM_HOST; pk.frames = 1;
        pk.pitch_bytes = 3 * (int64_t)dims.cols; pk.frame_stride_bytes = 0;
        return pk;
    }
    // the *Multi embeds around their C call: K stacked copies of one image as makeWatermarkKeys stacks them, one strength
    template <typename Call>
    std::vector<wm::Image> embedMulti(const char* where, const wm::Image& inputImage, const wm::Image& outputImage, float& watermarkStrength, int K,
                                      Call&& call) const
    {
        std::vector<wm::Image> copies = wm::Image::stack(K, outputImage.rows(), outputImage.cols(), outputImage.channels(), outputImage.type(), device);
        const wm_plane pin = inputImage.plane(), pbase = outputImage.plane();
        wm_plane pout = copies[0].plane();
        pout.frames = K;
        pout.frame_stride = (int64_t)outputImage.elements();
        float a = 0.0f;
        int st = 0;
        const int rc = call(&pin, &pbase, &pout, &a, &st);
        if (rc < 0) fail(rc, where);
        if (st != 0) return std::vector<wm::Image>((size_t)K, outputImage);
        watermarkStrength = a;
        return copies;
    }
    void check(int rc, const char* where) const
    {
        if (rc != WM_OK) fail(rc, where);
    }
    static void check_w(int rc, const std::string& path, dim_t rows, dim_t cols)
    {
        if (rc == WM_OK) return;
        if (rc == WM_ERR_W_OPEN)  // Watermark.cpp:65-66
            throw std::runtime_error(std::string("Error opening '" + path + "' file for Random noise W array\n"));
        if (rc == WM_ERR_W_SIZE) {  // Watermark.cpp:70-71
            std::ifstream f(path.c_str(), std::ios::binary);
            f.seekg(0, std::ios::end);
            const long long total = (long long)f.tellg();
            throw std::runtime_error(std::string("Error: W file total elements != image dimensions! W file total elements: " +
                                                 std::to_string(total / (long long)sizeof(float)) + ", Image width: " + std::to_string(cols) +
                                                 ", Image height: " + std::to_string(rows) + "\n"));
        }
        if (rc == WM_ERR_BAD_P) throw std::runtime_error("Wrong p parameter!\n");
        throw std::runtime_error(std::string("Watermark: ") + wm_strerror(rc) + "\n");
    }
};
