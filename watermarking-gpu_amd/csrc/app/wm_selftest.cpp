// wm_selftest: the reference's class surface exercised from C++ (include/Watermark.hpp over libwm_hip.so):
// constructor errors with the reference's messages, deep copies that share W, reinitialize, the embed()/detect()
// aliases, RGB bases, the unsolvable-system rule.  Prints one line per check; exit code = number of failed checks.
//   wm_selftest <work_dir>      (work_dir receives two generated W files)
#include "../../../include/Watermark.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond, what)                                                     \
    do {                                                                      \
        const bool ok_ = (cond);                                              \
        std::printf("%s  %s\n", ok_ ? "ok  " : "FAIL", what);                 \
        if (!ok_) ++failures;                                                 \
    } while (0)

static uint32_t hash32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
static float unit(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

static std::vector<float> make_w(int rows, int cols, uint32_t seed)
{
    std::vector<float> w((size_t)rows * cols);
    for (size_t i = 0; i < w.size(); ++i) {
        const float u1 = unit(hash32(seed + 2u * (uint32_t)i)) + 1e-7f, u2 = unit(hash32(seed + 2u * (uint32_t)i + 1u));
        w[i] = std::sqrt(-2.0f * std::log(u1)) * std::cos(6.2831853f * u2);
    }
    return w;
}
static std::vector<float> make_frame(int rows, int cols, uint32_t seed)
{
    std::vector<float> x((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            x[(size_t)r * cols + c] = 128.0f + 60.0f * std::sin(r * 0.07f) * std::cos(c * 0.05f) + 30.0f * (unit(hash32(seed + (uint32_t)(r * cols + c))) - 0.5f);
    return x;
}
static void write_w(const std::string& path, const std::vector<float>& w)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(w.data()), (std::streamsize)(w.size() * sizeof(float)));
}
template <typename F>
static std::string message_of(F&& f)
{
    try { f(); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int R = 96, C = 300, R2 = 130, C2 = 260;
    const std::string w1 = dir + "/w_96x300.dat", w2 = dir + "/w_130x260.dat";
    write_w(w1, make_w(R, C, 11));
    write_w(w2, make_w(R2, C2, 12));

    // ---- constructor errors (Watermark.cpp:24-25, 65-66, 70-71)
    CHECK(message_of([&] { Watermark w(R, C, w1, 4, 40.0f); }).find("Wrong p parameter: 4") != std::string::npos, "p = 4 is rejected with the reference's message");
    CHECK(message_of([&] { Watermark w(R, C, dir + "/missing.dat", 3, 40.0f); }).find("Error opening") != std::string::npos, "missing W file");
    CHECK(message_of([&] { Watermark w(R, C, w2, 3, 40.0f); }).find("W file total elements != image dimensions") != std::string::npos, "W file of another size");

    // ---- embed / detect, aliases
    Watermark wm1(R, C, w1, 3, 40.0f);
    const std::vector<float> x = make_frame(R, C, 5);
    const wm::Image gray = wm::Image::fromHost(x.data(), R, C, 1);
    float a_me = -1.0f, a_nvf = -1.0f, a_alias = -1.0f;
    const wm::Image y_me = wm1.makeWatermark(gray, gray, a_me, ME);
    const wm::Image y_nvf = wm1.makeWatermark(gray, gray, a_nvf, NVF);
    const wm::Image y_alias = wm1.embed(gray, gray, a_alias, ME);
    const float c_me = wm1.detectWatermark(y_me, ME), c_nvf = wm1.detectWatermark(y_nvf, NVF);
    CHECK(a_me > 0.0f && a_nvf > 0.0f && a_alias == a_me, "strengths are set; embed() is makeWatermark()");
    CHECK(c_me > 0.2f && c_nvf > 0.1f && wm1.detect(y_me, ME) == c_me, "marked images correlate; detect() is detectWatermark()");
    CHECK(std::fabs(wm1.detectWatermark(gray, ME)) < 0.05f, "an unmarked image does not");
    std::vector<float> yh((size_t)R * C), yh2((size_t)R * C);
    y_me.host(yh.data());
    {
        // the pair as one call (an addition to the reference's class): the same image, strength and score as the two calls
        float a_pair = -1.0f, c_pair = -1.0f;
        const wm::Image y_pair = wm1.makeAndDetectWatermark(gray, gray, a_pair, c_pair, ME);
        y_pair.host(yh2.data());
        CHECK(a_pair == a_me && std::fabs(c_pair - c_me) <= 2e-7f && yh2 == yh, "makeAndDetectWatermark: the two calls' results in one");
        wm1.setHandover(true);   // (no effect on the synchronous methods; the switch itself must work)
        float a_ho = -1.0f;
        const wm::Image y_ho = wm1.makeWatermark(gray, gray, a_ho, ME);
        CHECK(a_ho == a_me && wm1.detectWatermark(y_ho, ME) == c_me, "setHandover leaves the synchronous calls as they are");
        wm1.setHandover(false);
    }
    double mse = 0.0;
    for (size_t i = 0; i < yh.size(); ++i) mse += ((double)yh[i] - x[i]) * ((double)yh[i] - x[i]);
    const double psnr = 10.0 * std::log10(255.0 * 255.0 / (mse / (double)yh.size()));
    CHECK(std::fabs(psnr - 40.0) < 0.2, "the embed hits the requested PSNR");
    {
        // the same figure from the device (wm_quality): the host loop's mse to f32 rounding, an SSIM in (0.9, 1), and 1 for a copy
        const std::vector<wm::Quality> q = wm1.quality(gray, y_me), same = wm1.quality(gray, gray);
        const bool measured = q.size() == 1 && std::fabs((double)q[0].mse - mse / (double)yh.size()) <= 1e-6 * (double)q[0].mse &&
                              std::fabs((double)q[0].psnr - psnr) < 1e-4 && q[0].ssim > 0.9f && q[0].ssim < 1.0f && q[0].maxAbs > 0.0f;
        const bool identical = same.size() == 1 && same[0].mse == 0.0f && std::isinf(same[0].psnr) && same[0].ssim == 1.0f && same[0].maxAbs == 0.0f;
        CHECK(measured && identical, "quality: the device's mse, PSNR and SSIM of the marked image; a copy scores mse 0, SSIM 1");
    }

    // ---- RGB base: the same a*u is added to the three channels (main.cpp:169-190)
    std::vector<float> rgb((size_t)3 * R * C);
    for (int ch = 0; ch < 3; ++ch)
        for (size_t i = 0; i < x.size(); ++i) rgb[(size_t)ch * R * C + i] = std::fmin(255.0f, std::fmax(0.0f, x[i] + 10.0f * (ch - 1)));
    const wm::Image base = wm::Image::fromHost(rgb.data(), R, C, 3);
    float a_rgb = 0.0f;
    const wm::Image y_rgb = wm1.makeWatermark(gray, base, a_rgb, ME);
    std::vector<float> yr((size_t)3 * R * C);
    y_rgb.host(yr.data());
    bool rgb_ok = y_rgb.channels() == 3 && a_rgb == a_me;
    for (size_t i = 0; i < x.size() && rgb_ok; i += 97) {
        const float d0 = yr[i] - rgb[i], d1 = yr[(size_t)R * C + i] - rgb[(size_t)R * C + i];
        if (rgb[i] > 40.f && rgb[i] < 215.f && std::fabs(d0 - d1) > 1e-3f) rgb_ok = false;
    }
    CHECK(rgb_ok, "RGB base: 3 channels out, same strength, same increment per channel");

    // ---- the pixel-format front: interleaved bytes up, planes and grey on the device, the grey of the result, packed bytes down
    {
        std::vector<uint8_t> px((size_t)3 * R * C), px_back(px.size()), px_marked(px.size());
        for (size_t i = 0; i < x.size(); ++i)
            for (int ch = 0; ch < 3; ++ch) px[3 * i + ch] = (uint8_t)rgb[(size_t)ch * R * C + i];
        const std::pair<wm::Image, wm::Image> up = wm1.unpackRgb8(px.data(), true);
        std::vector<float> planar((size_t)3 * R * C), g((size_t)R * C), g2(g.size());
        up.first.host(planar.data());
        up.second.host(g.data());
        wm1.rgb2gray(up.first).host(g2.data());
        bool planes_ok = up.first.channels() == 3 && up.second.channels() == 1, gray_ok = g == g2;
        for (size_t i = 0; i < g.size(); ++i) {
            for (int ch = 0; ch < 3; ++ch) planes_ok = planes_ok && planar[(size_t)ch * R * C + i] == (float)px[3 * i + ch];
            gray_ok = gray_ok && g[i] == (0.299f * px[3 * i] + 0.587f * px[3 * i + 1]) + 0.114f * px[3 * i + 2];
        }
        CHECK(planes_ok, "unpackRgb8: the planes are the source bytes");
        CHECK(gray_ok, "unpackRgb8 / rgb2gray: (0.299 R + 0.587 G) + 0.114 B in f32, the same bits from both");
        wm1.packRgb8(up.first, px_back.data());
        CHECK(px_back == px, "packRgb8 of the unpacked planes returns the bytes");
        float a_px = 0.0f;
        const wm::Image y_px = wm1.makeWatermark(up.second, up.first, a_px, ME);
        const float c_px = wm1.detectWatermark(wm1.rgb2gray(y_px), ME);
        std::vector<float> yp((size_t)3 * R * C);
        y_px.host(yp.data());
        wm1.packRgb8(y_px, px_marked.data());
        bool cast_ok = true;
        for (size_t i = 0; i < g.size(); ++i)
            for (int ch = 0; ch < 3; ++ch) cast_ok = cast_ok && px_marked[3 * i + ch] == (uint8_t)yp[(size_t)ch * R * C + i];
        CHECK(a_px > 0.0f && c_px > 0.2f, "RGB round on the device: embed on the unpacked base, detect on the grey of the result");
        CHECK(cast_ok, "packRgb8 of a watermarked image is the cast to 8 bits");
    }

    // ---- 10-bit samples: every code survives unpack16 / pack16, makeWatermark16 marks a frame in place, detectWatermark16 finds it
    {
        std::vector<uint16_t> v((size_t)R * C), back(v.size()), marked;
        for (size_t i = 0; i < v.size(); ++i) v[i] = (uint16_t)std::lrint(x[i] * (1023.0f / 255.0f));
        for (size_t i = 0; i < 1024; ++i) v[i] = (uint16_t)i;
        const wm::Image up = wm1.unpack16(v.data(), 1, 10);
        std::vector<float> g((size_t)R * C);
        up.host(g.data());
        wm1.pack16(up, back.data(), 10);
        CHECK(g[0] == 0.0f && g[1023] == 255.0f && back == v, "unpack16 / pack16: full scale is 255, every 10-bit code comes back");
        marked = v;
        const float a16 = wm1.makeWatermark16(marked.data(), 10, ME);
        const float c16 = wm1.detectWatermark16(marked.data(), 10, ME);
        CHECK(a16 > 0.0f && marked != v && c16 > 0.2f && std::fabs(wm1.detectWatermark16(v.data(), 10, ME)) < 0.05f,
              "makeWatermark16 in place, detectWatermark16: the marked samples correlate, the source does not");
    }

    // ---- a key per frame: 3 generated keys, 4 frames with a schedule, embed, detect on the slot's output with the right schedule and
    // with the schedule rotated by one key
    {
        const int K = 3, F = 4;
        WatermarkKeys keys(R, C, K);
        for (int k = 0; k < K; ++k) keys.generate(k, 700u + (uint32_t)k);
        Watermark sel(R, C, w1, 3, 40.0f);  // (its own W is not used)
        sel.configure(2, F);
        const std::vector<int32_t> sched = Watermark::keySchedule(K, 2024, 100, F);
        std::vector<int32_t> rotated(sched);
        for (auto& k : rotated) k = (k + 1) % K;
        std::vector<wm::Image> frames = wm::Image::stack(F, R, C, 1);
        for (int f = 0; f < F; ++f) {
            const std::vector<float> xf = make_frame(R, C, 40u + (uint32_t)f);
            if (wm_memcpy_h2d(frames[(size_t)f].device_ptr(), xf.data(), xf.size() * sizeof(float)) != WM_OK) ++failures;
        }
        std::vector<float> a_sel;
        const std::vector<wm::Image> marked = sel.makeWatermarkSelect(frames, frames, keys, sched, a_sel, ME);
        // the detector reads the device copy of what the embed wrote (WM_MEM_SLOT_OUT), enqueued on slot 0
        wm_plane slot_out = marked[0].plane();
        slot_out.data = nullptr; slot_out.mem = WM_MEM_SLOT_OUT; slot_out.frames = F; slot_out.frame_stride = (int64_t)marked[0].elements();
        std::vector<float> right((size_t)F, 0.0f), wrong((size_t)F, 0.0f);
        sel.detectWatermarkSelectAsync(slot_out, keys, sched.data(), right.data(), nullptr, ME, 0);
        sel.detectWatermarkSelectAsync(slot_out, keys, rotated.data(), wrong.data(), nullptr, ME, 0);
        sel.sync(0);
        const std::vector<float> again = sel.detectWatermarkSelect(marked, keys, sched, ME);
        bool sched_ok = (int)sched.size() == F, split = true, strengths = (int)a_sel.size() == F;
        for (int f = 0; f < F; ++f) {
            sched_ok = sched_ok && sched[(size_t)f] >= 0 && sched[(size_t)f] < K && Watermark::keySchedule(K, 2024, 100 + (uint64_t)f, 1)[0] == sched[(size_t)f];
            strengths = strengths && a_sel[(size_t)f] > 0.0f;
            split = split && right[(size_t)f] > 0.2f && std::fabs(wrong[(size_t)f]) < 0.05f && again[(size_t)f] == right[(size_t)f];
            std::printf("      frame %d key %d: a = %.4f, score %.4f, with key %d %.4f\n", f, (int)sched[(size_t)f], a_sel[(size_t)f], right[(size_t)f],
                        (int)rotated[(size_t)f], wrong[(size_t)f]);
        }
        CHECK(sched_ok, "keySchedule: entries in range, a clip's schedule follows from its first frame");
        CHECK(strengths, "makeWatermarkSelect: one strength per frame");
        CHECK(split, "detectWatermarkSelect: the right schedule correlates, the rotated one does not; slot output and stack agree");
    }

    // ---- deep copy that shares W (Watermark.cpp:30-51): same results, independent lifetime
    float a_copy = 0.0f, a_assign = 0.0f;
    {
        Watermark copy(wm1);
        const wm::Image yc = copy.makeWatermark(gray, gray, a_copy, ME);
        yc.host(yh2.data());
        CHECK(a_copy == a_me && yh2 == yh && copy.detectWatermark(yc, ME) == c_me, "copy constructor: identical results");
    }
    Watermark other(R2, C2, w2, 3, 40.0f);
    other = wm1;
    const wm::Image ya = other.makeWatermark(gray, gray, a_assign, ME);
    CHECK(a_assign == a_me && other.size().rows == R && other.size().cols == C, "copy assignment replaces the engine");
    float a_after = 0.0f;
    wm1.makeWatermark(gray, gray, a_after, ME);
    CHECK(a_after == a_me, "the original still works after its copy was destroyed");

    // ---- reinitialize (Watermark.cpp:78-85)
    wm1.reinitialize(w2, R2, C2);
    const std::vector<float> x2 = make_frame(R2, C2, 6);
    const wm::Image gray2 = wm::Image::fromHost(x2.data(), R2, C2, 1);
    float a2 = 0.0f;
    const wm::Image y2 = wm1.makeWatermark(gray2, gray2, a2, ME);
    CHECK(a2 > 0.0f && wm1.detectWatermark(y2, ME) > 0.2f && y2.rows() == R2 && y2.cols() == C2, "reinitialize: new size, new W");
    CHECK(message_of([&] { float t; wm1.makeWatermark(gray, gray, t, ME); }).find("ERROR in makeWatermark") != std::string::npos, "an image of the old size is refused");
    CHECK(message_of([&] { wm1.reinitialize(w1, R2, C2); }).find("W file total elements != image dimensions") != std::string::npos, "reinitialize checks the W file size");

    // ---- unsolvable system (Watermark.cpp:164-165, 246-247): constant image
    const std::vector<float> flat((size_t)R2 * C2, 77.0f);
    const wm::Image fl = wm::Image::fromHost(flat.data(), R2, C2, 1);
    float a_flat = -123.0f;
    const wm::Image y_flat = wm1.makeWatermark(fl, fl, a_flat, ME);
    CHECK(a_flat == -123.0f && y_flat.same_buffer(fl), "unsolvable: the output image is returned as is, the strength is untouched");
    CHECK(wm1.detectWatermark(fl, ME) == 0.0f, "unsolvable: detect returns 0.0f");

    std::printf("%d check(s) failed\n", failures);
    return failures;
}
