// mi_cv.hpp -- header-only C++ adapter: the reference's cv::Mat-in / cv::Mat-out call surface on top
// of the C ABI (include/mi_lumaeq.h).  This is the host-side mirror of the interface the reference
// programs use for the hot path:
//
//   cv::equalizeHist(y_plane_in, y_plane_out);                       OpenCVequalHist.cpp:145
//   cv::equalizeHist(y_in /*view on input buffer*/, y_out /*view on output buffer*/);
//                                                                    nextimprovement.cpp:164-168
//   clahe = cv::createCLAHE(clip, cv::Size(t, t));                   clahevideo.cpp:184, :497
//   clahe->setClipLimit(..); clahe->setTilesGridSize(..);            clahevideo.cpp:187-188
//   clahe->apply(y_in /*ROI view, step = width*/, y_out);            clahevideo.cpp:195
//
// Semantics kept: src must be 8-bit single channel, otherwise an exception derived
// from std::exception is thrown (callers catch `const std::exception&`, OpenCVequalHist.cpp:189,
// clahevideo.cpp:273); an empty src is a no-op; dst is (re)created ONLY if its size/type does not
// already match, so a dst that wraps caller memory is written in place and never reallocated;
// src/dst may be ROI views (step > width) and may alias; the call is synchronous.
//
// Two front ends, same functions:
//   * namespace micv  -- a small self-contained Mat/Size/Rect/Ptr so the adapter (and its tests)
//     work where OpenCV is not installed (it is not in the authoring image);
//   * if <opencv2/core.hpp> is present and MI_CV_WITH_OPENCV is defined, overloads taking real
//     cv::Mat (`mi_cv::equalizeHist(const cv::Mat&, cv::Mat&)`, `mi_cv::createCLAHE`) are added;
//     a reference program switches by replacing `cv::equalizeHist` with `mi_cv::equalizeHist`
//     (INTEGRATION.md).
//
// Each calling thread lazily owns one mi_ctx per device ("one context per worker", the shape of
// OpenCLequalHist.cpp:142-152), so equalizeHist() is re-entrant across the reference's worker
// threads; a CLAHE object is not shared between threads (as in OpenCV).
#ifndef MI_CV_HPP_
#define MI_CV_HPP_

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mi_lumaeq.h"

namespace micv {

// ---- type codes (values as in OpenCV's interface.h so they mean the same thing to a reader) ----
constexpr int CV_8U = 0, CV_16U = 2, CV_32F = 5;
constexpr int MI_CN_SHIFT = 3;
constexpr int makeType(int depth, int cn) { return (depth & 7) + ((cn - 1) << MI_CN_SHIFT); }
constexpr int CV_8UC1 = makeType(CV_8U, 1), CV_8UC3 = makeType(CV_8U, 3), CV_16UC1 = makeType(CV_16U, 1),
              CV_32FC1 = makeType(CV_32F, 1);
inline int elemSizeOf(int type)
{
    static const int depth_bytes[8] = {1, 1, 2, 2, 4, 4, 8, 2};
    return depth_bytes[type & 7] * ((type >> MI_CN_SHIFT) + 1);
}

// ---- error type: mirrors cv::Exception's fields; derives from std::exception ----
class Exception : public std::exception {
public:
    Exception(int code_, std::string err_, std::string func_, std::string file_, int line_)
        : code(code_), err(std::move(err_)), func(std::move(func_)), file(std::move(file_)), line(line_)
    {
        msg = "mi_cv(" + std::to_string(code) + ") " + file + ":" + std::to_string(line) + ": error: " + err + " in function '" + func + "'";
    }
    const char* what() const noexcept override { return msg.c_str(); }
    int code;
    std::string err, func, file, msg;
    int line;
};
// OpenCV's numeric codes for the two cases that can occur on this path
constexpr int StsAssert = -215, StsBadArg = -5, StsNoMem = -4, GpuApiCallError = -217, GpuNotSupported = -216;

#define MI_CV_ERROR(code, text) throw ::micv::Exception((code), (text), __func__, __FILE__, __LINE__)
#define MI_CV_ASSERT(expr) \
    do { if (!(expr)) MI_CV_ERROR(::micv::StsAssert, #expr); } while (0)

struct Size {
    int width = 0, height = 0;
    Size() = default;
    Size(int w, int h) : width(w), height(h) {}
    int area() const { return width * height; }
    bool operator==(const Size& o) const { return width == o.width && height == o.height; }
    bool operator!=(const Size& o) const { return !(*this == o); }
};
struct Rect {
    int x = 0, y = 0, width = 0, height = 0;
    Rect() = default;
    Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

template <class T> using Ptr = std::shared_ptr<T>;

// ---- Mat: 2-D, reference counted when it owns memory, a plain view when it wraps caller memory ----
class Mat {
public:
    static constexpr size_t AUTO_STEP = 0;
    int rows = 0, cols = 0;
    size_t step = 0;
    unsigned char* data = nullptr;

    Mat() = default;
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(Size s, int type) { create(s.height, s.width, type); }
    // wraps external memory (no copy, never freed): cv::Mat(rows, cols, type, data, step)
    Mat(int r, int c, int type, void* ext, size_t step_ = AUTO_STEP)
        : rows(r), cols(c), step(step_ == AUTO_STEP ? (size_t)c * elemSizeOf(type) : step_), data((unsigned char*)ext), type_(type)
    {
        MI_CV_ASSERT(r >= 0 && c >= 0 && step >= (size_t)c * elemSizeOf(type));
    }
    // ROI view: cv::Mat(const Mat&, const Rect&)
    Mat(const Mat& m, const Rect& roi) : rows(roi.height), cols(roi.width), step(m.step), type_(m.type_), owner_(m.owner_)
    {
        MI_CV_ASSERT(0 <= roi.x && 0 <= roi.width && roi.x + roi.width <= m.cols && 0 <= roi.y && 0 <= roi.height && roi.y + roi.height <= m.rows);
        data = m.data + (size_t)roi.y * m.step + (size_t)roi.x * elemSizeOf(m.type_);
    }
    Mat operator()(const Rect& roi) const { return Mat(*this, roi); }

    // (re)allocate only when size or type differ -- Mat::create semantics
    void create(int r, int c, int type)
    {
        MI_CV_ASSERT(r >= 0 && c >= 0);
        if (data && rows == r && cols == c && type_ == type) return;
        rows = r; cols = c; type_ = type; step = (size_t)c * elemSizeOf(type);
        const size_t bytes = step * (size_t)r;
        if (bytes == 0) { owner_.reset(); data = nullptr; return; }
        void* p = nullptr;
        if (posix_memalign(&p, 64, bytes) != 0) MI_CV_ERROR(StsNoMem, "allocation failed");
        owner_ = std::shared_ptr<unsigned char>((unsigned char*)p, [](unsigned char* q) { free(q); });
        data = owner_.get();
    }
    void create(Size s, int type) { create(s.height, s.width, type); }

    int type() const { return type_; }
    int channels() const { return (type_ >> MI_CN_SHIFT) + 1; }
    int depth() const { return type_ & 7; }
    size_t elemSize() const { return (size_t)elemSizeOf(type_); }
    Size size() const { return Size(cols, rows); }
    size_t total() const { return (size_t)rows * cols; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    bool isContinuous() const { return rows <= 1 || step == (size_t)cols * elemSize(); }
    unsigned char* ptr(int y = 0) { return data + (size_t)y * step; }
    const unsigned char* ptr(int y = 0) const { return data + (size_t)y * step; }
    bool ownsMemory() const { return (bool)owner_; }

    Mat clone() const
    {
        Mat m;
        copyTo(m);
        return m;
    }
    void copyTo(Mat& dst) const
    {
        if (empty()) { dst = Mat(); return; }
        dst.create(rows, cols, type_);
        const size_t rb = (size_t)cols * elemSize();
        for (int y = 0; y < rows; ++y) memcpy(dst.ptr(y), ptr(y), rb);
    }
    Mat& setTo(unsigned char v)
    {
        const size_t rb = (size_t)cols * elemSize();
        for (int y = 0; y < rows; ++y) memset(ptr(y), v, rb);
        return *this;
    }

private:
    int type_ = CV_8UC1;
    std::shared_ptr<unsigned char> owner_;
};

// ---- per-thread contexts ----
namespace detail {
struct CtxDeleter { void operator()(mi_ctx* c) const { mi_ctx_destroy(c); } };
inline int& tls_device() { static thread_local int dev = 0; return dev; }
inline mi_ctx* thread_ctx()
{
    static thread_local std::map<int, std::unique_ptr<mi_ctx, CtxDeleter>> ctxs;
    const int dev = tls_device();
    auto it = ctxs.find(dev);
    if (it == ctxs.end()) {
        mi_ctx* c = nullptr;
        const mi_status st = mi_ctx_create(dev, &c);
        if (st != MI_OK)
            MI_CV_ERROR(st == MI_ERR_NO_DEVICE ? GpuNotSupported : GpuApiCallError,
                        std::string("mi_ctx_create(device=") + std::to_string(dev) + ") failed: " + mi_status_str(st) +
                            " (this backend has no CPU fallback)");
        it = ctxs.emplace(dev, std::unique_ptr<mi_ctx, CtxDeleter>(c)).first;
        // CLAHE's float steps as the program's OWN OpenCV build computes them: 0 = every multiply and add rounded (x86-64 baseline
        // builds, the default), 1 = GCC's FMA contraction (aarch64 builds such as the reference's board).  For programs that cannot
        // call setOption themselves -- an unmodified binary under the LD_PRELOAD interposer -- the environment decides;
        // tests/cxx/test_adapter_opencv finds out which of the two a given OpenCV needs.
        if (const char* e = std::getenv("MI_CV_CLAHE_FP_CONTRACT")) (void)mi_ctx_set_option(c, "clahe_fp_contract", std::atoi(e) != 0);
    }
    return it->second.get();
}
inline void check(mi_ctx* c, mi_status st, const char* what)
{
    if (st == MI_OK) return;
    const std::string detail = std::string(what) + ": " + mi_status_str(st) + " (" + mi_ctx_last_error_msg(c) + ")";
    switch (st) {
        case MI_ERR_BAD_ARG: MI_CV_ERROR(StsBadArg, detail);
        case MI_ERR_UNSUPPORTED: MI_CV_ERROR(StsAssert, detail);
        case MI_ERR_OOM: MI_CV_ERROR(StsNoMem, detail);
        case MI_ERR_NO_DEVICE: MI_CV_ERROR(GpuNotSupported, detail);
        default: MI_CV_ERROR(GpuApiCallError, detail);
    }
}
}  // namespace detail

// Device used by the calling thread's subsequent calls (a worker of an N-GPU pool calls this once).
inline void setDevice(int device) { detail::tls_device() = device; }
inline int getDevice() { return detail::tls_device(); }
inline int getDeviceCount() { return mi_device_count(); }
// Bind the CALLING thread to the CPUs next to `device` (its NUMA node) -- call it at the top of a worker, before the first
// micv:: call of that thread creates its context (mi_thread_bind_near_device; the reference's workers are not placed at all,
// OpenCVequalHist.cpp:397-402).  Returns the one-line description for a log; never throws for a platform without NUMA information.
inline std::string bindThreadNearDevice(int device)
{
    mi_numa_binding nb{};
    const mi_status st = mi_thread_bind_near_device(device, &nb);
    return st == MI_OK ? std::string(nb.why) : std::string("not bound: ") + mi_status_str(st);
}
// Library option of the calling thread's context on its current device (mi_ctx_set_option), e.g.
//   setOption("clahe_fp_contract", 1)  -- CLAHE interpolation with the fused multiply-adds a GCC build of OpenCV uses on
//   FMA targets (the reference's aarch64 board) instead of the separately rounded x86-64 baseline arithmetic.
inline void setOption(const char* name, int value)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_ctx_set_option(c, name, value), "mi_ctx_set_option");
}

// ---- cv::equalizeHist(InputArray src, OutputArray dst) ----
inline void equalizeHist(const Mat& src, Mat& dst)
{
    MI_CV_ASSERT(src.type() == CV_8UC1);          // histogram.cpp: CV_Assert(_src.type() == CV_8UC1)
    if (src.empty()) return;
    const Mat s = src;                            // keep src alive/unchanged if dst is the same header
    dst.create(s.rows, s.cols, CV_8UC1);
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_u8(c, s.data, s.step, dst.data, dst.step, s.cols, s.rows), "mi_equalize_hist_u8");
}

// ---- cv::CLAHE ----
class CLAHE {
public:
    virtual ~CLAHE() = default;
    virtual void apply(const Mat& src, Mat& dst) = 0;
    virtual void setClipLimit(double clipLimit) = 0;
    virtual double getClipLimit() const = 0;
    virtual void setTilesGridSize(Size tileGridSize) = 0;
    virtual Size getTilesGridSize() const = 0;
    virtual void collectGarbage() = 0;
};

namespace detail {
class CLAHE_Impl final : public CLAHE {
public:
    CLAHE_Impl(double clip, int tx, int ty) : clip_(clip), tx_(tx), ty_(ty) {}
    void apply(const Mat& src, Mat& dst) override
    {
        MI_CV_ASSERT(src.type() == CV_8UC1 || src.type() == CV_16UC1);     // clahe.cpp: CV_Assert(8UC1 || 16UC1)
        if (src.empty()) return;
        MI_CV_ASSERT(tx_ >= 1 && ty_ >= 1);
        const Mat s = src;
        dst.create(s.rows, s.cols, s.type());
        mi_ctx* c = thread_ctx();
        if (s.type() == CV_8UC1)
            check(c, mi_clahe_u8(c, s.data, s.step, dst.data, dst.step, s.cols, s.rows, clip_, tx_, ty_), "mi_clahe_u8");
        else                                                          // 65 536-bin path
            check(c, mi_clahe_u16(c, reinterpret_cast<const uint16_t*>(s.data), s.step, reinterpret_cast<uint16_t*>(dst.data), dst.step,
                                  s.cols, s.rows, clip_, tx_, ty_), "mi_clahe_u16");
    }
    void setClipLimit(double v) override { clip_ = v; }
    double getClipLimit() const override { return clip_; }
    void setTilesGridSize(Size s) override { tx_ = s.width; ty_ = s.height; }
    Size getTilesGridSize() const override { return Size(tx_, ty_); }
    void collectGarbage() override {}             // scratch lives in the per-thread mi_ctx, reused across frames
private:
    double clip_;
    int tx_, ty_;
};
}  // namespace detail

// cv::createCLAHE(double clipLimit = 40.0, Size tileGridSize = Size(8, 8))
inline Ptr<CLAHE> createCLAHE(double clipLimit = 40.0, Size tileGridSize = Size(8, 8))
{
    return std::make_shared<detail::CLAHE_Impl>(clipLimit, tileGridSize.width, tileGridSize.height);
}

// ---- colour-domain neighbours: the calls around the luma op in the reference's image benches ----
// cv::cvtColor(bgr, yuv, cv::COLOR_BGR2YUV) ... cv::cvtColor(yuv, bgr, cv::COLOR_YUV2BGR)   singlecolor.cpp:39/:66,
//                                                                                           clahe1frame.cpp:83/:102
constexpr int COLOR_BGR2YUV = MI_COLOR_BGR2YUV, COLOR_YUV2BGR = MI_COLOR_YUV2BGR;     // OpenCV's numeric values (82, 84)
// 4:2:0 codes: cv::cvtColor(bgr, yuv, cv::COLOR_BGR2YUV_I420) prepares the bench input at 1frameMeasure.cpp:32;
// COLOR_YUV2BGR_NV12 is its NV12 inverse (BASELINE config 5 read literally).  OpenCV's numeric values (128, 93).
constexpr int COLOR_BGR2YUV_I420 = MI_COLOR_BGR2YUV_I420, COLOR_YUV2BGR_NV12 = MI_COLOR_YUV2BGR_NV12;

inline void cvtColor(const Mat& src, Mat& dst, int code)
{
    MI_CV_ASSERT(code == COLOR_BGR2YUV || code == COLOR_YUV2BGR || code == COLOR_BGR2YUV_I420 || code == COLOR_YUV2BGR_NV12);
    if (code == COLOR_BGR2YUV_I420 || code == COLOR_YUV2BGR_NV12) {
        const bool enc = code == COLOR_BGR2YUV_I420;
        MI_CV_ASSERT(src.type() == (enc ? CV_8UC3 : CV_8UC1));
        if (src.empty()) return;
        const Mat s = src;                                               // keeps the data alive if dst aliases src
        const int w = s.cols, h = enc ? s.rows : s.rows * 2 / 3;
        MI_CV_ASSERT(w % 2 == 0 && (enc ? s.rows % 2 == 0 : s.rows % 3 == 0));   // OpenCV's own size checks
        dst.create(enc ? h * 3 / 2 : h, w, enc ? CV_8UC1 : CV_8UC3);
        mi_ctx* c = detail::thread_ctx();
        detail::check(c, mi_cvt_color_420_u8(c, s.data, s.step, dst.data, dst.step, w, h, code), "mi_cvt_color_420_u8");
        return;
    }
    MI_CV_ASSERT(src.type() == CV_8UC3);
    if (src.empty()) return;
    const Mat s = src;
    dst.create(s.rows, s.cols, CV_8UC3);
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_cvt_color_u8c3(c, s.data, s.step, dst.data, dst.step, s.cols, s.rows, code), "mi_cvt_color_u8c3");
}

// cv::split / cv::merge for 8-bit images (singlecolor.cpp:44/:61, clahe1frame.cpp:85/:100).  Pure byte shuffles of
// host Mats, kept on the host like Mat::clone/copyTo; the GPU pipeline below fuses them into the conversions instead.
inline void split(const Mat& src, std::vector<Mat>& planes)
{
    MI_CV_ASSERT(src.depth() == CV_8U);
    const int cn = src.channels();
    planes.resize((size_t)cn);
    for (int k = 0; k < cn; ++k) planes[(size_t)k].create(src.rows, src.cols, CV_8UC1);
    for (int y = 0; y < src.rows; ++y) {
        const unsigned char* s = src.ptr(y);
        for (int k = 0; k < cn; ++k) {
            unsigned char* d = planes[(size_t)k].ptr(y);
            for (int x = 0; x < src.cols; ++x) d[x] = s[(size_t)x * cn + k];
        }
    }
}
inline void merge(const std::vector<Mat>& planes, Mat& dst)
{
    MI_CV_ASSERT(!planes.empty());
    const int cn = (int)planes.size();
    for (const Mat& p : planes) MI_CV_ASSERT(p.type() == CV_8UC1 && p.rows == planes[0].rows && p.cols == planes[0].cols);
    const std::vector<Mat> keep = planes;                         // dst may alias one of the planes' headers
    dst.create(keep[0].rows, keep[0].cols, makeType(CV_8U, cn));
    for (int y = 0; y < dst.rows; ++y) {
        unsigned char* d = dst.ptr(y);
        for (int k = 0; k < cn; ++k) {
            const unsigned char* s = keep[(size_t)k].ptr(y);
            for (int x = 0; x < dst.cols; ++x) d[(size_t)x * cn + k] = s[x];
        }
    }
}

// One call for the whole sequence BGR2YUV -> split -> equalizeHist / CLAHE on Y -> merge -> YUV2BGR
// (singlecolor.cpp:39-66; clahe1frame.cpp:83-102), entirely on the GPU.
inline void equalizeHistLumaBGR(const Mat& bgr, Mat& dst)
{
    MI_CV_ASSERT(bgr.type() == CV_8UC3);
    if (bgr.empty()) return;
    const Mat s = bgr;
    dst.create(s.rows, s.cols, CV_8UC3);
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_bgr_luma_op_u8c3(c, s.data, s.step, dst.data, dst.step, s.cols, s.rows, MI_OP_EQUALIZE, 0.0, 1, 1), "mi_bgr_luma_op_u8c3");
}
inline void claheLumaBGR(const Mat& bgr, Mat& dst, double clipLimit, Size tiles)
{
    MI_CV_ASSERT(bgr.type() == CV_8UC3);
    if (bgr.empty()) return;
    const Mat s = bgr;
    dst.create(s.rows, s.cols, CV_8UC3);
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_bgr_luma_op_u8c3(c, s.data, s.step, dst.data, dst.step, s.cols, s.rows, MI_OP_CLAHE, clipLimit, tiles.width, tiles.height), "mi_bgr_luma_op_u8c3");
}

// ---- the reference's own device-vs-CPU check, 1frameMeasure.cpp:91-94, call for call:
//          cv::absdiff(y_ocv, y_fpga, diff);   float err_per;   xf::cv::analyzeDiff(diff, 1, err_per);
// absdiff: dst = |a - b| (CV_8UC1, same size).  analyzeDiff: err_per = percentage of pixels of `diff` that EXCEED err_thresh; the
// smallest / largest difference are returned through the optional pointers (Vitis Vision prints them).
inline void absdiff(const Mat& a, const Mat& b, Mat& dst)
{
    MI_CV_ASSERT(a.type() == CV_8UC1 && b.type() == CV_8UC1);
    MI_CV_ASSERT(a.rows == b.rows && a.cols == b.cols);
    if (a.empty()) return;
    const Mat x = a, y = b;
    dst.create(x.rows, x.cols, CV_8UC1);
    mi_ctx* c = detail::thread_ctx();
    mi_diff_stats st{};
    detail::check(c, mi_analyze_diff_u8(c, x.data, x.step, y.data, y.step, dst.data, dst.step, x.cols, x.rows, 0, &st), "mi_analyze_diff_u8");
}
inline void analyzeDiff(const Mat& diff, int err_thresh, float& err_per, int* min_diff = nullptr, int* max_diff = nullptr)
{
    MI_CV_ASSERT(diff.type() == CV_8UC1);
    err_per = 0.f;
    if (diff.empty()) return;
    mi_ctx* c = detail::thread_ctx();
    mi_diff_stats st{};
    detail::check(c, mi_analyze_diff_u8(c, diff.data, diff.step, nullptr, 0, nullptr, 0, diff.cols, diff.rows, err_thresh, &st), "mi_analyze_diff_u8");
    err_per = 100.f * (float)st.above / (float)st.total;
    if (min_diff) *min_diff = (int)st.min_diff;
    if (max_diff) *max_diff = (int)st.max_diff;
}

// Pin a recycled frame-buffer pool once so the host forms DMA straight from / into it (mi_host_register).
inline void registerHostBuffer(void* ptr, size_t bytes)
{
    const mi_status st = mi_host_register(ptr, bytes);
    if (st != MI_OK)
        MI_CV_ERROR(st == MI_ERR_NO_DEVICE ? GpuNotSupported : GpuApiCallError,
                    std::string("mi_host_register: ") + mi_status_str(st) + (st == MI_ERR_NO_DEVICE ? " (no HIP device: this backend has no CPU fallback)" : ""));
}
// Unpin it again BEFORE its memory is released.  Two forms:
//   tryUnregisterHostBuffer  never throws (destructors, clean-up paths): MI_OK = unpinned; MI_ERR_BUSY = a pipe still has a transfer queued on
//                            it, the buffer STAYS registered (wait for the pending frames or destroy the pool first, then ask again);
//                            MI_ERR_BAD_ARG = not the start of a registered range; MI_ERR_HIP = the runtime refused, still registered.
//   unregisterHostBuffer     returns false on the busy case and THROWS on every other failure -- not for destructors.
inline mi_status tryUnregisterHostBuffer(void* ptr) noexcept { return mi_host_unregister(ptr); }
inline bool unregisterHostBuffer(void* ptr)
{
    const mi_status st = tryUnregisterHostBuffer(ptr);
    if (st == MI_ERR_BUSY) return false;
    if (st != MI_OK) MI_CV_ERROR(st == MI_ERR_BAD_ARG ? StsBadArg : GpuApiCallError, std::string("mi_host_unregister: ") + mi_status_str(st));
    return true;
}

// ---- whole NV12 frame helpers (what every caller of the reference does around the call) ----
enum UVMode { UV_FILL128 = MI_UV_FILL128, UV_COPY = MI_UV_COPY };

// in/out: tightly packed NV12 (W*H + W*H/2 bytes).  Replaces the clone + equalizeHist + memcpy(Y) +
// memset/memcpy(UV) sequence of OpenCVequalHist.cpp:140-162 / ColoropenCVCwqualHist.cpp:146-165.
inline void equalizeHistNV12(const unsigned char* in, unsigned char* out, int width, int height, UVMode uv)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_nv12(c, in, out, width, height, (mi_uv_mode)uv), "mi_equalize_hist_nv12");
}
inline void claheNV12(const unsigned char* in, unsigned char* out, int width, int height, UVMode uv,
                      double clipLimit, Size tiles)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_nv12(c, in, out, width, height, (mi_uv_mode)uv, clipLimit, tiles.width, tiles.height), "mi_clahe_nv12");
}

// Packed 4:2:2 frames from a capture device (YUY2 / UYVY): rows of 2*W bytes at `pitch` (>= 2*W, a multiple of 4) in host memory.
// cv::extractChannel + equalizeHist / CLAHE::apply + cv::insertChannel on the CV_8UC2 view, without the two extra passes: the luma
// is equalized in place in the frame, the chroma copied or set to 128.  in == out is allowed.
enum PackedFormat { FMT_YUY2 = MI_FMT_YUY2, FMT_UYVY = MI_FMT_UYVY };
inline void equalizeHistPacked422(const unsigned char* in, size_t inPitch, unsigned char* out, size_t outPitch, int width, int height,
                                  PackedFormat format, UVMode uv)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_packed422(c, in, inPitch, out, outPitch, width, height, (int)format, (mi_uv_mode)uv),
                  "mi_equalize_hist_packed422");
}
inline void clahePacked422(const unsigned char* in, size_t inPitch, unsigned char* out, size_t outPitch, int width, int height,
                           PackedFormat format, UVMode uv, double clipLimit, Size tiles)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_packed422(c, in, inPitch, out, outPitch, width, height, (int)format, (mi_uv_mode)uv, clipLimit,
                                        tiles.width, tiles.height), "mi_clahe_packed422");
}
// The same frames in, NV12 out (what the encoder takes) in the pass that equalizes: the Y plane (H rows of W bytes at yPitch) and the
// interleaved UV plane (H/2 rows at uvPitch, the chroma halved vertically with rounding or set to 128) in host memory at any address
// and any pitch >= W.  Width and height are even; the outputs may not overlap the input or each other.
inline void equalizeHistPacked422ToNV12(const unsigned char* in, size_t inPitch, unsigned char* yOut, size_t yPitch,
                                        unsigned char* uvOut, size_t uvPitch, int width, int height, PackedFormat format, UVMode uv)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_packed422_to_nv12(c, in, inPitch, yOut, yPitch, uvOut, uvPitch, width, height, (int)format,
                                                        (mi_uv_mode)uv), "mi_equalize_hist_packed422_to_nv12");
}
inline void clahePacked422ToNV12(const unsigned char* in, size_t inPitch, unsigned char* yOut, size_t yPitch,
                                 unsigned char* uvOut, size_t uvPitch, int width, int height, PackedFormat format, UVMode uv,
                                 double clipLimit, Size tiles)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_packed422_to_nv12(c, in, inPitch, yOut, yPitch, uvOut, uvPitch, width, height, (int)format,
                                                (mi_uv_mode)uv, clipLimit, tiles.width, tiles.height), "mi_clahe_packed422_to_nv12");
}

// Tight NV12 frames from a decoder in, interleaved CV_8UC3 images out (BGR, or RGB) in the pass that equalizes: cv::equalizeHist /
// CLAHE::apply on the Y plane + cv::cvtColor(COLOR_YUV2BGR_NV12) without the NV12 frame in between.  `out`: H rows of 3*W bytes at
// outStep >= 3*W in host memory.  Width and height are even.
enum ChannelOrder { ORDER_BGR = MI_ORDER_BGR, ORDER_RGB = MI_ORDER_RGB };
inline void equalizeHistNV12ToBGR(const unsigned char* nv12, unsigned char* out, size_t outStep, int width, int height,
                                  ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_nv12_to_bgr(c, nv12, out, outStep, width, height, (int)order), "mi_equalize_hist_nv12_to_bgr");
}
inline void claheNV12ToBGR(const unsigned char* nv12, unsigned char* out, size_t outStep, int width, int height, double clipLimit,
                           Size tiles, ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_nv12_to_bgr(c, nv12, out, outStep, width, height, (int)order, clipLimit, tiles.width, tiles.height),
                  "mi_clahe_nv12_to_bgr");
}
// The opposite edge: one interleaved CV_8UC3 host image (BGR, or RGB) at inStep >= 3*W in, one tight NV12 frame of W*H*3/2 bytes for an
// encoder out: cv::cvtColor(COLOR_BGR2YUV_I420) + cv::equalizeHist / CLAHE::apply on the Y plane + the U/V interleave (UV_COPY) or
// chroma 128 (UV_FILL128) without the I420 frame in between.  Width and height are even.
inline void equalizeHistBGRToNV12(const unsigned char* in, size_t inStep, unsigned char* nv12Out, int width, int height,
                                  ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_bgr_to_nv12(c, in, inStep, nv12Out, width, height, (int)order, (mi_uv_mode)uv),
                  "mi_equalize_hist_bgr_to_nv12");
}
inline void claheBGRToNV12(const unsigned char* in, size_t inStep, unsigned char* nv12Out, int width, int height, double clipLimit,
                           Size tiles, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_bgr_to_nv12(c, in, inStep, nv12Out, width, height, (int)order, (mi_uv_mode)uv, clipLimit, tiles.width,
                                          tiles.height), "mi_clahe_bgr_to_nv12");
}

// One 8-bit 4:2:0 host frame whose planes lie where the view says: interleaved chroma (NV12) or planar (I420, YV12), tight or pitched,
// in one allocation or three.  cv::equalizeHist / CLAHE::apply on the Y plane, the chroma carried into the output view's layout
// (UV_COPY) or set to 128 (UV_FILL128): a software decoder's I420 frame -> an NV12 encoder surface, or the other way round, without
// plane copies or an interleave outside the library.  c0 is always the U plane and c1 the V plane.  Width and height are even; a plane
// may be processed in place when it is exactly the same plane in both views.
struct YUV420View {
    unsigned char* y = nullptr;  size_t yPitch = 0;
    unsigned char* c0 = nullptr; unsigned char* c1 = nullptr;      // interleaved: c0 = UV plane, c1 unused; planar: c0 = U, c1 = V
    size_t cPitch = 0;
    bool planar = false;
    // tight frames of width * height * 3 / 2 bytes at `p`
    static YUV420View nv12(unsigned char* p, int w, int h)
    {
        YUV420View v; v.y = p; v.yPitch = (size_t)w; v.c0 = p + (size_t)w * h; v.cPitch = (size_t)w; return v;
    }
    static YUV420View i420(unsigned char* p, int w, int h)
    {
        YUV420View v; v.y = p; v.yPitch = (size_t)w; v.c0 = p + (size_t)w * h; v.c1 = v.c0 + (size_t)(w / 2) * (h / 2);
        v.cPitch = (size_t)(w / 2); v.planar = true; return v;
    }
    static YUV420View yv12(unsigned char* p, int w, int h)
    {
        YUV420View v = i420(p, w, h); unsigned char* t = v.c0; v.c0 = v.c1; v.c1 = t; return v;
    }
    mi_yuv420_planes planes() const
    {
        mi_yuv420_planes d; d.y = y; d.y_pitch = yPitch; d.c0 = c0; d.c1 = c1; d.c_pitch = cPitch; d.frame_stride = 0;
        d.chroma = planar ? MI_CHROMA_PLANAR : MI_CHROMA_INTERLEAVED; return d;
    }
};
inline void equalizeHistYUV420(const YUV420View& in, const YUV420View& out, int width, int height, int uvMode)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes(), b = out.planes();
    detail::check(c, mi_equalize_hist_yuv420(c, &a, &b, width, height, (mi_uv_mode)uvMode), "mi_equalize_hist_yuv420");
}
inline void claheYUV420(const YUV420View& in, const YUV420View& out, int width, int height, int uvMode, double clipLimit, Size tiles)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes(), b = out.planes();
    detail::check(c, mi_clahe_yuv420(c, &a, &b, width, height, (mi_uv_mode)uvMode, clipLimit, tiles.width, tiles.height),
                  "mi_clahe_yuv420");
}
// The same frame views in, an interleaved CV_8UC3 image (BGR, or RGB) out in the pass that equalizes: cv::equalizeHist / CLAHE::apply on
// the Y plane + cv::cvtColor(COLOR_YUV2BGR_I420 / _YV12 / _NV12) without an interleave of U and V and without the frame in between: a
// software decoder's three planes -> a model, a display or an image writer.  `out`: H rows of 3*W bytes at outStep >= 3*W.
inline void equalizeHistYUV420ToBGR(const YUV420View& in, unsigned char* out, size_t outStep, int width, int height,
                                    ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes();
    detail::check(c, mi_equalize_hist_yuv420_to_bgr(c, &a, out, outStep, width, height, (int)order), "mi_equalize_hist_yuv420_to_bgr");
}
inline void claheYUV420ToBGR(const YUV420View& in, unsigned char* out, size_t outStep, int width, int height, double clipLimit,
                             Size tiles, ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes();
    detail::check(c, mi_clahe_yuv420_to_bgr(c, &a, out, outStep, width, height, (int)order, clipLimit, tiles.width, tiles.height),
                  "mi_clahe_yuv420_to_bgr");
}
// The same frame views in, an interleaved CV_8UC4 image (BGRA, or RGBA; A = 255) out: cv::equalizeHist / CLAHE::apply on the Y plane +
// cv::cvtColor(COLOR_YUV2BGRA_I420 / _YV12 / _NV12): a decoder's frame -> a display surface, a texture or a GUI image without a
// three-channel image in between.  `out`: H rows of 4*W bytes at outStep >= 4*W.
inline void equalizeHistYUV420ToBGRA(const YUV420View& in, unsigned char* out, size_t outStep, int width, int height,
                                     ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes();
    detail::check(c, mi_equalize_hist_yuv420_to_bgra(c, &a, out, outStep, width, height, (int)order), "mi_equalize_hist_yuv420_to_bgra");
}
inline void claheYUV420ToBGRA(const YUV420View& in, unsigned char* out, size_t outStep, int width, int height, double clipLimit,
                              Size tiles, ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes();
    detail::check(c, mi_clahe_yuv420_to_bgra(c, &a, out, outStep, width, height, (int)order, clipLimit, tiles.width, tiles.height),
                  "mi_clahe_yuv420_to_bgra");
}
// The capture edge of the same image: one packed 4:2:2 host frame (FMT_YUY2 exactly Y0 U Y1 V, FMT_UYVY exactly U Y0 V Y1; rows of 2*W
// bytes at inPitch, a multiple of 4) in, an interleaved CV_8UC4 image (BGRA, or RGBA; A = 255) out: cv::extractChannel +
// cv::equalizeHist / CLAHE::apply + cv::insertChannel + cv::cvtColor(COLOR_YUV2BGRA_YUY2 / _UYVY), every row with its own chroma: a
// capture card's frame -> a display surface, a texture or a GUI image.  `out`: H rows of 4*W bytes at outStep >= 4*W, any address.
inline void equalizeHistPacked422ToBGRA(const unsigned char* in, size_t inPitch, unsigned char* out, size_t outStep, int width, int height,
                                        PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_packed422_to_bgra(c, in, inPitch, out, outStep, width, height, (int)format, (int)order),
                  "mi_equalize_hist_packed422_to_bgra");
}
inline void clahePacked422ToBGRA(const unsigned char* in, size_t inPitch, unsigned char* out, size_t outStep, int width, int height,
                                 double clipLimit, Size tiles, PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_packed422_to_bgra(c, in, inPitch, out, outStep, width, height, (int)format, (int)order, clipLimit,
                                                tiles.width, tiles.height), "mi_clahe_packed422_to_bgra");
}
// The opposite edge: one interleaved CV_8UC3 host image (BGR, or RGB) at inStep >= 3*W in, the planes of the view out:
// cv::cvtColor(COLOR_BGR2YUV_I420) + cv::equalizeHist / CLAHE::apply on the Y plane, U into out.c0 and V into out.c1 (UV_COPY) or chroma
// 128 (UV_FILL128): a renderer's or a model's image -> the three pitched planes a software encoder takes, without an NV12 frame in
// between and without plane copies.  An interleaved view gives what equalizeHistBGRToNV12 gives, at the view's pitches.
inline void equalizeHistBGRToYUV420(const unsigned char* in, size_t inStep, const YUV420View& out, int width, int height,
                                    ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes b = out.planes();
    detail::check(c, mi_equalize_hist_bgr_to_yuv420(c, in, inStep, &b, width, height, (int)order, (mi_uv_mode)uv),
                  "mi_equalize_hist_bgr_to_yuv420");
}
inline void claheBGRToYUV420(const unsigned char* in, size_t inStep, const YUV420View& out, int width, int height, double clipLimit,
                             Size tiles, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes b = out.planes();
    detail::check(c, mi_clahe_bgr_to_yuv420(c, in, inStep, &b, width, height, (int)order, (mi_uv_mode)uv, clipLimit, tiles.width,
                                            tiles.height), "mi_clahe_bgr_to_yuv420");
}
// equalizeHistPacked422ToNV12 / clahePacked422ToNV12 with the planes of the view out (they stand here because the view does): one
// packed 4:2:2 host frame at inPitch (a multiple of 4) in; the Y plane, U into out.c0 and V into out.c1 -- the chroma halved vertically
// with rounding (UV_COPY) or 128 (UV_FILL128) -- in host memory at any address and any pitch: a capture card's frame -> the three
// pitched planes a software encoder takes, without an NV12 frame in between.  An interleaved view gives what the NV12 wrappers give.
inline void equalizeHistPacked422ToYUV420(const unsigned char* in, size_t inPitch, const YUV420View& out, int width, int height,
                                          PackedFormat format = FMT_YUY2, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes b = out.planes();
    detail::check(c, mi_equalize_hist_packed422_to_yuv420(c, in, inPitch, &b, width, height, (int)format, (mi_uv_mode)uv),
                  "mi_equalize_hist_packed422_to_yuv420");
}
inline void clahePacked422ToYUV420(const unsigned char* in, size_t inPitch, const YUV420View& out, int width, int height, double clipLimit,
                                   Size tiles, PackedFormat format = FMT_YUY2, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes b = out.planes();
    detail::check(c, mi_clahe_packed422_to_yuv420(c, in, inPitch, &b, width, height, (int)format, (mi_uv_mode)uv, clipLimit, tiles.width,
                                                  tiles.height), "mi_clahe_packed422_to_yuv420");
}
// The same edge for four-byte pixels: one interleaved CV_8UC4 host image (BGRA / BGRX, or RGBA / RGBX) at inStep >= 4*W in, the planes
// of the view out: cv::cvtColor(COLOR_BGRA2YUV_I420) + cv::equalizeHist / CLAHE::apply on the Y plane; the fourth byte takes no part.
// A render target's or a screen capture's surface -> an encoder's planes, without a three-channel copy in between.  Planar and
// interleaved views alike.
inline void equalizeHistBGRAToYUV420(const unsigned char* in, size_t inStep, const YUV420View& out, int width, int height,
                                     ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes b = out.planes();
    detail::check(c, mi_equalize_hist_bgra_to_yuv420(c, in, inStep, &b, width, height, (int)order, (mi_uv_mode)uv),
                  "mi_equalize_hist_bgra_to_yuv420");
}
inline void claheBGRAToYUV420(const unsigned char* in, size_t inStep, const YUV420View& out, int width, int height, double clipLimit,
                              Size tiles, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes b = out.planes();
    detail::check(c, mi_clahe_bgra_to_yuv420(c, in, inStep, &b, width, height, (int)order, (mi_uv_mode)uv, clipLimit, tiles.width,
                                             tiles.height), "mi_clahe_bgra_to_yuv420");
}
// The playout edge: one interleaved CV_8UC3 host image (BGR, or RGB) at inStep >= 3*W in, one packed 4:2:2 frame (FMT_YUY2 / FMT_UYVY) at
// outPitch >= 2*W out: the luma of cv::cvtColor(COLOR_BGR2YUV_I420) equalized, every row with the chroma of its own pixels (the left pixel
// of each macropixel, UV_COPY) or chroma 128 (UV_FILL128): a renderer's or a model's image -> a playout card, a v4l2 output or loopback
// device, a virtual camera.  Width is even; any height.
inline void equalizeHistBGRToPacked422(const unsigned char* in, size_t inStep, unsigned char* out, size_t outPitch, int width, int height,
                                       PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_bgr_to_packed422(c, in, inStep, out, outPitch, width, height, (int)order, (int)format, (mi_uv_mode)uv),
                  "mi_equalize_hist_bgr_to_packed422");
}
inline void claheBGRToPacked422(const unsigned char* in, size_t inStep, unsigned char* out, size_t outPitch, int width, int height,
                                double clipLimit, Size tiles, PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR,
                                UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_bgr_to_packed422(c, in, inStep, out, outPitch, width, height, (int)order, (int)format, (mi_uv_mode)uv, clipLimit,
                                               tiles.width, tiles.height), "mi_clahe_bgr_to_packed422");
}
// The same edge for four-byte pixels: one interleaved CV_8UC4 host image (BGRA / BGRX, or RGBA / RGBX) at inStep >= 4*W in, one packed
// 4:2:2 frame at outPitch >= 2*W out: the bytes of the three-channel call on the image with its fourth byte removed.  A render
// target's or a screen capture's surface -> a playout card, a v4l2 output or loopback device, a virtual camera, without a three-channel
// copy in between.  Width is even; any height.
inline void equalizeHistBGRAToPacked422(const unsigned char* in, size_t inStep, unsigned char* out, size_t outPitch, int width, int height,
                                        PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_equalize_hist_bgra_to_packed422(c, in, inStep, out, outPitch, width, height, (int)order, (int)format, (mi_uv_mode)uv),
                  "mi_equalize_hist_bgra_to_packed422");
}
inline void claheBGRAToPacked422(const unsigned char* in, size_t inStep, unsigned char* out, size_t outPitch, int width, int height,
                                 double clipLimit, Size tiles, PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR,
                                 UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_clahe_bgra_to_packed422(c, in, inStep, out, outPitch, width, height, (int)order, (int)format, (mi_uv_mode)uv, clipLimit,
                                                tiles.width, tiles.height), "mi_clahe_bgra_to_packed422");
}
// The decoder-to-playout edge: the planes of the view (NV12, I420 or YV12 in host memory) in, one packed 4:2:2 frame (FMT_YUY2 /
// FMT_UYVY) at outPitch >= 2*W out: cv::equalizeHist / CLAHE::apply on the Y plane, output rows 2r and 2r+1 both with input chroma row r
// unchanged (UV_COPY) or chroma 128 (UV_FILL128, the view's chroma is not read).  Width and height are even.
inline void equalizeHistYUV420ToPacked422(const YUV420View& in, unsigned char* out, size_t outPitch, int width, int height,
                                          PackedFormat format = FMT_YUY2, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes();
    detail::check(c, mi_equalize_hist_yuv420_to_packed422(c, &a, out, outPitch, width, height, (int)format, (mi_uv_mode)uv),
                  "mi_equalize_hist_yuv420_to_packed422");
}
inline void claheYUV420ToPacked422(const YUV420View& in, unsigned char* out, size_t outPitch, int width, int height, double clipLimit,
                                   Size tiles, PackedFormat format = FMT_YUY2, UVMode uv = UV_COPY)
{
    mi_ctx* c = detail::thread_ctx();
    const mi_yuv420_planes a = in.planes();
    detail::check(c, mi_clahe_yuv420_to_packed422(c, &a, out, outPitch, width, height, (int)format, (mi_uv_mode)uv, clipLimit, tiles.width,
                                                  tiles.height), "mi_clahe_yuv420_to_packed422");
}

// BASELINE.json config 5 read literally: cvtColor(COLOR_YUV2BGR_NV12) -> split -> equalizeHist on B, G and R -> merge ->
// cvtColor(COLOR_BGR2YUV_I420) + U/V interleave, NV12 in -> NV12 out in one call (no file of the reference does this;
// ColoropenCVCwqualHist.cpp itself is equalizeHistNV12(..., UV_COPY)).  Width and height must be even.
inline void equalizeHistChannelsNV12(const unsigned char* in, unsigned char* out, int width, int height)
{
    mi_ctx* c = detail::thread_ctx();
    detail::check(c, mi_nv12_bgr_equalize(c, in, out, width, height), "mi_nv12_bgr_equalize");
}

}  // namespace micv

// ---- real OpenCV front end (only when the including program already uses OpenCV) ----
#if defined(MI_CV_WITH_OPENCV) && defined(__has_include)
#if __has_include(<opencv2/core.hpp>) && __has_include(<opencv2/imgproc.hpp>)
#include <opencv2/core.hpp>
#include <opencv2/imgproc.hpp>      // cv::CLAHE
#define MI_CV_HAVE_OPENCV_FRONT_END 1
namespace mi_cv {
inline void throw_cv(mi_ctx* c, mi_status st, const char* what)
{
    if (st == MI_OK) return;
    cv::error(st == MI_ERR_BAD_ARG ? cv::Error::StsBadArg : (st == MI_ERR_UNSUPPORTED ? cv::Error::StsAssert : cv::Error::GpuApiCallError),
              std::string(what) + ": " + mi_status_str(st) + " (" + mi_ctx_last_error_msg(c) + ")", what, __FILE__, __LINE__);
}
// drop-in for cv::equalizeHist(InputArray, OutputArray) on host Mats
inline void equalizeHist(cv::InputArray _src, cv::OutputArray _dst)
{
    CV_Assert(_src.type() == CV_8UC1);
    if (_src.empty()) return;
    cv::Mat src = _src.getMat();
    _dst.create(src.size(), src.type());          // no reallocation when dst already matches (nextimprovement.cpp:164-168)
    cv::Mat dst = _dst.getMat();
    mi_ctx* c = micv::detail::thread_ctx();
    throw_cv(c, mi_equalize_hist_u8(c, src.data, src.step, dst.data, dst.step, src.cols, src.rows), "mi_equalize_hist_u8");
}
class CLAHE_MI final : public cv::CLAHE {
public:
    CLAHE_MI(double clip, cv::Size t) : clip_(clip), tiles_(t) {}
    void apply(cv::InputArray _src, cv::OutputArray _dst) CV_OVERRIDE
    {
        CV_Assert(_src.type() == CV_8UC1 || _src.type() == CV_16UC1);       // clahe.cpp accepts exactly these two
        if (_src.empty()) return;
        cv::Mat src = _src.getMat();
        _dst.create(src.size(), src.type());
        cv::Mat dst = _dst.getMat();
        mi_ctx* c = micv::detail::thread_ctx();
        if (src.type() == CV_8UC1)
            throw_cv(c, mi_clahe_u8(c, src.data, src.step, dst.data, dst.step, src.cols, src.rows, clip_, tiles_.width, tiles_.height), "mi_clahe_u8");
        else
            throw_cv(c, mi_clahe_u16(c, src.ptr<uint16_t>(), src.step, dst.ptr<uint16_t>(), dst.step, src.cols, src.rows, clip_, tiles_.width, tiles_.height), "mi_clahe_u16");
    }
    void setClipLimit(double v) CV_OVERRIDE { clip_ = v; }
    double getClipLimit() const CV_OVERRIDE { return clip_; }
    void setTilesGridSize(cv::Size s) CV_OVERRIDE { tiles_ = s; }
    cv::Size getTilesGridSize() const CV_OVERRIDE { return tiles_; }
    void collectGarbage() CV_OVERRIDE {}
private:
    double clip_;
    cv::Size tiles_;
};
inline cv::Ptr<cv::CLAHE> createCLAHE(double clipLimit = 40.0, cv::Size tileGridSize = cv::Size(8, 8))
{
    return cv::makePtr<CLAHE_MI>(clipLimit, tileGridSize);
}
}  // namespace mi_cv
#endif
#endif

#endif  // MI_CV_HPP_
