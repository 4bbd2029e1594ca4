/*
 * mi_lumaeq.h -- C ABI of the MI355X (gfx950) luma histogram-equalization library.
 *
 * This is the drop-in boundary for the ONE hot path of kimkimhun3/OpenCV-OpenCL: the call the
 * reference makes on the CV_8UC1 Y plane of every NV12 frame,
 *
 *     cv::equalizeHist(src, dst)                    OpenCVequalHist.cpp:145, nextimprovement.cpp:168,
 *                                                   AirplanMP4.cpp:90, 1frameMeasure.cpp:44
 *     cv::createCLAHE(clip, Size(t,t))->apply(..)   clahevideo.cpp:184-195/:497, clahe1frame.cpp:88-93,
 *                                                   CLAHECompare.cpp:144-150
 *
 * and for the accelerator backend the reference wires behind that call,
 *
 *     cl::Kernel "equalizeHist_accel"(in, ref, out, rows, cols)
 *                                                   OpenCLequalHist.cpp:346-365 (host sequence),
 *                                                   accel.cpp:36-61 (device kernel), 1frameMeasure.cpp:60-87
 *
 * Plain C: pointers, sizes, integer status codes.  No exceptions, no STL, no torch / OpenCV types.
 * The C++ adapter that presents the cv::Mat-in / cv::Mat-out surface on top of it is
 * opencv-opencl_amd/cxx/mi_cv.hpp; the binding a maintainer of the reference would add is shown
 * in INTEGRATION.md.
 *
 * Threading: every function is safe to call concurrently on DISTINCT contexts (the reference
 * runs 1..8 worker threads, OpenCVequalHist.cpp:274/:397-402 -> one context per worker).  A
 * context is internally locked, so sharing one between threads is safe but serialises.
 *
 * There is no CPU fallback: every entry point needs a HIP device and returns MI_ERR_NO_DEVICE /
 * MI_ERR_HIP otherwise.
 */
#ifndef MI_LUMAEQ_H_
#define MI_LUMAEQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_LUMAEQ_VERSION_MAJOR 0
#define MI_LUMAEQ_VERSION_MINOR 3

typedef enum mi_status {
    MI_OK = 0,
    MI_ERR_BAD_ARG = 1,          /* null pointer, negative size, step < width, tiles <= 0 ...        */
    MI_ERR_UNSUPPORTED = 2,      /* not CV_8UC1-shaped work (the adapter maps this to cv::Exception) */
    MI_ERR_HIP = 3,              /* a HIP call failed; see mi_ctx_last_hip_error()                   */
    MI_ERR_OOM = 4,              /* host or device allocation failed                                 */
    MI_ERR_NO_DEVICE = 5,        /* no usable HIP device / device index out of range                 */
    MI_ERR_BUSY = 6              /* mi_pipe_submit: `depth` frames are in flight, call mi_pipe_wait; any compute entry point
                                  * while frames are pending in the context's pipe; a second mi_pipe_create on a context  */
} mi_status;

/* UV handling of whole-NV12-frame entry points:
 *   MI_UV_FILL128 : memset(out + W*H, 128, W*H/2)      OpenCVequalHist.cpp:160-162, clahevideo.cpp:200-201
 *   MI_UV_COPY    : memcpy(out + W*H, in + W*H, W*H/2) ColoropenCVCwqualHist.cpp:165, improvement.cpp:163,
 *                                                      nextimprovement.cpp:160
 * On P010 / P012 / P016 frames (MI_FMT_P010, mi_clahe_p010*) the same two modes act on 16-bit samples: MI_UV_FILL128 sets every
 * chroma sample to 0x8000 -- 128 in the high byte, the neutral value of all three formats -- and MI_UV_COPY copies the chroma half
 * (W*H bytes) byte for byte. */
typedef enum mi_uv_mode { MI_UV_FILL128 = 0, MI_UV_COPY = 1 } mi_uv_mode;

typedef struct mi_ctx mi_ctx;    /* opaque: device id, streams, pinned staging, device scratch */

/* stream argument value selecting the context's own stream (see the device-resident forms) */
#define MI_STREAM_CTX ((void*)(uintptr_t)-1)

/* ---- context ------------------------------------------------------------------------------
 * Replaces the per-worker OpenCL objects of the reference (context/queue/kernel/3 buffers,
 * OpenCLequalHist.cpp:106-192): scratch is allocated lazily for the largest frame seen and
 * reused ("allocate once per size", OpenCLequalHist.cpp:175-186). */
mi_status   mi_ctx_create(int device, mi_ctx** out);
void        mi_ctx_destroy(mi_ctx* ctx);
int         mi_ctx_device(const mi_ctx* ctx);
int         mi_ctx_last_hip_error(const mi_ctx* ctx);      /* raw hipError_t of the last MI_ERR_HIP */
const char* mi_ctx_last_error_msg(const mi_ctx* ctx);      /* human readable, never NULL           */
const char* mi_status_str(mi_status s);
const char* mi_version(void);
int         mi_device_count(void);                         /* 0 when no HIP device is usable       */

/* ---- placement of a GPU's host worker -----------------------------------------------------------
 * The frame-sharded stream runs one host worker per GPU (reference: the worker pool of OpenCVequalHist.cpp:397-402, which
 * places nothing).  mi_thread_bind_near_device() binds the CALLING THREAD to the CPUs of the NUMA node the device's PCIe
 * root complex hangs off (device -> PCI address -> /sys/bus/pci/devices/<bdf>/numa_node -> that node's cpulist, intersected
 * with the CPUs the process may use; sched_setaffinity in-process).  Call it BEFORE mi_ctx_create / mi_pipe_create on that
 * thread: the pinned staging buffers they allocate are then first touched next to the GPU, and threads the library starts
 * later inherit the binding.  Never fatal: when the platform reports no node (-1) or none of its CPUs is available, the
 * thread stays where it is and `why` says so.  MI_LUMAEQ_NUMA_BIND=0 in the environment turns every call into a no-op. */
typedef struct mi_numa_binding {
    int  node;                   /* NUMA node of the device, -1 unknown                    */
    int  cpus;                   /* CPUs the thread is now bound to, 0 = left where it was */
    char why[192];               /* one line for a banner / log                            */
} mi_numa_binding;
mi_status mi_device_pci_bus_id(int device, char* buf, size_t buf_len);         /* "0000:c1:00.0" */
mi_status mi_thread_bind_near_device(int device, mi_numa_binding* out);        /* out may be NULL */

/* ---- host-pointer forms: the cv::Mat boundary -----------------------------------------------
 * Synchronous: on return dst is fully written in host memory (SURVEY 8b "Semantics to keep").
 * src/dst are CV_8UC1 planes with row pitch `*_step` >= width (ROI views: clahevideo.cpp:179);
 * dst may be the same memory as src (in place).  width==0 or height==0 is a no-op (MI_OK).
 * Replaces  cv::equalizeHist(y_in, y_out)  (OpenCVequalHist.cpp:145) and the whole blocking
 * write/write/task/read sequence of OpenCLequalHist.cpp:356-365.
 * Host memory: planes in PINNED memory (mi_host_register below, or hipHostMalloc / hipHostRegister by the caller) are DMA'd
 * as they are; anything else is packed through the context's own pinned staging buffers by the calling thread and one helper
 * thread of the context -- the library never hands the HIP runtime memory it did not pin itself.
 * Errors: whatever a host-pointer form returns, no copy on src / dst is in flight any more when it returns. */
mi_status mi_equalize_hist_u8(mi_ctx* ctx, const uint8_t* src, size_t src_step,
                              uint8_t* dst, size_t dst_step, int width, int height);

/* Replaces  clahe->apply(y_in, y_out)  with clahe = cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))
 * (clahevideo.cpp:184-195, clahe1frame.cpp:88-93). */
mi_status mi_clahe_u8(mi_ctx* ctx, const uint8_t* src, size_t src_step,
                      uint8_t* dst, size_t dst_step, int width, int height,
                      double clip_limit, int tiles_x, int tiles_y);

/* Whole tightly packed NV12 frame in host memory: Y op + UV fill/copy in one call, writing
 * straight into the caller's output frame (the zero-copy semantics of nextimprovement.cpp:159-168;
 * removes the Y clone + memcpy + memset of OpenCVequalHist.cpp:141/:160-162).
 * in/out hold width*height + width*height/2 bytes; in == out is allowed. */
mi_status mi_equalize_hist_nv12(mi_ctx* ctx, const uint8_t* in, uint8_t* out,
                                int width, int height, mi_uv_mode uv_mode);
mi_status mi_clahe_nv12(mi_ctx* ctx, const uint8_t* in, uint8_t* out, int width, int height,
                        mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);

/* ---- device-resident, batched, stream-ordered forms -------------------------------------------
 * Pointers are device pointers on the context's device.  `stream` is a hipStream_t passed as
 * void*, with HIP's own meaning: NULL is the device's default (null) stream -- what
 * torch.cuda.current_stream().cuda_stream is unless the caller switched streams.  Pass
 * MI_STREAM_CTX to use the context's private non-blocking stream (it does NOT order against the
 * null stream).  Asynchronous: the call returns after enqueueing.  A context owns one set of
 * scratch buffers: calls that share a context must be issued on one stream at a time (or be
 * ordered by the caller); use one context per concurrent stream.
 * Frame f of a batch lives at base + f * frame_stride.  These are what a per-GPU worker of the
 * frame-sharded pipeline (reference analogue: worker pool OpenCVequalHist.cpp:397-402)
 * calls, and what bench.py measures. */
mi_status mi_equalize_hist_u8_batch_dev(mi_ctx* ctx,
                                        const void* d_src, size_t src_step, size_t src_frame_stride,
                                        void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                        int width, int height, int n_frames, void* stream);

mi_status mi_clahe_u8_batch_dev(mi_ctx* ctx,
                                const void* d_src, size_t src_step, size_t src_frame_stride,
                                void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                int width, int height, int n_frames,
                                double clip_limit, int tiles_x, int tiles_y, void* stream);

/* n_frames tightly packed NV12 frames (frame pitch = W*H + W*H/2 bytes), Y op + UV fill/copy
 * fused into the same launches. d_in == d_out is allowed. */
mi_status mi_equalize_hist_nv12_batch_dev(mi_ctx* ctx, const void* d_in, void* d_out,
                                          int width, int height, int n_frames,
                                          mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_nv12_batch_dev(mi_ctx* ctx, const void* d_in, void* d_out,
                                  int width, int height, int n_frames, mi_uv_mode uv_mode,
                                  double clip_limit, int tiles_x, int tiles_y, void* stream);

/* A LIST of NV12 frames in device memory, each with its own Y and UV plane addresses: decoder surfaces from a pool (each its own
 * allocation, rows padded to a pitch, the UV plane at pitch * aligned_height), or a list of frame tensors.  `frames` is a host array
 * of n_frames entries, read only during the call; the pointers in it are device pointers on the context's device.  Every frame of
 * one call has the same width and height and the same four pitches (bytes between rows; each >= width):
 *   y_in  : H rows of W bytes at y_in_pitch        y_out  : H rows at y_out_pitch
 *   uv_in : H/2 rows of W bytes at uv_in_pitch     uv_out : H/2 rows at uv_out_pitch
 *           (read with MI_UV_COPY only; may be NULL with MI_UV_FILL128)
 * Plane addresses may have any alignment.  The Y output is byte for byte what the _nv12_batch_dev forms (cv::equalizeHist /
 * CLAHE::apply) return on the same pixels, the UV output is filled with 128 or copied; nothing outside the W bytes of each output
 * row is written (not the pitch padding, nor rows between the planes).  A frame may be processed in place (y_out == y_in and
 * uv_out == uv_in, with equal pitches); in place with MI_UV_COPY leaves the chroma as it is.  Outputs of DIFFERENT frames that
 * overlap each other give undefined results (not checked).  Stream rules as above; the call returns after enqueueing, and can be
 * captured into a hipGraph after one eager call of the same shape.  The options clahe_fp_contract and two_kernel_max_frames apply;
 * these frames never take the fused equalizeHist kernel.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, n_frames < 0, odd W or H, a pitch < W, a null Y plane or
 * uv_out, a null uv_in with MI_UV_COPY, an output plane that overlaps an input plane of the same frame other than exactly (same
 * address, same pitch), tiles <= 0, a bad uv_mode.  n_frames, width or height of 0: MI_OK, nothing written.  Nothing is enqueued
 * unless every frame passes the checks. */
typedef struct mi_nv12_frame_dev {
    const void* y_in;
    const void* uv_in;
    void*       y_out;
    void*       uv_out;
} mi_nv12_frame_dev;
mi_status mi_equalize_hist_nv12_frames_dev(mi_ctx* ctx, const mi_nv12_frame_dev* frames, int n_frames, int width, int height,
                                           size_t y_in_pitch, size_t uv_in_pitch, size_t y_out_pitch, size_t uv_out_pitch,
                                           mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_nv12_frames_dev(mi_ctx* ctx, const mi_nv12_frame_dev* frames, int n_frames, int width, int height,
                                   size_t y_in_pitch, size_t uv_in_pitch, size_t y_out_pitch, size_t uv_out_pitch,
                                   mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream);

/* ---- stage-level device entry points ---------------------------
 * The same kernels the fused forms launch, exposed one stage at a time so each can be checked
 * against the oracle and timed against its own roofline. */

/* A2: d_hist[f][256] (int32) = exact histogram of frame f. */
mi_status mi_hist_u8_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                               int width, int height, int n_frames, void* d_hist, void* stream);
/* A3: d_lut[f][256] (uint8) from d_hist[f][256]; total = width*height pixels per frame. */
mi_status mi_equalize_lut_batch_dev(mi_ctx* ctx, const void* d_hist, int64_t total, int n_frames,
                                    void* d_lut, void* stream);
/* A4: dst = lut_f[src] for every frame (the north-star roofline kernel). */
mi_status mi_lut_apply_u8_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                                    void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                    int width, int height, int n_frames, const void* d_lut, void* stream);
/* A6 steps 1-4: d_luts[f][tiles_y*tiles_x][256] (uint8) per-tile clipped LUTs. */
mi_status mi_clahe_tile_luts_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                                       int width, int height, int n_frames,
                                       double clip_limit, int tiles_x, int tiles_y,
                                       void* d_luts, void* stream);

/* ---- the reference's own parity check as an operator (1frameMeasure.cpp:91-100) ------------------------
 * The only test the reference holds compares its accelerator's plane with cv::equalizeHist's:
 *     cv::absdiff(y_ocv, y_fpga, diff);  xf::cv::analyzeDiff(diff, 1, err_per);      pass iff err_per == 0
 * (Vitis Vision's analyzeDiff walks the difference image, reports the smallest and the largest difference and the
 * percentage of pixels whose difference EXCEEDS the threshold).  Both steps in one pass, on planes wherever they are:
 * per frame f, stats[f] = { pixels with |a - b| > threshold, largest |a - b|, smallest |a - b|, pixels compared };
 * err_per = 100.0 * above / total.  `b` may be NULL: `a` then already is a difference image (analyzeDiff on its own);
 * `diff` may be NULL: no difference image is written (otherwise diff = |a - b|, cv::absdiff; it may alias a or b).
 * This library's own tests demand bit-exactness (max_diff == 0); the operator exists so a caller can keep the
 * reference's +-1 check, and so full-size device batches can be compared without a download. */
typedef struct mi_diff_stats { uint32_t above, max_diff, min_diff, total; } mi_diff_stats;
/* host planes (step >= width), blocking */
mi_status mi_analyze_diff_u8(mi_ctx* ctx, const uint8_t* a, size_t a_step, const uint8_t* b, size_t b_step,
                             uint8_t* diff, size_t diff_step, int width, int height, int threshold, mi_diff_stats* out);
/* device planes, batched, stream-ordered; d_stats = n_frames mi_diff_stats in device memory */
mi_status mi_analyze_diff_u8_batch_dev(mi_ctx* ctx, const void* d_a, size_t a_step, size_t a_frame_stride,
                                       const void* d_b, size_t b_step, size_t b_frame_stride,
                                       void* d_diff, size_t diff_step, size_t diff_frame_stride,
                                       int width, int height, int n_frames, int threshold, mi_diff_stats* d_stats, void* stream);

/* ---- CLAHE on CV_16UC1 (OpenCV surface beyond what the reference uses) ------------------------
 * cv::createCLAHE(clip, Size(tx,ty))->apply on 16-bit single-channel images: 65 536 bins, ushort LUTs.
 * Steps / frame strides in BYTES (>= 2*width).  In place allowed.  Results never depend on the content, speed does: frames
 * that populate at most 4096 values -- 10/12-bit samples in the LOW bits, or in the HIGH bits of the word as P010 / P016
 * video stores them (every value a multiple of 1 << shift) -- take one pass of tile histograms and one interpolation from
 * a single table; wider content is walked in windows of the value range.
 * Speed (never bytes) also depends on the context's HISTORY: tiles that could go with several shifts -- a flat letterbox bar of a
 * P010 frame -- take the shift the frames of the context's PREVIOUS call settled on (a video stream keeps its format), so the first
 * call after a change of sample format may run its frames through the slower per-frame LUT pass once.  Every tile of one
 * LAUNCH sees the same hint (a call on many frames is cut into chunks, one launch sequence per chunk): it is read-only while the
 * chunk's tile kernels run and rolled over by the chunk's first interpolation launch.  The hint affects speed only, never bytes. */
mi_status mi_clahe_u16(mi_ctx* ctx, const uint16_t* src, size_t src_step, uint16_t* dst, size_t dst_step,
                       int width, int height, double clip_limit, int tiles_x, int tiles_y);
mi_status mi_clahe_u16_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                                 void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                 int width, int height, int n_frames,
                                 double clip_limit, int tiles_x, int tiles_y, void* stream);

/* ---- CLAHE on 16-bit 4:2:0 video frames: P010, P012, P016 (what an HEVC Main10 / HDR decoder hands over) -------------------
 * A frame is W x H little-endian uint16 luma samples followed by H/2 rows of W interleaved uint16 U, V samples: 3*W*H bytes,
 * tightly packed, W and H even.  The layout is the same for P010, P012 and P016 and the operation never looks at the bit depth.
 *   luma   : cv::createCLAHE(clip, Size(tiles_x, tiles_y))->apply(y, y) on the CV_16UC1 view of the Y plane (row pitch 2*W),
 *            i.e. exactly what mi_clahe_u16* computes on that plane.  Output samples are NOT re-quantised to multiples of 64
 *            (or 16): OpenCV returns full 16-bit values for that view, and so does this.
 *   chroma : MI_UV_FILL128 = every sample 0x8000; MI_UV_COPY = copied byte for byte (in place: nothing moves).
 * equalizeHist has no 16-bit form in OpenCV (it asserts CV_8UC1): P010 offers CLAHE only.
 * Errors: odd W or H, a null pointer, a pointer that is not 2-byte aligned, tiles <= 0: MI_ERR_BAD_ARG; width, height or n_frames
 * of 0: MI_OK, nothing done; W*H beyond what mi_clahe_u16 accepts: MI_ERR_UNSUPPORTED.
 * mi_clahe_p010: host frames, synchronous, in == out allowed.  Only the Y plane crosses PCIe (directly when the frame is pinned,
 *   see mi_host_register); the chroma half is written on the host while the GPU works on Y.
 * mi_clahe_p010_batch_dev: n_frames frames at a frame pitch of 3*W*H bytes, stream-ordered like the other batched device forms;
 *   d_in == d_out allowed; capturable into a hipGraph after one eager call of the same shape. */
/* MI_FMT_YUY2 / MI_FMT_UYVY: packed 8-bit 4:2:2 frames, see mi_*_packed422* below.  MI_FMT_YUY2 = luma at byte offset 0 of each 2-byte
 * pixel (YUY2 / YUYV / YVYU: the chroma order is irrelevant, chroma is only copied or filled), MI_FMT_UYVY = luma at byte offset 1
 * (UYVY / VYUY). */
enum { MI_FMT_NV12 = 0, MI_FMT_P010 = 1, MI_FMT_YUY2 = 2, MI_FMT_UYVY = 3 };   /* P010 = any 16-bit LE 4:2:0 semi-planar frame: P010 / P012 / P016 */
mi_status mi_clahe_p010(mi_ctx* ctx, const uint16_t* in, uint16_t* out, int width, int height,
                        mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
mi_status mi_clahe_p010_batch_dev(mi_ctx* ctx, const void* d_in, void* d_out, int width, int height, int n_frames,
                                  mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_clahe_p010_frames_dev: a LIST of P010 frames in device memory, each with its own pitched Y and UV plane (a Main10 decoder's
 * surface pool), as mi_clahe_nv12_frames_dev takes NV12 frames.  mi_p010_frame_dev is mi_nv12_frame_dev: four plane addresses.
 * Pitches are in BYTES, shared by every frame of the call, even and each >= 2*W:
 *   y_in  : H rows of W uint16 at y_in_pitch                       y_out  : H rows at y_out_pitch
 *   uv_in : H/2 rows of W interleaved uint16 U, V at uv_in_pitch   uv_out : H/2 rows at uv_out_pitch
 *           (read with MI_UV_COPY only; may be NULL with MI_UV_FILL128)
 * Plane addresses are 2-byte aligned (16-byte aligned Y inputs with a pitch that is a multiple of 16 take the faster tile
 * histograms; anything else is slower, never different).  The luma is byte for byte what mi_clahe_p010_batch_dev / mi_clahe_u16*
 * return on the same pixels, the chroma is set to 0x8000 or copied; nothing outside the 2*W bytes of an output row is written.
 * In place is decided PER FRAME: a frame is in place when y_out == y_in (the pitches must then be equal), and one list may mix
 * in-place and out-of-place frames; in place with MI_UV_COPY leaves the chroma as it is.  Outputs of DIFFERENT frames that overlap
 * each other give undefined results (not checked).  Stream rules, hipGraph capture and the options as mi_clahe_nv12_frames_dev and
 * mi_clahe_u16_batch_dev (clahe16_*).  No equalizeHist form (OpenCV's is 8-bit only) and no host form.
 * Errors, MI_ERR_BAD_ARG: those of mi_clahe_nv12_frames_dev, plus an odd pitch, a pitch < 2*W and a plane address that is not
 * 2-byte aligned.  MI_ERR_UNSUPPORTED: sizes beyond what mi_clahe_u16 accepts.  n_frames, width or height of 0: MI_OK, nothing
 * written.  Nothing is enqueued unless every frame passes the checks. */
typedef mi_nv12_frame_dev mi_p010_frame_dev;
mi_status mi_clahe_p010_frames_dev(mi_ctx* ctx, const mi_p010_frame_dev* frames, int n_frames, int width, int height,
                                   size_t y_in_pitch, size_t uv_in_pitch, size_t y_out_pitch, size_t uv_out_pitch,
                                   mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream);

/* ---- equalizeHist and CLAHE on packed 4:2:2 frames: YUY2 / UYVY (what a capture device hands over: v4l2, SDI / HDMI cards) ----------
 * A frame is H rows of W 2-byte pixels, 2*W bytes per row at `pitch` bytes: macropixels Y0 U Y1 V (MI_FMT_YUY2) or U Y0 V Y1
 * (MI_FMT_UYVY).  Luma sample (x, y) is byte y * pitch + 2 * x + off, off = 0 (MI_FMT_YUY2) / 1 (MI_FMT_UYVY).  In OpenCV terms: the
 * Mat(H, W, CV_8UC2, data, pitch) view, cv::extractChannel(frame, y, off), cv::equalizeHist / CLAHE::apply on y, cv::insertChannel.
 *   luma   : byte for byte what mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev return on the gathered W x H plane (same
 *            clahe_fp_contract option, same REFLECT_101 padding when W or H is not divisible by the tile grid), written in place in
 *            the packed output frame; no plane is gathered or scattered.
 *   chroma : MI_UV_COPY copies the chroma bytes, MI_UV_FILL128 writes 128.  In place (d_out == d_in, equal pitch and frame stride)
 *            with MI_UV_COPY leaves them as they are.
 * Nothing outside the 2*W bytes of each output row is written: not the pitch padding, not the gap between frames.
 * `width` is even, `height` any value >= 1 (4:2:2 has no vertical subsampling).  Pointers, pitches and frame strides are multiples of
 * 4 -- a macropixel is always one aligned dword, and an ROI with an even x origin stays legal; 16-byte alignment is NOT required.
 * pitch >= 2*W.
 * _batch_dev forms: frame f at base + f * frame_stride; stream rules, MI_STREAM_CTX, hipGraph capture after one eager call of the
 *   same shape and MI_ERR_BUSY while a pipe has frames pending as the other batched device forms.  These forms never take the fused
 *   equalizeHist kernel nor the single-launch histogram + LUT kernel (option two_kernel_max_frames does not apply); their launches
 *   are charged to the profiling slots MI_K_HIST, MI_K_EQ_LUT, MI_K_LUT_APPLY, MI_K_TILE_HIST, MI_K_TILE_LUT, MI_K_CLAHE_INTERP by role.
 * mi_equalize_hist_packed422 / mi_clahe_packed422: host frames, synchronous, in == out allowed, like mi_equalize_hist_nv12 /
 *   mi_clahe_nv12 -- except that the whole frame crosses the bus in both directions (there is no luma plane to send on its own) and
 *   the kernels write the chroma.  Pitched host frames are accepted: only the 2*W bytes of each row are read and written.  Whatever
 *   the call returns, no copy on in / out is in flight any more when it returns.
 * Errors, MI_ERR_BAD_ARG: a null ctx or frame pointer, an odd width, a negative size, a pitch < 2*W, a pointer / pitch / frame stride
 * that is not a multiple of 4, a format other than the two, a bad uv_mode, tiles <= 0.  width, height or n_frames of 0: MI_OK, nothing
 * written.  Sizes and tile grids beyond what the planar forms accept: what those answer (MI_ERR_UNSUPPORTED).  Partially overlapping
 * input and output: undefined, as for the other batched forms. */
mi_status mi_equalize_hist_packed422_batch_dev(mi_ctx* ctx,
                                               const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_out, size_t out_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_packed422_batch_dev(mi_ctx* ctx,
                                       const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                       void* d_out, size_t out_pitch, size_t out_frame_stride,
                                       int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
                                       double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_packed422(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_pitch,
                                     int width, int height, int format, mi_uv_mode uv_mode);
mi_status mi_clahe_packed422(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_pitch,
                             int width, int height, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_packed422_frames_dev: a LIST of packed 4:2:2 frames in device memory, each at its own address -- a capture device's buffer
 * pool (v4l2, SDI / HDMI cards): every buffer its own allocation, rows padded to bytesperline, the base address at whatever alignment
 * the driver gave it.  `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device
 * pointers on the context's device.  Every frame of one call has the same width (even), height (any value >= 1), format and the same
 * two pitches (bytes between rows, each >= 2*W):
 *   in  : H rows of 2*W bytes at in_pitch          out : H rows of 2*W bytes at out_pitch
 * Addresses and pitches are multiples of 4; each frame may have its own alignment modulo 16 (slower never, different never).  The
 * same input may appear in several entries.  The luma and the chroma of every frame are byte for byte what
 * mi_*_packed422_batch_dev writes for that frame (same clahe_fp_contract option, same REFLECT_101 padding, same fallback for tile
 * grids too wide for the LDS tables); nothing outside the 2*W bytes of an output row is written.
 * In place is decided PER FRAME: a frame is in place when out == in (the two pitches must then be equal), and one list may mix
 * in-place and out-of-place frames; in place with MI_UV_COPY leaves the chroma as it is.  Outputs of DIFFERENT frames that overlap
 * each other give undefined results (not checked).  Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while a pipe has frames pending and
 * hipGraph capture after one eager call of the same shape as mi_*_nv12_frames_dev; profiling slots by role as the _batch_dev forms
 * above; never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, a negative size, an odd width, a format other than
 * MI_FMT_YUY2 / MI_FMT_UYVY, a bad uv_mode, tiles <= 0, a pitch < 2*W, a pitch or address that is not a multiple of 4, a null in or
 * out, out == in with unequal pitches, an output whose rows overlap the rows of its own frame's input other than exactly.  Sizes and
 * tile grids beyond what the planar forms accept: what those answer (MI_ERR_UNSUPPORTED).  n_frames, width or height of 0: MI_OK,
 * nothing written.  Nothing is enqueued unless every frame passes the checks. */
typedef struct mi_packed422_frame_dev { const void* in; void* out; } mi_packed422_frame_dev;
mi_status mi_equalize_hist_packed422_frames_dev(mi_ctx* ctx, const mi_packed422_frame_dev* frames, int n_frames,
                                                int width, int height, size_t in_pitch, size_t out_pitch,
                                                int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_packed422_frames_dev(mi_ctx* ctx, const mi_packed422_frame_dev* frames, int n_frames,
                                        int width, int height, size_t in_pitch, size_t out_pitch,
                                        int format, mi_uv_mode uv_mode,
                                        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_packed422_to_nv12_batch_dev: packed 4:2:2 frames in, NV12 frames out, in the pass that equalizes -- capture card -> encoder
 * without a format conversion of its own (every pipeline of the reference hands NV12 to its encoder).  The packed frame is read twice
 * (histograms, then map) exactly as by mi_*_packed422_batch_dev; the second pass writes 1.5*W*H bytes instead of 2*W*H.
 *   input  : exactly what mi_*_packed422_batch_dev takes.  `format` is MI_FMT_YUY2 or MI_FMT_UYVY; frame f lies at
 *            d_in + f * in_frame_stride, H rows of 2*W bytes at in_pitch; the pointer, the pitch and the frame stride are multiples
 *            of 4.  The input is never written.
 *   output : frame f has a Y plane at d_y_out + f * out_frame_stride, H rows of W bytes at y_pitch, and a UV plane at
 *            d_uv_out + f * out_frame_stride, H/2 rows of W bytes (interleaved U and V) at uv_pitch.  A tight NV12 batch is
 *            d_uv_out = d_y_out + W*H, both pitches W, out_frame_stride = W*H*3/2; pitched encoder surfaces in one allocation are the
 *            general case.  Both output pointers, both pitches and out_frame_stride are multiples of 4; y_pitch >= W, uv_pitch >= W.
 *            Consequence: a TIGHT NV12 batch with W % 4 == 2 has a pitch that is not a multiple of 4 and is refused -- such a caller
 *            pads the pitch.
 *   luma   : byte for byte what mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev return on the gathered W x H luma plane, hence
 *            also what mi_*_packed422_batch_dev put into the packed output (same clahe_fp_contract option, REFLECT_101 padding when
 *            the tile grid does not divide the frame, the same fallback for tile grids too wide for the LDS pair table).
 *   chroma : MI_UV_FILL128 sets every UV byte to 128.  MI_UV_COPY keeps the chroma and halves it vertically: for UV row r, the U (and
 *            the V) sample of macropixel m is the rounding mean of input rows 2r and 2r+1, (a + b + 1) >> 1 on the two input bytes.
 *            No horizontal filtering and no change of siting.  OpenCV has no call for this conversion and the reference has none: the
 *            rule is this header's own, it has no outside pin.
 * Nothing outside the W bytes of each output row is written: not the pitch padding, not the space between the planes, not the gap
 * between frames.  `width` is even; `height` is even too (NV12 has half as many chroma rows).
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 * the same shape as mi_*_packed422_batch_dev.  Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel; the
 * chroma is written by the launch that writes the luma (equalizeHist on up to one chunk of frames: one MI_K_HIST, one MI_K_EQ_LUT and
 * one MI_K_LUT_APPLY launch, for either uv_mode); launches are charged to the existing profiling slots by role.
 * Errors, MI_ERR_BAD_ARG: a null ctx or any null frame pointer, an odd width or an odd height, a negative size, in_pitch < 2*W,
 * y_pitch < W or uv_pitch < W, any pointer / pitch / stride that is not a multiple of 4, a format other than the two, a bad uv_mode,
 * tiles <= 0, d_y_out == d_in or d_uv_out == d_in (the layouts differ: there is no in-place form).  width, height or n_frames of 0:
 * MI_OK, nothing written -- except that the shape rules come first: an odd width or an odd height is MI_ERR_BAD_ARG even when another
 * size is 0 (as an odd width is for the packed forms).  Sizes and tile grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.
 * Any other overlap of input and output: undefined, not checked.  Nothing is enqueued unless all checks pass. */
mi_status mi_equalize_hist_packed422_to_nv12_batch_dev(mi_ctx* ctx,
        const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_packed422_to_nv12_batch_dev(mi_ctx* ctx,
        const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_packed422_to_nv12_frames_dev: the same conversion on a LIST of device frames, each at its own three addresses -- a capture
 * device's buffer pool in (every YUY2 / UYVY buffer its own allocation, as for mi_*_packed422_frames_dev), an encoder's surface pool
 * out (every NV12 surface its own pitched Y and UV plane, as for mi_*_nv12_frames_dev).  The contract is the union of the two forms it
 * joins.  `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device pointers on the
 * context's device.  Every frame of one call has the same width, height, format and the same three pitches (bytes between rows):
 *   in    : H rows of 2*W bytes at in_pitch >= 2*W       y_out : H rows of W bytes at y_pitch >= W
 *   uv_out: H/2 rows of W bytes (interleaved U and V) at uv_pitch >= W
 * Width and height are even.  Every address and every pitch is a multiple of 4; each frame may have its own alignment modulo 16
 * (slower never by design, different bytes never).  As in the batch form, a TIGHT NV12 pitch with W % 4 == 2 is not a multiple of 4
 * and is refused here: such a caller pads the pitch (the host form below accepts it).  The same input may appear in several entries.
 * The luma and the chroma of every frame are byte for byte what mi_*_packed422_to_nv12_batch_dev writes for that frame: the same
 * clahe_fp_contract option, REFLECT_101 padding, the same fallback for tile grids too wide for the LDS tables, (a + b + 1) >> 1 chroma
 * under MI_UV_COPY and 128 under MI_UV_FILL128.  Nothing outside the W bytes of each output row is written; the inputs are never
 * written.
 * There is no in-place form (the layouts differ): MI_ERR_BAD_ARG when the rows of a frame's Y or UV output meet the rows of its own
 * input, or when its Y rows meet its UV rows.  Outputs of DIFFERENT frames that overlap each other (or another frame's input) give
 * undefined results and are not checked.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 * the same shape as mi_*_packed422_frames_dev.  Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel;
 * launches are charged to the existing profiling slots by role (equalizeHist: one MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY
 * launch per chunk of the list, for either uv_mode).
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, a null in / y_out / uv_out, an odd width or an odd height
 * (refused even when another size is 0), a negative size, a format other than MI_FMT_YUY2 / MI_FMT_UYVY, a bad uv_mode, tiles <= 0,
 * in_pitch < 2*W, y_pitch < W or uv_pitch < W, any address or pitch that is not a multiple of 4, the overlaps above.  Sizes and tile
 * grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.  n_frames, width or height of 0: MI_OK,
 * nothing written.  Nothing is enqueued unless every frame passes the checks.
 *
 * mi_equalize_hist_packed422_to_nv12 / mi_clahe_packed422_to_nv12: ONE host frame, synchronous, like mi_*_packed422: the packed frame
 * goes up (2 bytes per pixel), the two planes come back (1.5 bytes per pixel).  The input side follows the rules of mi_*_packed422
 * (`in` and in_pitch multiples of 4, in_pitch >= 2*W; only the 2*W bytes of each row are read).  The output side is host memory the
 * kernels never see: y_out and uv_out may lie at ANY address, y_pitch and uv_pitch are any values >= W -- a tight host NV12 frame with
 * W % 4 == 2 is accepted (the device staging is pitched, the rows are copied out).  Only the W bytes of each output row are written.
 * Planes in memory registered with mi_host_register (or otherwise found pinned) that are tight, with W % 4 == 0 for the outputs, are
 * DMA'd as they are; everything else goes through the context's pinned staging (statistics "host_planes_direct" /
 * "host_planes_staged", three planes a call).  Whatever the call returns, no copy on in / y_out / uv_out is in flight any more when it
 * returns.  MI_ERR_BAD_ARG when the rows of an output plane meet the rows of the input or of the other plane; shape, mode, size and
 * zero-size rules as the device form above. */
typedef struct mi_packed422_nv12_frame_dev { const void* in; void* y_out; void* uv_out; } mi_packed422_nv12_frame_dev;
mi_status mi_equalize_hist_packed422_to_nv12_frames_dev(mi_ctx* ctx, const mi_packed422_nv12_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch,
        int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_packed422_to_nv12_frames_dev(mi_ctx* ctx, const mi_packed422_nv12_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch,
        int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_packed422_to_nv12(mi_ctx* ctx, const uint8_t* in, size_t in_pitch,
        uint8_t* y_out, size_t y_pitch, uint8_t* uv_out, size_t uv_pitch,
        int width, int height, int format, mi_uv_mode uv_mode);
mi_status mi_clahe_packed422_to_nv12(mi_ctx* ctx, const uint8_t* in, size_t in_pitch,
        uint8_t* y_out, size_t y_pitch, uint8_t* uv_out, size_t uv_pitch,
        int width, int height, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);

/* mi_*_nv12_to_bgr*: NV12 frames in, interleaved 8-bit BGR (or RGB) images out, in the pass that equalizes -- decoder -> display, image
 * writer or model without an NV12 intermediate.  Per frame the result is what OpenCV 4.4 gives for
 *     cv::Mat y = nv12(Rect(0, 0, W, H));  cv::equalizeHist(y, y)  /  clahe->apply(y, y);        (Y only, UV untouched)
 *     cv::cvtColor(nv12, bgr, cv::COLOR_YUV2BGR_NV12);                                           (COLOR_YUV2RGB_NV12 for MI_ORDER_RGB)
 * and byte for byte what mi_equalize_hist_nv12_batch_dev / mi_clahe_nv12_batch_dev with MI_UV_COPY followed by
 * mi_cvt_color_420_u8_batch_dev(..., MI_COLOR_YUV2BGR_NV12) writes in two calls: the same clahe_fp_contract option, the same REFLECT_101
 * padding when the tile grid does not divide the frame, the same limits on sizes and tile grids.  The two calls move 8.5 bytes per
 * pixel and need an NV12 batch in between; this form reads Y twice (histograms, then map), UV once, and writes 3 bytes per pixel: 5.5.
 *   input  : frame f has a Y plane at d_y + f * in_frame_stride, H rows of W bytes at y_pitch >= W, and a UV plane at
 *            d_uv + f * in_frame_stride, H/2 rows of W bytes (interleaved U and V) at uv_pitch >= W.  A tight NV12 batch is
 *            d_uv = d_y + W*H, both pitches W, in_frame_stride = W*H*3/2; pitched decoder surfaces in one allocation are the general
 *            case.  The input is never written.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 3*W bytes at out_pitch >= 3*W: B, G, R per pixel (MI_ORDER_BGR) or
 *            R, G, B (MI_ORDER_RGB).  Only the 3*W bytes of each output row are written: not the pitch padding, not the gap between
 *            frames.
 * Width and height are even.  No alignment is required of any pointer, pitch or stride: when W % 16 == 0 and every pointer, pitch and
 * frame stride is a multiple of 16 the kernels move 16 bytes per access, otherwise bytes -- slower, the same bytes out.
 * equalizeHist maps the luma and converts in one kernel.  CLAHE does so for the common shape -- the tile grid divides the frame,
 * tile width a multiple of 16, tiles_x <= 14, everything 16-byte aligned as above, clahe_fp_contract off; any other shape runs the planar
 * CLAHE into a scratch Y plane of the context and converts from there: the same bytes in one more pass (statistics "nv12_bgr_onepass" /
 * "nv12_bgr_twopass" count the calls of each kind).  Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel
 * (option two_kernel_max_frames does not apply).  Launches are charged to the existing profiling slots by role: MI_K_HIST, MI_K_EQ_LUT,
 * MI_K_TILE_HIST, MI_K_TILE_LUT for the histogram stages, MI_K_LUT_APPLY / MI_K_CLAHE_INTERP for the kernel that maps and converts,
 * MI_K_COLOR for the conversion of the two-pass fallback.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 * same shape as the other batched device forms.
 * mi_equalize_hist_nv12_to_bgr / mi_clahe_nv12_to_bgr: ONE tight NV12 frame in host memory (W*H*3/2 bytes) in, a CV_8UC3 image at
 *   out_step >= 3*W out; synchronous, staged like mi_nv12_bgr_equalize / mi_cvt_color_420_u8 (images in pinned memory that are tight are
 *   DMA'd as they are, everything else goes through the context's pinned staging).  Whatever the call returns, no copy on nv12_in / out is
 *   in flight any more when it returns.  W*H beyond what mi_cvt_color_420_u8 accepts: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx or plane pointer, an odd width or an odd height (refused even when another size is 0, as in the
 * packed -> NV12 forms), a negative size, a pitch below its row (y_pitch < W, uv_pitch < W, out_pitch < 3*W), an `order` other than the
 * two, tiles <= 0, d_out == d_y or d_out == d_uv (there is no in-place form).  Any other overlap of input and output: undefined, not
 * checked.  width, height or n_frames of 0: MI_OK, nothing written.  Sizes and tile grids the planar forms refuse: the status they give
 * (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued unless all checks pass. */
enum { MI_ORDER_BGR = 0, MI_ORDER_RGB = 1 };
mi_status mi_equalize_hist_nv12_to_bgr_batch_dev(mi_ctx* ctx, const void* d_y, size_t y_pitch, const void* d_uv, size_t uv_pitch,
        size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, void* stream);
mi_status mi_clahe_nv12_to_bgr_batch_dev(mi_ctx* ctx, const void* d_y, size_t y_pitch, const void* d_uv, size_t uv_pitch,
        size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_nv12_to_bgr(mi_ctx* ctx, const uint8_t* nv12_in, uint8_t* out, size_t out_step,
        int width, int height, int order);
mi_status mi_clahe_nv12_to_bgr(mi_ctx* ctx, const uint8_t* nv12_in, uint8_t* out, size_t out_step,
        int width, int height, int order, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_nv12_to_bgr_frames_dev: the same conversion on a LIST of device frames, each at its own three addresses -- a hardware decoder's
 * surface pool in (every NV12 surface its own allocation with a pitched Y and a pitched UV plane, as for mi_*_nv12_frames_dev), a pool of
 * images out.  Repacking such a pool into a batch costs 3 bytes per pixel moved on top of the 5.5 of the conversion; one batch call per
 * surface costs a launch sequence per frame.  `frames` is a host array of n_frames entries, read only during the call; the pointers in
 * it are device pointers on the context's device.
 * Shape: all frames of one call share width, height, order and the three pitches (bytes between rows); each has its own addresses:
 *   y  : H rows of W bytes at y_pitch >= W            uv : H/2 rows of W bytes (interleaved U and V) at uv_pitch >= W
 *   out: H rows of 3*W bytes at out_pitch >= 3*W -- B, G, R per pixel (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB)
 * Bytes: per frame exactly what mi_*_nv12_to_bgr_batch_dev writes for the same pixels at the same pitches -- cv::equalizeHist /
 * CLAHE::apply on Y, then cvtColor(COLOR_YUV2BGR_NV12 / COLOR_YUV2RGB_NV12); the clahe_fp_contract option is honoured, REFLECT_101
 * padding applies when the tile grid does not divide the frame, the limits on sizes and tile grids are the batch form's, with the
 * same statuses.
 * Writes: only the 3*W bytes of each output row are written, not the pitch padding; the input planes are never written.
 * Alignment: none is required of any address or pitch.  The per-frame alignment decides the access width: when W % 16 == 0 and the
 * three pitches are multiples of 16, a frame whose three addresses are multiples of 16 moves 16 bytes per access and any other frame
 * of the same call moves bytes, while its neighbours stay vectorised -- slower, the same bytes out.  equalizeHist always maps the luma
 * and converts in one kernel.  CLAHE does so when the shape is the batch form's one-pass shape (the tile grid divides the frame, tile
 * width a multiple of 16, tiles_x <= 14, the three pitches multiples of 16, clahe_fp_contract off) and every address of every frame of
 * the call is a multiple of 16; otherwise the whole call runs the planar CLAHE into scratch Y planes of the context and converts from
 * there: the same bytes in one more pass.  Statistics "nv12_bgr_onepass" / "nv12_bgr_twopass" count the calls of the list form too,
 * one count a call.  Launches are charged to the same profiling slots as the batch form, per chunk of 64 frames of the list.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image meet the rows of its own Y or UV plane
 * (compared as address ranges).  The same input planes may appear in several entries (inputs are only read).  Outputs that overlap
 * each other or ANOTHER frame's planes give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, a null y / uv / out in any entry, a negative size, an odd
 * width or an odd height (refused even when another size is 0, as in the batch form), a pitch below its row (y_pitch < W,
 * uv_pitch < W, out_pitch < 3*W), an `order` other than the two, tiles <= 0, the overlap above.  Sizes and tile grids the batch form
 * refuses: the status it gives (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written.
 * Nothing is enqueued unless every frame passes the checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 * the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
typedef struct mi_nv12_bgr_frame_dev { const void* y; const void* uv; void* out; } mi_nv12_bgr_frame_dev;
mi_status mi_equalize_hist_nv12_to_bgr_frames_dev(mi_ctx* ctx, const mi_nv12_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t uv_pitch, size_t out_pitch, int order, void* stream);
mi_status mi_clahe_nv12_to_bgr_frames_dev(mi_ctx* ctx, const mi_nv12_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t uv_pitch, size_t out_pitch, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);

/* mi_*_packed422_to_bgr*: packed 4:2:2 frames in (YUY2 / UYVY), interleaved 8-bit BGR (or RGB) images out, in the pass that equalizes --
 * capture card -> display, image writer or model.  Per frame the result is what OpenCV 4.4 gives for
 *     cv::extractChannel(frame, y, off);  cv::equalizeHist(y, y)  /  clahe->apply(y, y);  cv::insertChannel(y, frame, off);
 *     cv::cvtColor(frame, bgr, cv::COLOR_YUV2BGR_YUY2);              (_UYVY for MI_FMT_UYVY; COLOR_YUV2RGB_* for MI_ORDER_RGB)
 * The packed frame is read twice (histograms, then map) and 3 bytes per pixel are written: 7 bytes per pixel.  The two-call route,
 * mi_*_packed422_to_nv12_batch_dev followed by mi_cvt_color_420_u8_batch_dev(MI_COLOR_YUV2BGR_NV12), moves 5.5 + 4.5 = 10, needs an NV12
 * batch in between and gives DIFFERENT pixels: it halves the chroma vertically, this form keeps the chroma of every row.
 *   input  : exactly what mi_*_packed422_batch_dev takes: frame f at d_in + f * in_frame_stride, H rows of 2*W bytes at in_pitch >= 2*W;
 *            the pointer, the pitch and the frame stride are multiples of 4; `width` is even, `height` any value >= 1 (neither side
 *            subsamples vertically: odd heights are legal).  The input is never written.
 *   format : HERE THE CHROMA ORDER MATTERS, unlike in every other packed form (the comment on MI_FMT_YUY2 above, "the chroma order is
 *            irrelevant", does not hold for these entry points): MI_FMT_YUY2 means exactly Y0 U Y1 V, MI_FMT_UYVY exactly U Y0 V Y1.  A
 *            YVYU or VYUY frame passed as one of the two comes out with U and V swapped; those layouts are not supported by this form.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 3*W bytes at out_pitch >= 3*W: B, G, R per pixel (MI_ORDER_BGR) or
 *            R, G, B (MI_ORDER_RGB).  Only the 3*W bytes of each output row are written: not the pitch padding, not the gap between
 *            frames.  No alignment is required of d_out, out_pitch or out_frame_stride -- a tight image with W % 4 == 2 is accepted.
 *            Speed note: when d_out, out_pitch and out_frame_stride are multiples of 4 the kernels store 16 bytes per access (dwords
 *            in the ragged last 16-column group of a row), otherwise they take the byte-granular path -- slower, the same bytes out.
 *   luma   : byte for byte what mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev return on the gathered W x H luma plane (same
 *            clahe_fp_contract option, REFLECT_101 padding when the tile grid does not divide the frame, the same fallback for tile
 *            grids too wide for the LDS pair table as the other packed forms).
 *   pixels : (x, y) and (x+1, y) of a macropixel are decoded with that macropixel's own U and V, in the arithmetic of
 *            mi_cvt_color_420_u8 (MI_COLOR_YUV2BGR_NV12): OpenCV 4.4's ITUR_BT_601 integer decode, shift 20.  No vertical sharing, no
 *            filtering, and no uv_mode parameter (the NV12 -> BGR form has none either).
 * Every shape runs in one pass: there is no scratch Y plane and no two-pass fallback.  Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the
 * context's pipe has frames pending and hipGraph capture after one eager call of the same shape as the other batched device forms.
 * Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel; launches are charged to the existing profiling
 * slots by role: MI_K_HIST, MI_K_EQ_LUT, MI_K_LUT_APPLY, MI_K_TILE_HIST, MI_K_TILE_LUT, MI_K_CLAHE_INTERP (equalizeHist on up to one chunk
 * of frames: one MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch).  The frame-list form, mi_*_packed422_to_bgr_frames_dev, follows below.
 * mi_equalize_hist_packed422_to_bgr / mi_clahe_packed422_to_bgr: ONE packed host frame in, one image out, synchronous.  The input side
 *   follows the rules of mi_*_packed422 (`in` and in_pitch multiples of 4, in_pitch >= 2*W; only the 2*W bytes of each row are read),
 *   the output side those of mi_*_nv12_to_bgr (any address, any out_step >= 3*W; only the 3*W bytes of each row are written).  Tight
 *   buffers in pinned memory (mi_host_register) are DMA'd as they are, everything else goes through the context's pinned staging.
 *   Whatever the call returns, no copy on in / out is in flight any more when it returns.  MI_ERR_BAD_ARG when the rows of the image
 *   meet the rows of the input; W*H beyond what mi_cvt_color_420_u8 accepts: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx or frame pointer, an odd width (refused even when another size is 0, as in the packed forms), a
 * negative size, in_pitch < 2*W or out_pitch < 3*W, an input pointer / pitch / frame stride that is not a multiple of 4, a `format` or
 * an `order` other than the two, tiles <= 0, d_out == d_in (there is no in-place form).  Any other overlap of input and output:
 * undefined, not checked.  width, height or n_frames of 0: MI_OK, nothing written.  Sizes and tile grids the planar forms refuse: the
 * status they give (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued unless all checks pass. */
mi_status mi_equalize_hist_packed422_to_bgr_batch_dev(mi_ctx* ctx,
        const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, int order, void* stream);
mi_status mi_clahe_packed422_to_bgr_batch_dev(mi_ctx* ctx,
        const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_packed422_to_bgr(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
        int width, int height, int format, int order);
mi_status mi_clahe_packed422_to_bgr(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
        int width, int height, int format, int order, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_packed422_to_bgr_frames_dev: the same conversion on a LIST of device frames, each at its own two addresses -- a capture device's
 * buffer pool in (every YUY2 / UYVY buffer its own pitched allocation, as for mi_*_packed422_frames_dev), a pool of images out (one
 * tensor or cv::Mat per frame).  Repacking both pools into a batch moves 10 bytes per pixel on top of the 7 of the conversion; one batch
 * call per buffer costs a launch sequence per frame.  `frames` is a host array of n_frames entries, read only during the call; the
 * pointers in it are device pointers on the context's device.
 * Shape: all frames of one call share width, height, format, order and the two pitches (bytes between rows); each has its own addresses:
 *   in : H rows of 2*W bytes at in_pitch >= 2*W     out: H rows of 3*W bytes at out_pitch >= 3*W -- B, G, R per pixel (MI_ORDER_BGR) or
 *                                                        R, G, B (MI_ORDER_RGB)
 * Bytes: per frame exactly what mi_*_packed422_to_bgr_batch_dev writes for the same pixels -- the luma of the planar forms, every row
 * decoded with its own chroma, MI_FMT_YUY2 exactly Y0 U Y1 V and MI_FMT_UYVY exactly U Y0 V Y1 (the chroma order matters, as above); the
 * clahe_fp_contract and clahe_float_tables options apply as in the batch form, as do REFLECT_101 padding and the fallback for tile grids
 * too wide for the LDS pair table.  Every CLAHE shape runs in one pass: there is no scratch Y plane and no two-pass fallback.
 * Input side: the rules of mi_*_packed422_frames_dev.  Width is even, height any value >= 1; in_pitch is a multiple of 4; every `in` is
 * a multiple of 4, at its own alignment modulo 16.  The same input may appear in several entries.  The inputs are never written.
 * Output side: NO alignment rule -- any `out`, odd addresses included, any out_pitch >= 3*W, a tight image with W % 4 == 2 included.
 * Only the 3*W bytes of each output row are written, not the pitch padding.  The per-frame address decides the store width: when
 * out_pitch is a multiple of 4, a frame whose `out` is a multiple of 4 stores 16 bytes per access (dwords in the ragged last 16-column
 * group of a row) and any other frame of the same call stores bytes, while its neighbours stay wide -- slower, the same bytes out.
 * mi_ctx_get_stat "packed422_bgr_list_frames_wide" / "packed422_bgr_list_frames_bytes" count the FRAMES (not calls) of each kind, for
 * calls that were enqueued.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image meet the rows of its own input (compared as
 * address ranges).  Images that overlap each other or ANOTHER frame's input give undefined results and are not checked.
 * Launches are charged to the same profiling slots as the batch form, per chunk of 128 frames of the list (equalizeHist: one MI_K_HIST,
 * one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch per chunk).  Never the fused equalizeHist kernel nor the single-launch histogram + LUT
 * kernel.  Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call
 * of the same shape as the other device list forms; a captured graph holds the addresses it was captured with.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, a null in / out in any entry, an `in` that is not a multiple
 * of 4, an odd width (refused even when another size is 0), a negative size, in_pitch < 2*W or not a multiple of 4, out_pitch < 3*W, a
 * `format` or an `order` other than the two, tiles <= 0, the overlap above.  Sizes and tile grids the batch form refuses (more than 65535
 * tiles, a height above 65535 with tiles_x > 62, what the planar forms refuse): the status it gives (MI_ERR_UNSUPPORTED).  width,
 * height or n_frames of 0: MI_OK, nothing written.  Nothing is enqueued unless every frame passes the checks: a bad last entry leaves
 * the first frames' images untouched. */
typedef struct mi_packed422_bgr_frame_dev { const void* in; void* out; } mi_packed422_bgr_frame_dev;   /* 16 bytes on LP64 */
mi_status mi_equalize_hist_packed422_to_bgr_frames_dev(mi_ctx* ctx, const mi_packed422_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int format, int order, void* stream);
mi_status mi_clahe_packed422_to_bgr_frames_dev(mi_ctx* ctx, const mi_packed422_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int format, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_packed422_to_bgra*: packed 4:2:2 frames in (YUY2 / UYVY), interleaved 8-bit FOUR-channel images (CV_8UC4: BGRA, or RGBA) out, in
 * the pass that equalizes -- capture card -> display surface, swap-chain image, GL / Vulkan / interop texture or GUI image, without a
 * three-channel image in scratch and a widen to four channels outside the library.  Per frame the result is what OpenCV 4.4 gives for
 *     cv::extractChannel(frame, y, off);  cv::equalizeHist(y, y)  /  clahe->apply(y, y);  cv::insertChannel(y, frame, off);
 *     cv::cvtColor(frame, bgra, cv::COLOR_YUV2BGRA_YUY2);            (_UYVY for MI_FMT_UYVY; COLOR_YUV2RGBA_* for MI_ORDER_RGB)
 * The packed frame is read twice (histograms, then map) and 4 bytes per pixel are written: 8 bytes per pixel, where
 * mi_*_packed422_to_bgr_batch_dev into scratch plus a widen outside the library moves about 14.  The names, the argument order and
 * everything not said here are those of mi_*_packed422_to_bgr* above.
 *   pixels : the first three bytes of every pixel are byte for byte what mi_*_packed422_to_bgr* writes for the same call with the same
 *            `format` and `order`; the fourth byte is 255 (A), what OpenCV's four-channel YUV decodes write.  Every row is decoded with
 *            its own chroma.  THE CHROMA ORDER MATTERS as in that form: MI_FMT_YUY2 means exactly Y0 U Y1 V, MI_FMT_UYVY exactly
 *            U Y0 V Y1; YVYU and VYUY are not supported.
 *   input  : exactly the packed forms': frame f at d_in + f * in_frame_stride, H rows of 2*W bytes at in_pitch >= 2*W; the pointer, the
 *            pitch and the frame stride are multiples of 4; `width` is even, `height` any value >= 1 (odd heights are legal).  The input
 *            is never written.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 4*W bytes at out_pitch >= 4*W: B, G, R, A per pixel (MI_ORDER_BGR) or
 *            R, G, B, A (MI_ORDER_RGB).  Only the 4*W bytes of each output row are written: not the pitch padding, not the gap between
 *            frames.  No alignment is required of d_out, out_pitch or out_frame_stride: an odd address and an odd pitch are legal.
 *   stores : a frame is WIDE when its image address is a multiple of 4 and so are out_pitch and, for a batch, out_frame_stride.  A wide
 *            frame stores a 16-column group as four 16-byte stores (every dword one pixel: no pixel straddles a dword) and the ragged
 *            last group of a row (W % 16 != 0) as dword stores.  Any other frame stores bytes -- slower, the same bytes out.
 *   CLAHE  : every shape runs in one pass: there is no scratch Y plane and no two-pass fallback.  REFLECT_101 padding applies when the
 *            tile grid does not divide the frame; the clahe_fp_contract and clahe_float_tables options apply as in the three-channel
 *            form, as does the global-memory fallback for tile grids too wide for the LDS pair table.
 * Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel; launches are charged to the existing profiling
 * slots by role, as in the three-channel form.  Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and
 * hipGraph capture after one eager call of the same shape as the other batched device forms.
 * Counters (mi_ctx_get_stat): "packed422_bgra_wide" / "packed422_bgra_bytes" count the batch and host CALLS by the store path of their
 * launch; a call that returns an error or has nothing to do moves neither.  No existing counter moves on a call of this form.
 * mi_equalize_hist_packed422_to_bgra / mi_clahe_packed422_to_bgra: ONE packed host frame in, one CV_8UC4 image out, synchronous.  The
 *   input side follows the rules of mi_*_packed422 (`in` and in_pitch multiples of 4, in_pitch >= 2*W; only the 2*W bytes of each row are
 *   read); the output is host memory at any address and any out_step >= 4*W, only the 4*W bytes of each row are written.  Tight buffers
 *   in pinned memory (mi_host_register) are DMA'd as they are, everything else goes through the context's pinned staging; the device
 *   image is tight and aligned, so the call counts as wide.  Whatever the call returns, no copy on in / out is in flight any more when
 *   it returns.  MI_ERR_BAD_ARG when the rows of the image meet the rows of the input; W*H > 0x7fffffff / 4: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx or frame pointer, an odd width (refused even when another size is 0, as in the packed forms), a
 * negative size, in_pitch < 2*W or out_pitch < 4*W, an input pointer / pitch / frame stride that is not a multiple of 4, a `format` or
 * an `order` other than the two, tiles <= 0, d_out == d_in (there is no in-place form).  Any other overlap of input and output:
 * undefined, not checked.  width, height or n_frames of 0: MI_OK, nothing written.  Sizes and tile grids the three-channel form refuses
 * (more than 65535 tiles, a height above 65535 with tiles_x > 62, what the planar forms refuse): the status it gives
 * (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued unless all checks pass. */
mi_status mi_equalize_hist_packed422_to_bgra_batch_dev(mi_ctx* ctx,
        const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, int order, void* stream);
mi_status mi_clahe_packed422_to_bgra_batch_dev(mi_ctx* ctx,
        const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_packed422_to_bgra(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
        int width, int height, int format, int order);
mi_status mi_clahe_packed422_to_bgra(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
        int width, int height, int format, int order, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_packed422_to_bgra_frames_dev: the same conversion on a LIST of device frames, each at its own two addresses -- a capture
 * device's buffer pool in, a swap chain or a pool of CV_8UC4 surfaces, textures or cv::Mats out.  `frames` is a host array of n_frames
 * entries of the existing mi_packed422_bgr_frame_dev {in, out}, read only during the call; the pointers in it are device pointers on the
 * context's device.
 * Shape: all frames of one call share width, height, format, order and the two pitches (bytes between rows); each has its own addresses:
 *   in : H rows of 2*W bytes at in_pitch >= 2*W     out: H rows of 4*W bytes at out_pitch >= 4*W -- B, G, R, A per pixel (MI_ORDER_BGR)
 *                                                        or R, G, B, A (MI_ORDER_RGB), A = 255
 * Bytes: per frame exactly what mi_*_packed422_to_bgra_batch_dev writes for that frame alone at the same pitches; the clahe_fp_contract
 * and clahe_float_tables options, REFLECT_101 padding and the fallback for tile grids too wide for the LDS pair table apply as in the
 * batch form.  Every CLAHE shape runs in one pass: there is no scratch Y plane and no two-pass fallback.
 * Input side: the rules of mi_*_packed422_frames_dev.  Width is even, height any value >= 1; in_pitch is a multiple of 4; every `in` is
 * a multiple of 4, at its own alignment modulo 16.  The same input may appear in several entries.  The inputs are never written.
 * Output side: NO alignment rule -- any `out`, odd addresses included, any out_pitch >= 4*W.  Only the 4*W bytes of each output row are
 * written, not the pitch padding.  The store-path rule of the batch form is applied PER FRAME: when out_pitch is a multiple of 4, a
 * frame whose `out` is a multiple of 4 is wide and any other frame of the same call stores bytes, while its neighbours stay wide --
 * slower, the same bytes out.  mi_ctx_get_stat "packed422_bgra_list_frames_wide" / "packed422_bgra_list_frames_bytes" count the FRAMES
 * (not calls) of each kind, n_frames in total per call, for calls that were enqueued; list calls do not touch "packed422_bgra_wide" /
 * "packed422_bgra_bytes", and no existing counter moves.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image (4*W bytes each) meet the rows of its own input
 * (compared as address ranges).  Images that overlap each other or ANOTHER frame's input give undefined results and are not checked.
 * Launches are charged to the same profiling slots as the batch form, per chunk of 128 frames of the list (equalizeHist: one MI_K_HIST,
 * one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch per chunk).  Never the fused equalizeHist kernel nor the single-launch histogram + LUT
 * kernel.  Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call
 * of the same shape as the other device list forms; a captured graph holds the addresses it was captured with.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, a null in / out in any entry, an `in` that is not a multiple
 * of 4, an odd width (refused even when another size is 0), a negative size, in_pitch < 2*W or not a multiple of 4, out_pitch < 4*W, a
 * `format` or an `order` other than the two, tiles <= 0, the overlap above.  Sizes and tile grids the batch form refuses (more than 65535
 * tiles, a height above 65535 with tiles_x > 62, what the planar forms refuse): the status it gives (MI_ERR_UNSUPPORTED).  width,
 * height or n_frames of 0: MI_OK, nothing written.  Nothing is enqueued unless every frame passes the checks: a bad last entry leaves
 * the first frames' images untouched. */
mi_status mi_equalize_hist_packed422_to_bgra_frames_dev(mi_ctx* ctx, const mi_packed422_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int format, int order, void* stream);
mi_status mi_clahe_packed422_to_bgra_frames_dev(mi_ctx* ctx, const mi_packed422_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int format, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);

/* mi_*_bgr_to_nv12*: interleaved 8-bit BGR (or RGB) images in, pitched NV12 frames out with the luma equalized -- renderer, model output
 * or image reader -> hardware encoder without an I420 intermediate and without an interleave of U and V outside the library.  Per frame
 * the bytes are what OpenCV 4.4 gives for
 *     cv::cvtColor(bgr, i420, cv::COLOR_BGR2YUV_I420);                                           (COLOR_RGB2YUV_I420 for MI_ORDER_RGB)
 *     cv::Mat y = i420(Rect(0, 0, W, H));  cv::equalizeHist(y, y)  /  clahe->apply(y, y);        (Y only)
 * with the U and the V plane interleaved into an NV12 chroma plane (MI_UV_COPY) or every chroma byte 128 (MI_UV_FILL128).  Chroma comes
 * from the top-left pixel of each 2 x 2 block, without averaging, as in mi_cvt_color_420_u8 (MI_COLOR_BGR2YUV_I420).  The same
 * clahe_fp_contract option, the same REFLECT_101 padding when the tile grid does not divide the frame and the same limits on sizes and
 * tile grids as the planar forms.
 *   input  : frame f at d_in + f * in_frame_stride, H rows of 3*W bytes at in_pitch >= 3*W: B, G, R per pixel (MI_ORDER_BGR) or R, G, B
 *            (MI_ORDER_RGB).  The input is never written.
 *   output : frame f has a Y plane at d_y_out + f * out_frame_stride, H rows of W bytes at y_pitch >= W, and a UV plane at
 *            d_uv_out + f * out_frame_stride, H/2 rows of W bytes (interleaved U and V) at uv_pitch >= W.  A tight NV12 batch is
 *            d_uv_out = d_y_out + W*H, both pitches W, out_frame_stride = W*H*3/2; pitched encoder surfaces in one allocation are the
 *            general case.  Only the W bytes of each output row are written: not the pitch padding, not the gap between the planes,
 *            not the gaps between frames.
 * Width and height are even.  No alignment is required of any pointer, pitch or stride: when W % 16 == 0 and all three pointers, all
 * three pitches and both frame strides are multiples of 16 the conversion moves 16 bytes per access, otherwise bytes -- slower, the
 * same bytes out.
 * Two stages per chunk of 256 frames.  Y is not in the input, so stage 1 converts: ONE kernel (charged to MI_K_COLOR) reads the image
 * once, writes Y and UV into the caller's planes and, for equalizeHist, counts the luma bytes it has just produced.  Stage 2 maps the
 * luma IN PLACE in the output Y plane with the planar kernels: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no MI_K_HIST
 * launch; never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel, option two_kernel_max_frames does not
 * apply); CLAHE exactly what mi_clahe_u8_batch_dev launches for that plane, for every shape it takes -- no one-pass / two-pass split, no
 * scratch plane.  Bytes moved per pixel: equalizeHist 3 + 1.5 + 1 + 1 = 6.5, CLAHE 4.5 + 3 = 7.5.  Between the stages the output Y plane
 * holds the unequalized luma.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 * same shape as the other batched device forms.
 * mi_equalize_hist_bgr_to_nv12 / mi_clahe_bgr_to_nv12: ONE CV_8UC3 image in host memory at in_step >= 3*W, at any address, in, one tight
 *   NV12 frame of W*H*3/2 bytes out; synchronous, staged like mi_*_nv12_to_bgr (images in pinned memory that are tight are DMA'd as they
 *   are, everything else goes through the context's pinned staging).  Whatever the call returns, no copy on in / nv12_out is in flight
 *   any more when it returns.  W*H beyond what mi_cvt_color_420_u8 accepts: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx or a null pointer, an odd width or an odd height (refused even when another size is 0, as in the
 * NV12 -> BGR forms), a negative size, a pitch below its row (in_pitch < 3*W, y_pitch < W, uv_pitch < W), an `order` other than the two,
 * a bad uv_mode, tiles <= 0, d_y_out == d_in, d_uv_out == d_in or d_y_out == d_uv_out (there is no in-place form).  Any other overlap:
 * undefined, not checked.  width, height or n_frames of 0: MI_OK, nothing written.  Sizes and tile grids the planar forms refuse: the
 * status they give (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued unless all checks pass. */
mi_status mi_equalize_hist_bgr_to_nv12_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgr_to_nv12_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_bgr_to_nv12(mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* nv12_out,
        int width, int height, int order, mi_uv_mode uv_mode);
mi_status mi_clahe_bgr_to_nv12(mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* nv12_out,
        int width, int height, int order, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_bgr_to_nv12_frames_dev: the same conversion on a LIST of device frames, each at its own three addresses -- a pool of images in
 * (one tensor or buffer per frame, as renderers, models and image readers hand them over), a hardware encoder's surface pool out (every
 * NV12 surface its own allocation with a pitched Y and a pitched UV plane, as for mi_*_nv12_frames_dev).  Repacking such pools into a
 * batch and copying the planes out costs 3 + 1.5 bytes per pixel moved on top of the 6.5 / 7.5 of the conversion; one batch call per
 * surface costs a launch sequence per frame.  `frames` is a host array of n_frames entries, read only during the call; the pointers in
 * it are device pointers on the context's device.
 * Shape: all frames of one call share width, height, order, uv_mode and the three pitches (bytes between rows); each has its own
 * addresses:
 *   in : H rows of 3*W bytes at in_pitch >= 3*W -- B, G, R per pixel (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB)
 *   y  : H rows of W bytes at y_pitch >= W            uv : H/2 rows of W bytes (interleaved U and V) at uv_pitch >= W
 * Bytes: per frame exactly what mi_*_bgr_to_nv12_batch_dev writes for the same pixels at the same pitches -- cvtColor(COLOR_BGR2YUV_I420
 * / COLOR_RGB2YUV_I420) with U and V interleaved (MI_UV_COPY) or every chroma byte 128 (MI_UV_FILL128), then cv::equalizeHist /
 * CLAHE::apply on Y; the clahe_fp_contract option is honoured, REFLECT_101 padding applies when the tile grid does not divide the
 * frame, the limits on sizes and tile grids are the batch form's, with the same statuses.
 * Writes: only the W bytes of each output row are written, not the pitch padding; the images are never written.
 * Alignment: none is required of any address or pitch.  The per-frame alignment decides the access width of the conversion: when
 * W % 16 == 0 and the three pitches are multiples of 16, a frame whose three addresses are multiples of 16 moves 16 bytes per access
 * and any other frame of the same call moves bytes, while its neighbours stay vectorised -- slower, the same bytes out.
 * Two stages per chunk of 64 frames of the list, as in the batch form: ONE conversion kernel (MI_K_COLOR) reads the chunk's images once,
 * writes Y and UV and, for equalizeHist, counts the luma it has produced; then the luma is mapped IN PLACE in the Y planes:
 * equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no MI_K_HIST launch; never the fused equalizeHist kernel nor the
 * single-launch histogram + LUT kernel), CLAHE exactly what mi_clahe_nv12_frames_dev launches in place on the same Y planes.  Launches
 * are charged to the same profiling slots as the batch form.  Between the stages the Y planes hold the unequalized luma.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image meet the rows of its own Y or UV plane, or the
 * rows of its Y plane those of its own UV plane (compared as address ranges).  The same image may appear in several entries (inputs are
 * only read).  Outputs that overlap each other or ANOTHER frame's planes or image give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `frames` with n_frames > 0, a null in / y / uv in any entry, a negative size, an odd
 * width or an odd height (refused even when another size is 0, as in the batch form), a pitch below its row (in_pitch < 3*W,
 * y_pitch < W, uv_pitch < W), an `order` other than the two, a bad uv_mode, tiles <= 0, the overlap above.  Sizes and tile grids the
 * batch form refuses: the status it gives (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written.
 * Nothing is enqueued unless every frame passes the checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 * the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
typedef struct mi_bgr_nv12_frame_dev { const void* in; void* y; void* uv; } mi_bgr_nv12_frame_dev;
mi_status mi_equalize_hist_bgr_to_nv12_frames_dev(mi_ctx* ctx, const mi_bgr_nv12_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch, int order, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgr_to_nv12_frames_dev(mi_ctx* ctx, const mi_bgr_nv12_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch, int order, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);

/* mi_*_yuv420*: equalizeHist / CLAHE on the luma of 8-bit 4:2:0 frames whose two sides each say where their planes lie and whether
 * their chroma is interleaved (NV12: one plane of U, V pairs) or planar (I420 / YV12: a U plane and a V plane).  One form gives
 * I420 / YV12 -> I420 / YV12 (pitched planes, separately allocated planes, in place), I420 / YV12 -> NV12 (software decoder -> hardware
 * encoder surface), NV12 -> I420 / YV12 (hardware decoder or camera -> software encoder) and NV12 -> NV12, without plane copies or an
 * interleave of U and V outside the library.  c0 is always the U (Cb) plane and c1 the V (Cr) plane: YV12 needs no name of its own, a
 * YV12 caller passes the address of the SECOND chroma plane of its frame as c0 and that of the first as c1.  NV21 is not supported.
 * Both descriptors are read only during the call.  The planes of `in` are never written, except where a plane is processed in place.
 * Luma: for frame f the output Y plane is byte for byte what mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev write for the plane
 *   (in->y, in->y_pitch, in->frame_stride) -> (out->y, out->y_pitch, out->frame_stride): the same kernels chosen the same way for the
 *   batch (the fused equalizeHist kernel included, where it applies), the same clahe_fp_contract and two_kernel_max_frames options, the
 *   same REFLECT_101 padding when the tile grid does not divide the frame, the same limits on sizes and tile grids, the same statuses.
 * Chroma, MI_UV_COPY: every chroma sample is carried over unchanged into the output's layout.  planar -> interleaved:
 *   uv[r][2i] = U[r][i], uv[r][2i+1] = V[r][i]; interleaved -> planar: the inverse; same layout: a row copy.
 * Chroma, MI_UV_FILL128: every chroma byte of the output is 128.  in->c0 / in->c1 are not read and may be NULL; in->c_pitch and
 *   in->chroma's planes take no part in the checks below (in->chroma itself must still be one of the two values).
 * Writes: only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each output row are written: not the pitch padding, not
 *   the gaps between planes, not the gaps between frames.
 * Width and height are even.  No alignment is required of any pointer, pitch or stride.  A layout change moves 16 bytes per access
 *   when W % 32 == 0 and all chroma pointers, both c_pitch and both frame_stride are multiples of 16 (the Y side plays no part), and
 *   one U, V sample pair per access with byte loads and stores otherwise -- slower, the same bytes out.  A same-layout move and a fill
 *   have no rule: every row is written with aligned 16-byte stores and at most 15 + 15 byte stores at its ends, wherever it lies.
 * In place: a plane may be processed in place when it is EXACTLY the same plane on both sides: the same address, the same pitch, the
 *   same frame_stride and, for a chroma plane, the same layout.  In-place chroma with MI_UV_COPY moves nothing; with MI_UV_FILL128 it
 *   writes 128.  Y may be in place while the chroma is converted into other memory, and the other way round.
 * Launches: the luma is what the planar form launches for the whole batch; the chroma is ONE launch of its own per chunk of 256 frames,
 *   charged to MI_K_LUT_APPLY like the chroma kernels of the NV12 and P010 forms (no launch at all when every chroma plane is copied in
 *   place).  mi_ctx_get_stat "yuv420_chroma_vec" / "yuv420_chroma_bytes" count the calls whose chroma launch moved 16 bytes per access
 *   (every same-layout move and fill, and the layout changes the rule above admits) / changed the layout with byte accesses; a call that
 *   launches no chroma kernel counts in neither.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 *   same shape as the other batched device forms.
 * mi_equalize_hist_yuv420 / mi_clahe_yuv420: ONE frame with `in` / `out` holding HOST pointers, at any address and any pitch;
 *   frame_stride is ignored.  Synchronous, staged like mi_*_packed422_to_nv12: planes in pinned memory that are tight are DMA'd as they
 *   are, everything else goes through the context's pinned staging; on the device the frame is tight at the kernels' own pitches.
 *   Whatever the call returns, no copy on the caller's memory is in flight any more when it returns.  W*H beyond what
 *   mi_cvt_color_420_u8 accepts: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx, `in` or `out`; a null y; a null out->c0; a null out->c1 on a PLANAR output; a null input chroma
 *   pointer that MI_UV_COPY needs; a `chroma` other than the two values; a bad uv_mode; a negative size; an odd width or an odd height
 *   (refused even when another size is 0, as in the sibling forms); y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar);
 *   tiles <= 0; two output plane pointers of the call that are equal; an output plane pointer equal to an input plane pointer other than
 *   that exact in-place case (a c1 of an INTERLEAVED side is ignored throughout).  Any other overlap: undefined, not checked.  width,
 *   height or n_frames of 0: MI_OK, nothing written.  Sizes and tile grids the planar forms refuse: the status they give
 *   (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued unless all checks pass. */
enum { MI_CHROMA_INTERLEAVED = 0, MI_CHROMA_PLANAR = 1 };
typedef struct mi_yuv420_planes {
    void*  y;   size_t y_pitch;        /* H rows of W bytes */
    void*  c0;  void*  c1;             /* INTERLEAVED: c0 = UV plane, H/2 rows of W bytes (U first), c1 ignored (may be NULL)
                                          PLANAR:      c0 = U plane, c1 = V plane, each H/2 rows of W/2 bytes            */
    size_t c_pitch;                    /* bytes between chroma rows (both planes of a PLANAR side share it) */
    size_t frame_stride;               /* frame f: every plane pointer + f * frame_stride (ignored by the host forms) */
    int    chroma;                     /* MI_CHROMA_* */
} mi_yuv420_planes;                    /* 56 bytes on LP64 */
mi_status mi_equalize_hist_yuv420_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
        int width, int height, int n_frames, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_yuv420_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
        int width, int height, int n_frames, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_yuv420(mi_ctx* ctx, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
        int width, int height, mi_uv_mode uv_mode);
mi_status mi_clahe_yuv420(mi_ctx* ctx, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
        int width, int height, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_yuv420_frames_dev: the same on a LIST of device frames, each plane at its own address -- a software decoder's frame pool (every
 * frame three separately allocated, pitched planes: data[0..2], linesize[0..2]) in, a hardware encoder's surface pool (every NV12
 * surface its own allocation) out, or any other pairing of the two layouts.  The batch form needs the whole batch in one allocation at
 * a constant frame stride; one n_frames = 1 batch call per frame costs a launch sequence per frame, and repacking a pool into a batch
 * moves every byte twice more.  `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device
 * pointers on the context's device.
 * Shape: all frames of one call share width, height, uv_mode, the two layouts and the four pitches (bytes between rows: y_in_pitch and
 *   y_out_pitch >= W; c_in_pitch and c_out_pitch >= W for an INTERLEAVED side, >= W/2 for a PLANAR one, both planes of a planar side
 *   sharing theirs); each has its own addresses.  There are no per-frame pitches.
 * Chroma layout: in_chroma / out_chroma are MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR.  c0 is always the U plane and c1 the V plane: a
 *   YV12 caller exchanges the two addresses.  The c1 of an INTERLEAVED side is ignored and may be NULL.  With MI_UV_FILL128 the input
 *   chroma pointers and c_in_pitch are ignored (in_chroma must still be one of the two values).
 * Bytes: for every frame the output planes are byte for byte what mi_*_yuv420_batch_dev writes for that frame alone with n_frames = 1
 *   at the same pitches: cv::equalizeHist / CLAHE::apply on Y -- the clahe_fp_contract option is honoured, REFLECT_101 padding applies
 *   when the tile grid does not divide the frame -- and every chroma sample carried over into the output's layout (MI_UV_COPY) or every
 *   chroma byte 128 (MI_UV_FILL128).
 * Writes: only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each output row are written, not the pitch padding; the
 *   input planes are never written, except where a plane is processed in place.
 * Alignment: none is required of any address or pitch.  The per-frame alignment decides the access width of a layout change: when
 *   W % 32 == 0 and both c_pitch are multiples of 16 -- the batch form's rule without the frame-stride term -- a frame whose own chroma
 *   pointers are multiples of 16 moves 16 bytes per access, and any other frame of the same call moves one U, V sample pair per access
 *   while its neighbours stay vectorised -- slower, the same bytes out.  The Y side plays no part; a same-layout move and a fill have
 *   no rule.
 * In place, per frame: a plane is processed in place when it is EXACTLY the same plane on both sides of its entry: the same address,
 *   the same pitch and, for a chroma plane, the same layout.  In-place chroma with MI_UV_COPY moves nothing; with MI_UV_FILL128 it
 *   writes 128.  One list may mix in-place and out-of-place frames; Y may be in place while the chroma is not, and the other way round.
 * Launches, per chunk of 64 frames of the list: the luma is what mi_*_nv12_frames_dev launches for the same Y planes (the planar
 *   kernels' frame-list entries; never the fused equalizeHist kernel), then ONE launch of the chroma kernel's list entry, charged to
 *   MI_K_LUT_APPLY like the batch form's -- none for a chunk in which every frame copies all of its chroma in place.  Launches are
 *   charged to the same profiling slots as the batch form.  mi_ctx_get_stat "yuv420_list_frames_vec" / "yuv420_list_frames_bytes" count
 *   the FRAMES (not calls) of list calls that changed the layout under MI_UV_COPY with 16-byte / with byte accesses;
 *   "yuv420_chroma_vec" / "yuv420_chroma_bytes" are not touched by list calls.
 * Overlap: MI_ERR_BAD_ARG for two equal output plane pointers within a frame, and for an output plane pointer equal to an input plane
 *   pointer of the same frame other than the exact in-place case.  The checks are pointer equality, not address ranges, on purpose: a
 *   layout with the U and V rows side by side in one pitched plane (c1 = c0 + W/2, c_pitch = W) is legal here, as it is in the batch
 *   form.  Any other overlap -- within a frame, between outputs, with ANOTHER frame's planes -- is undefined and not checked.  The same
 *   input planes may appear in several entries (inputs are only read).
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; in any entry a null y_in / y_out, a null c0_out, a null c1_out
 *   on a PLANAR output, a null input chroma pointer that MI_UV_COPY needs; an in_chroma / out_chroma other than the two values; a bad
 *   uv_mode; a negative size; an odd width or an odd height (refused even when another size is 0, as in the batch form); a y pitch < W;
 *   a c pitch below its row; tiles <= 0; the overlap above.  Sizes and tile grids the planar forms refuse: the status they give
 *   (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written.  Nothing is enqueued unless every frame passes the
 *   checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
typedef struct mi_yuv420_frame_dev {
    const void* y_in;  const void* c0_in;  const void* c1_in;
    void*       y_out; void*       c0_out; void*       c1_out;
} mi_yuv420_frame_dev;                       /* 48 bytes on LP64 */
mi_status mi_equalize_hist_yuv420_frames_dev(mi_ctx* ctx, const mi_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t y_in_pitch, size_t c_in_pitch, int in_chroma,
        size_t y_out_pitch, size_t c_out_pitch, int out_chroma, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_yuv420_frames_dev(mi_ctx* ctx, const mi_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t y_in_pitch, size_t c_in_pitch, int in_chroma,
        size_t y_out_pitch, size_t c_out_pitch, int out_chroma, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_yuv420_to_bgr*: 4:2:0 frames described by mi_yuv420_planes in -- planar chroma (I420 / YV12: what a software decoder hands
 * over, ffmpeg yuv420p, libvpx, dav1d) or interleaved (NV12) -- interleaved 8-bit BGR (or RGB) images out, in the pass that equalizes:
 * software decoder -> model, display or image writer without an interleave of U and V outside the library and without an NV12
 * intermediate.  In OpenCV terms cv::equalizeHist / CLAHE::apply on the Y plane, then cv::cvtColor(COLOR_YUV2BGR_I420 / _YV12), the
 * RGB codes for MI_ORDER_RGB.  Y is read twice (histograms, then map), U and V once, 3 bytes per pixel are written: 5.5 B/px.
 *   input  : `in` is read only during the call.  Frame f has every plane at pointer + f * in->frame_stride: Y, H rows of W bytes at
 *            y_pitch >= W; PLANAR: c0 = U and c1 = V, each H/2 rows of W/2 bytes at c_pitch >= W/2; INTERLEAVED: c0 = the UV plane, H/2
 *            rows of W bytes at c_pitch >= W.  c0 is always U and c1 always V: a YV12 caller passes its second chroma plane as c0.
 *            The input is never written.
 *   output : as in the NV12 form: frame f at d_out + f * out_frame_stride, H rows of 3*W bytes at out_pitch >= 3*W, B, G, R per pixel
 *            (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB).  Only the 3*W bytes of each output row are written: not the pitch padding, not
 *            the gap between frames.  There is no in-place form.
 * Bytes: per frame byte for byte what mi_equalize_hist_nv12_to_bgr_batch_dev / mi_clahe_nv12_to_bgr_batch_dev writes for the same
 *   pixels with U and V interleaved, and what the two-call composition mi_*_yuv420_batch_dev(I420 -> NV12, MI_UV_COPY) followed by
 *   mi_cvt_color_420_u8_batch_dev(..., MI_COLOR_YUV2BGR_NV12) writes (8.5 B/px and a tight NV12 batch in between): the same
 *   clahe_fp_contract option, the same REFLECT_101 padding when the tile grid does not divide the frame, the planar forms' own limits on
 *   sizes and tile grids with their statuses.  Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel, as in
 *   the NV12 form.
 * in->chroma == MI_CHROMA_INTERLEAVED: the call IS the NV12 form's (d_y = in->y, d_uv = in->c0, uv_pitch = in->c_pitch,
 *   in_frame_stride = in->frame_stride; in->c1 ignored): the same kernels, the same alignment rule (multiples of 16 throughout), the
 *   same "nv12_bgr_onepass" / "nv12_bgr_twopass" counters; none of the counters below moves.
 * Alignment (MI_CHROMA_PLANAR): none is required of any pointer, pitch or stride.  A call moves 16 x 2 pixel groups per lane when
 *   W % 16 == 0; in->y, in->y_pitch, in->frame_stride, d_out, out_pitch and out_frame_stride are multiples of 16; and in->c0, in->c1
 *   and in->c_pitch are multiples of 8 (not 16: a lane makes two 16-byte Y loads, one 8-byte U load, one 8-byte V load and six 16-byte
 *   stores).  Otherwise it processes 2 x 2 pixel blocks with byte accesses -- slower, the same bytes out.  CLAHE maps and converts in
 *   one kernel when that rule holds and the shape is the NV12 form's one-pass shape (the tile grid divides the frame, tile width a
 *   multiple of 16, tiles_x <= 14, clahe_fp_contract off); any other call runs the planar CLAHE into scratch Y planes of the context
 *   and then the conversion alone: the same bytes in one more pass.
 * Counters (mi_ctx_get_stat), PLANAR-input calls only: "yuv420_bgr_onepass" / "yuv420_bgr_twopass", one count per call (equalizeHist
 *   always counts as one-pass, as in the NV12 form); "yuv420_bgr_vec" / "yuv420_bgr_bytes", one count per call by the walk the
 *   pixel-writing kernel took.  Every planar call with work to do moves exactly one counter of each pair; a call that returns an error
 *   or has a zero size moves none.
 * Launches run in chunks of 256 frames and are charged to the existing profiling slots by role, as the NV12 form's.  Stream rules,
 *   MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the same shape
 *   as the other batched device forms.
 * mi_equalize_hist_yuv420_to_bgr / mi_clahe_yuv420_to_bgr: ONE frame with `in` holding HOST pointers at any address and pitch
 *   (frame_stride is ignored), a CV_8UC3 image at out_step >= 3*W out.  Synchronous; the planes are staged like mi_*_yuv420's (planes
 *   in pinned memory that are tight are DMA'd as they are, everything else goes through the context's pinned staging) and the image
 *   comes back like mi_*_nv12_to_bgr's.  On the device the frame is tight with every plane at a 16-byte aligned offset, so a
 *   W % 16 == 0 frame takes the 16 x 2 groups.  Whatever the call returns, no copy on the caller's memory is in flight any more when
 *   it returns.  W*H beyond what mi_*_nv12_to_bgr accepts: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx or `in`; a `chroma` other than the two values; an `order` other than the two; a negative size; an
 *   odd width or an odd height (refused even when another size is 0, as in the sibling forms); tiles <= 0; a null in->y, in->c0 or
 *   d_out; a null in->c1 on a PLANAR input; y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar); out_pitch < 3*W; d_out
 *   equal to any input plane pointer of the call.  Any other overlap: undefined, not checked.  width, height or n_frames of 0: MI_OK,
 *   nothing written.  Sizes and tile grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.
 *   Nothing is enqueued unless every check passes. */
mi_status mi_equalize_hist_yuv420_to_bgr_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
        size_t out_frame_stride, int width, int height, int n_frames, int order, void* stream);
mi_status mi_clahe_yuv420_to_bgr_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
        size_t out_frame_stride, int width, int height, int n_frames, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_yuv420_to_bgr(mi_ctx* ctx, const mi_yuv420_planes* in, uint8_t* out, size_t out_step,
        int width, int height, int order);
mi_status mi_clahe_yuv420_to_bgr(mi_ctx* ctx, const mi_yuv420_planes* in, uint8_t* out, size_t out_step,
        int width, int height, int order, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_yuv420_to_bgr_frames_dev: the same conversion on a LIST of device frames, each at its own four addresses -- a software decoder's
 * frame pool in (every frame three separately allocated, pitched planes: data[0..2], linesize[0..2]), a pool of CV_8UC3 images out.
 * The batch form needs the whole batch in one allocation at a constant frame stride; one n_frames = 1 batch call per frame costs a
 * launch sequence per frame, and repacking a pool into a batch and copying the images out moves 1.5 + 3 bytes per pixel more each way.
 * `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device pointers on the context's
 * device.
 * Shape: all frames of one call share width, height, order, chroma and the three pitches (bytes between rows); each has its own
 *   addresses.  There are no per-frame pitches.
 *   y  : H rows of W bytes at y_pitch >= W
 *   c0, c1 (MI_CHROMA_PLANAR): the U and the V plane, each H/2 rows of W/2 bytes at c_pitch >= W/2 (both planes share the pitch).  c0 is
 *        always U and c1 always V: a YV12 caller exchanges the two addresses.
 *   out: H rows of 3*W bytes at out_pitch >= 3*W -- B, G, R per pixel (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB)
 * Bytes: per frame the output is byte for byte what mi_*_yuv420_to_bgr_batch_dev writes for that frame alone at the same pitches --
 *   cv::equalizeHist / CLAHE::apply on Y, then cvtColor(COLOR_YUV2BGR_I420 / _YV12, or the RGB codes); the clahe_fp_contract option is
 *   honoured, REFLECT_101 padding applies when the tile grid does not divide the frame, the limits on sizes and tile grids are the
 *   batch form's, with the same statuses.
 * Writes: only the 3*W bytes of each output row are written, not the pitch padding; the input planes are never written.
 * chroma == MI_CHROMA_INTERLEAVED: the call IS mi_*_nv12_to_bgr_frames_dev on {y, c0, out} with uv_pitch = c_pitch (c0 = the UV plane,
 *   H/2 rows of W bytes at c_pitch >= W; c1 is ignored and may be NULL): that form's checks, its kernels, its rule of multiples of 16
 *   throughout and its "nv12_bgr_onepass" / "nv12_bgr_twopass" counters; none of the counters below moves.
 * Alignment (MI_CHROMA_PLANAR): none is required of any address or pitch.  The per-frame alignment decides the access width: the
 *   shape allows 16 x 2 pixel groups when W % 16 == 0, y_pitch and out_pitch are multiples of 16 and c_pitch is a multiple of 8 (not
 *   16: a lane makes two 16-byte Y loads, one 8-byte U load, one 8-byte V load and six 16-byte stores); a frame then takes the groups
 *   when its y and out are multiples of 16 and its c0 and c1 multiples of 8, and any other frame of the same call processes 2 x 2
 *   pixel blocks with byte accesses while its neighbours stay vectorised -- slower, the same bytes out.  equalizeHist always maps the
 *   luma and converts in one kernel.  CLAHE does so when the shape is the batch form's one-pass shape (the tile grid divides the frame,
 *   tile width a multiple of 16, tiles_x <= 14, clahe_fp_contract off), the shape rule above holds and every frame of the call
 *   satisfies the address rule; otherwise the whole call runs the planar CLAHE into scratch Y planes of the context and converts from
 *   there: the same bytes in one more pass.  (In that fallback the Y address the rule sees is the scratch plane's, which is aligned;
 *   the pitches are still the caller's.)
 * Counters (mi_ctx_get_stat), PLANAR lists only: "yuv420_bgr_onepass" / "yuv420_bgr_twopass" count the calls of the list form too,
 *   one count a call (equalizeHist always counts as one-pass).  "yuv420_bgr_list_frames_vec" / "yuv420_bgr_list_frames_bytes" count the
 *   FRAMES (not calls) of list calls by the walk their pixel-writing kernel took: 16 x 2 groups / 2 x 2 blocks.  "yuv420_bgr_vec" /
 *   "yuv420_bgr_bytes" are not touched by list calls.  A call that returns an error or has nothing to do moves none.
 * Launches are charged to the same profiling slots as the batch form, per chunk of 64 frames of the list.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image meet the rows of its own Y, U or V plane
 *   (compared as address ranges).  Input planes are not compared with each other: the U and V rows may lie side by side in one pitched
 *   plane (c1 = c0 + W/2, c_pitch = W).  The same input planes may appear in several entries (inputs are only read).  Outputs that
 *   overlap each other or ANOTHER frame's planes give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null y, c0 or out in any entry; a null c1 in any entry on a
 *   PLANAR input; a `chroma` other than the two values; an `order` other than the two; a negative size; an odd width or an odd height
 *   (refused even when another size is 0, as in the batch form); y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar);
 *   out_pitch < 3*W; tiles <= 0; the overlap above.  Sizes and tile grids the planar forms refuse: the status they give
 *   (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written.  Nothing is enqueued unless every frame passes the
 *   checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
typedef struct mi_yuv420_bgr_frame_dev { const void* y; const void* c0; const void* c1; void* out; } mi_yuv420_bgr_frame_dev;  /* 32 bytes on LP64 */
mi_status mi_equalize_hist_yuv420_to_bgr_frames_dev(mi_ctx* ctx, const mi_yuv420_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order, void* stream);
mi_status mi_clahe_yuv420_to_bgr_frames_dev(mi_ctx* ctx, const mi_yuv420_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_bgr_to_yuv420*: interleaved 8-bit BGR (or RGB) images in, 4:2:0 frames described by mi_yuv420_planes out with the luma equalized
 * -- planar chroma (I420 / YV12: the three pitched planes a software encoder takes, data[0..2] / linesize[0..2]: x264, libvpx, SVT-AV1)
 * or interleaved (NV12) -- renderer, model output or image reader -> encoder without an NV12 intermediate and without plane copies
 * outside the library.  Per frame the bytes are what OpenCV 4.4 gives for
 *     cv::cvtColor(bgr, i420, cv::COLOR_BGR2YUV_I420);                                           (COLOR_RGB2YUV_I420 for MI_ORDER_RGB)
 *     cv::Mat y = i420(Rect(0, 0, W, H));  cv::equalizeHist(y, y)  /  clahe->apply(y, y);        (Y only)
 * with the U plane going to out->c0 and the V plane to out->c1 (MI_UV_COPY) or every chroma byte 128 (MI_UV_FILL128).  Chroma comes
 * from the top-left pixel of each 2 x 2 block, without averaging.  The luma is byte for byte the Y plane of mi_*_bgr_to_nv12_batch_dev
 * for the same pixels; U and V are that call's UV plane de-interleaved and equal the U and V rows of
 * mi_cvt_color_420_u8_batch_dev(MI_COLOR_BGR2YUV_I420).  c0 is always U and c1 always V: a YV12 caller passes the address of its second
 * chroma plane as c0.  The same clahe_fp_contract option, the same REFLECT_101 padding when the tile grid does not divide the frame and
 * the same limits on sizes and tile grids as the planar forms, with the same statuses.
 *   input  : as in mi_*_bgr_to_nv12_batch_dev: frame f at d_in + f * in_frame_stride, H rows of 3*W bytes at in_pitch >= 3*W: B, G, R per
 *            pixel (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB).  The input is never written.
 *   output : `out` is read only during the call.  Frame f has every plane at its pointer + f * out->frame_stride: Y, H rows of W bytes
 *            at y_pitch >= W; PLANAR: c0 = U and c1 = V, each H/2 rows of W/2 bytes at c_pitch >= W/2; INTERLEAVED: c0 = the UV plane,
 *            H/2 rows of W bytes at c_pitch >= W.  Only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each output row
 *            are written: not the pitch padding, not the gaps between the planes, not the gaps between frames.
 * out->chroma == MI_CHROMA_INTERLEAVED: the call IS the NV12 form's (d_y_out = out->y, d_uv_out = out->c0, uv_pitch = out->c_pitch,
 *   out_frame_stride = out->frame_stride; out->c1 ignored): the same kernels, the same alignment rule (multiples of 16 throughout), the
 *   same checks; none of the counters below moves.
 * Alignment (MI_CHROMA_PLANAR): none is required of any pointer, pitch or stride.  A call moves 16 x 2 pixel groups per lane when
 *   W % 16 == 0; d_in, in_pitch, in_frame_stride, out->y, out->y_pitch and out->frame_stride are multiples of 16; and out->c0, out->c1
 *   and out->c_pitch are multiples of 8 (not 16: a lane makes six 16-byte loads, two 16-byte Y stores, one 8-byte U store and one
 *   8-byte V store -- the mirror of the loads of the 4:2:0 -> BGR forms).  Otherwise it processes 2 x 2 pixel blocks with byte accesses
 *   -- slower, the same bytes out.
 * Two stages per chunk of 256 frames, as in the NV12 form.  Y is not in the input, so stage 1 converts: ONE kernel (charged to
 *   MI_K_COLOR) reads the image once, writes Y, U and V into the caller's planes and, for equalizeHist, counts the luma bytes it has
 *   just produced.  Stage 2 maps the luma IN PLACE in out->y with the planar kernels: equalizeHist one MI_K_EQ_LUT and one
 *   MI_K_LUT_APPLY launch (no MI_K_HIST launch; never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel, option
 *   two_kernel_max_frames does not apply); CLAHE exactly what mi_clahe_u8_batch_dev launches for that plane in place.  Bytes moved per
 *   pixel: equalizeHist 3 + 1.5 + 1 + 1 = 6.5, CLAHE 4.5 + 3 = 7.5.  Between the stages out->y holds the unequalized luma.
 * Counters (mi_ctx_get_stat), PLANAR-output calls only: "bgr_yuv420_vec" / "bgr_yuv420_bytes", one count per call by the walk the
 *   conversion kernel took (16 x 2 groups / 2 x 2 blocks).  A call with work to do moves exactly one of them; a call that returns an
 *   error or has a zero size moves neither.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 *   same shape as the other batched device forms.
 * mi_equalize_hist_bgr_to_yuv420 / mi_clahe_bgr_to_yuv420: ONE CV_8UC3 image in host memory at in_step >= 3*W, at any address, in; `out`
 *   holds HOST pointers at any address and pitch (frame_stride is ignored).  Synchronous; the image is staged in like
 *   mi_*_bgr_to_nv12's and the planes come back like mi_*_yuv420's (planes in pinned memory that are tight are DMA'd as they are,
 *   everything else goes through the context's pinned staging).  On the device the frame is tight with every plane at a 16-byte
 *   aligned offset, so a W % 16 == 0 frame takes the 16 x 2 groups.  Whatever the call returns, no copy on the caller's memory is in
 *   flight any more when it returns.  W*H beyond what mi_*_bgr_to_nv12 accepts: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx, d_in or `out`; a null out->y or out->c0; a null out->c1 on a PLANAR output; a `chroma` other than
 *   the two values; an `order` other than the two; a bad uv_mode; a negative size; an odd width or an odd height (refused even when
 *   another size is 0, as in the sibling forms); in_pitch < 3*W; y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar);
 *   tiles <= 0; two output plane pointers of the call that are equal; an output plane pointer equal to d_in (there is no in-place
 *   form).  Any other overlap: undefined, not checked; U and V rows side by side in one pitched plane (c1 = c0 + W/2, c_pitch = W) are
 *   legal, as in mi_*_yuv420*.  width, height or n_frames of 0: MI_OK, nothing written (pointers and pitches are not looked at then).
 *   Sizes and tile grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued
 *   unless every check passes. */
mi_status mi_equalize_hist_bgr_to_yuv420_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        const mi_yuv420_planes* out, int width, int height, int n_frames, int order, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgr_to_yuv420_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        const mi_yuv420_planes* out, int width, int height, int n_frames, int order, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_bgr_to_yuv420(mi_ctx* ctx, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out,
        int width, int height, int order, mi_uv_mode uv_mode);
mi_status mi_clahe_bgr_to_yuv420(mi_ctx* ctx, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out,
        int width, int height, int order, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_bgr_to_yuv420_frames_dev: the same conversion on a LIST of device frames, each at its own four addresses -- a pool of CV_8UC3
 * images in (a renderer or a model hands over one image per frame), a software encoder's frame pool out (x264, libvpx, SVT-AV1: every
 * frame three separately allocated, pitched planes, data[0..2] / linesize[0..2]).  The batch form needs both sides in one allocation
 * each at a constant frame stride; one n_frames = 1 batch call per frame costs a launch sequence per frame with tiny grids, and
 * repacking both pools into strided scratch and copying the planes out moves 3 + 1.5 bytes per pixel more each way.
 * `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device pointers on the context's
 * device.
 * Shape: all frames of one call share width, height, order, uv_mode, chroma and the three pitches (bytes between rows); each has its
 *   own addresses.  There are no per-frame pitches.
 *   in : H rows of 3*W bytes at in_pitch >= 3*W -- B, G, R per pixel (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB)
 *   y  : H rows of W bytes at y_pitch >= W
 *   c0, c1 (MI_CHROMA_PLANAR): the U and the V plane, each H/2 rows of W/2 bytes at c_pitch >= W/2 (both planes share the pitch).  c0 is
 *        always U and c1 always V: a YV12 caller exchanges the two addresses.
 * Bytes: per frame the output is byte for byte what mi_*_bgr_to_yuv420_batch_dev writes for that frame alone at the same pitches --
 *   cvtColor(COLOR_BGR2YUV_I420, or the RGB code), then cv::equalizeHist / CLAHE::apply on Y, U and V of the conversion (MI_UV_COPY) or
 *   every chroma byte 128 (MI_UV_FILL128); the clahe_fp_contract option is honoured, REFLECT_101 padding applies when the tile grid
 *   does not divide the frame, the limits on sizes and tile grids are the batch form's, with the same statuses.
 * Writes: only the W bytes of each Y row and the W/2 bytes of each U and V row are written: not the pitch padding, not the gaps
 *   between planes or frames.  The images are never written.
 * chroma == MI_CHROMA_INTERLEAVED: the call IS mi_*_bgr_to_nv12_frames_dev on {in, y, c0} with uv_pitch = c_pitch (c0 = the UV plane,
 *   H/2 rows of W bytes at c_pitch >= W; c1 is ignored and may be NULL): that form's checks, its kernels and its rule of multiples of
 *   16 throughout; none of the counters below moves.
 * Alignment (MI_CHROMA_PLANAR): none is required of any address or pitch.  The per-frame alignment decides the access width: the
 *   shape allows 16 x 2 pixel groups when W % 16 == 0, in_pitch and y_pitch are multiples of 16 and c_pitch is a multiple of 8; a
 *   frame then takes the groups when its in and y are multiples of 16 and its c0 and c1 multiples of 8 (8, not 16: a lane makes six
 *   16-byte loads, two 16-byte Y stores, one 8-byte U store and one 8-byte V store), and any other frame of the same call processes
 *   2 x 2 pixel blocks with byte accesses while its neighbours stay vectorised -- slower, the same bytes out.
 * Stages, per chunk of 64 frames of the list (not the batch form's 256): stage 1 is ONE launch charged to MI_K_COLOR that converts
 *   into the caller's planes and, for equalizeHist, counts the luma bytes it has just produced.  Stage 2 maps the luma IN PLACE on the
 *   chunk's Y planes: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no MI_K_HIST launch; never the fused equalizeHist
 *   kernel nor the single-launch histogram + LUT kernel, option two_kernel_max_frames does not apply); CLAHE exactly what
 *   mi_clahe_nv12_frames_dev launches in place on those Y planes.  Launches are charged to the same profiling slots as the batch form.
 *   Between the stages a frame's y holds the unequalized luma.
 * Counters (mi_ctx_get_stat), PLANAR lists only: "bgr_yuv420_list_frames_vec" / "bgr_yuv420_list_frames_bytes" count the FRAMES (not
 *   calls) of list calls by the walk their stage-1 kernel took: 16 x 2 groups / 2 x 2 blocks.  "bgr_yuv420_vec" / "bgr_yuv420_bytes"
 *   are not touched by list calls.  A call that returns an error or has nothing to do moves none.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image meet the rows of its own Y, U or V plane, or
 *   the rows of its Y plane meet the rows of its own U or V plane (compared as address ranges), and when c0 == c1.  U and V are
 *   otherwise not compared with each other: the U and V rows may lie side by side in one pitched plane (c1 = c0 + W/2, c_pitch = W),
 *   as in the batch form.  The same image may appear in several entries (inputs are only read).  Outputs that overlap ANOTHER frame's
 *   planes give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null in, y or c0 in any entry; a null c1 in any entry on a
 *   PLANAR list; a `chroma` other than the two values; an `order` other than the two; a bad uv_mode; a negative size; an odd width or
 *   an odd height (refused even when another size is 0, as in the batch form); in_pitch < 3*W; y_pitch < W; a c_pitch below its row
 *   (W interleaved, W/2 planar); tiles <= 0; the overlap above.  Sizes and tile grids the planar forms refuse: the status they give
 *   (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written.  Nothing is enqueued unless every frame passes the
 *   checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
typedef struct mi_bgr_yuv420_frame_dev { const void* in; void* y; void* c0; void* c1; } mi_bgr_yuv420_frame_dev;  /* 32 bytes on LP64 */
mi_status mi_equalize_hist_bgr_to_yuv420_frames_dev(mi_ctx* ctx, const mi_bgr_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgr_to_yuv420_frames_dev(mi_ctx* ctx, const mi_bgr_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_packed422_to_yuv420*: packed 4:2:2 frames in (YUY2 / UYVY: what a capture card hands over), 4:2:0 frames described by
 * mi_yuv420_planes out with the luma equalized -- planar chroma (I420 / YV12: the three pitched planes data[0..2] / linesize[0..2] a
 * software encoder takes) or interleaved chroma (NV12) -- in the pass that equalizes, without an NV12 intermediate and without a
 * de-interleave of the UV plane outside the library.  The packed frame is read twice (histograms, then map) exactly as by
 * mi_*_packed422_to_nv12_batch_dev; the second pass writes 1.5*W*H bytes.
 *   input  : exactly what mi_*_packed422_batch_dev takes.  `format` is MI_FMT_YUY2 or MI_FMT_UYVY; frame f lies at
 *            d_in + f * in_frame_stride, H rows of 2*W bytes at in_pitch; the pointer, the pitch and the frame stride are multiples
 *            of 4.  The input is never written.
 *   output : frame f has its planes at out->y / out->c0 / out->c1 + f * out->frame_stride: Y, H rows of W bytes at y_pitch >= W;
 *            MI_CHROMA_PLANAR: c0 is always U and c1 always V, each H/2 rows of W/2 bytes at c_pitch >= W/2 (both planes share the
 *            pitch; a YV12 caller exchanges the two addresses).  U and V rows side by side in one pitched plane (c1 = c0 + W/2,
 *            c_pitch = W) are legal.
 *   luma   : byte for byte the Y plane of mi_*_packed422_to_nv12_batch_dev on the same input (same clahe_fp_contract option,
 *            REFLECT_101 padding when the tile grid does not divide the frame, the same fallback for tile grids too wide for the LDS
 *            pair table).
 *   chroma : that call's UV plane de-interleaved.  MI_UV_FILL128 sets every byte of both planes to 128.  MI_UV_COPY keeps the chroma
 *            and halves it vertically: for chroma row r, the U (and the V) sample of macropixel m is the rounding mean of input rows 2r
 *            and 2r+1, (a + b + 1) >> 1 on the two input bytes.  No horizontal filtering and no change of siting.  OpenCV has no call
 *            for this conversion and the reference has none: the rule is this header's own, it has no outside pin.
 * out->chroma == MI_CHROMA_INTERLEAVED: the call IS the NV12 form's (d_y_out = out->y, d_uv_out = out->c0, uv_pitch = out->c_pitch,
 * out_frame_stride = out->frame_stride; c1 is ignored and may be NULL): its checks, its launches, its bytes.
 * Alignment (MI_CHROMA_PLANAR, device forms): out->y, y_pitch, c0, c1, c_pitch and frame_stride are multiples of 4.  Consequence: a
 * TIGHT planar frame with W % 8 != 0 has a chroma pitch W/2 that is not a multiple of 4 and is refused (as the NV12 form refuses a tight
 * W % 4 == 2 frame) -- such a caller pads the pitch, or uses the host form.
 * Nothing outside the W bytes of each Y row and the W/2 bytes of each chroma row is written: not the pitch padding, not the space
 * between the planes, not the gap between frames.  `width` and `height` are even.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 * the same shape as mi_*_packed422_to_nv12_batch_dev.  Never the fused equalizeHist kernel nor the single-launch histogram + LUT
 * kernel; exactly the launches the NV12 form makes per chunk (equalizeHist: one MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY
 * launch, for either uv_mode): the chroma is written by the launch that writes the luma, there is no chroma launch.
 * Errors, MI_ERR_BAD_ARG: a null ctx, a null `out`, a chroma other than the two values, any null frame or plane pointer (a null c1 on
 * a planar output included), an odd width or an odd height (refused even when another size is 0), a negative size, in_pitch < 2*W,
 * y_pitch < W, a c_pitch below its row (W interleaved, W/2 planar), any pointer / pitch / stride that is not a multiple of 4, a format
 * other than the two, a bad uv_mode, tiles <= 0, two output planes at one address, an output plane whose rows meet the rows of its
 * own frame's input or a Y plane whose rows meet a chroma plane of its own frame (there is no in-place form; U and V are compared by
 * address only, so that the side-by-side layout stays legal).  width, height or n_frames of 0: MI_OK, nothing written.  Sizes and tile
 * grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.  Outputs of DIFFERENT frames that overlap
 * each other: undefined, not checked.  Nothing is enqueued unless all checks pass.
 *
 * mi_*_packed422_to_yuv420_frames_dev: the same conversion on a LIST of device frames, each at its own four addresses {in, y, c0, c1}
 * (a capture device's buffer pool in, a software encoder's frame pool out).  `frames` is a host array of n_frames entries, read only
 * during the call.  Every frame of one call has the same width, height, format, out_chroma and the same three pitches.  Every address
 * and every pitch is a multiple of 4; each frame may have its own alignment modulo 16 (different bytes never).  The same input may
 * appear in several entries.  Per frame the bytes are the batch form's.  out_chroma == MI_CHROMA_INTERLEAVED: the call IS
 * mi_*_packed422_to_nv12_frames_dev on {in, y, c0} with uv_pitch = c_pitch.  Errors as above per entry, and a null `frames` with
 * n_frames > 0; nothing is enqueued unless every frame passes the checks: a bad last entry leaves the first frames' outputs untouched.
 *
 * mi_equalize_hist_packed422_to_yuv420 / mi_clahe_packed422_to_yuv420: ONE host frame, synchronous.  The input side follows the rules of
 * mi_*_packed422 (`in` and in_pitch multiples of 4, in_pitch >= 2*W).  `out` holds host pointers the kernels never see: any address,
 * y_pitch any value >= W and c_pitch any value >= W/2 -- a tight frame with W % 8 != 0 is accepted; frame_stride is ignored.  Staged
 * like mi_*_packed422_to_nv12 with three output planes: the device planes lie at pitches align4(W) and align4(W/2); pinned tight planes
 * whose device rows are tight too are DMA'd as they are, everything else goes through the context's pinned staging (statistics
 * "host_planes_direct" / "host_planes_staged", four planes a planar call).  MI_ERR_BAD_ARG when the rows of an output plane meet the
 * rows of the input or the Y rows those of a chroma plane; shape, mode, size and zero-size rules as the device form above. */
mi_status mi_equalize_hist_packed422_to_yuv420_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        const mi_yuv420_planes* out, int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_packed422_to_yuv420_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        const mi_yuv420_planes* out, int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_packed422_to_yuv420(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, const mi_yuv420_planes* out,
        int width, int height, int format, mi_uv_mode uv_mode);
mi_status mi_clahe_packed422_to_yuv420(mi_ctx* ctx, const uint8_t* in, size_t in_pitch, const mi_yuv420_planes* out,
        int width, int height, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
typedef mi_bgr_yuv420_frame_dev mi_packed422_yuv420_frame_dev;       /* { in, y, c0, c1 } */
mi_status mi_equalize_hist_packed422_to_yuv420_frames_dev(mi_ctx* ctx, const mi_packed422_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int out_chroma,
        int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_packed422_to_yuv420_frames_dev(mi_ctx* ctx, const mi_packed422_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int out_chroma,
        int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_bgr_to_packed422*: interleaved 8-bit BGR (or RGB) images in, packed 4:2:2 frames (YUY2 / UYVY) out with the luma equalized --
 * renderer, model output or image reader -> SDI / HDMI playout card, v4l2 output or loopback device, virtual camera, without an NV12
 * intermediate (which has already dropped every second chroma row) and without an interleave outside the library.
 * Pixels, per frame:
 *   luma   : Y = bt601_y(b, g, r) for every pixel -- the Y of cv::cvtColor(COLOR_BGR2YUV_I420) (COLOR_RGB2YUV_I420 for MI_ORDER_RGB) as
 *            mi_cvt_color_420_u8 computes it -- then cv::equalizeHist / clahe->apply on the W x H luma plane: byte for byte what
 *            mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev return on that plane.  The same clahe_fp_contract option, the same
 *            REFLECT_101 padding when the tile grid does not divide the frame and the same limits on sizes and tile grids as those
 *            forms.
 *   chroma : MI_UV_COPY: the U and V of macropixel (k, y) are bt601_uv of the LEFT pixel (2k, y) of that row, without averaging -- the
 *            library's 4:2:0 rule (top-left pixel of each 2 x 2 block) applied to every row on its own.  MI_UV_FILL128: every chroma
 *            byte 128, the chroma arithmetic is skipped.
 *   This is the library's own definition, consistent with its decode: mi_*_packed422_to_bgr* reads back the same U and V for both
 *   pixels of the macropixel.  No claim is made about COLOR_BGR2YUV_YUY2 / COLOR_BGR2YUV_UYVY of OpenCV releases later than the 4.4
 *   the oracle restates (4.4 has no such codes).
 *   MI_FMT_YUY2 writes exactly Y0 U Y1 V, MI_FMT_UYVY exactly U Y0 V Y1.  MI_ORDER_BGR reads B, G, R per pixel, MI_ORDER_RGB reads R, G, B.
 *   input  : frame f at d_in + f * in_frame_stride, H rows of 3*W bytes at in_pitch >= 3*W, at any address.  The input is never written.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 2*W bytes at out_pitch >= 2*W; d_out, out_pitch and out_frame_stride
 *            are multiples of 4 (the packed forms' rule).  Only the 2*W bytes of each output row are written: not the pitch padding,
 *            not the gaps between frames.
 * Width is even; height is any value >= 1, odd heights are legal.
 * Alignment: a call moves 16 pixels of one row per lane (three 16-byte loads, two 16-byte stores) when W % 16 == 0 and d_in, in_pitch,
 *   in_frame_stride, d_out, out_pitch and out_frame_stride are all multiples of 16.  Otherwise it processes one macropixel per lane
 *   with six byte loads and one aligned dword store -- slower, the same bytes out.
 * Two stages per chunk of 256 frames, as in mi_*_bgr_to_nv12_batch_dev.  Y is not in the input, so stage 1 converts: ONE kernel (charged
 *   to MI_K_COLOR) reads the image once, writes the packed frame with unequalized luma into d_out and, for equalizeHist, counts the
 *   luma bytes it has just produced.  Stage 2 is the packed form's own kernels IN PLACE on the output frame, the chroma bytes kept
 *   whatever uv_mode is: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no MI_K_HIST launch); CLAHE exactly what
 *   mi_clahe_packed422_batch_dev launches for those frames in place, every shape in one pass.  Never the fused equalizeHist kernel nor
 *   the single-launch histogram + LUT kernel: option two_kernel_max_frames does not apply.  Bytes moved per pixel: equalizeHist
 *   3 + 2 + 2 + 2 = 9, CLAHE 5 + 2 + 4 = 11.  Between the stages d_out holds the unequalized luma.
 * Counters (mi_ctx_get_stat): "bgr_packed422_vec" / "bgr_packed422_bytes", one count per call by the walk stage 1 took (16-pixel
 *   groups / macropixels).  A device or host call with work to do moves exactly one of them; a call that returns an error or has a
 *   zero size moves neither.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 *   same shape as the other batched device forms.
 * mi_equalize_hist_bgr_to_packed422 / mi_clahe_bgr_to_packed422: ONE CV_8UC3 image in host memory at in_step >= 3*W, at any address, in;
 *   one packed frame in host memory at any address and any out_pitch >= 2*W out.  Synchronous; the image is staged in like
 *   mi_*_bgr_to_yuv420's and the frame comes back like mi_*_packed422's (frames in pinned memory that are tight are DMA'd as they are,
 *   everything else goes through the context's pinned staging).  On the device the frame is tight and 16-byte aligned, so a
 *   W % 16 == 0 image takes the 16-pixel groups.  Whatever the call returns, no copy on the caller's memory is in flight any more when
 *   it returns.  W*H beyond what mi_*_bgr_to_nv12 accepts: MI_ERR_UNSUPPORTED.
 * There is no in-place form: d_out == d_in is MI_ERR_BAD_ARG; any other overlap of input and output is undefined, not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx, d_in or d_out; an odd width (refused even when another size is 0, as in the packed forms); a
 *   negative size; in_pitch < 3*W; out_pitch < 2*W; a d_out, out_pitch or out_frame_stride of the device form that is not a multiple
 *   of 4; an `order` other than the two; a `format` other than the two; a bad uv_mode; tiles <= 0.  width, height or n_frames of 0:
 *   MI_OK, nothing written (pointers and pitches are not looked at then).  Sizes and tile grids the packed or planar forms refuse:
 *   MI_ERR_UNSUPPORTED, nothing written.  Nothing is enqueued unless every check passes.
 * The frame-list form mi_*_bgr_to_packed422_frames_dev is described below; four-channel (BGRA / RGBA, CV_8UC4) input is
 * mi_*_bgra_to_packed422* further below.  Not built: YVYU / VYUY, chroma averaging. */
mi_status mi_equalize_hist_bgr_to_packed422_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgr_to_packed422_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_bgr_to_packed422(mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
        int width, int height, int order, int format, mi_uv_mode uv_mode);
mi_status mi_clahe_bgr_to_packed422(mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
        int width, int height, int order, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_bgr_to_packed422_frames_dev: the same conversion on a LIST of device frames, each at its own two addresses -- a pool of CV_8UC3
 * images in (a renderer or a model hands over one image per frame), a playout card's, a v4l2 output queue's or a virtual camera's
 * buffer pool out (every packed frame its own allocation, padded to bytesperline, at whatever alignment the driver chose).  The batch
 * form needs both sides in one allocation each at a constant frame stride; one n_frames = 1 batch call per frame costs a launch
 * sequence per frame with tiny grids, and repacking both pools into strided scratch and back moves 3 + 2 bytes per pixel more.
 * `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device pointers on the context's
 * device.
 * Shape: all frames of one call share width, height, the pair of pitches (bytes between rows), order, format and uv_mode; each has its
 *   own two addresses.  There are no per-frame pitches.
 *   in  : H rows of 3*W bytes at in_pitch >= 3*W, at any address -- B, G, R per pixel (MI_ORDER_BGR) or R, G, B (MI_ORDER_RGB).  The
 *         images are never written.
 *   out : H rows of 2*W bytes at out_pitch >= 2*W; every `out` and out_pitch are multiples of 4 (the packed forms' rule).  Only the
 *         2*W bytes of each output row are written: not the pitch padding, nothing before or behind a frame.
 * Bytes: per frame the output is byte for byte exactly what mi_*_bgr_to_packed422_batch_dev writes for that frame alone at the same
 *   pitches -- luma and chroma as defined there (bt601_y of every pixel, then cv::equalizeHist / CLAHE::apply; bt601_uv of the LEFT
 *   pixel of each macropixel, or every chroma byte 128), MI_FMT_YUY2 exactly Y0 U Y1 V, MI_FMT_UYVY exactly U Y0 V Y1; the
 *   clahe_fp_contract option is honoured, REFLECT_101 padding applies when the tile grid does not divide the frame, width is even, odd
 *   heights are legal, and the limits on sizes and tile grids are the batch form's, with the same statuses.
 * Alignment: beyond the multiples of 4 above, none is required.  The per-frame alignment decides the walk of stage 1: the shape
 *   allows 16-pixel groups (three 16-byte loads, two 16-byte stores per lane) when W % 16 == 0 and in_pitch and out_pitch are multiples
 *   of 16; a frame then takes the groups when its own `in` and `out` are both multiples of 16, and any other frame of the same call
 *   processes one macropixel per lane with six byte loads and one aligned dword store while its neighbours stay vectorised -- slower,
 *   the same bytes out.
 * Stages, per chunk of 128 frames of the list (not the batch form's 256): stage 1 is ONE launch charged to MI_K_COLOR that converts
 *   into the caller's frames and, for equalizeHist, counts the luma bytes it has just produced.  Stage 2 maps the luma IN PLACE on the
 *   chunk's output frames, the chroma bytes kept whatever uv_mode is: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no
 *   MI_K_HIST launch; never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel, option two_kernel_max_frames
 *   does not apply); CLAHE exactly what mi_clahe_packed422_frames_dev launches in place on those frames, every shape in one pass.
 *   Between the stages a frame's `out` holds the unequalized luma.
 * Counters (mi_ctx_get_stat): "bgr_packed422_list_frames_vec" / "bgr_packed422_list_frames_bytes" count the FRAMES (not calls) of list
 *   calls by the walk their stage-1 kernel took: 16-pixel groups / macropixels.  A list call moves the two by n_frames in total and
 *   does not touch "bgr_packed422_vec" / "bgr_packed422_bytes".  A call that returns an error or has nothing to do moves none.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image meet the rows of its own output frame (compared
 *   as address ranges).  The same image may appear in several entries (inputs are only read).  Outputs that overlap ANOTHER frame's
 *   image or output give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null `in` or `out` in any entry; an `out` in any entry or
 *   an out_pitch that is not a multiple of 4; an `order` other than the two; a `format` other than the two; a bad uv_mode; a negative
 *   size; an odd width (refused even when another size is 0, as in the batch form); in_pitch < 3*W; out_pitch < 2*W; tiles <= 0; the
 *   overlap above.  Sizes and tile grids the packed or planar forms refuse: MI_ERR_UNSUPPORTED.  width, height or n_frames of 0: MI_OK,
 *   nothing written (the entries and the pitches are not looked at then; n_frames == 0 with a null list is MI_OK).  Nothing is enqueued
 *   unless every frame passes the checks: a bad last entry leaves the earlier frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
typedef struct mi_bgr_packed422_frame_dev { const void* in; void* out; } mi_bgr_packed422_frame_dev;  /* 16 bytes on LP64 */
mi_status mi_equalize_hist_bgr_to_packed422_frames_dev(mi_ctx* ctx, const mi_bgr_packed422_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int order, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgr_to_packed422_frames_dev(mi_ctx* ctx, const mi_bgr_packed422_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int order, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_yuv420_to_packed422*: 4:2:0 frames (NV12, or planar I420 / YV12) in, packed 4:2:2 frames (YUY2 / UYVY) out with the luma
 * equalized -- the decoder-to-playout path: a hardware decoder hands over NV12 and a software decoder I420 / YV12; SDI / HDMI playout
 * cards, v4l2 output and loopback devices and virtual cameras take YUY2 / UYVY.  One pass instead of mi_*_yuv420_batch_dev /
 * mi_*_nv12_batch_dev into scratch followed by a scatter of Y and a row-repeated UV plane outside the library.
 * Pixels, per frame:
 *   input  : as for mi_*_yuv420_to_bgr_batch_dev: `in` describes frame 0, frame f lies in->frame_stride bytes further in every plane;
 *            in->chroma is MI_CHROMA_INTERLEAVED (NV12: c0 = the UV plane, c1 ignored) or MI_CHROMA_PLANAR (I420: c0 = U, c1 = V, both
 *            at c_pitch).  A YV12 caller exchanges c0 and c1: c0 is always U.  Any address and any pitch are accepted (y_pitch >= W;
 *            c_pitch >= W interleaved, >= W/2 planar).  The input is never written.  Width and height are even.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 2*W bytes at out_pitch >= 2*W.  MI_FMT_YUY2 writes exactly Y0 U Y1 V,
 *            MI_FMT_UYVY exactly U Y0 V Y1.  d_out, out_pitch and out_frame_stride are multiples of 4 (the packed forms' rule).
 *            Only the 2*W bytes of each output row are written: not the pitch padding, not the gaps between frames.
 *   luma   : cv::equalizeHist / clahe->apply on the W x H Y plane: byte for byte what mi_equalize_hist_u8_batch_dev /
 *            mi_clahe_u8_batch_dev give on the input Y plane.  The same clahe_fp_contract option, the same REFLECT_101 padding when the
 *            tile grid does not divide the frame and the same limits on sizes and tile grids, with the same statuses, as those forms.
 *   chroma : MI_UV_COPY: output rows 2r and 2r+1 both carry input chroma row r unchanged: macropixel k of both rows gets U[r][k],
 *            V[r][k].  There is no vertical interpolation and no change of siting.  MI_UV_FILL128: every chroma byte 128; in->c0,
 *            in->c1 and in->c_pitch are not read and the pointers may be NULL, as in mi_*_yuv420*.
 *   This chroma rule is the library's own definition, consistent with the rest of the library: it is the chroma that
 *   mi_*_nv12_to_bgr* / mi_*_yuv420_to_bgr* already apply to both rows of a pair, and mi_*_packed422_to_nv12* maps it back to the same
 *   NV12 chroma, because (a + a + 1) >> 1 == a.  OpenCV has no call for it.
 * Alignment: a lane moves a 16 x 2 pixel group (two 16-byte Y loads, one 16-byte UV load or two 8-byte loads from the U and V planes,
 *   four 16-byte stores) when W % 16 == 0, in->y, y_pitch, in->frame_stride, d_out, out_pitch and out_frame_stride are all multiples of
 *   16 and, under MI_UV_COPY, c0 and c_pitch are multiples of 16 (interleaved) or c0, c1 and c_pitch multiples of 8 (planar).  Otherwise
 *   it processes a 2 x 2 block per lane with byte loads and one aligned dword store per macropixel -- slower, the same bytes out.
 * Stages, per chunk of 256 frames: Y is a plane, so the histogram stages are the planar forms' own.  equalizeHist: one MI_K_HIST, one
 *   MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (LUT apply + pack), for either uv_mode.  CLAHE: the tile histograms and LUTs of
 *   mi_clahe_u8_batch_dev, then ONE kernel charged to MI_K_CLAHE_INTERP that blends and packs (one pass, no MI_K_COLOR launch) when the
 *   tile grid divides the frame, the tile width is a multiple of 16, clahe_fp_contract is off and the alignment above holds;
 *   everything else runs mi_clahe_u8_batch_dev's launches into scratch Y planes and then one MI_K_COLOR launch that packs (two passes,
 *   the same bytes).  Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel: option two_kernel_max_frames
 *   does not apply.  Bytes moved per pixel: equalizeHist 1 + 1.5 + 2 = 4.5, one-pass CLAHE 4.5, two-pass CLAHE 6.5.
 * Counters (mi_ctx_get_stat): "yuv420_packed422_onepass" / "yuv420_packed422_twopass" and "yuv420_packed422_vec" /
 *   "yuv420_packed422_bytes" (the walk the pixel-writing kernel took: 16 x 2 groups / 2 x 2 blocks).  A device or host call with work
 *   to do moves exactly one of each pair, NV12 and planar input alike; a call that returns an error or has a zero size moves none.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 *   same shape as the other batched device forms.
 * mi_equalize_hist_yuv420_to_packed422 / mi_clahe_yuv420_to_packed422: ONE frame whose planes lie in host memory (in->frame_stride is
 *   ignored) in; one packed frame in host memory at any address and any out_pitch >= 2*W out.  Synchronous; the planes are staged in
 *   like mi_*_yuv420_to_bgr's and the frame comes back like mi_*_bgr_to_packed422's (tight planes and frames in pinned memory are DMA'd
 *   as they are, everything else goes through the context's pinned staging).  On the device the frame is tight with every plane 16-byte
 *   aligned, so a W % 16 == 0 frame takes the 16 x 2 groups.  Whatever the call returns, no copy on the caller's memory is in flight
 *   any more when it returns.
 * There is no in-place form: d_out equal to any input plane pointer is MI_ERR_BAD_ARG; any other overlap of input and output is
 *   undefined, not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx, `in`, in->y or d_out; under MI_UV_COPY a null c0 (or c1, planar); an odd width or an odd height
 *   (refused even when another size is 0); a negative size; y_pitch < W; c_pitch below its row; out_pitch < 2*W; a d_out, out_pitch or
 *   out_frame_stride of the device form that is not a multiple of 4; a `format` other than the two; a `chroma` other than the two; a
 *   bad uv_mode; tiles <= 0.  width, height or n_frames of 0: MI_OK, nothing written (pointers and pitches are not looked at then).
 *   Sizes and tile grids the planar forms refuse: MI_ERR_UNSUPPORTED, nothing written.  Nothing is enqueued unless every check passes.
 * Not built: a frame-list form, a mi_pipe format, YVYU / VYUY, NV21, vertical chroma interpolation. */
mi_status mi_equalize_hist_yuv420_to_packed422_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_yuv420_to_packed422_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_yuv420_to_packed422(mi_ctx* ctx, const mi_yuv420_planes* in,
        uint8_t* out, size_t out_pitch, int width, int height, int format, mi_uv_mode uv_mode);
mi_status mi_clahe_yuv420_to_packed422(mi_ctx* ctx, const mi_yuv420_planes* in,
        uint8_t* out, size_t out_pitch, int width, int height, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y);
/* mi_*_yuv420_to_packed422_frames_dev: the same conversion on a LIST of device frames, each at its own four addresses -- the form in
 * which both real sides are pools: a decoder hands out surfaces whose Y, U and V (or UV) planes are separate pitched allocations
 * (data[0..2], linesize[0..2]); a playout card, a v4l2 output queue or a virtual camera hands out one buffer per frame, padded to
 * bytesperline.  The batch form needs each side in one allocation at a constant frame stride; one n_frames = 1 batch call per frame
 * costs a launch sequence per frame with tiny grids, and repacking both pools through strided scratch moves 1.5 + 2 bytes per pixel
 * more each way.  `frames` is a host array of n_frames entries, read only during the call; the pointers in it are device pointers on
 * the context's device.
 * Shape: all frames of one call share width, height (both even), y_pitch, c_pitch, chroma, out_pitch, format and uv_mode; each has
 *   its own four addresses.  There are no per-frame pitches.
 *   y  : H rows of W bytes at y_pitch >= W
 *   chroma == MI_CHROMA_INTERLEAVED: c0 is the UV plane, H/2 rows of W bytes at c_pitch >= W; c1 is ignored and may be NULL.
 *   chroma == MI_CHROMA_PLANAR: c0 is always U and c1 always V, each H/2 rows of W/2 bytes at c_pitch >= W/2 (both planes share the
 *        pitch): a YV12 caller exchanges the two addresses.
 *   out: H rows of 2*W bytes at out_pitch >= 2*W; every `out` and out_pitch are multiples of 4 (the packed forms' rule).
 *   Unlike mi_*_yuv420_to_bgr_frames_dev an interleaved list is not handed to another form: one pair of entry points and one set of
 *   counters serves both layouts.
 * Bytes: per frame the output is byte for byte what mi_*_yuv420_to_packed422_batch_dev writes for that frame alone at the same pitches:
 *   MI_FMT_YUY2 exactly Y0 U Y1 V, MI_FMT_UYVY exactly U Y0 V Y1; the luma is cv::equalizeHist / CLAHE::apply on the Y plane (what the
 *   planar forms give); input chroma row r goes unchanged under output rows 2r and 2r+1, or every chroma byte is 128.  The
 *   clahe_fp_contract option is honoured, REFLECT_101 padding applies when the tile grid does not divide the frame, and the limits on
 *   sizes and tile grids are the batch form's, with the same statuses.
 * Writes: only the 2*W bytes of each output row are written, not the pitch padding, nothing before or behind a frame; the input planes
 *   are never written.
 * MI_UV_FILL128: c0, c1 and c_pitch are not read and decide nothing -- not the walk, not the overlap check, not an error; the pointers
 *   may be NULL.
 * Alignment: beyond the multiples of 4 above, none is required.  The per-frame alignment decides the access width: the shape allows
 *   16 x 2 pixel groups when W % 16 == 0, y_pitch and out_pitch are multiples of 16 and, under MI_UV_COPY, c_pitch is a multiple of 16
 *   (interleaved) or 8 (planar); a frame then takes the groups when its y and out are multiples of 16 and, under MI_UV_COPY, its c0 is
 *   a multiple of 16 (interleaved) or its c0 and c1 are multiples of 8 (planar), and any other frame of the same call processes 2 x 2
 *   blocks with byte loads and one aligned dword store per macropixel while its neighbours stay vectorised -- slower, the same bytes out.
 * Stages, per chunk of 64 frames of the list (not the batch form's 256): equalizeHist is one MI_K_HIST, one MI_K_EQ_LUT and one
 *   MI_K_LUT_APPLY launch (LUT apply + pack), for either uv_mode; never the fused equalizeHist kernel nor the single-launch histogram
 *   + LUT kernel (option two_kernel_max_frames does not apply).  CLAHE runs in one pass (the tile LUTs, then ONE MI_K_CLAHE_INTERP
 *   launch that blends and packs) when the shape is the batch form's one-pass shape (the tile grid divides the frame, tile width a
 *   multiple of 16, tiles_x <= 14), clahe_fp_contract is off, the shape rule above holds and every frame of the call satisfies the
 *   address rule; otherwise the whole call runs the planar CLAHE into scratch Y planes of the context and then one MI_K_COLOR launch
 *   that packs from there: the same bytes in one more pass.  (In that fallback the Y address the rule sees is the scratch plane's,
 *   which is aligned: the frame's y drops out of its rule; the pitches are still the caller's.)  Launches are charged to the same
 *   profiling slots as the batch form.
 * Counters (mi_ctx_get_stat): "yuv420_packed422_onepass" / "yuv420_packed422_twopass" count the calls of the list form too, one count
 *   a call (equalizeHist always counts as one-pass).  "yuv420_packed422_list_frames_vec" / "yuv420_packed422_list_frames_bytes" count
 *   the FRAMES (not calls) of list calls by the walk their pixel-writing kernel took, n_frames in total per call.
 *   "yuv420_packed422_vec" / "yuv420_packed422_bytes" are not touched by list calls.  A call that returns an error or has nothing to do
 *   moves none.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's `out` meet the rows of its own Y plane or, under
 *   MI_UV_COPY, of its own chroma plane(s) (compared as address ranges).  U and V are not compared with each other: they may be the two
 *   halves of the rows of one pitched plane (c1 = c0 + W/2, c_pitch = W).  The same input planes may appear in several entries (inputs
 *   are only read).  Outputs that overlap each other or ANOTHER frame's planes give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null y or out in any entry; under MI_UV_COPY a null c0 (or
 *   c1, planar) in any entry; an `out` in any entry or an out_pitch that is not a multiple of 4; a `format` other than the two; a
 *   `chroma` other than the two; a bad uv_mode; a negative size; an odd width or an odd height (refused even when another size is 0, as
 *   in the batch form); y_pitch < W; under MI_UV_COPY a c_pitch below its row (W interleaved, W/2 planar); out_pitch < 2*W; tiles <= 0;
 *   the overlap above.  Sizes and tile grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED).  width, height or
 *   n_frames of 0: MI_OK, nothing written (n_frames == 0 with a null list is MI_OK).  Nothing is enqueued unless every frame passes the
 *   checks: a bad last entry leaves the earlier frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with.
 * Not built: a mi_pipe format, per-frame pitches, YVYU / VYUY, NV21, vertical chroma interpolation. */
typedef struct mi_yuv420_packed422_frame_dev { const void* y; const void* c0; const void* c1; void* out; } mi_yuv420_packed422_frame_dev;  /* 32 bytes on LP64 */
mi_status mi_equalize_hist_yuv420_to_packed422_frames_dev(mi_ctx* ctx, const mi_yuv420_packed422_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_yuv420_to_packed422_frames_dev(mi_ctx* ctx, const mi_yuv420_packed422_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_bgra_to_yuv420*: interleaved 8-bit FOUR-channel images (CV_8UC4: BGRA / BGRX, or RGBA / RGBX) in, 4:2:0 frames described by
 * mi_yuv420_planes out with the luma equalized -- what render targets, swap-chain images, screen and window capture, compositor
 * surfaces, browser canvases and GL / Vulkan / D3D interop buffers hold -> hardware encoder (NV12) or software encoder (I420 / YV12:
 * data[0..2] / linesize[0..2]) in one pass over the 4 B/px surface, without a slice-and-copy to three channels outside the library.
 * Per frame the bytes are what OpenCV 4.4 gives for
 *     cv::cvtColor(bgra, i420, cv::COLOR_BGRA2YUV_I420);                                         (COLOR_RGBA2YUV_I420 for MI_ORDER_RGB)
 *     cv::Mat y = i420(Rect(0, 0, W, H));  cv::equalizeHist(y, y)  /  clahe->apply(y, y);        (Y only)
 * with the U plane going to out->c0 and the V plane to out->c1 (MI_UV_COPY) or every chroma byte 128 (MI_UV_FILL128).  Chroma comes
 * from the top-left pixel of each 2 x 2 block, without averaging.  The fourth byte X (alpha or padding) takes no part in any output
 * byte: the output is byte for byte what mi_*_bgr_to_yuv420* of the same kind writes for the image with X removed, at the same output
 * layout.  c0 is always U and c1 always V: a YV12 caller passes the address of its second chroma plane as c0.  The same
 * clahe_fp_contract option, the same REFLECT_101 padding when the tile grid does not divide the frame and the same limits on sizes and
 * tile grids as the planar forms, with the same statuses.
 *   input  : frame f at d_in + f * in_frame_stride, H rows of 4*W bytes at in_pitch >= 4*W: B, G, R, X per pixel (MI_ORDER_BGR) or
 *            R, G, B, X (MI_ORDER_RGB).  The input is never written.
 *   output : `out` is read only during the call.  Frame f has every plane at its pointer + f * out->frame_stride: Y, H rows of W bytes
 *            at y_pitch >= W; PLANAR: c0 = U and c1 = V, each H/2 rows of W/2 bytes at c_pitch >= W/2; INTERLEAVED: c0 = the UV plane,
 *            H/2 rows of W bytes at c_pitch >= W, c1 ignored.  Only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each
 *            output row are written: not the pitch padding, not the gaps between the planes, not the gaps between frames.
 * Both chroma layouts are this form's own kernels: unlike mi_*_bgr_to_yuv420*, an MI_CHROMA_INTERLEAVED output is not handed to another
 *   form, and the counters below count both layouts.
 * Alignment: none is required of any pointer, pitch or stride.  A call moves 16 x 2 pixel groups per lane when W % 16 == 0; d_in,
 *   in_pitch, in_frame_stride, out->y, out->y_pitch and out->frame_stride are multiples of 16; and the chroma terms are multiples of 16
 *   for interleaved chroma (out->c0 and out->c_pitch: one 16-byte UV store) and of 8 for planar chroma (out->c0, out->c1 and
 *   out->c_pitch: one 8-byte U store and one 8-byte V store).  A lane then makes eight 16-byte loads (every dword one pixel) and two
 *   16-byte Y stores.  Otherwise the call processes 2 x 2 pixel blocks with byte accesses -- slower, the same bytes out.
 * Two stages per chunk of 256 frames, as in mi_*_bgr_to_yuv420*.  Y is not in the input, so stage 1 converts: ONE kernel (charged to
 *   MI_K_COLOR) reads the image once, writes Y and the chroma into the caller's planes and, for equalizeHist, counts the luma bytes it
 *   has just produced.  Stage 2 maps the luma IN PLACE in out->y with the planar kernels: equalizeHist one MI_K_EQ_LUT and one
 *   MI_K_LUT_APPLY launch (no MI_K_HIST launch; never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel, option
 *   two_kernel_max_frames does not apply); CLAHE exactly what mi_clahe_u8_batch_dev launches for that plane in place.  Bytes moved per
 *   pixel: equalizeHist 4 + 1.5 + 1 + 1 = 7.5, CLAHE 5.5 + 3 = 8.5.  Between the stages out->y holds the unequalized luma.
 * Counters (mi_ctx_get_stat): "bgra_yuv420_vec" / "bgra_yuv420_bytes", one count per call by the walk the conversion kernel took
 *   (16 x 2 groups / 2 x 2 blocks).  A device or host call with work to do moves exactly one of them; a call that returns an error or
 *   has a zero size moves neither.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 *   same shape as the other batched device forms.
 * mi_equalize_hist_bgra_to_yuv420 / mi_clahe_bgra_to_yuv420: ONE CV_8UC4 image in host memory at in_step >= 4*W, at any address, in;
 *   `out` holds HOST pointers at any address and pitch (frame_stride is ignored).  Synchronous; the image is staged in like
 *   mi_*_bgr_to_yuv420's, with a row of 4*W bytes, and the planes come back like mi_*_yuv420's (planes in pinned memory that are tight
 *   are DMA'd as they are, everything else goes through the context's pinned staging).  On the device the frame is tight with every
 *   plane at a 16-byte aligned offset, so a W % 16 == 0 frame takes the 16 x 2 groups.  Whatever the call returns, no copy on the
 *   caller's memory is in flight any more when it returns.  W*H > 0x7fffffff / 4: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx, d_in or `out`; a null out->y or out->c0; a null out->c1 on a PLANAR output; a `chroma` other than
 *   the two values; an `order` other than the two; a bad uv_mode; a negative size; an odd width or an odd height (refused even when
 *   another size is 0, as in the sibling forms); in_pitch < 4*W; y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar);
 *   tiles <= 0; two output plane pointers of the call that are equal; an output plane pointer equal to d_in (there is no in-place
 *   form).  Any other overlap: undefined, not checked; U and V rows side by side in one pitched plane (c1 = c0 + W/2, c_pitch = W) are
 *   legal, as in mi_*_yuv420*.  width, height or n_frames of 0: MI_OK, nothing written (pointers and pitches are not looked at then).
 *   Sizes and tile grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.  Nothing is enqueued
 *   unless every check passes.
 * 4:2:0 in, BGRA out is mi_*_yuv420_to_bgra* below, packed 4:2:2 in, BGRA out mi_*_packed422_to_bgra* above, BGRA in, packed 4:2:2 out mi_*_bgra_to_packed422* below.  Not built: a four-channel mi_bgr_luma_op; a mi_pipe format. */
mi_status mi_equalize_hist_bgra_to_yuv420_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        const mi_yuv420_planes* out, int width, int height, int n_frames, int order, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgra_to_yuv420_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        const mi_yuv420_planes* out, int width, int height, int n_frames, int order, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_bgra_to_yuv420(mi_ctx* ctx, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out,
        int width, int height, int order, mi_uv_mode uv_mode);
mi_status mi_clahe_bgra_to_yuv420(mi_ctx* ctx, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out,
        int width, int height, int order, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_bgra_to_yuv420_frames_dev: the same conversion on a LIST of device frames, each at its own addresses -- a pool of CV_8UC4
 * surfaces in (a renderer, a compositor or a capture API hands over one surface per frame), an encoder's frame pool out (NV12: a
 * pitched Y and a pitched UV plane per surface; x264, libvpx, SVT-AV1: three separately allocated, pitched planes).  The batch form
 * needs both sides in one allocation each at a constant frame stride; one n_frames = 1 batch call per frame costs a launch sequence
 * per frame with tiny grids, and repacking both pools into strided scratch moves 4 + 1.5 bytes per pixel more each way.
 * `frames` is a host array of n_frames entries of the existing mi_bgr_yuv420_frame_dev {in, y, c0, c1}, read only during the call; the
 * pointers in it are device pointers on the context's device.
 * Shape: all frames of one call share width, height, order, uv_mode, chroma and the three pitches (bytes between rows); each has its
 *   own addresses.  There are no per-frame pitches.
 *   in : H rows of 4*W bytes at in_pitch >= 4*W -- B, G, R, X per pixel (MI_ORDER_BGR) or R, G, B, X (MI_ORDER_RGB); X takes no part
 *   y  : H rows of W bytes at y_pitch >= W
 *   chroma == MI_CHROMA_PLANAR: c0 is always U and c1 always V, each H/2 rows of W/2 bytes at c_pitch >= W/2 (both planes share the
 *        pitch): a YV12 caller exchanges the two addresses.
 *   chroma == MI_CHROMA_INTERLEAVED: c0 is the UV plane, H/2 rows of W bytes at c_pitch >= W; c1 is ignored and may be NULL.  The list is
 *        not handed to another form: one pair of entry points and one set of counters serves both layouts.
 * Bytes: per frame the output is byte for byte what mi_*_bgra_to_yuv420_batch_dev writes for that frame alone at the same pitches --
 *   cvtColor(COLOR_BGRA2YUV_I420, or the RGBA code), then cv::equalizeHist / CLAHE::apply on Y, U and V of the conversion (MI_UV_COPY) or
 *   every chroma byte 128 (MI_UV_FILL128); the clahe_fp_contract option is honoured, REFLECT_101 padding applies when the tile grid
 *   does not divide the frame, the limits on sizes and tile grids are the batch form's, with the same statuses.
 * Writes: only the W bytes of each Y and interleaved UV row and the W/2 bytes of each planar U and V row are written: not the pitch
 *   padding, not the gaps between planes or frames.  The images are never written.
 * Alignment: none is required of any address or pitch.  The shape decides what is allowed: 16 x 2 pixel groups when W % 16 == 0,
 *   in_pitch and y_pitch are multiples of 16 and c_pitch is a multiple of 16 (interleaved) or 8 (planar).  Each frame then decides by
 *   its own addresses: it takes the groups when its in and y are multiples of 16 and its c0 is a multiple of 16 (interleaved) or its
 *   c0 and c1 are multiples of 8 (planar), and any other frame of the same call processes 2 x 2 pixel blocks with byte accesses while
 *   its neighbours stay vectorised -- slower, the same bytes out.
 * Stages, per chunk of 64 frames of the list (not the batch form's 256): stage 1 is ONE launch charged to MI_K_COLOR that converts
 *   into the caller's planes and, for equalizeHist, counts the luma bytes it has just produced.  Stage 2 maps the luma IN PLACE on the
 *   chunk's Y planes: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no MI_K_HIST launch; never the fused equalizeHist
 *   kernel nor the single-launch histogram + LUT kernel, option two_kernel_max_frames does not apply); CLAHE exactly what
 *   mi_clahe_nv12_frames_dev launches in place on those Y planes.  Launches are charged to the same profiling slots as the batch form.
 *   Between the stages a frame's y holds the unequalized luma.
 * Counters (mi_ctx_get_stat): "bgra_yuv420_list_frames_vec" / "bgra_yuv420_list_frames_bytes" count the FRAMES (not calls) of list
 *   calls by the walk their stage-1 kernel took: 16 x 2 groups / 2 x 2 blocks, n_frames in total per call.  "bgra_yuv420_vec" /
 *   "bgra_yuv420_bytes" are not touched by list calls.  A call that returns an error or has nothing to do moves none.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image (4*W bytes each) meet the rows of a plane of
 *   its own frame, or the rows of its Y plane meet the rows of a chroma plane of its own (compared as address ranges), and on a PLANAR
 *   list when c0 == c1.  U and V are otherwise not compared with each other: the U and V rows may lie side by side in one pitched
 *   plane (c1 = c0 + W/2, c_pitch = W), as in the batch form.  The same image may appear in several entries (inputs are only read).
 *   Outputs that overlap ANOTHER frame's planes give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null in, y or c0 in any entry; a null c1 in any entry on a
 *   PLANAR list; a `chroma` other than the two values; an `order` other than the two; a bad uv_mode; a negative size; an odd width or
 *   an odd height (refused even when another size is 0, as in the batch form); in_pitch < 4*W; y_pitch < W; a c_pitch below its row
 *   (W interleaved, W/2 planar); tiles <= 0; the overlap above.  Sizes and tile grids the planar forms refuse: the status they give
 *   (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written (n_frames == 0 with a null list is MI_OK).  Nothing
 *   is enqueued unless every frame passes the checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
mi_status mi_equalize_hist_bgra_to_yuv420_frames_dev(mi_ctx* ctx, const mi_bgr_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgra_to_yuv420_frames_dev(mi_ctx* ctx, const mi_bgr_yuv420_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_bgra_to_packed422*: interleaved 8-bit FOUR-channel images (CV_8UC4: BGRA / BGRX, or RGBA / RGBX) in, packed 4:2:2 frames
 * (YUY2 / UYVY) out with the luma equalized -- render target, swap-chain image, screen or window capture, GL / Vulkan interop buffer
 * -> SDI / HDMI playout card, v4l2 output or loopback device, virtual camera, in one pass over the 4 B/px surface: without slicing the
 * first three channels into a contiguous scratch batch outside the library for mi_*_bgr_to_packed422_batch_dev, and without an NV12
 * intermediate (which has dropped every second chroma row).  The signatures are those of mi_*_bgr_to_packed422*.
 * Bytes: the output is byte for byte what mi_*_bgr_to_packed422* writes for the image with its fourth byte removed:
 *   luma   : Y = bt601_y(b, g, r) of every pixel, then cv::equalizeHist / CLAHE::apply on the W x H luma plane; the clahe_fp_contract
 *            option is honoured and REFLECT_101 padding applies when the tile grid does not divide the frame.
 *   chroma : MI_UV_COPY: U and V of macropixel (k, y) are bt601_uv of the LEFT pixel (2k, y) of that row, without averaging.
 *            MI_UV_FILL128: every chroma byte 128, the chroma arithmetic is skipped.
 *   MI_FMT_YUY2 writes exactly Y0 U Y1 V, MI_FMT_UYVY exactly U Y0 V Y1.  MI_ORDER_BGR reads B, G, R, X per pixel, MI_ORDER_RGB reads
 *   R, G, B, X.  The fourth byte X (alpha or padding) is read with its pixel and takes part in nothing.
 *   input  : frame f at d_in + f * in_frame_stride, H rows of 4*W bytes at in_pitch >= 4*W, at any address.  The input is never written.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 2*W bytes at out_pitch >= 2*W; d_out, out_pitch and out_frame_stride
 *            are multiples of 4 (the packed forms' rule).  Only the 2*W bytes of each output row are written: not the pitch padding,
 *            not the gaps between frames.
 * Width is even; height is any value >= 1, odd heights are legal.  Every CLAHE shape runs in one pass.  The limits on sizes and tile
 *   grids are those of mi_*_bgr_to_packed422*, with the same statuses.
 * Alignment: a call moves 16 pixels of one row per lane (four 16-byte loads, every dword one pixel, and two 16-byte stores) when
 *   W % 16 == 0 and d_in, in_pitch, in_frame_stride, d_out, out_pitch and out_frame_stride are all multiples of 16.  Otherwise it
 *   processes one macropixel per lane with byte loads at 8*mx + {0,1,2} and 8*mx + 4 + {0,1,2} and one aligned dword store -- slower,
 *   the same bytes out.
 * Two stages per chunk of 256 frames, as in mi_*_bgr_to_packed422_batch_dev.  Stage 1 converts: ONE kernel (charged to MI_K_COLOR)
 *   reads the image once, writes the packed frame with unequalized luma into d_out and, for equalizeHist, counts the luma bytes it has
 *   just produced.  Stage 2 is exactly that form's: the packed form's own kernels IN PLACE on the output frame, the chroma bytes kept
 *   whatever uv_mode is: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no MI_K_HIST launch); CLAHE exactly what
 *   mi_clahe_packed422_batch_dev launches for those frames in place.  Never the fused equalizeHist kernel nor the single-launch
 *   histogram + LUT kernel: option two_kernel_max_frames does not apply.  Bytes moved per pixel: equalizeHist 4 + 2 + 2 + 2 = 10,
 *   CLAHE 6 + 2 + 4 = 12.  Between the stages d_out holds the unequalized luma.
 * Counters (mi_ctx_get_stat): "bgra_packed422_vec" / "bgra_packed422_bytes", one count per call by the walk stage 1 took (16-pixel
 *   groups / macropixels).  A device or host call with work to do moves exactly one of them; a call that returns an error or has a
 *   zero size moves neither.  No call of this form moves a bgr_packed422* counter.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of the
 *   same shape as the other batched device forms.
 * mi_equalize_hist_bgra_to_packed422 / mi_clahe_bgra_to_packed422: ONE CV_8UC4 image in host memory at in_step >= 4*W, at any address,
 *   in; one packed frame in host memory at any address and any out_pitch >= 2*W out.  Synchronous; the image is staged in like
 *   mi_*_bgra_to_yuv420's, with a row of 4*W bytes, and the frame comes back like mi_*_bgr_to_packed422's (frames in pinned memory that
 *   are tight are DMA'd as they are, everything else goes through the context's pinned staging).  On the device the frame is tight and
 *   16-byte aligned, so a W % 16 == 0 image takes the 16-pixel groups.  Whatever the call returns, no copy on the caller's memory is in
 *   flight any more when it returns.  W*H > 0x7fffffff / 4: MI_ERR_UNSUPPORTED.
 * There is no in-place form: d_out == d_in is MI_ERR_BAD_ARG; any other overlap of input and output is undefined, not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx, d_in or d_out; an odd width (refused even when another size is 0, as in the packed forms); a
 *   negative size; in_pitch < 4*W; out_pitch < 2*W; a d_out, out_pitch or out_frame_stride of the device form that is not a multiple
 *   of 4; an `order` other than the two; a `format` other than the two; a bad uv_mode; tiles <= 0.  width, height or n_frames of 0:
 *   MI_OK, nothing written (pointers and pitches are not looked at then).  Sizes and tile grids the packed or planar forms refuse:
 *   MI_ERR_UNSUPPORTED, nothing written.  Nothing is enqueued unless every check passes.
 * The frame-list form mi_*_bgra_to_packed422_frames_dev is described below.  Out of scope, not built: YVYU / VYUY, chroma averaging,
 * a use for the alpha byte, P010 / 16-bit. */
mi_status mi_equalize_hist_bgra_to_packed422_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgra_to_packed422_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride,
        void* d_out, size_t out_pitch, size_t out_frame_stride,
        int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_bgra_to_packed422(mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
        int width, int height, int order, int format, mi_uv_mode uv_mode);
mi_status mi_clahe_bgra_to_packed422(mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
        int width, int height, int order, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_bgra_to_packed422_frames_dev: the same conversion on a LIST of device frames, each at its own two addresses -- a pool of CV_8UC4
 * surfaces in (a renderer, a compositor or a capture API hands over one surface per frame), a playout card's, a v4l2 output queue's or
 * a virtual camera's buffer pool out.  `frames` is a host array of n_frames entries of the existing mi_bgr_packed422_frame_dev
 * {in, out}, read only during the call; the pointers in it are device pointers on the context's device.  No new struct, enum or
 * version.
 * Shape: all frames of one call share width, height, the pair of pitches (bytes between rows), order, format and uv_mode; each has its
 *   own two addresses.  There are no per-frame pitches.
 *   in  : H rows of 4*W bytes at in_pitch >= 4*W, at any address -- B, G, R, X per pixel (MI_ORDER_BGR) or R, G, B, X (MI_ORDER_RGB);
 *         X takes no part.  The images are never written.
 *   out : H rows of 2*W bytes at out_pitch >= 2*W; every `out` and out_pitch are multiples of 4 (the packed forms' rule).  Only the
 *         2*W bytes of each output row are written: not the pitch padding, nothing before or behind a frame.
 * Bytes: per frame the output is byte for byte exactly what mi_*_bgra_to_packed422_batch_dev writes for that frame alone at the same
 *   pitches; width is even, odd heights are legal, and the limits on sizes and tile grids are the batch form's, with the same statuses.
 * Alignment: beyond the multiples of 4 above, none is required.  The shape allows 16-pixel groups (four 16-byte loads, two 16-byte
 *   stores per lane) when W % 16 == 0 and in_pitch and out_pitch are multiples of 16; a frame then takes the groups when its own `in`
 *   and `out` are both multiples of 16, and any other frame of the same call processes one macropixel per lane with byte loads and one
 *   aligned dword store while its neighbours stay vectorised -- slower, the same bytes out.  One rule, which the kernel decides by and
 *   the host counts by.
 * Stages, per chunk of 128 frames of the list (not the batch form's 256): stage 1 is ONE launch charged to MI_K_COLOR that converts
 *   into the caller's frames and, for equalizeHist, counts the luma bytes it has just produced.  Stage 2 maps the luma IN PLACE on the
 *   chunk's output frames, the chroma bytes kept whatever uv_mode is: equalizeHist one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch (no
 *   MI_K_HIST launch; never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel, option two_kernel_max_frames
 *   does not apply); CLAHE exactly what mi_clahe_packed422_frames_dev launches in place on those frames, every shape in one pass.
 *   Between the stages a frame's `out` holds the unequalized luma.
 * Counters (mi_ctx_get_stat): "bgra_packed422_list_frames_vec" / "bgra_packed422_list_frames_bytes" count the FRAMES (not calls) of
 *   list calls by the walk their stage-1 kernel took: 16-pixel groups / macropixels.  A list call moves the two by n_frames in total
 *   and does not touch "bgra_packed422_vec" / "bgra_packed422_bytes" nor any bgr_packed422* counter.  A call that returns an error or
 *   has nothing to do moves none.
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image (4*W bytes each) meet the rows of its own
 *   output frame (compared as address ranges).  The same image may appear in several entries (inputs are only read).  Outputs that
 *   overlap ANOTHER frame's image or output give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null `in` or `out` in any entry; an `out` in any entry or
 *   an out_pitch that is not a multiple of 4; an `order` other than the two; a `format` other than the two; a bad uv_mode; a negative
 *   size; an odd width (refused even when another size is 0, as in the batch form); in_pitch < 4*W; out_pitch < 2*W; tiles <= 0; the
 *   overlap above.  Sizes and tile grids the packed or planar forms refuse: MI_ERR_UNSUPPORTED.  width, height or n_frames of 0: MI_OK,
 *   nothing written (the entries and the pitches are not looked at then; n_frames == 0 with a null list is MI_OK).  Nothing is enqueued
 *   unless every frame passes the checks: a bad last entry leaves the earlier frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
mi_status mi_equalize_hist_bgra_to_packed422_frames_dev(mi_ctx* ctx, const mi_bgr_packed422_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int order, int format, mi_uv_mode uv_mode, void* stream);
mi_status mi_clahe_bgra_to_packed422_frames_dev(mi_ctx* ctx, const mi_bgr_packed422_frame_dev* frames, int n_frames,
        int width, int height, size_t in_pitch, size_t out_pitch, int order, int format, mi_uv_mode uv_mode,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
/* mi_*_yuv420_to_bgra*: 4:2:0 frames described by mi_yuv420_planes in -- interleaved chroma (NV12: a hardware decoder's surfaces) or
 * planar chroma (I420 / YV12: ffmpeg yuv420p, libvpx, dav1d) -- interleaved 8-bit FOUR-channel images (CV_8UC4: BGRA, or RGBA) out, in
 * the pass that equalizes: decoder -> display surface, swap-chain image, GL / Vulkan / interop texture, Qt / SDL / Wayland buffer or
 * GUI image, without a three-channel image in scratch and a widen to four channels outside the library.  In OpenCV terms
 * cv::equalizeHist / CLAHE::apply on the Y plane, then cv::cvtColor with COLOR_YUV2BGRA_NV12, COLOR_YUV2BGRA_I420 or
 * COLOR_YUV2BGRA_YV12 (MI_ORDER_BGR), or with COLOR_YUV2RGBA_NV12, COLOR_YUV2RGBA_I420 or COLOR_YUV2RGBA_YV12 (MI_ORDER_RGB).  Y is
 * read twice (histograms, then map), the chroma once, 4 bytes per pixel are written: 6.5 B/px, where mi_*_yuv420_to_bgr_batch_dev into
 * scratch plus a widen outside the library moves about 12.5.
 *   input  : as in mi_*_yuv420_to_bgr*: `in` is read only during the call.  Frame f has every plane at pointer + f * in->frame_stride:
 *            Y, H rows of W bytes at y_pitch >= W; MI_CHROMA_PLANAR: c0 is always U and c1 always V, each H/2 rows of W/2 bytes at
 *            c_pitch >= W/2 (a YV12 caller passes its second chroma plane as c0); MI_CHROMA_INTERLEAVED: c0 is the UV plane, H/2 rows of
 *            W bytes at c_pitch >= W, c1 is ignored and may be NULL.  Width and height must be even.  The input is never written.
 *   output : frame f at d_out + f * out_frame_stride, H rows of 4*W bytes at out_pitch >= 4*W: B, G, R, A per pixel (MI_ORDER_BGR) or
 *            R, G, B, A (MI_ORDER_RGB) with A = 255 in every pixel, what OpenCV's four-channel YUV decodes write.  Only the 4*W bytes
 *            of each output row are written: not the pitch padding, not the gap between frames.  There is no in-place form.
 * Bytes: the first three bytes of every pixel are byte for byte what mi_*_yuv420_to_bgr_batch_dev writes for the same call with the
 *   same `order`, and the rest of the arithmetic contract is that form's: the clahe_fp_contract option is honoured (by the fallback),
 *   REFLECT_101 padding applies when the tile grid does not divide the frame, the limits on sizes and tile grids are the planar
 *   forms', with their statuses.  Never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel.
 * Both chroma layouts are this form's own kernels: unlike mi_*_yuv420_to_bgr*, an MI_CHROMA_INTERLEAVED input is not handed to the NV12
 *   form, mi_*_nv12_to_bgr* is unchanged, and the counters below count both layouts.
 * Alignment: none is required of any pointer, pitch or stride.  A call moves 16 x 2 pixel groups per lane when W % 16 == 0; in->y,
 *   in->y_pitch, in->frame_stride, d_out, out_pitch and out_frame_stride are multiples of 16; and the chroma terms in->c0, in->c1 and
 *   in->c_pitch are multiples of 16 for interleaved chroma (c1 not looked at) and of 8 for planar chroma.  A lane then makes two
 *   16-byte Y loads, one 16-byte UV load or one 8-byte U load plus one 8-byte V load, and eight 16-byte stores (every dword one
 *   pixel).  Otherwise the call processes 2 x 2 pixel blocks with byte accesses -- slower, the same bytes out.
 * CLAHE maps and converts in one kernel (one pass) when that alignment rule holds and the shape is the NV12 form's one-pass shape
 *   (the tile grid divides the frame, tile width a multiple of 16, tiles_x <= 14, clahe_fp_contract off); any other call runs the
 *   planar CLAHE into scratch Y planes of the context and then the conversion alone: the same bytes in one more pass (two-pass).
 *   equalizeHist always counts as one-pass.
 * Counters (mi_ctx_get_stat): "yuv420_bgra_onepass" / "yuv420_bgra_twopass", one count per call; "yuv420_bgra_vec" /
 *   "yuv420_bgra_bytes", one count per batch or host call by the walk the pixel-writing kernel took (16 x 2 groups / 2 x 2 blocks).
 *   Every batch or host call with work to do moves exactly one counter of each pair; a call that returns an error or has a zero size
 *   moves none.  No existing counter moves: not the "nv12_bgr_*" pair on an interleaved input, not the "yuv420_bgr_*" ones.
 * Launches run in chunks of 256 frames and are charged to the existing profiling slots by role: MI_K_HIST, MI_K_EQ_LUT and
 *   MI_K_LUT_APPLY (map + decode) for equalizeHist; the tile-LUT slots and MI_K_CLAHE_INTERP (blend + decode) for one-pass CLAHE;
 *   MI_K_COLOR for the decode alone behind the planar CLAHE.  Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has
 *   frames pending and hipGraph capture after one eager call of the same shape as the other batched device forms.
 * mi_equalize_hist_yuv420_to_bgra / mi_clahe_yuv420_to_bgra: ONE frame with `in` holding HOST pointers at any address and pitch
 *   (frame_stride is ignored), a CV_8UC4 image at out_step >= 4*W out.  Synchronous; the planes are staged like
 *   mi_*_yuv420_to_bgr's (planes in pinned memory that are tight are DMA'd as they are, everything else goes through the context's
 *   pinned staging) and the image comes back like that form's, at a row of 4*W bytes.  On the device the frame is tight with every
 *   plane at a 16-byte aligned offset, so a W % 16 == 0 frame takes the 16 x 2 groups.  Whatever the call returns, no copy on the
 *   caller's memory is in flight any more when it returns.  W*H > 0x7fffffff / 4: MI_ERR_UNSUPPORTED.
 * Errors, MI_ERR_BAD_ARG: a null ctx or `in`; a `chroma` other than the two values; an `order` other than the two; a negative size; an
 *   odd width or an odd height (refused even when another size is 0, as in the sibling forms); tiles <= 0; a null in->y, in->c0 or
 *   d_out; a null in->c1 on a PLANAR input; y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar); out_pitch < 4*W; d_out
 *   equal to any input plane pointer of the call.  Any other overlap: undefined, not checked.  width, height or n_frames of 0: MI_OK,
 *   nothing written.  Sizes and tile grids the planar forms refuse: the status they give (MI_ERR_UNSUPPORTED), nothing written.
 *   Nothing is enqueued unless every check passes. */
mi_status mi_equalize_hist_yuv420_to_bgra_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
        size_t out_frame_stride, int width, int height, int n_frames, int order, void* stream);
mi_status mi_clahe_yuv420_to_bgra_batch_dev(mi_ctx* ctx, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
        size_t out_frame_stride, int width, int height, int n_frames, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);
mi_status mi_equalize_hist_yuv420_to_bgra(mi_ctx* ctx, const mi_yuv420_planes* in, uint8_t* out, size_t out_step,
        int width, int height, int order);
mi_status mi_clahe_yuv420_to_bgra(mi_ctx* ctx, const mi_yuv420_planes* in, uint8_t* out, size_t out_step,
        int width, int height, int order, double clip_limit, int tiles_x, int tiles_y);
/* mi_*_yuv420_to_bgra_frames_dev: the same conversion on a LIST of device frames, each at its own addresses -- a decoder's frame pool
 * in (a software decoder: three separately allocated, pitched planes a frame, data[0..2] / linesize[0..2]; a hardware decoder: a Y
 * and a UV plane a surface), a pool of CV_8UC4 surfaces or textures out.  `frames` is a host array of n_frames entries of the existing
 * mi_yuv420_bgr_frame_dev {y, c0, c1, out}, read only during the call; the pointers in it are device pointers on the context's device.
 * Shape: all frames of one call share width, height, order, chroma and the three pitches (bytes between rows); each has its own
 *   addresses.  There are no per-frame pitches.
 *   y  : H rows of W bytes at y_pitch >= W
 *   chroma == MI_CHROMA_PLANAR: c0 is always U and c1 always V, each H/2 rows of W/2 bytes at c_pitch >= W/2 (both planes share the
 *        pitch): a YV12 caller exchanges the two addresses.
 *   chroma == MI_CHROMA_INTERLEAVED: c0 is the UV plane, H/2 rows of W bytes at c_pitch >= W; c1 is ignored and may be NULL.  The list is
 *        not handed to another form: one pair of entry points and one set of counters serves both layouts.
 *   out: H rows of 4*W bytes at out_pitch >= 4*W -- B, G, R, A per pixel (MI_ORDER_BGR) or R, G, B, A (MI_ORDER_RGB), A = 255
 * Bytes: per frame the output is byte for byte what mi_*_yuv420_to_bgra_batch_dev writes for that frame alone at the same pitches; the
 *   clahe_fp_contract option is honoured, REFLECT_101 padding applies when the tile grid does not divide the frame, the limits on
 *   sizes and tile grids are the batch form's, with the same statuses.
 * Writes: only the 4*W bytes of each output row are written, not the pitch padding; the input planes are never written.
 * Alignment: none is required of any address or pitch.  The shape decides what is allowed: 16 x 2 pixel groups when W % 16 == 0,
 *   y_pitch and out_pitch are multiples of 16 and c_pitch is a multiple of 16 (interleaved) or 8 (planar).  Each frame then decides by
 *   its own addresses: it takes the groups when its y and out are multiples of 16 and its c0 is a multiple of 16 (interleaved) or its
 *   c0 and c1 are multiples of 8 (planar), and any other frame of the same call processes 2 x 2 pixel blocks with byte accesses while
 *   its neighbours stay vectorised -- slower, the same bytes out.  equalizeHist always maps the luma and converts in one kernel.
 *   CLAHE does so when the shape is the batch form's one-pass shape, the shape rule above holds and every frame of the call satisfies
 *   the address rule; otherwise the whole call runs the planar CLAHE into scratch Y planes of the context and converts from there:
 *   the same bytes in one more pass.  (In that fallback the Y address the rule sees is the scratch plane's, which is aligned; the
 *   pitches are still the caller's.)
 * Counters (mi_ctx_get_stat): "yuv420_bgra_onepass" / "yuv420_bgra_twopass" count the calls of the list form too, one count a call
 *   (equalizeHist always counts as one-pass).  "yuv420_bgra_list_frames_vec" / "yuv420_bgra_list_frames_bytes" count the FRAMES (not
 *   calls) of list calls by the walk their pixel-writing kernel took: 16 x 2 groups / 2 x 2 blocks, n_frames in total per call.
 *   "yuv420_bgra_vec" / "yuv420_bgra_bytes" are not touched by list calls.  A call that returns an error or has nothing to do moves
 *   none; no existing counter moves.
 * Launches are charged to the same profiling slots as the batch form, per chunk of 64 frames of the list (not the batch form's 256).
 * Overlap: there is no in-place form.  MI_ERR_BAD_ARG when the rows of a frame's image (4*W bytes each) meet the rows of its own Y, U
 *   or V plane (or UV plane; compared as address ranges).  Input planes are not compared with each other: the U and V rows may lie
 *   side by side in one pitched plane (c1 = c0 + W/2, c_pitch = W).  The same input planes may appear in several entries (inputs are
 *   only read).  Outputs that overlap each other or ANOTHER frame's planes give undefined results and are not checked.
 * Errors, MI_ERR_BAD_ARG: a null ctx; a null `frames` with n_frames > 0; a null y, c0 or out in any entry; a null c1 in any entry on a
 *   PLANAR list; a `chroma` other than the two values; an `order` other than the two; a negative size; an odd width or an odd height
 *   (refused even when another size is 0, as in the batch form); y_pitch < W; a c_pitch below its row (W interleaved, W/2 planar);
 *   out_pitch < 4*W; tiles <= 0; the overlap above.  Sizes and tile grids the planar forms refuse: the status they give
 *   (MI_ERR_UNSUPPORTED).  width, height or n_frames of 0: MI_OK, nothing written.  Nothing is enqueued unless every frame passes the
 *   checks: a bad last entry leaves the first frames' outputs untouched.
 * Stream rules, MI_STREAM_CTX, MI_ERR_BUSY while the context's pipe has frames pending and hipGraph capture after one eager call of
 *   the same shape as the other device list forms; a captured graph holds the addresses it was captured with. */
mi_status mi_equalize_hist_yuv420_to_bgra_frames_dev(mi_ctx* ctx, const mi_yuv420_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order, void* stream);
mi_status mi_clahe_yuv420_to_bgra_frames_dev(mi_ctx* ctx, const mi_yuv420_bgr_frame_dev* frames, int n_frames,
        int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order,
        double clip_limit, int tiles_x, int tiles_y, void* stream);

/* ---- optional: pin caller-owned host buffers----------------------------------------------------------------
 * Video pipelines recycle a small pool of frame buffers (GstBufferPool; the reference maps such buffers at
 * OpenCVequalHist.cpp:115/:158).  Registering a pool's memory once lets the host-pointer forms DMA straight
 * from / into it instead of staging through the context's pinned buffers (contiguous planes only; anything
 * else still stages).  Process-wide, thread-safe; the memory must stay valid -- and must not be freed -- until
 * mi_host_unregister() has returned MI_OK.
 * mi_host_unregister returns MI_ERR_BUSY, and leaves the buffer registered, while a pipe still has a transfer queued on it
 * (between the mi_pipe_submit that took the frame and the mi_pipe_wait that returns it, or the pipe's destruction): unpinning
 * pages under the copy engine is a GPU access to an ordinary heap address, which ends the process.  The reference's accelerator
 * path has the same window and no guard (OpenCLequalHist.cpp:356-367).  MI_ERR_BAD_ARG: `ptr` is not the start of a registered range.
 * MI_ERR_HIP: the runtime refused to unpin although the pages are still pinned; the buffer is STILL registered -- ask again, do not
 * free it yet.  If the runtime refuses because it no longer knows the pages as pinned (the caller unpinned them itself with
 * hipHostUnregister, a runtime teardown did), the entry is dropped and MI_OK returned: nothing is left to undo.
 * mi_host_unregister may wait for the device; it does not hold up other threads' mi_pipe_submit / host-form calls meanwhile (the
 * range being unpinned is simply not treated as pinned any more).  A second thread unregistering the same buffer (same `ptr`) at that
 * moment gets BUSY; when it asks again after the first thread is through it gets MI_ERR_BAD_ARG, which then means "already
 * unregistered" -- only the thread that received MI_OK may free the memory on the strength of its own call.
 * Memory the caller pinned by other means (hipHostMalloc, hipHostRegister) is recognised as pinned when the whole plane lies in ONE
 * such allocation; releasing it while frames are pending is the caller's responsibility. */
mi_status mi_host_register(void* ptr, size_t bytes);
mi_status mi_host_unregister(void* ptr);

/* ---- asynchronous in-order frame pipeline: the per-GPU worker of the frame-sharded stream ---------------------
 * The reference's worker maps a frame, runs the op, rebuilds the NV12 frame and pushes it downstream, one frame at
 * a time (OpenCVequalHist.cpp:102-196); its accelerator variant blocks on each of write, write, task, read
 * (OpenCLequalHist.cpp:356-365).  A pipe is that worker's device side with up to `depth` frames in flight: the upload
 * of frame k+2, the kernels of frame k+1 and the download of frame k run concurrently (two upload lanes, one compute
 * stream, two download lanes per device, shared by all pipes of the process; both DMA directions busy), so ONE host
 * thread per GPU keeps the link full.  Frames are tightly packed NV12 in host memory
 * (W*H + W*H/2 bytes), caller-owned from mi_pipe_submit until the mi_pipe_wait that returns them; completion is in
 * submission order.  Register recycled frame buffers once with mi_host_register (a GstBufferPool's memory): their
 * copies are then fully asynchronous.  Unpinned (pageable) memory is accepted -- the calling thread copies it into / out of
 * pinned staging buffers of the pipe (in mi_pipe_submit / mi_pipe_wait), the DMA itself stays asynchronous.
 *   op         MI_OP_EQUALIZE (OpenCVequalHist.cpp:145), MI_OP_CLAHE (clahevideo.cpp:195), or MI_OP_CHANNELS
 *              (NV12 -> BGR -> equalizeHist on B, G, R -> NV12: mi_nv12_bgr_equalize; ignores uv_mode)
 *   uv_policy  MI_PIPE_UV_HOST (= AUTO for the Y-only ops): only the Y plane crosses PCIe; the UV half is filled with
 *              128 / copied by the calling thread inside mi_pipe_wait while the engines work (the reference's own
 *              memset / memcpy, OpenCVequalHist.cpp:160-162, ColoropenCVCwqualHist.cpp:165);
 *              MI_PIPE_UV_DEVICE: whole frames cross the bus and the kernels write the UV half (no host CPU work)
 *   depth      frames in flight, 2..16; 0 = by frame size: 3 for frames of 8 MiB and more (4K), 6 below (measured: a thread that
 *              submits and waits on 4K frames is fastest with three in flight, 1080p frames want six; a pool whose worker is fed
 *              by another thread runs 4K best with four -- cxx/mi_pool.hpp passes its own)
 * mi_pipe_submit returns MI_ERR_BUSY when `depth` frames are pending.  mi_pipe_wait blocks for the OLDEST pending
 * frame and returns its tag and output pointer.  A pipe uses its context's scratch and lock: ONE pipe per context (a
 * second mi_pipe_create answers MI_ERR_BUSY), destroy it before the context; the context's other compute entry points may
 * be used while no frame is pending and answer MI_ERR_BUSY otherwise.
 * Errors keep caller and pipe in step: a failed mi_pipe_submit occupies no slot and leaves no copy in flight on in / out;
 * a failed mi_pipe_wait has still retired the oldest frame (its tag is returned, its buffers are idle) -- one mi_pipe_wait
 * call, one frame gone, whatever the status.
 * mi_pipe_destroy with frames still pending (submitted, never waited for): the pipe's streams are drained first, so on return NO
 * transfer touches any `in` / `out` buffer any more and registered buffers may be unregistered -- but the CONTENT of those frames'
 * `out` buffers is UNDEFINED: the work mi_pipe_wait does for a frame never happened.  Concretely: under MI_PIPE_UV_HOST the UV half
 * was not written (stale bytes), a registered `out` may or may not hold the finished Y plane, an unpinned `out` received nothing
 * (its result sits in staging that is freed).  Ownership follows the reference's rule for a buffer that was pushed and then dropped
 * (OpenCVequalHist.cpp:183-187: ownership passes on push, a failed push is unref'd, never read): discard such outputs.  A caller
 * that wants every frame calls mi_pipe_wait until mi_pipe_pending() is 0 before destroying the pipe; micv::FramePool::finish()
 * and nv12_stream do exactly that and never rely on destroy to complete a frame.
 *   format     MI_FMT_NV12 (0, the default of a zeroed config) or MI_FMT_P010 (16-bit frames of 3*W*H bytes, see mi_clahe_p010;
 *              in / out are then those frames' bytes).  P010 takes MI_OP_CLAHE only -- the other ops answer MI_ERR_UNSUPPORTED at
 *              mi_pipe_create -- and runs it through the 16-bit path; under MI_PIPE_UV_HOST only Y crosses and the waiting thread
 *              writes the chroma, under MI_PIPE_UV_DEVICE whole frames cross and a kernel writes it.  Default depth by frame bytes.
 *              MI_FMT_YUY2 / MI_FMT_UYVY: packed 4:2:2 frames of 2*W*H bytes, tight (pitch 2*W), W even, any H (see
 *              mi_equalize_hist_packed422); MI_OP_EQUALIZE and MI_OP_CLAHE, MI_OP_CHANNELS answers MI_ERR_UNSUPPORTED.  There is no
 *              luma plane to send on its own: whole frames cross the bus in both directions and the kernels write the chroma --
 *              that is what MI_PIPE_UV_AUTO and MI_PIPE_UV_DEVICE mean here, MI_PIPE_UV_HOST answers MI_ERR_UNSUPPORTED at
 *              mi_pipe_create.  Default depth by frame bytes. */
typedef struct mi_pipe mi_pipe;
enum { MI_OP_EQUALIZE = 0, MI_OP_CLAHE = 1, MI_OP_CHANNELS = 2 };
enum { MI_PIPE_UV_AUTO = 0, MI_PIPE_UV_HOST = 1, MI_PIPE_UV_DEVICE = 2 };
typedef struct mi_pipe_config {
    int width, height;
    int op;                      /* MI_OP_EQUALIZE | MI_OP_CLAHE | MI_OP_CHANNELS */
    mi_uv_mode uv_mode;
    double clip_limit;           /* MI_OP_CLAHE */
    int tiles_x, tiles_y;        /* MI_OP_CLAHE */
    int depth;
    int uv_policy;
    int format;                  /* MI_FMT_NV12 | MI_FMT_P010 | MI_FMT_YUY2 | MI_FMT_UYVY (appended in 0.3: keep it the last member) */
} mi_pipe_config;
mi_status mi_pipe_create(mi_ctx* ctx, const mi_pipe_config* cfg, mi_pipe** out);
void      mi_pipe_destroy(mi_pipe* pipe);
mi_status mi_pipe_submit(mi_pipe* pipe, const uint8_t* in, uint8_t* out, uint64_t tag);
mi_status mi_pipe_wait(mi_pipe* pipe, uint64_t* tag, uint8_t** out_frame);
int       mi_pipe_pending(const mi_pipe* pipe);
int       mi_pipe_depth(const mi_pipe* pipe);

/* ---- colour-domain neighbours of the path (parity unpinned, see oracle/color_oracle.c) ------
 * CV_8UC3 interleaved images, row pitch >= 3*width.
 * mi_cvt_color_u8c3: cv::cvtColor(src, dst, code) for code = MI_COLOR_BGR2YUV (cv::COLOR_BGR2YUV = 82,
 *   singlecolor.cpp:39, clahe1frame.cpp:83) or MI_COLOR_YUV2BGR (cv::COLOR_YUV2BGR = 84, singlecolor.cpp:66,
 *   clahe1frame.cpp:102).  src == dst allowed.
 * mi_bgr_luma_op_u8c3: the whole image-bench sequence in one call -- cvtColor(BGR2YUV) -> split -> equalizeHist
 *   (op = MI_OP_EQUALIZE, singlecolor.cpp:39-66) or CLAHE (op = MI_OP_CLAHE, clahe1frame.cpp:83-102) on the Y
 *   plane -> merge -> cvtColor(YUV2BGR); split/merge are fused into the conversion kernels. */
enum { MI_COLOR_BGR2YUV = 82, MI_COLOR_YUV2BGR = 84 };
mi_status mi_cvt_color_u8c3(mi_ctx* ctx, const uint8_t* src, size_t src_step, uint8_t* dst, size_t dst_step,
                            int width, int height, int code);
mi_status mi_cvt_color_u8c3_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                                      void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                      int width, int height, int n_frames, int code, void* stream);
mi_status mi_bgr_luma_op_u8c3(mi_ctx* ctx, const uint8_t* src, size_t src_step, uint8_t* dst, size_t dst_step,
                              int width, int height, int op, double clip_limit, int tiles_x, int tiles_y);
mi_status mi_bgr_luma_op_u8c3_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                                        void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                        int width, int height, int n_frames, int op,
                                        double clip_limit, int tiles_x, int tiles_y, void* stream);

/* ---- BASELINE.json config 5 read literally (second half; parity unpinned) --------------------------
 * NV12 frame -> BGR -> cv::equalizeHist on each of B, G and R -> NV12.  No file of the reference does this
 * (ColoropenCVCwqualHist.cpp, which the config names, equalizes Y only and copies UV: :146, :165 -- that behaviour is
 * mi_equalize_hist_nv12(..., MI_UV_COPY)).  The entry points below stand for the OpenCV 4.4 sequence a maintainer
 * would write for the config's wording:
 *     cv::cvtColor(nv12, bgr, cv::COLOR_YUV2BGR_NV12); cv::split; cv::equalizeHist x3; cv::merge;
 *     cv::cvtColor(bgr, i420, cv::COLOR_BGR2YUV_I420); U and V interleaved back into an NV12 chroma plane
 * restated in oracle/color_oracle.c (orc_nv12_bgr_equalize).  Tight NV12 frames (W*H luma bytes, then H/2 rows of W
 * interleaved U,V bytes); width and height must be even (OpenCV asserts the same); in == out allowed. */
mi_status mi_nv12_bgr_equalize(mi_ctx* ctx, const uint8_t* nv12_in, uint8_t* nv12_out, int width, int height);
mi_status mi_nv12_bgr_equalize_batch_dev(mi_ctx* ctx, const void* d_in, size_t in_frame_stride,
                                         void* d_out, size_t out_frame_stride,
                                         int width, int height, int n_frames, void* stream);

/* cv::cvtColor's 4:2:0 codes on their own (same arithmetic as the pipeline above; parity unpinned):
 *   MI_COLOR_BGR2YUV_I420 (cv::COLOR_BGR2YUV_I420 = 128; 1frameMeasure.cpp:32 prepares its bench input with it):
 *     src CV_8UC3 W x H (pitch >= 3W) -> dst CV_8UC1 W x H*3/2 (pitch >= W): Y rows, then the U and the V plane packed
 *     the way OpenCV packs them (as if the W x H*3/2 matrix were tight, then laid out with dst_step);
 *   MI_COLOR_YUV2BGR_NV12 (cv::COLOR_YUV2BGR_NV12 = 93): src CV_8UC1 W x H*3/2 NV12 -> dst CV_8UC3 W x H.
 * width/height are the picture's (even).  The device form wants the planar side tight (step == width). */
enum { MI_COLOR_YUV2BGR_NV12 = 93, MI_COLOR_BGR2YUV_I420 = 128 };
mi_status mi_cvt_color_420_u8(mi_ctx* ctx, const uint8_t* src, size_t src_step, uint8_t* dst, size_t dst_step,
                              int width, int height, int code);
mi_status mi_cvt_color_420_u8_batch_dev(mi_ctx* ctx, const void* d_src, size_t src_step, size_t src_frame_stride,
                                        void* d_dst, size_t dst_step, size_t dst_frame_stride,
                                        int width, int height, int n_frames, int code, void* stream);

/* ---- stream completion, fail-soft behaviour of the fused kernel, statistics -------------------------------
 * The batched equalizeHist forms normally run as ONE fused launch whose workgroups hand data to each
 * other through bounded waits (they need a frame's slices co-resident on the GPU).  If such a wait
 * expires -- another tenant holds the compute units, a queue was preempted for longer than the bound --
 * the launch drains, and the small finish kernel that follows EVERY fused launch on the same stream
 * redoes exactly the parts that were not written, with no inter-workgroup dependency.  The caller's
 * stream therefore always carries correct output, whoever synchronises it and however; the event is
 * only counted: mi_ctx_get_stat("fused_fallbacks" | "fused_frames_repaired" | "fused_hard_errors" |
 * "fused_last_status").  (The reference's accelerator path ignores device errors altogether:
 * OpenCLequalHist.cpp:367 catches a type nobody throws.)
 * mi_ctx_synchronize() waits for `stream`; it returns MI_ERR_HIP only if a frame's state contradicted the
 * protocol and the repair refused to guess ("fused_hard_errors"; the host-pointer forms check the same).
 * hipGraph: a batched call issued inside a stream capture is recorded as it is -- all per-launch state of
 * the fused path lives in device memory -- and the graph can be replayed.  Size the scratch with one
 * eager call of the same shape first: scratch growth inside a capture returns MI_ERR_UNSUPPORTED, and
 * once a context has seen a capture it never frees scratch a graph node may reference.
 * A context that keeps being repaired gives the fused path up for a while ("demotion"): `fused_demote_after` repaired launches
 * within 32 fused launches route the following calls through the three-kernel path (no inter-workgroup dependency, nothing to
 * stall) for `fused_reprobe_ms`; then one fused launch probes again, and a repair during the probe doubles the period (up to
 * 64x).  mi_ctx_get_stat("fused_demotions" | "fused_demoted").  The bytes are the same on either path.
 * Options that change BEHAVIOUR (mi_ctx_set_option; the speed-only ones are in mi_lumaeq_tuning.h):
 *   "fused"              1/0, default 1: single-read fused kernel vs the three-kernel path for the batched equalizeHist forms
 *   "fused_timeout_ms"   bound of every inter-workgroup wait of the fused kernel, default 50
 *   "fused_demote_after" 0..32, default 3: repaired launches per window that demote the fused path (0 = never demote)
 *   "fused_reprobe_ms"   first demotion period in milliseconds, default 1000
 *   "clahe_fp_contract"  1/0, default 0: CLAHE interpolation arithmetic.  0 = every multiply and add rounded separately, what an
 *                        x86-64 baseline build of OpenCV computes; 1 = the fused multiply-adds GCC forms from clahe.cpp's
 *                        expressions on FMA targets under its default -ffp-contract=fast, i.e. OpenCV on aarch64 -- the
 *                        reference's own board: txf = fma(x, 1/tw, -0.5), res = fma(fma(l11, xa1, l12*xa), ya1,
 *                        fma(l21, xa1, l22*xa) * ya).  The two differ by 1 in about 0.03 % of the pixels.
 * Other statistics (mi_ctx_get_stat): "error_drains" (error returns that had to wait for a stream first),
 * "host_copies_shared" (staging copies of the host forms the context's helper thread took half of), "host_planes_staged" /
 * "host_planes_direct" (host planes -- inputs and outputs of the host forms and of pipe frames -- packed through the library's
 * pinned staging / DMA'd as the caller pinned them: the library never gives the runtime memory it did not find pinned),
 * "clahe16_mid_launches" (mi_clahe_u16* calls that launched the 16384-entry interpolation kernel for 14-bit content; see
 * MI_OPT_CLAHE16_WIDE in mi_lumaeq_tuning.h), "nv12_bgr_onepass" / "nv12_bgr_twopass" (mi_*_nv12_to_bgr* calls that mapped and converted
 * in one kernel / that took the planar CLAHE + conversion fallback). */
mi_status mi_ctx_synchronize(mi_ctx* ctx, void* stream);
mi_status mi_ctx_set_option(mi_ctx* ctx, const char* name, int value);
mi_status mi_ctx_get_stat(mi_ctx* ctx, const char* name, uint64_t* out);

/* ---- timing of the library's own kernels -------------------------------------------------------
 * With profiling on, every kernel the library launches carries a start and a stop hipEvent stamped by
 * its own dispatch on the stream it is launched on (hipExtLaunchKernelGGL; the reference reads its kernel's
 * CL_PROFILING_COMMAND_START/END the same way, 1frameMeasure.cpp:77-85).  mi_ctx_profile_read() synchronises those events and accumulates. */
enum { MI_K_HIST = 0, MI_K_EQ_LUT = 1, MI_K_LUT_APPLY = 2, MI_K_TILE_HIST = 3, MI_K_TILE_LUT = 4,
       MI_K_CLAHE_INTERP = 5, MI_K_FUSED = 6, MI_K_COLOR = 7, MI_K_FUSED_FINISH = 8, MI_K_DIFF = 9, MI_K_COUNT = 10 };
typedef struct mi_profile {
    double   total_ms[MI_K_COUNT];   /* summed kernel durations since the last reset */
    uint64_t launches[MI_K_COUNT];
    double   min_ms[MI_K_COUNT], p10_ms[MI_K_COUNT], p50_ms[MI_K_COUNT], p90_ms[MI_K_COUNT], max_ms[MI_K_COUNT];
                                     /* distribution of the per-launch durations since the last reset (over at most the
                                      * 65 536 most recent launches of each kernel; 0 when there were none) */
} mi_profile;
mi_status   mi_ctx_set_profiling(mi_ctx* ctx, int enabled);   /* 0 off; 1 every kernel (what bench.py's timed region uses: its line
                                                                * lists the finish launches too); 2 every kernel except the
                                                                * few-microsecond housekeeping launch behind each fused kernel (two
                                                                * events fewer per batch) */
mi_status   mi_ctx_profile_read(mi_ctx* ctx, mi_profile* out, int reset);
const char* mi_kernel_name(int k);

#ifdef __cplusplus
}
#endif
#endif /* MI_LUMAEQ_H_ */
