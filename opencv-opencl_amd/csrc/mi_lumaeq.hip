// mi_lumaeq.hip -- C ABI (include/mi_lumaeq.h) over the gfx950 kernels in lumaeq_kernels.hip.h.
//
// Boundary being replaced (reference file:line):
//   cv::equalizeHist call site            OpenCVequalHist.cpp:145, nextimprovement.cpp:168
//   cv::CLAHE::apply call site            clahevideo.cpp:195, clahe1frame.cpp:93
//   FPGA backend host sequence            OpenCLequalHist.cpp:346-365 (setArg x5, write x2, task, read)
//   per-worker device objects + buffers   OpenCLequalHist.cpp:142-152, :175-186
// There is NO CPU fallback in this file: without a HIP device every entry point fails loudly.
#include "../../include/mi_lumaeq.h"
#include "lumaeq_kernels.hip.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "host/drain_guard.hpp"           // stand-alone helpers (CPU-testable: tests/cxx/test_host_helpers.cpp)
#include "host/copy_crew.hpp"
#include "host/pending_ranges.hpp"
#include "host/pin_registry.hpp"
#include "host/numa_affinity.hpp"
#include "host/wide_hint.hpp"
#include "host/p010_chroma.hpp"

using namespace mi;

// The host side lives in host/*.inc.hpp, included in dependency order (ONE translation unit on purpose: the
// kernels are templates/inline device code and the anonymous-namespace helpers are shared).
#include "host/context.inc.hpp"          // opens the anonymous namespace of the launch helpers
#include "host/equalize_fused.inc.hpp"
#include "host/clahe.inc.hpp"
#include "host/host_forms.inc.hpp"       // closes it
#include "host/capi.inc.hpp"
#include "host/color.inc.hpp"
#include "host/clahe16.inc.hpp"
#include "host/p010.inc.hpp"            // 16-bit 4:2:0 frames: CLAHE on Y (clahe16) + the chroma kernel
#include "host/nv12_frames.inc.hpp"     // NV12 frames as a list of pitched plane addresses (decoder surfaces, tensor lists)
#include "host/p010_frames.inc.hpp"     // P010 frames as such a list (the 16-bit kernels' *_frames_kernel entries)
#include "host/packed422.inc.hpp"      // packed 4:2:2 frames (YUY2 / UYVY): luma at a 2-byte sample stride, in place in the frame
#include "host/packed422_frames.inc.hpp"   // packed 4:2:2 frames as a list of pitched buffers (a capture device's buffer pool)
#include "host/packed422_nv12.inc.hpp"     // packed 4:2:2 frames in, NV12 frames out (capture card -> encoder in one pass)
#include "host/packed422_nv12_frames.inc.hpp"   // ... as lists of pitched device frames (buffer pool in, surface pool out) and as one host frame
#include "host/packed422_yuv420.inc.hpp"   // packed 4:2:2 frames in, planar 4:2:0 (I420 / YV12) or NV12 out (capture card -> software encoder in one pass)
#include "host/packed422_yuv420_frames.inc.hpp"   // ... as lists of pitched device frames (buffer pool in, frame pool out) and as one host frame
#include "host/packed422_bgr.inc.hpp"      // packed 4:2:2 frames in, interleaved BGR / RGB out, every row with its own chroma (capture card -> display / writer / model)
#include "host/packed422_bgr_frames.inc.hpp"   // ... as a list of pitched device frames (a capture device's buffer pool in, an image pool out)
#include "host/nv12_bgr.inc.hpp"       // NV12 frames in, interleaved BGR / RGB out in the pass that maps the luma (decoder -> display / writer / model)
#include "host/nv12_bgr_frames.inc.hpp"   // ... as a list of pitched device frames (a decoder's surface pool in, an image pool out)
#include "host/bgr_nv12.inc.hpp"       // interleaved BGR / RGB in, pitched NV12 out: convert and count, then map the luma in place (renderer / model -> encoder)
#include "host/bgr_nv12_frames.inc.hpp"   // ... as a list of pitched device frames (an image pool in, an encoder's surface pool out)
#include "host/yuv420.inc.hpp"         // 4:2:0 frames whose sides say where their planes lie: I420 / YV12 / NV12 in, any of them out
#include "host/yuv420_frames.inc.hpp"  // ... as a list of separately allocated, pitched planes (a decoder's frame pool in, an encoder's surface pool out)
#include "host/yuv420_bgr.inc.hpp"     // planar 4:2:0 (I420 / YV12) or NV12 frames in, interleaved BGR / RGB out in the pass that maps the luma (software decoder -> model)
#include "host/yuv420_bgr_frames.inc.hpp"   // ... as a list of separately allocated, pitched planes (a decoder's frame pool in, an image pool out)
#include "host/bgr_yuv420.inc.hpp"     // interleaved BGR / RGB in, planar 4:2:0 (I420 / YV12) or NV12 out: convert and count, then map the luma in place (renderer / model -> software encoder)
#include "host/bgr_yuv420_frames.inc.hpp"   // ... as a list of pitched device frames (an image pool in, a software encoder's frame pool out)
#include "host/bgr_packed422.inc.hpp"  // interleaved BGR / RGB in, packed 4:2:2 (YUY2 / UYVY) out: convert and count, then map the luma in place in the packed frame (renderer / model -> playout)
#include "host/bgr_packed422_frames.inc.hpp"  // the same on a list of frames, each at its own two addresses (image pool -> playout / v4l2 output buffer pool)
#include "host/yuv420_packed422.inc.hpp"  // NV12 or planar 4:2:0 (I420 / YV12) in, packed 4:2:2 (YUY2 / UYVY) out in the pass that maps the luma (decoder -> playout)
#include "host/yuv420_packed422_frames.inc.hpp"  // the same on a list of frames, each at its own four addresses (decoder surface pool -> playout / v4l2 output buffer pool)
#include "host/bgra_yuv420.inc.hpp"    // four-channel BGRA / RGBA (CV_8UC4) in, planar 4:2:0 (I420 / YV12) or NV12 out: convert and count, then map the luma in place (render target / capture -> encoder)
#include "host/bgra_yuv420_frames.inc.hpp"  // ... as a list of pitched device frames (a surface pool in, an encoder's frame pool out)
#include "host/yuv420_bgra.inc.hpp"    // planar 4:2:0 (I420 / YV12) or NV12 in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out in the pass that maps the luma (decoder -> display surface / texture)
#include "host/yuv420_bgra_frames.inc.hpp"  // ... as a list of pitched device frames (a decoder's frame pool in, a surface pool out)
#include "host/packed422_bgra.inc.hpp"  // packed 4:2:2 (YUY2 / UYVY) in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out, every row with its own chroma (capture card -> display surface / texture)
#include "host/packed422_bgra_frames.inc.hpp"  // ... as a list of pitched device frames (a capture device's buffer pool in, a surface pool out)
#include "host/bgra_packed422.inc.hpp"  // four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 (YUY2 / UYVY) out: convert and count, then map the luma in place in the packed frame (render target / capture -> playout / virtual camera)
#include "host/bgra_packed422_frames.inc.hpp"  // ... as a list of frames, each at its own two addresses (a surface pool in, a playout / v4l2 output buffer pool out)
#include "host/pipe.inc.hpp"
#include "host/diff.inc.hpp"
