// lumaeq_kernels.hip.h -- hand-written gfx950 (CDNA4, wave64) kernels for the luma-equalization path.
//
// What they compute is fixed by OpenCV 4.4's cv::equalizeHist / CLAHE::apply as the reference calls
// them (OpenCVequalHist.cpp:145, clahevideo.cpp:195); how they compute it is MI355X-first:
//   * everything is byte/LUT work bound by HBM (no MFMA): 16 B/lane coalesced loads and stores,
//     grid sized to ~8 workgroups/CU, a batch of frames per launch (grid.y / grid.z = frame);
//   * histograms are privatised in LDS as hist[bin][32]: the copy a lane uses is (lane & 31), so
//     its LDS bank is fixed by the lane and a ds_add_u32 wave-instruction is bank-conflict free
//     whatever the pixel values are (a constant frame costs the same as noise);
//   * the equalizeHist LUT is replicated the same way (lut[value][32]) so the per-pixel gather is
//     conflict free as well;
//   * float steps (LUT scale, CLAHE blend) must round every multiply and add separately.  What guarantees
//     it is the BUILD FLAG -ffp-contract=off (csrc/Makefile forces it with `override`): ROCm 7.2's
//     __fmul_rn/__fadd_rn are plain `*` / `+` unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so on their
//     own they contract to v_fma under hipcc's default -ffp-contract=fast (checked in the ISA: 125 FMAs in
//     the interpolation kernel), and that mode also disregards `#pragma clang fp contract(off)`.  They are
//     kept as documentation of intent; a library built without the flag refuses to create a context
//     (contract_probe_kernel, run once per process by mi_ctx_create).
// The staged kernels (K1..K6) never synchronise between workgroups inside a launch: stage results
// cross kernel boundaries only (partials -> LUT -> apply).  The fused equalizeHist kernel (KF) is the
// one exception: its workgroups hand a frame's histogram/LUT to each other through a bounded,
// checksum-verified protocol (kernels/equalize_fused.hip.h).
//
//   kernels/common.hip.h          types, batch descriptors, bank-replicated LDS histogram, scans
//   kernels/equalize.hip.h        K1 hist partials, K2 CDF->LUT, K3 LUT apply (+UV)
//   kernels/equalize_fused.hip.h  KF fused single-read equalizeHist
//   kernels/clahe.hip.h           K4 tile hist, K5 clip/redistribute/LUT, K6 interpolation
//   kernels/clahe16.hip.h         CLAHE on CV_16UC1 (N4)
//   kernels/color.hip.h           cvtColor BGR2YUV / YUV2BGR + fused split/merge, 4:2:0 codes, NV12 per-channel equalize (N3)
//   kernels/color_clahe.hip.h     CLAHE on the luma of interleaved BGR in two passes (N3)
//   kernels/diff.hip.h            absdiff + analyzeDiff: the reference's own device-vs-CPU check (1frameMeasure.cpp:91-100)
//   kernels/p010.hip.h            chroma half of 16-bit 4:2:0 frames (P010 / P012 / P016): copy or fill 0x8000
//   kernels/packed422.hip.h       the pixel-touching stages on packed 4:2:2 frames (YUY2 / UYVY): luma at a 2-byte sample stride
//   kernels/packed422_nv12.hip.h  the pixel-writing stages of packed 4:2:2 in, NV12 out: Y plane + vertically halved chroma in one pass
//   kernels/packed422_yuv420.hip.h the pixel-writing stages of packed 4:2:2 in, planar 4:2:0 (I420 / YV12) out: that walk, the halved chroma
//                                  de-interleaved in registers and stored into a U and a V plane
//   kernels/nv12_bgr.hip.h         the pixel-writing stages of NV12 in, interleaved BGR / RGB out: LUT apply + decode, CLAHE blend + decode
//   kernels/bgr_nv12.hip.h         stage 1 of interleaved BGR / RGB in, NV12 out: convert into pitched planes and count the luma written
//   kernels/bgr_yuv420.hip.h       that stage with planar 4:2:0 (I420 / YV12) out: the chroma stored into a U and a V plane
//   kernels/bgr_packed422.hip.h    that stage with packed 4:2:2 (YUY2 / UYVY) out: every row with its own chroma, one dword per macropixel
//   kernels/yuv420_packed422.hip.h the pixel-writing stages of 4:2:0 (NV12 / I420 / YV12) in, packed 4:2:2 (YUY2 / UYVY) out: LUT apply / CLAHE
//                                  blend + pack, a byte zip of the mapped luma with the chroma row both output rows share
//   kernels/yuv420.hip.h           the chroma of 4:2:0 frames between planar (I420 / YV12) and interleaved (NV12) layouts: copy, relayout or fill,
//                                  on a batch at a frame stride or on a list of per-frame plane addresses
//   kernels/yuv420_bgr.hip.h       the pixel-writing stages of planar 4:2:0 (I420 / YV12) in, interleaved BGR / RGB out: those of nv12_bgr.hip.h
//                                  with the chroma loaded from two planes and zipped in registers; their *_frames_kernel entries on a
//                                  list of {y, u, v, out} addresses
//   kernels/packed422_bgr.hip.h    the pixel-writing stages of packed 4:2:2 in, interleaved BGR / RGB out: LUT apply / CLAHE blend + decode,
//                                  every row with its own chroma; the LUT-apply and the interpolation body are templates on the block
//                                  type and a store policy (Store422Bgr: 3 B/px), written once for every image form
//   kernels/bgra_yuv420.hip.h      stage 1 of four-channel BGRA / RGBA (CV_8UC4) in, 4:2:0 out: one body for NV12 and planar chroma, for a
//                                  strided batch and a list of {in, y, c0, c1} addresses; the fourth byte takes part in nothing
//   kernels/yuv420_bgra.hip.h      the pixel-writing stages of 4:2:0 in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out: LUT apply / CLAHE
//                                  blend + decode, one body each for NV12 and planar chroma, for a strided batch and a list of
//                                  {y, c0, c1, out} addresses; every pixel one dword, a 16-pixel group four 16-byte stores
//   kernels/packed422_bgra.hip.h   the pixel-writing stages of packed 4:2:2 in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out: its block, its
//                                  store policy (Store422Bgra: that dword-per-pixel store) and the entries that wrap the bodies of
//                                  packed422_bgr.hip.h with them; the wide-grid fallback body is written out
//   kernels/bgra_packed422.hip.h   stage 1 of four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 (YUY2 / UYVY) out: one body for a strided
//                                  batch and a list of {in, out} addresses; 16 pixel dwords in, eight macropixel dwords out per lane
#pragma once
#include "kernels/common.hip.h"
#include "kernels/equalize.hip.h"
#include "kernels/equalize_fused.hip.h"
#include "kernels/clahe.hip.h"
#include "kernels/clahe16.hip.h"
#include "kernels/color.hip.h"
#include "kernels/color_clahe.hip.h"
#include "kernels/diff.hip.h"
#include "kernels/p010.hip.h"
#include "kernels/packed422.hip.h"
#include "kernels/packed422_nv12.hip.h"
#include "kernels/packed422_yuv420.hip.h"
#include "kernels/nv12_bgr.hip.h"
#include "kernels/bgr_nv12.hip.h"
#include "kernels/bgr_yuv420.hip.h"
#include "kernels/bgr_packed422.hip.h"
#include "kernels/yuv420_packed422.hip.h"
#include "kernels/yuv420.hip.h"
#include "kernels/yuv420_bgr.hip.h"
#include "kernels/packed422_bgr.hip.h"
#include "kernels/bgra_yuv420.hip.h"
#include "kernels/yuv420_bgra.hip.h"
#include "kernels/packed422_bgra.hip.h"
#include "kernels/bgra_packed422.hip.h"
