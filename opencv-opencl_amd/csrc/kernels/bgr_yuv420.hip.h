// bgr_yuv420.hip.h -- interleaved 8-bit BGR / RGB images in, pitched planar 4:2:0 frames (I420 / YV12) out, counting the luma the conversion produces
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"
#include "color.hip.h"

namespace mi {
// =============================================================================================
// cv::cvtColor(COLOR_BGR2YUV_I420) (or the RGB order) into three pitched planes, then cv::equalizeHist / CLAHE::apply on Y: stage 1 of
// bgr_nv12.hip.h with the chroma going to a U and a V plane instead of one interleaved plane -- what a software encoder takes
// (data[0..2] / linesize[0..2]).  Stage 2 is the same: the planar kernels map the luma IN PLACE in the output Y plane.
// Bytes per pixel as there: equalizeHist 3 read + 1.5 written here, then 1 + 1 by the in-place map: 6.5; CLAHE 4.5 here, then 3: 7.5.
// The body is written out next to bgr_to_nv12_hist_body, not shared with it through a chroma-store policy, as yuv420_bgr.hip.h is
// written out next to nv12_bgr.hip.h: the NV12-out kernels keep their text and their ISA.  What differs is only where the chroma goes.
// The arithmetic is color.hip.h's encode (bt601_y, bt601_uv: cvt420_kernel<0>): chroma from the top-left pixel of each 2 x 2 block.
// ORDER 0: B, G, R in memory (MI_ORDER_BGR); 1: R, G, B (MI_ORDER_RGB).  UVMODE 0: every chroma byte 128 (MI_UV_FILL128, the chroma
// arithmetic is skipped); 1: U, V of the conversion (MI_UV_COPY).
// =============================================================================================
struct BgrYuv420Job {
    const uint8_t* in;                        // H rows of 3*W bytes
    uint8_t* y; uint8_t* u; uint8_t* v;       // Y plane: H rows of W bytes; U and V planes: H/2 rows of W/2 bytes each
    long long in_step, y_step, c_step;        // bytes between rows (the two chroma planes share theirs)
    long long in_frame, out_frame;            // bytes between frames (the three output planes share theirs)
    int width, height;                        // both even
    int vec;                                  // 1: W % 16 == 0, in / y terms multiples of 16, chroma terms of 8 -> 16 x 2 pixel groups
};

// ---------------------------------------------------------------------------------------------
// Stage 1.  grid = (B, n_frames), 256 threads.  With HIST: partial[(f * B + part) * 256 + bin], the layout of hist_partial_kernel,
// which equalize_lut_kernel reads.
// vec: a lane owns a 16 x 2 pixel group -- two load_bgr16 (six 16-byte loads), two 16-byte Y stores, one 8-byte store of 8 U bytes
// and one of 8 V bytes (hence the modulus 8 of the chroma terms, the mirror of yuv420_to_bgr_kernel's loads) -- on the carried
// (by, gx) walk of bgr_to_nv12_hist_body (no 64-bit division per group); otherwise a 2 x 2 block with byte accesses.  Only the W bytes
// of each Y row and the W/2 bytes of each U and V row are written.
// Workgroup size and histogram copies: 256 threads and hist[bin][32], as there.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgr_to_yuv420_hist_kernel(BgrYuv420Job j, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t h[HIST ? 256 * kCopies : 1];
    const int t = threadIdx.x, f = blockIdx.y;
    if (HIST) {
        for (int i = t; i < 256 * kCopies; i += kThreads) h[i] = 0;
        __syncthreads();
    }
    const uint32_t copy = t & (kCopies - 1);
    const uint8_t* ip = j.in + (long long)f * j.in_frame;
    uint8_t* yp = j.y + (long long)f * j.out_frame;
    uint8_t* up = j.u + (long long)f * j.out_frame;
    uint8_t* vp = j.v + (long long)f * j.out_frame;
    constexpr uint32_t kFill = 0x80808080u;
    if (j.vec) {
        const int gx_n = j.width >> 4;
        const int groups = gx_n * (j.height >> 1);            // < 2^26 (W*H < 2^31)
        const int stride = (int)gridDim.x * kThreads, dby = stride / gx_n, dgx = stride - dby * gx_n;
        int gi = (int)blockIdx.x * kThreads + t;
        int by = gi / gx_n, gx = gi - by * gx_n;
        for (; gi < groups; gi += stride, by += dby, gx += dgx) {
            if (gx >= gx_n) { gx -= gx_n; ++by; }
            const uint8_t* r0 = ip + (long long)(2 * by) * j.in_step + 48 * gx;
            uint32_t a0[16], g0[16], c0[16], a1[16], g1[16], c1[16];       // a: first channel in memory, c: third
            load_bgr16(r0, a0, g0, c0);
            load_bgr16(r0 + j.in_step, a1, g1, c1);
            const uint32_t* b0 = ORDER == 0 ? a0 : c0; const uint32_t* q0 = ORDER == 0 ? c0 : a0;
            const uint32_t* b1 = ORDER == 0 ? a1 : c1; const uint32_t* q1 = ORDER == 0 ? c1 : a1;
            uint32_t y0[4] = {0, 0, 0, 0}, y1[4] = {0, 0, 0, 0}, wu[2] = {kFill, kFill}, wv[2] = {kFill, kFill};
            if (UVMODE) { wu[0] = wu[1] = wv[0] = wv[1] = 0; }
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                const uint32_t Y0 = bt601_y(b0[px], g0[px], q0[px]), Y1 = bt601_y(b1[px], g1[px], q1[px]);
                y0[px >> 2] |= Y0 << (8 * (px & 3));
                y1[px >> 2] |= Y1 << (8 * (px & 3));
                if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
                if (UVMODE && (px & 1) == 0) {                   // chroma from the top-left pixel of each 2 x 2 block
                    uint32_t U, V;
                    bt601_uv(b0[px], g0[px], q0[px], U, V);
                    wu[px >> 3] |= U << (8 * ((px >> 1) & 3));
                    wv[px >> 3] |= V << (8 * ((px >> 1) & 3));
                }
            }
            const u32x4 o0 = {y0[0], y0[1], y0[2], y0[3]}, o1 = {y1[0], y1[1], y1[2], y1[3]};
            uint8_t* d0 = yp + (long long)(2 * by) * j.y_step + (gx << 4);
            *reinterpret_cast<u32x4*>(d0) = o0;
            *reinterpret_cast<u32x4*>(d0 + j.y_step) = o1;
            const long long co = (long long)by * j.c_step + (gx << 3);
            *reinterpret_cast<uint2*>(up + co) = make_uint2(wu[0], wu[1]);
            *reinterpret_cast<uint2*>(vp + co) = make_uint2(wv[0], wv[1]);
        }
    } else {                                            // one 2 x 2 block per lane
        const int bx_n = j.width >> 1;
        const long long blocks = (long long)bx_n * (j.height >> 1);
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        for (long long bi = (long long)blockIdx.x * kThreads + t; bi < blocks; bi += (long long)gridDim.x * kThreads) {
            const int by = (int)(bi / bx_n), bx = (int)(bi - (long long)by * bx_n);
            const uint8_t* r0 = ip + (long long)(2 * by) * j.in_step + 6 * bx;
            const uint8_t* r1 = r0 + j.in_step;
            uint8_t* d0 = yp + (long long)(2 * by) * j.y_step + 2 * bx;
            uint8_t* d1 = d0 + j.y_step;
            const long long co = (long long)by * j.c_step + bx;
            const uint32_t b00 = r0[B], g00 = r0[1], q00 = r0[R];
            const uint32_t Y00 = bt601_y(b00, g00, q00), Y01 = bt601_y(r0[3 + B], r0[4], r0[3 + R]);
            const uint32_t Y10 = bt601_y(r1[B], r1[1], r1[R]), Y11 = bt601_y(r1[3 + B], r1[4], r1[3 + R]);
            uint32_t U = 128, V = 128;
            if (UVMODE) bt601_uv(b00, g00, q00, U, V);
            d0[0] = (uint8_t)Y00; d0[1] = (uint8_t)Y01; d1[0] = (uint8_t)Y10; d1[1] = (uint8_t)Y11;
            up[co] = (uint8_t)U; vp[co] = (uint8_t)V;
            if (HIST) {
                lds_inc(h, (Y00 << kCopyShift) + copy); lds_inc(h, (Y01 << kCopyShift) + copy);
                lds_inc(h, (Y10 << kCopyShift) + copy); lds_inc(h, (Y11 << kCopyShift) + copy);
            }
        }
    }
    if (HIST) {
        __syncthreads();
        partial[((size_t)f * gridDim.x + blockIdx.x) * 256 + t] = lds_hist_bin(h, t);      // kThreads == 256 bins
    }
}
static_assert(kThreads == 256, "bgr_to_yuv420_hist_kernel writes one bin per thread");

}  // namespace mi
