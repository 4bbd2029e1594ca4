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

// =============================================================================================
// The same on a list of frames, each at its own four addresses (mi_*_bgr_to_yuv420_frames_dev: a pool of images in, a software
// encoder's frame pool out, every frame three separately allocated planes).  The {in, y, u, v} entries travel BY VALUE in the kernel
// arguments like BgrNv12List (bgr_nv12.hip.h) -- 64 x 32 B = 2 KiB -- and are read with scalar kernarg loads indexed by the frame's
// grid coordinate.  The shape (pitches, width, height) is the launch's BgrYuv420Job, whose in / y / u / v / *_frame a table launch
// ignores and whose vec says what the SHAPE allows (W % 16 == 0, the image and Y pitches multiples of 16, the chroma pitch of 8):
// whether frame f takes the 16 x 2 groups is then decided by its own four addresses -- per frame, so uniform for a workgroup.
// The kernel is a COPY of the one above with the frame's addresses read from the table, as yuv420_bgr.hip.h has its list kernels: a
// change there is made here too.  The other form in the tree -- one body as a template on a frame-address policy, StridedBgrNv12 /
// TableBgrNv12 in bgr_nv12.hip.h -- was tried first and changed the ISA of all eight bgr_to_yuv420_hist_kernel instantiations (the
// byte extraction of the unpacking came out with other instructions, 679-1087 became 679-1097 instructions), which the batch form
// must not pay for the list form.
// =============================================================================================
struct BgrYuv420Frame { const uint8_t* in; uint8_t* y; uint8_t* u; uint8_t* v; };
struct BgrYuv420List { BgrYuv420Frame f[kFramesPerLaunch]; };
static_assert(sizeof(BgrYuv420Frame) == 32, "four addresses an entry");

// THE rule "does this frame of a list take the 16 x 2 groups": what the shape allows, and the frame's own image and Y addresses
// multiples of 16, its U and V addresses of 8 (the chroma stores are 8-byte stores).  The kernel decides by it and the host counts by it.
__host__ __device__ __forceinline__ bool bgr_yuv420_frame_vec(int shape_vec, const void* in, const void* y, const void* u, const void* v)
{
    return shape_vec && ((((uintptr_t)in | (uintptr_t)y) & 15) | (((uintptr_t)u | (uintptr_t)v) & 7)) == 0;
}

// bgr_to_yuv420_hist_kernel on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either
// walk -- a byte-path frame of a vector-shaped launch takes more steps.  The partials are those of the chunk's frames in list order:
// partial[(f * gridDim.x + blockIdx.x) * 256 + bin].
template <int ORDER, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgr_to_yuv420_hist_frames_kernel(BgrYuv420Job j, BgrYuv420List l, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t h[HIST ? 256 * kCopies : 1];
    const int t = threadIdx.x, f = blockIdx.y;
    if (HIST) {
        for (int i = t; i < 256 * kCopies; i += kThreads) h[i] = 0;
        __syncthreads();
    }
    const uint32_t copy = t & (kCopies - 1);
    const uint8_t* ip = l.f[f].in;
    uint8_t* yp = l.f[f].y;
    uint8_t* up = l.f[f].u;
    uint8_t* vp = l.f[f].v;
    constexpr uint32_t kFill = 0x80808080u;
    if (bgr_yuv420_frame_vec(j.vec, ip, yp, up, vp)) {
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
// 256: the implicit arguments a code object carries behind the explicit ones
static_assert(sizeof(BgrYuv420List) == (size_t)kFramesPerLaunch * 32 && sizeof(BgrYuv420List) <= 2048, "the table is at most 2 KiB");
static_assert(sizeof(BgrYuv420Job) + sizeof(BgrYuv420List) + sizeof(uint32_t*) + 256 <= 4096,
              "the table and the remaining arguments of bgr_to_yuv420_hist_frames_kernel stay below HIP's 4 KiB of kernel arguments");

}  // namespace mi
