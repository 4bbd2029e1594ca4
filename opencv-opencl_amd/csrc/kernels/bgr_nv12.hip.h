// bgr_nv12.hip.h -- interleaved 8-bit BGR / RGB images in, pitched NV12 frames out, counting the luma the conversion produces
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"
#include "color.hip.h"

namespace mi {
// =============================================================================================
// cv::cvtColor(COLOR_BGR2YUV_I420) (or the RGB order) with U and V interleaved into an NV12 chroma plane, then cv::equalizeHist /
// CLAHE::apply on Y: the encoder-side mirror of nv12_bgr.hip.h.  Y is not in the input -- it exists only after the conversion -- so
// the conversion is stage 1 and counts the luma bytes it has just produced; stage 2 maps the luma IN PLACE in the output Y plane with
// the planar kernels unchanged (equalize_lut_kernel + lut_apply_kernel; the planar CLAHE with src == dst).
// Bytes per pixel: equalizeHist 3 read + 1.5 written here, then 1 read + 1 written by the in-place map: 6.5.  CLAHE: 4.5 here (no
// histogram), then the tile histograms read Y and the interpolation reads and writes it: 7.5.  (A histogram pass over BGR followed by
// a map-and-convert pass over BGR, as nv12_bgr.hip.h mirrors it, moves 3 + 3 + 1.5 = 7.5 for both and needs a kernel more per op.)
// The arithmetic is color.hip.h's encode (bt601_y, bt601_uv: cvt420_kernel<0>): chroma from the top-left pixel of each 2 x 2 block.
// ORDER 0: B, G, R in memory (MI_ORDER_BGR); 1: R, G, B (MI_ORDER_RGB).  UVMODE 0: every chroma byte 128 (MI_UV_FILL128, the chroma
// arithmetic is skipped); 1: U, V of the conversion (MI_UV_COPY).
// =============================================================================================
struct BgrNv12Job {
    const uint8_t* in;                        // H rows of 3*W bytes
    uint8_t* y; uint8_t* uv;                  // Y plane: H rows of W bytes; UV plane: H/2 rows of W bytes (interleaved U, V)
    long long in_step, y_step, uv_step;       // bytes between rows
    long long in_frame, out_frame;            // bytes between frames (the two output planes share theirs)
    int width, height;                        // both even
    int vec;                                  // 1: W % 16 == 0 and every base / pitch / frame stride a multiple of 16 -> 16 x 2 pixel groups
};

// Where frame f of a launch lives, as StridedNv12Bgr / TableNv12Bgr (nv12_bgr.hip.h) say it for the opposite direction: the body below
// is a template on one of these two policies.  The batch entry wraps it with the strided one -- the arithmetic it always had, on the
// kernel's own argument -- the *_frames_kernel entry with the table.
struct StridedBgrNv12 {
    const BgrNv12Job& j;
    __device__ __forceinline__ const uint8_t* in_of(long long f) const { return j.in + f * j.in_frame; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return j.y + f * j.out_frame; }
    __device__ __forceinline__ uint8_t* uv_of(long long f) const { return j.uv + f * j.out_frame; }
    __device__ __forceinline__ bool vec(long long) const { return j.vec; }              // decided by the host for the whole launch
};

// A list of such frames, each at its own three addresses (mi_*_bgr_to_nv12_frames_dev: a pool of images in, an encoder's surface pool
// out).  The {in, y, uv} entries travel BY VALUE in the kernel arguments like FrameList -- 64 x 24 B = 1.5 KiB -- and are read with
// scalar kernarg loads indexed by the frame's grid coordinate.  The shape (pitches, width, height) is the launch's BgrNv12Job, whose
// in / y / uv / *_frame a table launch ignores and whose vec says what the SHAPE allows (W % 16 == 0, the three pitches multiples of
// 16): whether frame f takes the 16 x 2 groups is then decided by its own three addresses -- per frame, so uniform for a workgroup.
struct BgrNv12Frame { const uint8_t* in; uint8_t* y; uint8_t* uv; };
struct BgrNv12List { BgrNv12Frame f[kFramesPerLaunch]; };
static_assert(sizeof(BgrNv12Frame) == 24, "three addresses an entry");
struct TableBgrNv12 {
    const BgrNv12List& l;
    const BgrNv12Job& j;
    __device__ __forceinline__ const uint8_t* in_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return l.f[f].y; }
    __device__ __forceinline__ uint8_t* uv_of(long long f) const { return l.f[f].uv; }
    __device__ __forceinline__ bool vec(long long f) const
    {
        return j.vec && (((uintptr_t)l.f[f].in | (uintptr_t)l.f[f].y | (uintptr_t)l.f[f].uv) & 15) == 0;
    }
};

// ---------------------------------------------------------------------------------------------
// Stage 1.  grid = (B, n_frames), 256 threads.  With HIST: partial[(f * B + part) * 256 + bin], the layout of hist_partial_kernel,
// which equalize_lut_kernel reads.
// vec: a lane owns a 16 x 2 pixel group -- two load_bgr16 (six 16-byte loads), two 16-byte Y stores, one 16-byte store of 8 U,V pairs
// -- on the carried (by, gx) walk of cvt420_kernel (no 64-bit division per group); otherwise a 2 x 2 block with byte accesses.  Only
// the W bytes of each output row are written.
// Workgroup size and histogram copies: 256 threads and hist[bin][32] as in hist_partial_kernel.  32 copies = the number of LDS banks,
// so a lane's bank is fixed by the lane and a constant-colour frame counts as fast as noise.  A lane of the vector path holds two
// rows of 16 pixels unpacked next to the words it packs: about 80 VGPRs, which allow 6 waves per SIMD; five 256-thread workgroups
// fit the 160 KiB of LDS of a CU, which gives 5.  512-thread workgroups (bgr_luma_hist_kernel's choice) would reach the sixth wave and
// halve the tables zeroed and folded; that has not been measured here, and 256 threads keep the grid rule, the byte basis (4.5 B/px
// moved) and the loop shapes of nv12_to_bgr_kernel and cvt420_kernel, so one derivation of the loop bounds serves all three.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int UVMODE, bool HIST, class Frames>
__device__ __forceinline__ void bgr_to_nv12_hist_body(const BgrNv12Job& j, const Frames& fr, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t h[HIST ? 256 * kCopies : 1];
    const int t = threadIdx.x, f = blockIdx.y;
    if (HIST) {
        for (int i = t; i < 256 * kCopies; i += kThreads) h[i] = 0;
        __syncthreads();
    }
    const uint32_t copy = t & (kCopies - 1);
    const uint8_t* ip = fr.in_of(f);
    uint8_t* yp = fr.y_of(f);
    uint8_t* uvp = fr.uv_of(f);
    constexpr uint32_t kFill = 0x80808080u;
    if (fr.vec(f)) {
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
            uint32_t y0[4] = {0, 0, 0, 0}, y1[4] = {0, 0, 0, 0}, wuv[4] = {kFill, kFill, kFill, kFill};
            if (UVMODE) { wuv[0] = wuv[1] = wuv[2] = wuv[3] = 0; }
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                const uint32_t Y0 = bt601_y(b0[px], g0[px], q0[px]), Y1 = bt601_y(b1[px], g1[px], q1[px]);
                y0[px >> 2] |= Y0 << (8 * (px & 3));
                y1[px >> 2] |= Y1 << (8 * (px & 3));
                if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
                if (UVMODE && (px & 1) == 0) {                   // chroma from the top-left pixel of each 2 x 2 block
                    uint32_t U, V;
                    bt601_uv(b0[px], g0[px], q0[px], U, V);
                    wuv[px >> 2] |= (U | (V << 8)) << (8 * (px & 2));
                }
            }
            const u32x4 o0 = {y0[0], y0[1], y0[2], y0[3]}, o1 = {y1[0], y1[1], y1[2], y1[3]}, ouv = {wuv[0], wuv[1], wuv[2], wuv[3]};
            uint8_t* d0 = yp + (long long)(2 * by) * j.y_step + (gx << 4);
            *reinterpret_cast<u32x4*>(d0) = o0;
            *reinterpret_cast<u32x4*>(d0 + j.y_step) = o1;
            *reinterpret_cast<u32x4*>(uvp + (long long)by * j.uv_step + (gx << 4)) = ouv;
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
            uint8_t* duv = uvp + (long long)by * j.uv_step + 2 * bx;
            const uint32_t b00 = r0[B], g00 = r0[1], q00 = r0[R];
            const uint32_t Y00 = bt601_y(b00, g00, q00), Y01 = bt601_y(r0[3 + B], r0[4], r0[3 + R]);
            const uint32_t Y10 = bt601_y(r1[B], r1[1], r1[R]), Y11 = bt601_y(r1[3 + B], r1[4], r1[3 + R]);
            uint32_t U = 128, V = 128;
            if (UVMODE) bt601_uv(b00, g00, q00, U, V);
            d0[0] = (uint8_t)Y00; d0[1] = (uint8_t)Y01; d1[0] = (uint8_t)Y10; d1[1] = (uint8_t)Y11;
            duv[0] = (uint8_t)U; duv[1] = (uint8_t)V;
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
template <int ORDER, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgr_to_nv12_hist_kernel(BgrNv12Job j, uint32_t* __restrict__ partial)
{
    bgr_to_nv12_hist_body<ORDER, UVMODE, HIST>(j, StridedBgrNv12{j}, partial);
}
// the same on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either kind; the
// partials are those of the chunk's frames in list order
template <int ORDER, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgr_to_nv12_hist_frames_kernel(BgrNv12Job j, BgrNv12List l, uint32_t* __restrict__ partial)
{
    bgr_to_nv12_hist_body<ORDER, UVMODE, HIST>(j, TableBgrNv12{l, j}, partial);
}
static_assert(kThreads == 256, "bgr_to_nv12_hist_body writes one bin per thread");
// 256: the implicit arguments a code object carries behind the explicit ones
static_assert(sizeof(BgrNv12Job) + sizeof(BgrNv12List) + sizeof(uint32_t*) + 256 <= 4096,
              "the table and the remaining arguments of bgr_to_nv12_hist_frames_kernel stay below HIP's 4 KiB of kernel arguments");

}  // namespace mi
