// bgra_yuv420.hip.h -- interleaved 8-bit four-channel images (BGRA / BGRX, RGBA / RGBX: CV_8UC4) in, pitched 4:2:0 frames (I420 / YV12
// planes, or NV12) out, counting the luma the conversion produces
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"
#include "color.hip.h"

namespace mi {
// =============================================================================================
// cv::cvtColor(COLOR_BGRA2YUV_I420) (or the RGBA code) into pitched planes, then cv::equalizeHist / CLAHE::apply on Y: stage 1 of
// bgr_nv12.hip.h / bgr_yuv420.hip.h on the four-byte pixels of render targets, capture surfaces and interop buffers.  The fourth byte
// (alpha or padding) is loaded with its pixel and takes part in nothing.  Stage 2 is the same: the planar kernels map the luma IN PLACE
// in the output Y plane.
// Bytes per pixel: equalizeHist 4 read + 1.5 written here, then 1 + 1 by the in-place map: 7.5; CLAHE 5.5 here, then 3: 8.5.
// These are new kernels, so there is ONE body: a template on the chroma layout (CHROMA 0: U, V interleaved into one plane, NV12;
// 1: a U and a V plane) and on a frame-address policy (strided batch / by-value table), the shape of bgr_to_nv12_hist_body.  No
// existing kernel is touched.
// The arithmetic is color.hip.h's encode (bt601_y, bt601_uv: cvt420_kernel<0>): chroma from the top-left pixel of each 2 x 2 block.
// ORDER 0: B, G, R, X in memory (MI_ORDER_BGR); 1: R, G, B, X (MI_ORDER_RGB).  UVMODE 0: every chroma byte 128 (MI_UV_FILL128, the
// chroma arithmetic is skipped); 1: U, V of the conversion (MI_UV_COPY).
// =============================================================================================
struct BgraYuv420Job {
    const uint8_t* in;                        // H rows of 4*W bytes
    uint8_t* y; uint8_t* c0; uint8_t* c1;     // Y plane: H rows of W bytes; planar: c0 = U, c1 = V, H/2 rows of W/2 bytes each;
                                              // interleaved: c0 = the UV plane, H/2 rows of W bytes, c1 unused
    long long in_step, y_step, c_step;        // bytes between rows (two chroma planes share theirs)
    long long in_frame, out_frame;            // bytes between frames (the output planes share theirs)
    int width, height;                        // both even
    int vec;                                  // 1: W % 16 == 0, in / y terms multiples of 16, chroma terms of 16 (interleaved) or 8 (planar)
};

// THE rule "does a frame at these addresses take the 16 x 2 groups": what the shape allows, and the frame's own image and Y addresses
// multiples of 16, its UV address of 16 (one 16-byte store) or its U and V addresses of 8 (two 8-byte stores).  The kernel decides by
// it and the host counts by it.
__host__ __device__ __forceinline__ bool bgra_yuv420_frame_vec(int shape_vec, bool planar, const void* in, const void* y, const void* c0,
                                                               const void* c1)
{
    const uintptr_t chroma = planar ? (((uintptr_t)c0 | (uintptr_t)c1) & 7) : ((uintptr_t)c0 & 15);
    return shape_vec && ((((uintptr_t)in | (uintptr_t)y) & 15) | chroma) == 0;
}

// Where frame f of a launch lives, as StridedBgrNv12 / TableBgrNv12 (bgr_nv12.hip.h) say it: the body below is a template on one of
// these two policies.
struct StridedBgraYuv420 {
    const BgraYuv420Job& j;
    __device__ __forceinline__ const uint8_t* in_of(long long f) const { return j.in + f * j.in_frame; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return j.y + f * j.out_frame; }
    __device__ __forceinline__ uint8_t* c0_of(long long f) const { return j.c0 + f * j.out_frame; }
    __device__ __forceinline__ uint8_t* c1_of(long long f) const { return j.c1 + f * j.out_frame; }
    __device__ __forceinline__ bool vec(bool, long long) const { return j.vec; }          // decided by the host for the whole launch
};

// A list of such frames, each at its own four addresses (mi_*_bgra_to_yuv420_frames_dev: a pool of surfaces in, an encoder's frame pool
// out).  The {in, y, c0, c1} entries travel BY VALUE in the kernel arguments like BgrYuv420List -- 64 x 32 B = 2 KiB -- and are read
// with scalar kernarg loads indexed by the frame's grid coordinate.  The shape (pitches, width, height) is the launch's BgraYuv420Job,
// whose in / y / c0 / c1 / *_frame a table launch ignores and whose vec says what the SHAPE allows: whether frame f takes the 16 x 2
// groups is then decided by its own addresses -- per frame, so uniform for a workgroup.
struct BgraYuv420Frame { const uint8_t* in; uint8_t* y; uint8_t* c0; uint8_t* c1; };
struct BgraYuv420List { BgraYuv420Frame f[kFramesPerLaunch]; };
static_assert(sizeof(BgraYuv420Frame) == 32, "four addresses an entry");
struct TableBgraYuv420 {
    const BgraYuv420List& l;
    const BgraYuv420Job& j;
    __device__ __forceinline__ const uint8_t* in_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return l.f[f].y; }
    __device__ __forceinline__ uint8_t* c0_of(long long f) const { return l.f[f].c0; }
    __device__ __forceinline__ uint8_t* c1_of(long long f) const { return l.f[f].c1; }
    __device__ __forceinline__ bool vec(bool planar, long long f) const
    {
        return bgra_yuv420_frame_vec(j.vec, planar, l.f[f].in, l.f[f].y, l.f[f].c0, l.f[f].c1);
    }
};

// one pixel dword of either order: its blue, green and red bytes (the fourth byte is dropped here)
template <int ORDER>
__device__ __forceinline__ void bgra_px(uint32_t w, uint32_t& b, uint32_t& g, uint32_t& r)
{
    const uint32_t a = w & 0xffu, c = (w >> 16) & 0xffu;       // a: first channel in memory, c: third
    g = (w >> 8) & 0xffu;
    b = ORDER == 0 ? a : c;
    r = ORDER == 0 ? c : a;
}

// ---------------------------------------------------------------------------------------------
// Stage 1.  grid = (B, n_frames), 256 threads.  With HIST: partial[(f * B + part) * 256 + bin], the layout of hist_partial_kernel,
// which equalize_lut_kernel reads.
// vec: a lane owns a 16 x 2 pixel group -- four 16-byte loads a row, all eight issued before the first use; every dword is one pixel,
// so the channels are byte extracts of a dword (none of load_bgr16's unpacking across dwords) -- two 16-byte Y stores and the chroma
// as one 16-byte store of 8 U,V pairs (interleaved) or one 8-byte store of 8 U bytes and one of 8 V bytes (planar), on the carried
// (by, gx) walk of bgr_to_nv12_hist_body (no 64-bit division per group); otherwise a 2 x 2 block with byte accesses at 4*bx + {0,1,2}
// and 4*bx + 4 + {0,1,2}.  Only the W bytes of each Y and interleaved UV row and the W/2 bytes of each planar U and V row are written.
// Plain loads and stores: the Y written here is read again by stage 2 and must stay in the caches; the once-read input has no
// non-temporal policy (not measured).
// Workgroup size and histogram copies: 256 threads and hist[bin][32], as there.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int CHROMA, int UVMODE, bool HIST, class Frames>
__device__ __forceinline__ void bgra_to_yuv420_hist_body(const BgraYuv420Job& j, const Frames& fr, uint32_t* __restrict__ partial)
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
    uint8_t* p0 = fr.c0_of(f);
    uint8_t* p1 = CHROMA ? fr.c1_of(f) : nullptr;
    constexpr uint32_t kFill = 0x80808080u;
    if (fr.vec(CHROMA != 0, f)) {
        const int gx_n = j.width >> 4;
        const int groups = gx_n * (j.height >> 1);            // < 2^26 (W*H < 2^31)
        const int stride = (int)gridDim.x * kThreads, dby = stride / gx_n, dgx = stride - dby * gx_n;
        int gi = (int)blockIdx.x * kThreads + t;
        int by = gi / gx_n, gx = gi - by * gx_n;
        for (; gi < groups; gi += stride, by += dby, gx += dgx) {
            if (gx >= gx_n) { gx -= gx_n; ++by; }
            const u32x4* r0 = reinterpret_cast<const u32x4*>(ip + (long long)(2 * by) * j.in_step + 64 * gx);
            const u32x4* r1 = reinterpret_cast<const u32x4*>(ip + (long long)(2 * by + 1) * j.in_step + 64 * gx);
            const u32x4 q0[4] = {r0[0], r0[1], r0[2], r0[3]}, q1[4] = {r1[0], r1[1], r1[2], r1[3]};      // eight loads in flight
            uint32_t y0[4] = {0, 0, 0, 0}, y1[4] = {0, 0, 0, 0}, wc[4] = {kFill, kFill, kFill, kFill};
            if (UVMODE) { wc[0] = wc[1] = wc[2] = wc[3] = 0; }
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                const u32x4& v0 = q0[px >> 2];
                const u32x4& v1 = q1[px >> 2];
                const uint32_t w0 = (px & 3) == 0 ? v0.x : ((px & 3) == 1 ? v0.y : ((px & 3) == 2 ? v0.z : v0.w));
                const uint32_t w1 = (px & 3) == 0 ? v1.x : ((px & 3) == 1 ? v1.y : ((px & 3) == 2 ? v1.z : v1.w));
                uint32_t b0, g0, c0, b1, g1, c1;
                bgra_px<ORDER>(w0, b0, g0, c0);
                bgra_px<ORDER>(w1, b1, g1, c1);
                const uint32_t Y0 = bt601_y(b0, g0, c0), Y1 = bt601_y(b1, g1, c1);
                y0[px >> 2] |= Y0 << (8 * (px & 3));
                y1[px >> 2] |= Y1 << (8 * (px & 3));
                if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
                if (UVMODE && (px & 1) == 0) {                   // chroma from the top-left pixel of each 2 x 2 block
                    uint32_t U, V;
                    bt601_uv(b0, g0, c0, U, V);
                    if (CHROMA) {                                // wc[0..1]: 8 U bytes, wc[2..3]: 8 V bytes
                        wc[px >> 3] |= U << (8 * ((px >> 1) & 3));
                        wc[2 + (px >> 3)] |= V << (8 * ((px >> 1) & 3));
                    } else {                                     // 8 U,V pairs
                        wc[px >> 2] |= (U | (V << 8)) << (8 * (px & 2));
                    }
                }
            }
            const u32x4 o0 = {y0[0], y0[1], y0[2], y0[3]}, o1 = {y1[0], y1[1], y1[2], y1[3]};
            uint8_t* d0 = yp + (long long)(2 * by) * j.y_step + (gx << 4);
            *reinterpret_cast<u32x4*>(d0) = o0;
            *reinterpret_cast<u32x4*>(d0 + j.y_step) = o1;
            if (CHROMA) {
                const long long co = (long long)by * j.c_step + (gx << 3);
                *reinterpret_cast<uint2*>(p0 + co) = make_uint2(wc[0], wc[1]);
                *reinterpret_cast<uint2*>(p1 + co) = make_uint2(wc[2], wc[3]);
            } else {
                const u32x4 ouv = {wc[0], wc[1], wc[2], wc[3]};
                *reinterpret_cast<u32x4*>(p0 + (long long)by * j.c_step + (gx << 4)) = ouv;
            }
        }
    } else {                                            // one 2 x 2 block per lane
        const int bx_n = j.width >> 1;
        const long long blocks = (long long)bx_n * (j.height >> 1);
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        for (long long bi = (long long)blockIdx.x * kThreads + t; bi < blocks; bi += (long long)gridDim.x * kThreads) {
            const int by = (int)(bi / bx_n), bx = (int)(bi - (long long)by * bx_n);
            const uint8_t* r0 = ip + (long long)(2 * by) * j.in_step + 8 * bx;
            const uint8_t* r1 = r0 + j.in_step;
            uint8_t* d0 = yp + (long long)(2 * by) * j.y_step + 2 * bx;
            uint8_t* d1 = d0 + j.y_step;
            const uint32_t b00 = r0[B], g00 = r0[1], q00 = r0[R];
            const uint32_t Y00 = bt601_y(b00, g00, q00), Y01 = bt601_y(r0[4 + B], r0[5], r0[4 + R]);
            const uint32_t Y10 = bt601_y(r1[B], r1[1], r1[R]), Y11 = bt601_y(r1[4 + B], r1[5], r1[4 + R]);
            uint32_t U = 128, V = 128;
            if (UVMODE) bt601_uv(b00, g00, q00, U, V);
            d0[0] = (uint8_t)Y00; d0[1] = (uint8_t)Y01; d1[0] = (uint8_t)Y10; d1[1] = (uint8_t)Y11;
            if (CHROMA) {
                const long long co = (long long)by * j.c_step + bx;
                p0[co] = (uint8_t)U; p1[co] = (uint8_t)V;
            } else {
                uint8_t* duv = p0 + (long long)by * j.c_step + 2 * bx;
                duv[0] = (uint8_t)U; duv[1] = (uint8_t)V;
            }
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
template <int ORDER, int CHROMA, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgra_to_yuv420_hist_kernel(BgraYuv420Job j, uint32_t* __restrict__ partial)
{
    bgra_to_yuv420_hist_body<ORDER, CHROMA, UVMODE, HIST>(j, StridedBgraYuv420{j}, partial);
}
// the same on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either walk -- a
// byte-path frame of a vector-shaped launch takes more steps; the partials are those of the chunk's frames in list order
template <int ORDER, int CHROMA, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgra_to_yuv420_hist_frames_kernel(BgraYuv420Job j, BgraYuv420List l, uint32_t* __restrict__ partial)
{
    bgra_to_yuv420_hist_body<ORDER, CHROMA, UVMODE, HIST>(j, TableBgraYuv420{l, j}, partial);
}
static_assert(kThreads == 256, "bgra_to_yuv420_hist_body writes one bin per thread");
// 256: the implicit arguments a code object carries behind the explicit ones
static_assert(sizeof(BgraYuv420List) == (size_t)kFramesPerLaunch * 32 && sizeof(BgraYuv420List) <= 2048, "the table is at most 2 KiB");
static_assert(sizeof(BgraYuv420Job) + sizeof(BgraYuv420List) + sizeof(uint32_t*) + 256 <= 4096,
              "the table and the remaining arguments of bgra_to_yuv420_hist_frames_kernel stay below HIP's 4 KiB of kernel arguments");

}  // namespace mi
