// bgra_packed422.hip.h -- interleaved 8-bit four-channel images (BGRA / BGRX, RGBA / RGBX: CV_8UC4) in, pitched packed 4:2:2 frames
// (YUY2 / UYVY) out, counting the luma the conversion produces
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"
#include "color.hip.h"
#include "packed422.hip.h"
#include "bgra_yuv420.hip.h"                  // bgra_px

namespace mi {
// =============================================================================================
// Stage 1 of bgr_packed422.hip.h on the four-byte pixels of render targets, swap-chain images, screen captures and interop buffers:
// one dword per macropixel out, Y0 U Y1 V (OFF = 0, MI_FMT_YUY2) or U Y0 V Y1 (OFF = 1, MI_FMT_UYVY).  The fourth byte (alpha or
// padding) is loaded with its pixel and takes part in nothing.  Stage 2 is the same: the packed form's own kernels IN PLACE on the
// output frame, the chroma bytes of every dword kept.
// Bytes per pixel: equalizeHist 4 read + 2 written here, then 2 + 2 by the in-place map: 10.  CLAHE: 6 here (no histogram), then the
// tile histograms read the frame (2) and the interpolation reads and writes it (4): 12.
// These are new kernels, so there is ONE body: a template on a frame-address policy (strided batch / by-value table), the shape of
// bgra_to_yuv420_hist_body.  bgr_packed422.hip.h says why its kernels are copies; no existing kernel is touched.
// The arithmetic is color.hip.h's encode: Y = bt601_y of every pixel; U, V = bt601_uv of the LEFT pixel of each macropixel of each
// row, without averaging -- the bytes of bgr_to_packed422_hist_kernel on the image with its fourth byte removed.
// ORDER 0: B, G, R, X in memory (MI_ORDER_BGR); 1: R, G, B, X (MI_ORDER_RGB).  UVMODE 0: every chroma byte 128 (MI_UV_FILL128, the
// chroma arithmetic is skipped); 1: U, V of the conversion (MI_UV_COPY).
// =============================================================================================
struct BgraPacked422Job {
    const uint8_t* in;                        // H rows of 4*W bytes
    uint8_t* out;                             // H rows of 2*W bytes (W/2 macropixel dwords); a multiple of 4, as out_step and out_frame
    long long in_step, out_step;              // bytes between rows
    long long in_frame, out_frame;            // bytes between frames
    int width, height;                        // width even; height any
    int vec;                                  // 1: W % 16 == 0 and every base / pitch / frame stride a multiple of 16 -> 16 x 1 pixel groups
};

// THE rule "does a frame at these addresses take the 16 x 1 groups": what the shape allows, and the frame's own image and frame
// addresses multiples of 16 (four 16-byte loads, two 16-byte stores).  The kernel decides by it and the host counts by it.
__host__ __device__ __forceinline__ bool bgra_packed422_frame_vec(int shape_vec, const void* in, const void* out)
{
    return shape_vec && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
}

// Where frame f of a launch lives: the body below is a template on one of these two policies.
struct StridedBgraPacked422 {
    const BgraPacked422Job& j;
    __device__ __forceinline__ const uint8_t* in_of(long long f) const { return j.in + f * j.in_frame; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return j.out + f * j.out_frame; }
    __device__ __forceinline__ bool vec(long long) const { return j.vec; }                // decided by the host for the whole launch
};

// A list of such frames, each at its own two addresses (mi_*_bgra_to_packed422_frames_dev: a pool of surfaces in, a playout card's or
// a v4l2 output queue's buffer pool out).  An entry is packed422.hip.h's own {in, out} pair, so the table is its Packed422List: BY
// VALUE in the kernel arguments, 128 x 16 B = 2 KiB, read with scalar kernarg loads indexed by the frame's grid coordinate, and one
// chunk size serves this stage and the in-place stage 2.  The shape (pitches, width, height) is the launch's BgraPacked422Job, whose
// in / out / *_frame a table launch ignores and whose vec says what the SHAPE allows: whether frame f takes the 16 x 1 groups is then
// decided by its own two addresses -- per frame, so uniform for a workgroup.
struct TableBgraPacked422 {
    const Packed422List& l;
    const BgraPacked422Job& j;
    __device__ __forceinline__ const uint8_t* in_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return l.f[f].out; }
    __device__ __forceinline__ bool vec(long long f) const { return bgra_packed422_frame_vec(j.vec, l.f[f].in, l.f[f].out); }
};

// ---------------------------------------------------------------------------------------------
// Stage 1.  grid = (B, n_frames), 256 threads.  With HIST: partial[(f * B + part) * 256 + bin], the layout of hist_partial_kernel,
// which equalize_lut_kernel reads.
// vec: a lane owns 16 pixels of ONE row -- four 16-byte loads, all issued before the first use; every dword is one pixel, so the
// channels are byte extracts of a dword (bgra_px; none of load_bgr16's unpacking across dwords: 16 dwords held where the three-channel
// body holds 48 channel words) -- and two 16-byte stores of four macropixels each, on the carried (y, gx) walk of
// bgr_to_packed422_hist_kernel (no 64-bit division per group); otherwise one macropixel per lane: byte loads at 8*mx + {0,1,2} and
// 8*mx + 4 + {0,1,2} and one aligned dword store.  Only the 2*W bytes of each output row are written.
// Plain loads and stores: the frame written here is read again by stage 2 and must stay in the caches; the once-read input has no
// non-temporal policy (not measured).
// Workgroup size and histogram copies: 256 threads and hist[bin][32], as there.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int OFF, int UVMODE, bool HIST, class Frames>
__device__ __forceinline__ void bgra_to_packed422_hist_body(const BgraPacked422Job& j, const Frames& fr, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t h[HIST ? 256 * kCopies : 1];
    const int t = threadIdx.x, f = blockIdx.y;
    if (HIST) {
        for (int i = t; i < 256 * kCopies; i += kThreads) h[i] = 0;
        __syncthreads();
    }
    const uint32_t copy = t & (kCopies - 1);
    const uint8_t* ip = fr.in_of(f);
    uint8_t* op = fr.out_of(f);
    // the chroma bytes of a dword: bytes 1 and 3 (OFF = 0) or 0 and 2 (OFF = 1); U is the lower of the two
    constexpr int kUShift = OFF ? 0 : 8, kVShift = kUShift + 16;
    constexpr uint32_t kFill = (0x80u << kUShift) | (0x80u << kVShift);
    if (fr.vec(f)) {
        const int gx_n = j.width >> 4;
        const int groups = gx_n * j.height;                   // < 2^27 (W*H < 2^31)
        const int stride = (int)gridDim.x * kThreads, dy = stride / gx_n, dgx = stride - dy * gx_n;
        int gi = (int)blockIdx.x * kThreads + t;
        int y = gi / gx_n, gx = gi - y * gx_n;
        for (; gi < groups; gi += stride, y += dy, gx += dgx) {
            if (gx >= gx_n) { gx -= gx_n; ++y; }
            const u32x4* r = reinterpret_cast<const u32x4*>(ip + (long long)y * j.in_step + 64 * gx);
            const u32x4 q[4] = {r[0], r[1], r[2], r[3]};        // four loads in flight
            uint32_t w[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {                     // macropixel k: pixels 2k and 2k + 1, the dwords of one half of q[k / 2]
                const u32x4& v = q[k >> 1];
                const uint32_t p0 = (k & 1) ? v.z : v.x, p1 = (k & 1) ? v.w : v.y;
                uint32_t b0, g0, c0, b1, g1, c1;
                bgra_px<ORDER>(p0, b0, g0, c0);
                bgra_px<ORDER>(p1, b1, g1, c1);
                const uint32_t Y0 = bt601_y(b0, g0, c0), Y1 = bt601_y(b1, g1, c1);
                if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
                uint32_t cw = kFill;
                if (UVMODE) {                                 // chroma from the left pixel of the macropixel
                    uint32_t U, V;
                    bt601_uv(b0, g0, c0, U, V);
                    cw = (U << kUShift) | (V << kVShift);
                }
                w[k] = put_y<OFF>(Y0, Y1) | cw;
            }
            const u32x4 o0 = {w[0], w[1], w[2], w[3]}, o1 = {w[4], w[5], w[6], w[7]};
            uint8_t* d = op + (long long)y * j.out_step + (gx << 5);
            *reinterpret_cast<u32x4*>(d) = o0;
            *reinterpret_cast<u32x4*>(d + 16) = o1;
        }
    } else {                                            // one macropixel per lane
        const int mx_n = j.width >> 1;
        const long long items = (long long)mx_n * j.height;
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        for (long long mi = (long long)blockIdx.x * kThreads + t; mi < items; mi += (long long)gridDim.x * kThreads) {
            const int y = (int)(mi / mx_n), mx = (int)(mi - (long long)y * mx_n);
            const uint8_t* r = ip + (long long)y * j.in_step + 8 * mx;
            const uint32_t b0 = r[B], g0 = r[1], q0 = r[R];
            const uint32_t Y0 = bt601_y(b0, g0, q0), Y1 = bt601_y(r[4 + B], r[5], r[4 + R]);
            uint32_t cw = kFill;
            if (UVMODE) {
                uint32_t U, V;
                bt601_uv(b0, g0, q0, U, V);
                cw = (U << kUShift) | (V << kVShift);
            }
            *reinterpret_cast<uint32_t*>(op + (long long)y * j.out_step + 4 * mx) = put_y<OFF>(Y0, Y1) | cw;
            if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
        }
    }
    if (HIST) {
        __syncthreads();
        partial[((size_t)f * gridDim.x + blockIdx.x) * 256 + t] = lds_hist_bin(h, t);      // kThreads == 256 bins
    }
}
template <int ORDER, int OFF, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgra_to_packed422_hist_kernel(BgraPacked422Job j, uint32_t* __restrict__ partial)
{
    bgra_to_packed422_hist_body<ORDER, OFF, UVMODE, HIST>(j, StridedBgraPacked422{j}, partial);
}
// the same on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either walk -- a
// byte-walk frame of a vector-shaped launch takes more steps; the partials are those of the chunk's frames in list order
template <int ORDER, int OFF, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgra_to_packed422_hist_frames_kernel(BgraPacked422Job j, Packed422List l, uint32_t* __restrict__ partial)
{
    bgra_to_packed422_hist_body<ORDER, OFF, UVMODE, HIST>(j, TableBgraPacked422{l, j}, partial);
}
static_assert(kThreads == 256, "bgra_to_packed422_hist_body writes one bin per thread");
// 256: the implicit arguments a code object carries behind the explicit ones
static_assert(sizeof(Packed422List) == (size_t)kPacked422FramesPerLaunch * 16 && sizeof(Packed422List) <= 2048, "the table is at most 2 KiB");
static_assert(sizeof(BgraPacked422Job) + sizeof(Packed422List) + sizeof(uint32_t*) + 256 <= 4096,
              "the table and the remaining arguments of bgra_to_packed422_hist_frames_kernel stay below HIP's 4 KiB of kernel arguments");

}  // namespace mi
