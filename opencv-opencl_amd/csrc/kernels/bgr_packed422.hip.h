// bgr_packed422.hip.h -- interleaved 8-bit BGR / RGB images in, pitched packed 4:2:2 frames (YUY2 / UYVY) out, counting the luma the conversion produces
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"
#include "color.hip.h"
#include "packed422.hip.h"

namespace mi {
// =============================================================================================
// Stage 1 of bgr_nv12.hip.h with a packed 4:2:2 frame out -- what SDI / HDMI playout cards, v4l2 output and loopback devices and
// virtual cameras take: one dword per macropixel, Y0 U Y1 V (OFF = 0, MI_FMT_YUY2) or U Y0 V Y1 (OFF = 1, MI_FMT_UYVY).  Y is not in
// the input, so the conversion is stage 1 and counts the luma bytes it has just produced; stage 2 is the packed form's own kernels IN
// PLACE on the output frame (packed422.hip.h: lut_apply422_kernel, the tile histograms and the interpolation with src == dst, the
// chroma bytes of every dword kept).
// Bytes per pixel: equalizeHist 3 read + 2 written here, then 2 read + 2 written by the in-place map: 9.  CLAHE: 5 here (no
// histogram), then the tile histograms read the frame (2) and the interpolation reads and writes it (4): 11.
// The arithmetic is color.hip.h's encode: Y = bt601_y of every pixel; U, V = bt601_uv of the LEFT pixel (2k, y) of macropixel (k, y),
// without averaging -- the 4:2:0 rule of bgr_to_nv12_hist_body (top-left pixel of a 2 x 2 block) applied to every row on its own,
// and what the decode of packed422_bgr.hip.h reads back for both pixels of the macropixel.
// ORDER 0: B, G, R in memory (MI_ORDER_BGR); 1: R, G, B (MI_ORDER_RGB).  UVMODE 0: every chroma byte 128 (MI_UV_FILL128, the chroma
// arithmetic is skipped); 1: U, V of the conversion (MI_UV_COPY).
// =============================================================================================
struct BgrPacked422Job {
    const uint8_t* in;                        // H rows of 3*W bytes
    uint8_t* out;                             // H rows of 2*W bytes (W/2 macropixel dwords); a multiple of 4, as out_step and out_frame
    long long in_step, out_step;              // bytes between rows
    long long in_frame, out_frame;            // bytes between frames
    int width, height;                        // width even; height any
    int vec;                                  // 1: W % 16 == 0 and every base / pitch / frame stride a multiple of 16 -> 16 x 1 pixel groups
};

// ---------------------------------------------------------------------------------------------
// grid = (B, n_frames), 256 threads.  With HIST: partial[(f * B + part) * 256 + bin], the layout of hist_partial_kernel, which
// equalize_lut_kernel reads.
// vec: a lane owns 16 pixels of ONE row -- one load_bgr16 (three 16-byte loads), two 16-byte stores of four macropixels each -- on the
// carried (row, gx) walk of bgr_to_nv12_hist_body (no 64-bit division per group); otherwise one macropixel per lane: six byte loads and
// one aligned dword store.  Only the 2*W bytes of each output row are written.
// Workgroup size and histogram copies: 256 threads and hist[bin][32], as there.  A lane of the vector path holds ONE row of 16 pixels
// unpacked (half of what the 16 x 2 groups of the 4:2:0 writers hold) next to the eight dwords it packs.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int OFF, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgr_to_packed422_hist_kernel(BgrPacked422Job j, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t h[HIST ? 256 * kCopies : 1];
    const int t = threadIdx.x, f = blockIdx.y;
    if (HIST) {
        for (int i = t; i < 256 * kCopies; i += kThreads) h[i] = 0;
        __syncthreads();
    }
    const uint32_t copy = t & (kCopies - 1);
    const uint8_t* ip = j.in + (long long)f * j.in_frame;
    uint8_t* op = j.out + (long long)f * j.out_frame;
    // the chroma bytes of a dword: bytes 1 and 3 (OFF = 0) or 0 and 2 (OFF = 1); U is the lower of the two
    constexpr int kUShift = OFF ? 0 : 8, kVShift = kUShift + 16;
    constexpr uint32_t kFill = (0x80u << kUShift) | (0x80u << kVShift);
    if (j.vec) {
        const int gx_n = j.width >> 4;
        const int groups = gx_n * j.height;                   // < 2^27 (W*H < 2^31)
        const int stride = (int)gridDim.x * kThreads, dy = stride / gx_n, dgx = stride - dy * gx_n;
        int gi = (int)blockIdx.x * kThreads + t;
        int y = gi / gx_n, gx = gi - y * gx_n;
        for (; gi < groups; gi += stride, y += dy, gx += dgx) {
            if (gx >= gx_n) { gx -= gx_n; ++y; }
            uint32_t a[16], g[16], c[16];                     // a: first channel in memory, c: third
            load_bgr16(ip + (long long)y * j.in_step + 48 * gx, a, g, c);
            const uint32_t* b = ORDER == 0 ? a : c; const uint32_t* q = ORDER == 0 ? c : a;
            uint32_t w[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {                     // macropixel k: pixels 2k and 2k + 1
                const uint32_t Y0 = bt601_y(b[2 * k], g[2 * k], q[2 * k]), Y1 = bt601_y(b[2 * k + 1], g[2 * k + 1], q[2 * k + 1]);
                if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
                uint32_t cw = kFill;
                if (UVMODE) {                                 // chroma from the left pixel of the macropixel
                    uint32_t U, V;
                    bt601_uv(b[2 * k], g[2 * k], q[2 * k], U, V);
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
            const uint8_t* r = ip + (long long)y * j.in_step + 6 * mx;
            const uint32_t b0 = r[B], g0 = r[1], q0 = r[R];
            const uint32_t Y0 = bt601_y(b0, g0, q0), Y1 = bt601_y(r[3 + B], r[4], r[3 + R]);
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
static_assert(kThreads == 256, "bgr_to_packed422_hist_kernel writes one bin per thread");

// =============================================================================================
// The same on a list of frames, each at its own two addresses (mi_*_bgr_to_packed422_frames_dev: a pool of images in, a playout
// card's or a v4l2 output queue's buffer pool out).  An entry is packed422.hip.h's own {in, out} pair -- `in` the image, `out` the
// packed frame -- so the table is its Packed422List: BY VALUE in the kernel arguments, 16 B an entry, read with scalar kernarg loads
// indexed by the frame's grid coordinate, and one chunk size serves this stage and the in-place stage 2.  The shape (pitches, width,
// height) is the launch's BgrPacked422Job, whose in / out / *_frame a table launch ignores and whose vec says what the SHAPE allows
// (W % 16 == 0, both pitches multiples of 16): whether frame f takes the 16 x 1 groups is then decided by its own two addresses -- per
// frame, so uniform for a workgroup.
// The kernel is a COPY of the one above with the frame's addresses read from the table, as bgr_yuv420.hip.h has its list kernel: a
// change there is made here too.  The other form in the tree -- one body as a template on a frame-address policy, StridedBgrNv12 /
// TableBgrNv12 in bgr_nv12.hip.h -- was built first and changed the ISA of all sixteen bgr_to_packed422_hist_kernel instantiations
// (the sums of bt601_y came out in another order, the 856 instructions of the equalizeHist instantiations became 866).  The policy is
// not the cause: the parent's text moved unchanged into a __device__ __forceinline__ function that the kernel calls with its own
// argument, by value or by reference, gives the same sixteen differences -- a body that is a function is optimised once on its own
// and once more inside the kernel -- so no function-shaped body keeps the batch form's ISA, which it must not pay for the list form
// (DESIGN.md).  Tried once more when the host side of the image forms became one implementation, with the two policies of
// bgra_packed422.hip.h (StridedBgraPacked422 / TableBgraPacked422) word for word: all 32 instantiations of the two kernels changed
// (docs/experiments.md, R39).  The copy stays.
// =============================================================================================
static_assert(sizeof(Packed422Frame) == 16, "two addresses an entry");

// THE rule "does this frame of a list take the 16 x 1 groups": what the shape allows, and the frame's own image and frame addresses
// multiples of 16.  The kernel decides by it and the host counts by it.
__host__ __device__ __forceinline__ bool bgr_packed422_frame_vec(int shape_vec, const void* in, const void* out)
{
    return shape_vec && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
}

// bgr_to_packed422_hist_kernel on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames on
// either walk -- a byte-walk frame of a vector-shaped launch takes more steps.  The partials are those of the chunk's frames in list
// order: partial[(f * gridDim.x + blockIdx.x) * 256 + bin].
template <int ORDER, int OFF, int UVMODE, bool HIST>
__global__ __launch_bounds__(kThreads) void bgr_to_packed422_hist_frames_kernel(BgrPacked422Job j, Packed422List l, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t h[HIST ? 256 * kCopies : 1];
    const int t = threadIdx.x, f = blockIdx.y;
    if (HIST) {
        for (int i = t; i < 256 * kCopies; i += kThreads) h[i] = 0;
        __syncthreads();
    }
    const uint32_t copy = t & (kCopies - 1);
    const uint8_t* ip = l.f[f].in;                  // scalar kernarg loads: f is uniform for the workgroup
    uint8_t* op = l.f[f].out;
    // the chroma bytes of a dword: bytes 1 and 3 (OFF = 0) or 0 and 2 (OFF = 1); U is the lower of the two
    constexpr int kUShift = OFF ? 0 : 8, kVShift = kUShift + 16;
    constexpr uint32_t kFill = (0x80u << kUShift) | (0x80u << kVShift);
    if (bgr_packed422_frame_vec(j.vec, ip, op)) {
        const int gx_n = j.width >> 4;
        const int groups = gx_n * j.height;                   // < 2^27 (W*H < 2^31)
        const int stride = (int)gridDim.x * kThreads, dy = stride / gx_n, dgx = stride - dy * gx_n;
        int gi = (int)blockIdx.x * kThreads + t;
        int y = gi / gx_n, gx = gi - y * gx_n;
        for (; gi < groups; gi += stride, y += dy, gx += dgx) {
            if (gx >= gx_n) { gx -= gx_n; ++y; }
            uint32_t a[16], g[16], c[16];                     // a: first channel in memory, c: third
            load_bgr16(ip + (long long)y * j.in_step + 48 * gx, a, g, c);
            const uint32_t* b = ORDER == 0 ? a : c; const uint32_t* q = ORDER == 0 ? c : a;
            uint32_t w[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {                     // macropixel k: pixels 2k and 2k + 1
                const uint32_t Y0 = bt601_y(b[2 * k], g[2 * k], q[2 * k]), Y1 = bt601_y(b[2 * k + 1], g[2 * k + 1], q[2 * k + 1]);
                if (HIST) { lds_inc(h, (Y0 << kCopyShift) + copy); lds_inc(h, (Y1 << kCopyShift) + copy); }
                uint32_t cw = kFill;
                if (UVMODE) {                                 // chroma from the left pixel of the macropixel
                    uint32_t U, V;
                    bt601_uv(b[2 * k], g[2 * k], q[2 * k], U, V);
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
            const uint8_t* r = ip + (long long)y * j.in_step + 6 * mx;
            const uint32_t b0 = r[B], g0 = r[1], q0 = r[R];
            const uint32_t Y0 = bt601_y(b0, g0, q0), Y1 = bt601_y(r[3 + B], r[4], r[3 + R]);
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
static_assert(kThreads == 256, "bgr_to_packed422_hist_frames_kernel writes one bin per thread");
// 256: the implicit arguments a code object carries behind the explicit ones
static_assert(sizeof(BgrPacked422Job) + sizeof(Packed422List) + sizeof(uint32_t*) + 256 <= 4096,
              "the table and the remaining arguments of bgr_to_packed422_hist_frames_kernel stay below HIP's 4 KiB of kernel arguments");

}  // namespace mi
