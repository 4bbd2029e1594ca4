// yuv420_bgra.hip.h -- pitched 4:2:0 frames (I420 / YV12 planes, or NV12) in, interleaved 8-bit four-channel images (BGRA / RGBA:
// CV_8UC4, A = 255) out, in the pass that maps the luma
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "nv12_bgr.hip.h"
#include "yuv420_bgr.hip.h"

namespace mi {
// =============================================================================================
// cv::equalizeHist / CLAHE::apply on the Y plane of a 4:2:0 frame, then cv::cvtColor(COLOR_YUV2BGRA_NV12 / _I420 / _YV12) (or the RGBA
// codes): the two pixel-writing stages of yuv420_bgr.hip.h with a four-byte pixel -- what display surfaces, swap-chain images, interop
// textures and GUI image types hold.  The first three bytes of a pixel are the three-channel form's, the fourth is 255.  The histogram
// stages are the planar kernels (Y is a plane).
// Bytes per pixel: Y read twice (histograms, then map), the chroma once (0.5), 4 written: 6.5; the pixel-writing kernel alone 5.5.
// These are new kernels, so there is ONE body each: a template on ORDER, on the chroma layout (CHROMA 0: U, V interleaved in one plane,
// NV12; 1: a U and a V plane) and on a frame-address policy (strided batch / by-value table), the shape of bgra_yuv420.hip.h and of
// nv12_bgr.hip.h's Strided* / Table* structs.  No existing kernel is touched; an interleaved input is NOT handed to nv12_bgr.hip.h.
// The store is the friendly one: every pixel is a dword, a 16-pixel group four aligned 16-byte stores, none of store_bgr16's shuffling
// of 48 bytes into three.
// ORDER 0: B, G, R, A in memory (MI_ORDER_BGR); 1: R, G, B, A (MI_ORDER_RGB).  c0 is always U (or the UV plane) and c1 always V; a YV12
// frame is the same planes at exchanged addresses, decided by the caller.
// =============================================================================================
struct Yuv420BgraJob {
    const uint8_t* y; const uint8_t* c0; const uint8_t* c1;  // Y: H rows of W bytes; planar: c0 = U, c1 = V, H/2 rows of W/2 bytes each;
                                                             // interleaved: c0 = the UV plane, H/2 rows of W bytes, c1 unused
    uint8_t* out;                                            // H rows of 4*W bytes
    long long y_step, c_step, out_step;                      // bytes between rows (two chroma planes share theirs)
    long long y_frame, c_frame, out_frame;                   // bytes between frames (the Y planes of the two-pass fallback lie in scratch: a stride of their own)
    int width, height;                                       // both even
    int vec;                                                 // 1: W % 16 == 0, the Y and output terms multiples of 16, the chroma terms of 16 (interleaved) or 8 (planar)
};

// THE rule "does a frame at these addresses take the 16 x 2 groups": what the shape allows, and the frame's own Y and image addresses
// multiples of 16, its UV address of 16 (one 16-byte load) or its U and V addresses of 8 (two 8-byte loads).  The kernel decides by it
// and the host counts by it.
__host__ __device__ __forceinline__ bool yuv420_bgra_frame_vec(int shape_vec, bool planar, const void* y, const void* c0, const void* c1,
                                                               const void* out)
{
    const uintptr_t chroma = planar ? (((uintptr_t)c0 | (uintptr_t)c1) & 7) : ((uintptr_t)c0 & 15);
    return shape_vec && ((((uintptr_t)y | (uintptr_t)out) & 15) | chroma) == 0;
}

// Where frame f of a launch lives, as StridedNv12Bgr / TableNv12Bgr (nv12_bgr.hip.h) say it: the bodies below are templates on one of
// these two policies.
struct StridedYuv420Bgra {
    const Yuv420BgraJob& j;
    __device__ __forceinline__ const uint8_t* y_of(long long f) const { return j.y + f * j.y_frame; }
    __device__ __forceinline__ const uint8_t* c0_of(long long f) const { return j.c0 + f * j.c_frame; }
    __device__ __forceinline__ const uint8_t* c1_of(long long f) const { return j.c1 + f * j.c_frame; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return j.out + f * j.out_frame; }
    __device__ __forceinline__ bool vec(bool, long long) const { return j.vec; }          // decided by the host for the whole launch
};

// A list of such frames, each at its own four addresses (mi_*_yuv420_to_bgra_frames_dev: a decoder's frame pool in, a pool of surfaces
// out).  The {y, c0, c1, out} entries travel BY VALUE in the kernel arguments like Yuv420BgrList -- 64 x 32 B = 2 KiB -- and are read
// with scalar kernarg loads indexed by the frame's grid coordinate.  The shape (pitches, width, height) is the launch's Yuv420BgraJob,
// whose y / c0 / c1 / out / *_frame a table launch ignores and whose vec says what the SHAPE allows: whether frame f takes the 16 x 2
// groups is then decided by its own addresses -- per frame, so uniform for a workgroup.
struct Yuv420BgraFrame { const uint8_t* y; const uint8_t* c0; const uint8_t* c1; uint8_t* out; };
struct Yuv420BgraList { Yuv420BgraFrame f[kFramesPerLaunch]; };
static_assert(sizeof(Yuv420BgraFrame) == 32, "four addresses an entry");
struct TableYuv420Bgra {
    const Yuv420BgraList& l;
    const Yuv420BgraJob& j;
    __device__ __forceinline__ const uint8_t* y_of(long long f) const { return l.f[f].y; }
    __device__ __forceinline__ const uint8_t* c0_of(long long f) const { return l.f[f].c0; }
    __device__ __forceinline__ const uint8_t* c1_of(long long f) const { return l.f[f].c1; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return l.f[f].out; }
    __device__ __forceinline__ bool vec(bool planar, long long f) const
    {
        return yuv420_bgra_frame_vec(j.vec, planar, l.f[f].y, l.f[f].c0, l.f[f].c1, l.f[f].out);
    }
};

// The 8 U,V pairs of the 16-pixel group at pixel column x of the chroma row at byte offset `row`: one 16-byte load from the UV plane,
// or one 8-byte load from each of the U and the V plane, zipped (zip_uv8).  p1 is not looked at for CHROMA 0.
template <int CHROMA>
__device__ __forceinline__ u32x4 load_uv16(const uint8_t* p0, const uint8_t* p1, long long row, int x)
{
    if (CHROMA == 0) return *reinterpret_cast<const u32x4*>(p0 + row + x);
    const long long co = row + (x >> 1);
    return zip_uv8(*reinterpret_cast<const uint2*>(p0 + co), *reinterpret_cast<const uint2*>(p1 + co));
}

// one pixel dword of either order, alpha 255
template <int ORDER>
__device__ __forceinline__ uint32_t bgra_dword(uint32_t b, uint32_t g, uint32_t r)
{
    return (ORDER == 0 ? b : r) | (g << 8) | ((ORDER == 0 ? r : b) << 16) | 0xff000000u;
}

// 16 luma bytes (already mapped) + the 8 U,V pairs above / below them -> 16 pixels, 64 bytes at p (16-byte aligned): decode_store16 of
// nv12_bgr.hip.h with every pixel its own dword.  Four pixels are packed and stored at a time, so four output dwords are live beside
// the inputs, not sixteen.
template <int ORDER>
__device__ __forceinline__ void decode_store16_4(uint8_t* p, const u32x4& y, const u32x4& uv)
{
    u32x4* d = reinterpret_cast<u32x4*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t w[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * q + h;                          // chroma sample k serves pixels 2k and 2k + 1
            int ruv, guv, buv;
            bt601_uv_terms(byte_of(uv, 2 * k), byte_of(uv, 2 * k + 1), ruv, guv, buv);
            uint32_t b, g, r;
            bt601_px_bgr(byte_of(y, 2 * k), ruv, guv, buv, b, g, r);     w[2 * h] = bgra_dword<ORDER>(b, g, r);
            bt601_px_bgr(byte_of(y, 2 * k + 1), ruv, guv, buv, b, g, r); w[2 * h + 1] = bgra_dword<ORDER>(b, g, r);
        }
        const u32x4 o = {w[0], w[1], w[2], w[3]};
        d[q] = o;
    }
}

// ---------------------------------------------------------------------------------------------
// LUT apply + decode (equalizeHist), and with LUT = false the decode alone (second pass of the CLAHE fallback, whose Y planes are the
// planar CLAHE's output in scratch): the grid, the carried walk, the frame order and the LDS LUT of yuv420_to_bgr_kernel.
// grid = (B, n_frames), 256 threads.
// vec: a lane owns a 16 x 2 pixel group -- two 16-byte Y loads, one 16-byte UV load or one 8-byte U load plus one 8-byte V load, eight
// 16-byte stores; otherwise a 2 x 2 block with byte accesses, four byte stores per pixel, the last of them 255.  Only the 4*W bytes of
// each output row are written.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int CHROMA, bool LUT, class Frames>
__device__ __forceinline__ void yuv420_to_bgra_body(const Yuv420BgraJob& j, const Frames& fr, const uint8_t* __restrict__ luts)
{
    __shared__ uint32_t lut[LUT ? 256 * kCopies : 1];
    const int t = threadIdx.x;
    // frame order as nv12_to_bgr_body: last-to-first behind the histogram pass, first-to-last behind the interpolation
    const int f = LUT ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
    const uint32_t copy = t & (kCopies - 1);
    if (LUT) {
        const uint32_t v = luts[(size_t)f * 256 + t];
#pragma unroll
        for (int k = 0; k < kCopies; ++k) lut[(t << kCopyShift) + ((k + t) & (kCopies - 1))] = v;
        __syncthreads();
    }
    const uint8_t* yp = fr.y_of(f);
    const uint8_t* p0 = fr.c0_of(f);
    const uint8_t* p1 = CHROMA ? fr.c1_of(f) : nullptr;
    uint8_t* op = fr.out_of(f);
    if (fr.vec(CHROMA != 0, f)) {
        const int gx_n = j.width >> 4;
        const int groups = gx_n * (j.height >> 1);            // < 2^26 (W*H < 2^31)
        const int stride = (int)gridDim.x * kThreads, dby = stride / gx_n, dgx = stride - dby * gx_n;
        int gi = (int)blockIdx.x * kThreads + t;
        int by = gi / gx_n, gx = gi - by * gx_n;
        for (; gi < groups; gi += stride, by += dby, gx += dgx) {
            if (gx >= gx_n) { gx -= gx_n; ++by; }
            const uint8_t* y0p = yp + (long long)(2 * by) * j.y_step + (gx << 4);
            u32x4 y0 = *reinterpret_cast<const u32x4*>(y0p);
            u32x4 y1 = *reinterpret_cast<const u32x4*>(y0p + j.y_step);
            const u32x4 uv = load_uv16<CHROMA>(p0, p1, (long long)by * j.c_step, gx << 4);
            if (LUT) { y0 = lut_vec(lut, y0, copy); y1 = lut_vec(lut, y1, copy); }
            uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 64 * gx;
            decode_store16_4<ORDER>(d0, y0, uv);
            decode_store16_4<ORDER>(d0 + j.out_step, y1, uv);
        }
        return;
    }
    const int bx_n = j.width >> 1;
    const long long blocks = (long long)bx_n * (j.height >> 1);
    for (long long bi = (long long)blockIdx.x * kThreads + t; bi < blocks; bi += (long long)gridDim.x * kThreads) {
        const int by = (int)(bi / bx_n), bx = (int)(bi - (long long)by * bx_n);
        const uint8_t* r0 = yp + (long long)(2 * by) * j.y_step + 2 * bx;
        const uint8_t* r1 = r0 + j.y_step;
        uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 8 * bx;
        uint8_t* d1 = d0 + j.out_step;
        uint32_t Y00 = r0[0], Y01 = r0[1], Y10 = r1[0], Y11 = r1[1];
        if (LUT) {
            Y00 = lut[(Y00 << kCopyShift) + copy]; Y01 = lut[(Y01 << kCopyShift) + copy];
            Y10 = lut[(Y10 << kCopyShift) + copy]; Y11 = lut[(Y11 << kCopyShift) + copy];
        }
        uint32_t U, V;
        if (CHROMA) {
            const long long co = (long long)by * j.c_step + bx;
            U = p0[co]; V = p1[co];
        } else {
            const uint8_t* uv = p0 + (long long)by * j.c_step + 2 * bx;
            U = uv[0]; V = uv[1];
        }
        int ruv, guv, buv;
        bt601_uv_terms(U, V, ruv, guv, buv);
        uint32_t b, g, r;
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        bt601_px_bgr(Y00, ruv, guv, buv, b, g, r); d0[B] = (uint8_t)b; d0[1] = (uint8_t)g; d0[R] = (uint8_t)r; d0[3] = 255;
        bt601_px_bgr(Y01, ruv, guv, buv, b, g, r); d0[4 + B] = (uint8_t)b; d0[5] = (uint8_t)g; d0[4 + R] = (uint8_t)r; d0[7] = 255;
        bt601_px_bgr(Y10, ruv, guv, buv, b, g, r); d1[B] = (uint8_t)b; d1[1] = (uint8_t)g; d1[R] = (uint8_t)r; d1[3] = 255;
        bt601_px_bgr(Y11, ruv, guv, buv, b, g, r); d1[4 + B] = (uint8_t)b; d1[5] = (uint8_t)g; d1[4 + R] = (uint8_t)r; d1[7] = 255;
    }
}
template <int ORDER, int CHROMA, bool LUT>
__global__ __launch_bounds__(kThreads) void yuv420_to_bgra_kernel(Yuv420BgraJob j, const uint8_t* __restrict__ luts)
{
    yuv420_to_bgra_body<ORDER, CHROMA, LUT>(j, StridedYuv420Bgra{j}, luts);
}
// the same on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either walk -- a
// byte-path frame of a vector-shaped launch takes more steps
template <int ORDER, int CHROMA, bool LUT>
__global__ __launch_bounds__(kThreads) void yuv420_to_bgra_frames_kernel(Yuv420BgraList l, Yuv420BgraJob j, const uint8_t* __restrict__ luts)
{
    yuv420_to_bgra_body<ORDER, CHROMA, LUT>(j, TableYuv420Bgra{l, j}, luts);
}

// ---------------------------------------------------------------------------------------------
// CLAHE blend + decode: the body of yuv420_bgr_clahe_interp_kernel (pair-table fill into dynamic LDS, bands / sub-bands / column
// segments, clahe_vec16_f32<false>) with the chroma load of the template's layout, decode_store16_4 and dst = out + x0 * 4.
// grid = (bands*subs, n_frames, col_segments).  No byte path: taken for the common shape only (host: no REFLECT_101 padding,
// tile_w % 16 == 0, the alignment rule of yuv420_bgra_frame_vec for every frame, tiles_x + 1 <= kMaxPairsLdsF32, no clahe_fp_contract);
// everything else runs the planar CLAHE into scratch and the decode above.
// ---------------------------------------------------------------------------------------------
template <int ORDER, int CHROMA, class Frames>
__device__ __forceinline__ void yuv420_bgra_clahe_interp_body(const Yuv420BgraJob& j, const Frames& fr, const ClaheGeom& g,
                                                              const uint8_t* __restrict__ luts, int subs, int groups)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t quad[];
    f32x4* quadf = reinterpret_cast<f32x4*>(quad);
    const int t = threadIdx.x, f = (int)gridDim.y - 1 - (int)blockIdx.y;      // last-to-first, see clahe_interp_kernel
    const int band = blockIdx.x / subs, sub = blockIdx.x - band * subs;
    const int ty1u = band - 1;
    const int ty1 = max(ty1u, 0), ty2 = min(ty1u + 1, g.tiles_y - 1);
    const uint8_t* lf = luts + (size_t)f * g.tiles_x * g.tiles_y * 256;
    const uint8_t* l1 = lf + (size_t)ty1 * g.tiles_x * 256;
    const uint8_t* l2 = lf + (size_t)ty2 * g.tiles_x * 256;
    const int npairs = g.tiles_x + 1;
    for (int i = t; i < npairs * 256; i += kThreads) {
        const int pr = i >> 8, v = i & 255;
        const int ta = max(pr - 1, 0), tb = min(pr, g.tiles_x - 1);
        const f32x4 e = {(float)l1[ta * 256 + v], (float)l2[ta * 256 + v], (float)l1[tb * 256 + v], (float)l2[tb * 256 + v]};   // {a, c, b, d}
        quadf[i] = e;
    }
    __syncthreads();
    const int y_lo_band = (int)max(0LL, ((long long)(2 * band - 1) * g.tile_h) / 2 - kBandMargin);
    const int y_hi_band = (int)min((long long)g.height, ((long long)(2 * band + 1) * g.tile_h + 1) / 2 + kBandMargin);
    const int nrows = max(0, y_hi_band - y_lo_band);
    const int y_lo = y_lo_band + (int)((long long)nrows * sub / subs);
    const int y_hi = y_lo_band + (int)((long long)nrows * (sub + 1) / subs);
    const int phases = kThreads / groups;
    const int grp = t % groups, phase = t / groups;
    const int x0 = (blockIdx.z * groups + grp) * kInterpPx;
    if (phase >= phases || x0 >= g.width) return;
    f32x2 xw[kInterpPx];
    int poff[kInterpPx];
#pragma unroll
    for (int k = 0; k < kInterpPx; ++k) {
        const float txf = tile_coord<false>(x0 + k, g.inv_tw);
        const int tx1 = floor_f32_to_int(txf);
        const float xa = __fsub_rn(txf, (float)tx1);
        xw[k].x = __fsub_rn(1.0f, xa); xw[k].y = xa;
        int pr = tx1 + 1;
        pr = pr < 0 ? 0 : (pr > g.tiles_x ? g.tiles_x : pr);
        poff[k] = pr << 8;
    }
    const uint8_t* yp = fr.y_of(f) + x0;
    const uint8_t* p0 = fr.c0_of(f);
    const uint8_t* p1 = CHROMA ? fr.c1_of(f) : nullptr;
    uint8_t* dst = fr.out_of(f) + (long long)x0 * 4;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<false>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    for (int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases; y < ya_hi; y += phases) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(yp + (long long)y * j.y_step);
        const u32x4 uv = load_uv16<CHROMA>(p0, p1, (long long)(y >> 1) * j.c_step, x0);
        const float tyf = tile_coord<false>(y, g.inv_th);
        const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
        const u32x4 yo = clahe_vec16_f32<false>(quadf, q, poff, xw, ya, ya1);       // the host takes the fallback for ClaheGeom::contract
        decode_store16_4<ORDER>(dst + (long long)y * j.out_step, yo, uv);
    }
}
template <int ORDER, int CHROMA>
__global__ __launch_bounds__(kThreads) void yuv420_bgra_clahe_interp_kernel(Yuv420BgraJob j, ClaheGeom g, const uint8_t* __restrict__ luts, int subs,
                                                                           int groups)
{
    yuv420_bgra_clahe_interp_body<ORDER, CHROMA>(j, StridedYuv420Bgra{j}, g, luts, subs, groups);
}
// the same on a frame list.  The host takes this kernel only when every frame of the call passes yuv420_bgra_frame_vec.
template <int ORDER, int CHROMA>
__global__ __launch_bounds__(kThreads) void yuv420_bgra_clahe_interp_frames_kernel(Yuv420BgraList l, Yuv420BgraJob j, ClaheGeom g,
                                                                                  const uint8_t* __restrict__ luts, int subs, int groups)
{
    yuv420_bgra_clahe_interp_body<ORDER, CHROMA>(j, TableYuv420Bgra{l, j}, g, luts, subs, groups);
}
// yuv420_bgra_clahe_interp_frames_kernel(l, j, g, luts, subs, groups) is the longer list of the two; 256: the implicit arguments a code
// object carries behind the explicit ones
static_assert(sizeof(Yuv420BgraList) == (size_t)kFramesPerLaunch * 32 && sizeof(Yuv420BgraList) <= 2048, "the table is at most 2 KiB");
static_assert(sizeof(Yuv420BgraList) + sizeof(Yuv420BgraJob) + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 2 * sizeof(int) + 8 + 256 <= 4096,
              "the table and the remaining arguments of either *_frames_kernel stay below HIP's 4 KiB of kernel arguments");
static_assert(sizeof(Yuv420BgraList) + sizeof(Yuv420BgraJob) + sizeof(const uint8_t*) + 8 + 256 <= 4096, "yuv420_to_bgra_frames_kernel's arguments");

}  // namespace mi
