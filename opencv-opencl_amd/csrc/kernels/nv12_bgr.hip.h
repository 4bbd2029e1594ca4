// nv12_bgr.hip.h -- NV12 frames in, interleaved 8-bit BGR / RGB out, in the pass that maps the luma
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"
#include "clahe.hip.h"
#include "color.hip.h"

namespace mi {
// =============================================================================================
// cv::equalizeHist / CLAHE::apply on the Y plane of an NV12 frame, then cv::cvtColor(COLOR_YUV2BGR_NV12) (or the RGB order): what
// mi_*_nv12_batch_dev(MI_UV_COPY) followed by mi_cvt_color_420_u8_batch_dev(MI_COLOR_YUV2BGR_NV12) writes in two calls and 8.5 B/px
// (4 + 4.5), here in 5.5 B/px: Y read twice (histograms, then map), UV read once, 3 B/px written; no intermediate NV12 batch.
// Y is a plane, so the histogram stages are the planar kernels unchanged (hist_partial_kernel -> equalize_lut_kernel; tile_hist*).  Only
// the two pixel-writing stages are new: the decode of color.hip.h (bt601_uv_terms / bt601_px_bgr / store_bgr16, the arithmetic of
// cvt420_kernel<1>) behind the LUT gather of lut_apply_kernel and behind the blend of clahe_interp_kernel.
// ORDER 0: B, G, R in memory (MI_ORDER_BGR); 1: R, G, B (MI_ORDER_RGB).
// =============================================================================================
struct Nv12BgrJob {
    const uint8_t* y; const uint8_t* uv;      // Y plane: H rows of W bytes; UV plane: H/2 rows of W bytes (interleaved U, V)
    uint8_t* out;                             // H rows of 3*W bytes
    long long y_step, uv_step, out_step;      // bytes between rows
    long long y_frame, uv_frame, out_frame;   // bytes between frames (the Y planes of the two-pass fallback lie in scratch: a stride of their own)
    int width, height;                        // both even
    int vec;                                  // 1: W % 16 == 0 and every base / pitch / frame stride a multiple of 16 -> 16 x 2 pixel groups
};

// Where frame f of a launch lives, as StridedFrames / TableFrames (common.hip.h) say it for the planar kernels: the bodies below are
// templates on one of these two policies.  The batch entries wrap them with the strided one -- the arithmetic they always had, on the
// kernel's own argument -- the *_frames_kernel entries with the table.
struct StridedNv12Bgr {
    const Nv12BgrJob& j;
    __device__ __forceinline__ const uint8_t* y_of(long long f) const { return j.y + f * j.y_frame; }
    __device__ __forceinline__ const uint8_t* uv_of(long long f) const { return j.uv + f * j.uv_frame; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return j.out + f * j.out_frame; }
    __device__ __forceinline__ bool vec(long long) const { return j.vec; }              // decided by the host for the whole launch
};

// A list of such frames, each at its own three addresses (mi_*_nv12_to_bgr_frames_dev: a decoder's surface pool in, an image pool
// out).  The {y, uv, out} entries travel BY VALUE in the kernel arguments like FrameList -- 64 x 24 B = 1.5 KiB -- and are read with
// scalar kernarg loads indexed by the frame's grid coordinate.  The shape (pitches, width, height) is the launch's Nv12BgrJob, whose
// y / uv / out / *_frame a table launch ignores and whose vec says what the SHAPE allows (W % 16 == 0, the three pitches multiples of
// 16): whether frame f takes the 16 x 2 groups is then decided by its own three addresses -- per frame, so uniform for a workgroup.
struct Nv12BgrFrame { const uint8_t* y; const uint8_t* uv; uint8_t* out; };
struct Nv12BgrList { Nv12BgrFrame f[kFramesPerLaunch]; };
static_assert(sizeof(Nv12BgrFrame) == 24, "three addresses an entry");
struct TableNv12Bgr {
    const Nv12BgrList& l;
    const Nv12BgrJob& j;
    __device__ __forceinline__ const uint8_t* y_of(long long f) const { return l.f[f].y; }
    __device__ __forceinline__ const uint8_t* uv_of(long long f) const { return l.f[f].uv; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return l.f[f].out; }
    __device__ __forceinline__ bool vec(long long f) const
    {
        return j.vec && (((uintptr_t)l.f[f].y | (uintptr_t)l.f[f].uv | (uintptr_t)l.f[f].out) & 15) == 0;
    }
};

template <int ORDER>
__device__ __forceinline__ void store_px16(uint8_t* p, const uint32_t* b, const uint32_t* g, const uint32_t* r)
{
    if (ORDER == 0) store_bgr16(p, b, g, r); else store_bgr16(p, r, g, b);
}

// 16 luma bytes (already mapped) + the 8 U,V pairs above / below them -> 16 pixels, 48 bytes at p (16-byte aligned)
template <int ORDER>
__device__ __forceinline__ void decode_store16(uint8_t* p, const u32x4& y, const u32x4& uv)
{
    uint32_t b[16], g[16], r[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int ruv, guv, buv;
        bt601_uv_terms(byte_of(uv, 2 * k), byte_of(uv, 2 * k + 1), ruv, guv, buv);
        bt601_px_bgr(byte_of(y, 2 * k), ruv, guv, buv, b[2 * k], g[2 * k], r[2 * k]);
        bt601_px_bgr(byte_of(y, 2 * k + 1), ruv, guv, buv, b[2 * k + 1], g[2 * k + 1], r[2 * k + 1]);
    }
    store_px16<ORDER>(p, b, g, r);
}

// ---------------------------------------------------------------------------------------------
// LUT apply + decode (equalizeHist), and with LUT = false the decode alone (second pass of the CLAHE fallback, whose Y planes are the
// planar CLAHE's output in scratch).  grid = (B, n_frames), 256 threads.  LDS: lut[value][32] replicated as in lut_apply_kernel, so
// the gather is bank-conflict free whatever the pixel values are.
// vec: a lane owns a 16 x 2 pixel group -- two 16-byte Y loads, one 16-byte UV load, six 16-byte stores (as cvt420_kernel<1>);
// otherwise a 2 x 2 block with byte accesses.  Only the 3*W bytes of each output row are written.
// ---------------------------------------------------------------------------------------------
template <int ORDER, bool LUT, class Frames>
__device__ __forceinline__ void nv12_to_bgr_body(const Nv12BgrJob& j, const Frames& fr, const uint8_t* __restrict__ luts)
{
    __shared__ uint32_t lut[LUT ? 256 * kCopies : 1];
    const int t = threadIdx.x;
    // LUT: frames last-to-first, the histogram pass streamed the batch first-to-last and its tail is still in the Infinity Cache;
    // decode alone: first-to-last, the interpolation before it walked last-to-first
    const int f = LUT ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;
    const uint32_t copy = t & (kCopies - 1);
    if (LUT) {
        const uint32_t v = luts[(size_t)f * 256 + t];
#pragma unroll
        for (int k = 0; k < kCopies; ++k) lut[(t << kCopyShift) + ((k + t) & (kCopies - 1))] = v;
        __syncthreads();
    }
    const uint8_t* yp = fr.y_of(f);
    const uint8_t* uvp = fr.uv_of(f);
    uint8_t* op = fr.out_of(f);
    if (fr.vec(f)) {
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
            const u32x4 uv = *reinterpret_cast<const u32x4*>(uvp + (long long)by * j.uv_step + (gx << 4));
            if (LUT) { y0 = lut_vec(lut, y0, copy); y1 = lut_vec(lut, y1, copy); }
            uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 48 * gx;
            decode_store16<ORDER>(d0, y0, uv);
            decode_store16<ORDER>(d0 + j.out_step, y1, uv);
        }
        return;
    }
    const int bx_n = j.width >> 1;
    const long long blocks = (long long)bx_n * (j.height >> 1);
    for (long long bi = (long long)blockIdx.x * kThreads + t; bi < blocks; bi += (long long)gridDim.x * kThreads) {
        const int by = (int)(bi / bx_n), bx = (int)(bi - (long long)by * bx_n);
        const uint8_t* r0 = yp + (long long)(2 * by) * j.y_step + 2 * bx;
        const uint8_t* r1 = r0 + j.y_step;
        const uint8_t* uv = uvp + (long long)by * j.uv_step + 2 * bx;
        uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 6 * bx;
        uint8_t* d1 = d0 + j.out_step;
        uint32_t Y00 = r0[0], Y01 = r0[1], Y10 = r1[0], Y11 = r1[1];
        if (LUT) {
            Y00 = lut[(Y00 << kCopyShift) + copy]; Y01 = lut[(Y01 << kCopyShift) + copy];
            Y10 = lut[(Y10 << kCopyShift) + copy]; Y11 = lut[(Y11 << kCopyShift) + copy];
        }
        int ruv, guv, buv;
        bt601_uv_terms(uv[0], uv[1], ruv, guv, buv);
        uint32_t b, g, r;
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        bt601_px_bgr(Y00, ruv, guv, buv, b, g, r); d0[B] = (uint8_t)b; d0[1] = (uint8_t)g; d0[R] = (uint8_t)r;
        bt601_px_bgr(Y01, ruv, guv, buv, b, g, r); d0[3 + B] = (uint8_t)b; d0[4] = (uint8_t)g; d0[3 + R] = (uint8_t)r;
        bt601_px_bgr(Y10, ruv, guv, buv, b, g, r); d1[B] = (uint8_t)b; d1[1] = (uint8_t)g; d1[R] = (uint8_t)r;
        bt601_px_bgr(Y11, ruv, guv, buv, b, g, r); d1[3 + B] = (uint8_t)b; d1[4] = (uint8_t)g; d1[3 + R] = (uint8_t)r;
    }
}
template <int ORDER, bool LUT>
__global__ __launch_bounds__(kThreads) void nv12_to_bgr_kernel(Nv12BgrJob j, const uint8_t* __restrict__ luts)
{
    nv12_to_bgr_body<ORDER, LUT>(j, StridedNv12Bgr{j}, luts);
}
// the same on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either kind
template <int ORDER, bool LUT>
__global__ __launch_bounds__(kThreads) void nv12_to_bgr_frames_kernel(Nv12BgrList l, Nv12BgrJob j, const uint8_t* __restrict__ luts)
{
    nv12_to_bgr_body<ORDER, LUT>(j, TableNv12Bgr{l, j}, luts);
}

// ---------------------------------------------------------------------------------------------
// CLAHE blend + decode: the bands, sub-bands, column segments, f32 pair tables and rounding of clahe_interp_kernel<true, false> /
// bgr_clahe_interp_kernel; a lane's 16 blended luma bytes meet the 8 U,V pairs of chroma row y >> 1 and leave as 48 bytes.  Rows 2r
// and 2r+1 may belong to different bands (and workgroups): each loads its own chroma.  grid = (bands*subs, n_frames, col_segments).
// Taken for the common shape only (host: no REFLECT_101 padding, tile_w % 16 == 0, every base / pitch / stride a multiple of 16,
// tiles_x + 1 <= kMaxPairsLdsF32, no clahe_fp_contract); everything else runs the planar CLAHE into scratch and the decode above.
// ---------------------------------------------------------------------------------------------
template <int ORDER>
__global__ __launch_bounds__(kThreads) void nv12_bgr_clahe_interp_kernel(Nv12BgrJob j, ClaheGeom g, const uint8_t* __restrict__ luts, int subs, int groups)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t quad[];
    f32x4* quadf = reinterpret_cast<f32x4*>(quad);
    // A copy of interp_stage<true, false> (clahe.hip.h) without the column-segment window, then of the column weights and the row
    // trim: calling interp_stage here changed this kernel's table fill loop, so the copy stays; a change there is made here too.
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
    const uint8_t* yp = j.y + (long long)f * j.y_frame + x0;
    const uint8_t* uvp = j.uv + (long long)f * j.uv_frame + x0;            // pair k of the group: bytes x0 + 2k, x0 + 2k + 1 of the UV row
    uint8_t* dst = j.out + (long long)f * j.out_frame + (long long)x0 * 3;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<false>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    auto do_row = [&](int y, const u32x4& yq, const u32x4& uv) {
        const float tyf = tile_coord<false>(y, g.inv_th);
        const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
        const u32x4 yo = clahe_vec16_f32<false>(quadf, yq, poff, xw, ya, ya1);       // the host takes the fallback for ClaheGeom::contract
        decode_store16<ORDER>(dst + (long long)y * j.out_step, yo, uv);
    };
    for (int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases; y < ya_hi; y += phases) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(yp + (long long)y * j.y_step);
        const u32x4 uv = *reinterpret_cast<const u32x4*>(uvp + (long long)(y >> 1) * j.uv_step);
        do_row(y, q, uv);
    }
}
// The same kernel on a frame list, and a COPY of it: a body shared through the frame policy, as nv12_to_bgr_body is, was tried and
// changed the table fill loop of the kernel above the way calling interp_stage had (other address arithmetic in the loop's preheader,
// whether the whole body or only the rows behind the barrier went through the shared function), so that kernel keeps its
// text and this one repeats it with frame f's addresses read from the table: a change there is made here too.  No byte path: the host
// takes this kernel only when every address of every frame of the call is a multiple of 16.
template <int ORDER>
__global__ __launch_bounds__(kThreads) void nv12_bgr_clahe_interp_frames_kernel(Nv12BgrList l, Nv12BgrJob j, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                               int subs, int groups)
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
    const TableNv12Bgr fr{l, j};
    const uint8_t* yp = fr.y_of(f) + x0;
    const uint8_t* uvp = fr.uv_of(f) + x0;
    uint8_t* dst = fr.out_of(f) + (long long)x0 * 3;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<false>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    auto do_row = [&](int y, const u32x4& yq, const u32x4& uv) {
        const float tyf = tile_coord<false>(y, g.inv_th);
        const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
        const u32x4 yo = clahe_vec16_f32<false>(quadf, yq, poff, xw, ya, ya1);       // the host takes the fallback for ClaheGeom::contract
        decode_store16<ORDER>(dst + (long long)y * j.out_step, yo, uv);
    };
    for (int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases; y < ya_hi; y += phases) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(yp + (long long)y * j.y_step);
        const u32x4 uv = *reinterpret_cast<const u32x4*>(uvp + (long long)(y >> 1) * j.uv_step);
        do_row(y, q, uv);
    }
}
// nv12_bgr_clahe_interp_frames_kernel(l, j, g, luts, subs, groups) is the longer list of the two; 256: the implicit arguments a code
// object carries behind the explicit ones
static_assert(sizeof(Nv12BgrList) + sizeof(Nv12BgrJob) + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 2 * sizeof(int) + 8 + 256 <= 4096,
              "the table and the remaining arguments of either *_frames_kernel stay below HIP's 4 KiB of kernel arguments");
static_assert(sizeof(Nv12BgrList) + sizeof(Nv12BgrJob) + sizeof(const uint8_t*) + 8 + 256 <= 4096, "nv12_to_bgr_frames_kernel's arguments");

}  // namespace mi
