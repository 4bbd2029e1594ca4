// yuv420_bgr.hip.h -- planar 4:2:0 frames (I420 / YV12) in, interleaved 8-bit BGR / RGB out, in the pass that maps the luma
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "nv12_bgr.hip.h"
#include "yuv420.hip.h"

namespace mi {
// =============================================================================================
// cv::equalizeHist / CLAHE::apply on the Y plane of an I420 / YV12 frame, then cv::cvtColor(COLOR_YUV2BGR_I420 / _YV12) (or the RGB
// order): what mi_*_nv12_to_bgr* writes for the same pixels with U and V interleaved, from a software decoder's three planes.  The
// histogram stages are the planar kernels (Y is a plane).  The two pixel-writing stages are those of nv12_bgr.hip.h with the chroma
// load replaced: a 16-pixel group needs 8 U bytes and 8 V bytes -- one 8-byte load from each plane where the NV12 kernels make one
// 16-byte load -- zipped in registers (kZipLo / kZipHi of yuv420.hip.h, four v_perm_b32) into the u32x4 of U, V pairs that
// decode_store16 takes.  5.5 B/px as the NV12 form: Y read twice, U and V once, 3 B/px written.
// The NV12 kernels keep their text (the bodies below are written out, not shared through a chroma-load policy), so their ISA is what it
// was: DESIGN.md §9 has the comparison.
// u is always the U (Cb) plane and v the V (Cr) plane; a YV12 frame is the same planes at exchanged addresses, decided by the caller.
// =============================================================================================
struct Yuv420BgrJob {
    const uint8_t* y; const uint8_t* u; const uint8_t* v;    // Y: H rows of W bytes; U, V: H/2 rows of W/2 bytes each
    uint8_t* out;                                            // H rows of 3*W bytes
    long long y_step, c_step, out_step;                      // bytes between rows (both chroma planes share theirs)
    long long y_frame, c_frame, out_frame;                   // bytes between frames (the Y planes of the two-pass fallback lie in scratch: a stride of their own)
    int width, height;                                       // both even
    int vec;                                                 // 1: W % 16 == 0, the Y and output terms multiples of 16, the chroma terms of 8 -> 16 x 2 pixel groups
};

// 8 U bytes and 8 V bytes -> the 8 U, V pairs of a 16-pixel group, as an NV12 row holds them
__device__ __forceinline__ u32x4 zip_uv8(const uint2 u, const uint2 v)
{
    u32x4 uv;
    uv.x = __builtin_amdgcn_perm(v.x, u.x, kZipLo); uv.y = __builtin_amdgcn_perm(v.x, u.x, kZipHi);
    uv.z = __builtin_amdgcn_perm(v.y, u.y, kZipLo); uv.w = __builtin_amdgcn_perm(v.y, u.y, kZipHi);
    return uv;
}

// ---------------------------------------------------------------------------------------------
// LUT apply + decode (equalizeHist), and with LUT = false the decode alone (second pass of the CLAHE fallback): the grid, the walk and
// the LDS LUT of nv12_to_bgr_body.  grid = (B, n_frames), 256 threads.
// vec: a lane owns a 16 x 2 pixel group -- two 16-byte Y loads, one 8-byte U load, one 8-byte V load, six 16-byte stores; otherwise a
// 2 x 2 block with byte accesses (one U byte, one V byte).  Only the 3*W bytes of each output row are written.
// ---------------------------------------------------------------------------------------------
template <int ORDER, bool LUT>
__global__ __launch_bounds__(kThreads) void yuv420_to_bgr_kernel(Yuv420BgrJob j, const uint8_t* __restrict__ luts)
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
    const uint8_t* yp = j.y + (long long)f * j.y_frame;
    const uint8_t* up = j.u + (long long)f * j.c_frame;
    const uint8_t* vp = j.v + (long long)f * j.c_frame;
    uint8_t* op = j.out + (long long)f * j.out_frame;
    if (j.vec) {
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
            const long long co = (long long)by * j.c_step + (gx << 3);
            const u32x4 uv = zip_uv8(*reinterpret_cast<const uint2*>(up + co), *reinterpret_cast<const uint2*>(vp + co));
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
        const long long co = (long long)by * j.c_step + bx;
        uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 6 * bx;
        uint8_t* d1 = d0 + j.out_step;
        uint32_t Y00 = r0[0], Y01 = r0[1], Y10 = r1[0], Y11 = r1[1];
        if (LUT) {
            Y00 = lut[(Y00 << kCopyShift) + copy]; Y01 = lut[(Y01 << kCopyShift) + copy];
            Y10 = lut[(Y10 << kCopyShift) + copy]; Y11 = lut[(Y11 << kCopyShift) + copy];
        }
        int ruv, guv, buv;
        bt601_uv_terms(up[co], vp[co], ruv, guv, buv);
        uint32_t b, g, r;
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        bt601_px_bgr(Y00, ruv, guv, buv, b, g, r); d0[B] = (uint8_t)b; d0[1] = (uint8_t)g; d0[R] = (uint8_t)r;
        bt601_px_bgr(Y01, ruv, guv, buv, b, g, r); d0[3 + B] = (uint8_t)b; d0[4] = (uint8_t)g; d0[3 + R] = (uint8_t)r;
        bt601_px_bgr(Y10, ruv, guv, buv, b, g, r); d1[B] = (uint8_t)b; d1[1] = (uint8_t)g; d1[R] = (uint8_t)r;
        bt601_px_bgr(Y11, ruv, guv, buv, b, g, r); d1[3 + B] = (uint8_t)b; d1[4] = (uint8_t)g; d1[3 + R] = (uint8_t)r;
    }
}

// ---------------------------------------------------------------------------------------------
// CLAHE blend + decode, planar chroma: a COPY of nv12_bgr_clahe_interp_kernel (nv12_bgr.hip.h) with its one chroma load replaced by
// two 8-byte loads at x0 / 2 of chroma row y >> 1, zipped.  A shared body changed that kernel's table fill loop, so it
// keeps its text and this one repeats it: a change there is made here too.  grid = (bands*subs, n_frames, col_segments).
// Taken for the common shape only (host: no REFLECT_101 padding, tile_w % 16 == 0, the Y and output terms multiples of 16 and the
// chroma terms of 8, tiles_x + 1 <= kMaxPairsLdsF32, no clahe_fp_contract); everything else runs the planar CLAHE into scratch and the
// decode above.
// ---------------------------------------------------------------------------------------------
template <int ORDER>
__global__ __launch_bounds__(kThreads) void yuv420_bgr_clahe_interp_kernel(Yuv420BgrJob j, ClaheGeom g, const uint8_t* __restrict__ luts, int subs, int groups)
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
    const uint8_t* yp = j.y + (long long)f * j.y_frame + x0;
    const uint8_t* up = j.u + (long long)f * j.c_frame + (x0 >> 1);        // sample k of the group: byte x0 / 2 + k of the U and of the V row
    const uint8_t* vp = j.v + (long long)f * j.c_frame + (x0 >> 1);
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
        const long long co = (long long)(y >> 1) * j.c_step;
        const u32x4 uv = zip_uv8(*reinterpret_cast<const uint2*>(up + co), *reinterpret_cast<const uint2*>(vp + co));
        do_row(y, q, uv);
    }
}

// =============================================================================================
// The same two stages on a LIST of frames, each at its own four addresses (mi_*_yuv420_to_bgr_frames_dev: a software decoder's frame
// pool in -- three separately allocated planes a frame -- an image pool out).  The {y, u, v, out} entries travel BY VALUE in the kernel
// arguments like Nv12BgrList -- 64 x 32 B = 2 KiB -- and are read with scalar kernarg loads indexed by the frame's grid coordinate.
// The shape (pitches, width, height) is the launch's Yuv420BgrJob, whose y / u / v / out / *_frame a table launch ignores and whose vec
// says what the SHAPE allows (W % 16 == 0, the Y and output pitches multiples of 16, the chroma pitch of 8): whether frame f takes the
// 16 x 2 groups is then decided by its own four addresses -- per frame, so uniform for a workgroup.
// Both kernels are COPIES of the two above with the frame's addresses read from the table, so that those keep their ISA:
// a change there is made here too.
// =============================================================================================
struct Yuv420BgrFrame { const uint8_t* y; const uint8_t* u; const uint8_t* v; uint8_t* out; };
struct Yuv420BgrList { Yuv420BgrFrame f[kFramesPerLaunch]; };
static_assert(sizeof(Yuv420BgrFrame) == 32, "four addresses an entry");

// THE rule "does this frame of a list take the 16 x 2 groups": what the shape allows, and the frame's own Y and image addresses
// multiples of 16, its U and V addresses of 8.  The kernel decides by it and the host counts by it.
__host__ __device__ __forceinline__ bool yuv420_bgr_frame_vec(int shape_vec, const void* y, const void* u, const void* v, const void* out)
{
    return shape_vec && ((((uintptr_t)y | (uintptr_t)out) & 15) | (((uintptr_t)u | (uintptr_t)v) & 7)) == 0;
}

// yuv420_to_bgr_kernel on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of either walk
template <int ORDER, bool LUT>
__global__ __launch_bounds__(kThreads) void yuv420_to_bgr_frames_kernel(Yuv420BgrList l, Yuv420BgrJob j, const uint8_t* __restrict__ luts)
{
    __shared__ uint32_t lut[LUT ? 256 * kCopies : 1];
    const int t = threadIdx.x;
    const int f = LUT ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;      // frame order as yuv420_to_bgr_kernel
    const uint32_t copy = t & (kCopies - 1);
    if (LUT) {
        const uint32_t v = luts[(size_t)f * 256 + t];
#pragma unroll
        for (int k = 0; k < kCopies; ++k) lut[(t << kCopyShift) + ((k + t) & (kCopies - 1))] = v;
        __syncthreads();
    }
    const uint8_t* yp = l.f[f].y;
    const uint8_t* up = l.f[f].u;
    const uint8_t* vp = l.f[f].v;
    uint8_t* op = l.f[f].out;
    if (yuv420_bgr_frame_vec(j.vec, yp, up, vp, op)) {
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
            const long long co = (long long)by * j.c_step + (gx << 3);
            const u32x4 uv = zip_uv8(*reinterpret_cast<const uint2*>(up + co), *reinterpret_cast<const uint2*>(vp + co));
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
        const long long co = (long long)by * j.c_step + bx;
        uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 6 * bx;
        uint8_t* d1 = d0 + j.out_step;
        uint32_t Y00 = r0[0], Y01 = r0[1], Y10 = r1[0], Y11 = r1[1];
        if (LUT) {
            Y00 = lut[(Y00 << kCopyShift) + copy]; Y01 = lut[(Y01 << kCopyShift) + copy];
            Y10 = lut[(Y10 << kCopyShift) + copy]; Y11 = lut[(Y11 << kCopyShift) + copy];
        }
        int ruv, guv, buv;
        bt601_uv_terms(up[co], vp[co], ruv, guv, buv);
        uint32_t b, g, r;
        constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
        bt601_px_bgr(Y00, ruv, guv, buv, b, g, r); d0[B] = (uint8_t)b; d0[1] = (uint8_t)g; d0[R] = (uint8_t)r;
        bt601_px_bgr(Y01, ruv, guv, buv, b, g, r); d0[3 + B] = (uint8_t)b; d0[4] = (uint8_t)g; d0[3 + R] = (uint8_t)r;
        bt601_px_bgr(Y10, ruv, guv, buv, b, g, r); d1[B] = (uint8_t)b; d1[1] = (uint8_t)g; d1[R] = (uint8_t)r;
        bt601_px_bgr(Y11, ruv, guv, buv, b, g, r); d1[3 + B] = (uint8_t)b; d1[4] = (uint8_t)g; d1[3 + R] = (uint8_t)r;
    }
}

// yuv420_bgr_clahe_interp_kernel on a frame list.  No byte path: the host takes this kernel only when every frame of the call passes
// yuv420_bgr_frame_vec.
template <int ORDER>
__global__ __launch_bounds__(kThreads) void yuv420_bgr_clahe_interp_frames_kernel(Yuv420BgrList l, Yuv420BgrJob j, ClaheGeom g, const uint8_t* __restrict__ luts,
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
    const uint8_t* yp = l.f[f].y + x0;
    const uint8_t* up = l.f[f].u + (x0 >> 1);        // sample k of the group: byte x0 / 2 + k of the U and of the V row
    const uint8_t* vp = l.f[f].v + (x0 >> 1);
    uint8_t* dst = l.f[f].out + (long long)x0 * 3;
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
        const long long co = (long long)(y >> 1) * j.c_step;
        const u32x4 uv = zip_uv8(*reinterpret_cast<const uint2*>(up + co), *reinterpret_cast<const uint2*>(vp + co));
        do_row(y, q, uv);
    }
}
// yuv420_bgr_clahe_interp_frames_kernel(l, j, g, luts, subs, groups) is the longer list of the two; 256: the implicit arguments a code
// object carries behind the explicit ones
static_assert(sizeof(Yuv420BgrList) == (size_t)kFramesPerLaunch * 32 && sizeof(Yuv420BgrList) <= 2048, "the table is at most 2 KiB");
static_assert(sizeof(Yuv420BgrList) + sizeof(Yuv420BgrJob) + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 2 * sizeof(int) + 8 + 256 <= 4096,
              "the table and the remaining arguments of either *_frames_kernel stay below HIP's 4 KiB of kernel arguments");
static_assert(sizeof(Yuv420BgrList) + sizeof(Yuv420BgrJob) + sizeof(const uint8_t*) + 8 + 256 <= 4096, "yuv420_to_bgr_frames_kernel's arguments");

}  // namespace mi
