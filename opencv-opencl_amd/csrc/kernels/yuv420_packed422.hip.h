// yuv420_packed422.hip.h -- 4:2:0 frames (NV12, or planar I420 / YV12) in, pitched packed 4:2:2 frames (YUY2 / UYVY) out, in the pass that maps the luma
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "yuv420_bgr.hip.h"
#include "packed422.hip.h"

namespace mi {
// =============================================================================================
// cv::equalizeHist / CLAHE::apply on the Y plane of a 4:2:0 frame, written as a packed 4:2:2 frame -- the decoder-to-playout path: a
// hardware decoder's NV12 or a software decoder's three planes in, what SDI / HDMI playout cards, v4l2 output and loopback devices and
// virtual cameras take out: one dword per macropixel, Y0 U Y1 V (OFF = 0, MI_FMT_YUY2) or U Y0 V Y1 (OFF = 1, MI_FMT_UYVY).
// Y is a plane, so the histogram stages are the planar kernels unchanged (hist_partial_kernel -> equalize_lut_kernel; tile_hist*).  Only
// the two pixel-writing stages are new: those of nv12_bgr.hip.h / yuv420_bgr.hip.h with the 48-byte decode-and-store replaced by a
// 32-byte pack-and-store.  There is no arithmetic on the chroma: output rows 2r and 2r+1 both carry input chroma row r unchanged,
// macropixel k of both rows gets U[r][k], V[r][k] -- the chroma the decodes of nv12_bgr.hip.h / yuv420_bgr.hip.h apply to both rows of a
// pair, and what packed422_nv12.hip.h maps back to the same 4:2:0 chroma ((a + a + 1) >> 1 == a).  An NV12 chroma row U0 V0 U1 V1 ..
// is already the chroma a YUY2 row needs, so packing 16 pixels is a byte zip of the 16 mapped luma bytes with 16 UV bytes: eight
// v_perm_b32 (kZipLo / kZipHi of yuv420.hip.h).  Planar chroma is zipped into that row first (zip_uv8, four more).
// Bytes per pixel: equalizeHist 1 (histogram) + 1.5 read + 2 written = 4.5; one-pass CLAHE the same 4.5; the two-pass CLAHE fallback
// 6.5 (the planar CLAHE reads Y twice and writes it to scratch, then 1.5 read + 2 written here).
// PLANAR false: c0 is the interleaved UV plane (H/2 rows of W bytes), c1 unused; true: c0 the U (Cb) and c1 the V (Cr) plane (H/2 rows
// of W/2 bytes each) -- a YV12 frame is the same planes at exchanged addresses, decided by the caller.  copy_uv 0: every chroma byte
// 128 (MI_UV_FILL128) and no chroma is loaded.
// =============================================================================================
struct Yuv420P422Job {
    const uint8_t* y; const uint8_t* c0; const uint8_t* c1;  // Y: H rows of W bytes
    uint8_t* out;                                            // H rows of 2*W bytes (W/2 macropixel dwords); a multiple of 4, as out_step and out_frame
    long long y_step, c_step, out_step;                      // bytes between rows (both planar chroma planes share theirs)
    long long y_frame, c_frame, out_frame;                   // bytes between frames (the Y planes of the two-pass fallback lie in scratch: a stride of their own)
    int width, height;                                       // both even
    int vec;                                                 // 1: W % 16 == 0, the Y and output terms multiples of 16, the chroma terms of 16 (interleaved) or 8 (planar) -> 16 x 2 pixel groups
    int copy_uv;                                             // 0: MI_UV_FILL128, the chroma pointers are not dereferenced
};

constexpr uint32_t kChroma128 = 0x80808080u;

// 16 luma bytes (already mapped) + the 8 U,V pairs above / below them -> 8 macropixel dwords, 32 bytes at p (16-byte aligned)
template <int OFF>
__device__ __forceinline__ void pack_store16(uint8_t* p, const u32x4& y, const u32x4& uv)
{
    u32x4 o0, o1;
    if (OFF == 0) {                                          // Y0 U0 Y1 V0 | Y2 U1 Y3 V1: the luma word is the low one of the zip
        o0.x = __builtin_amdgcn_perm(uv.x, y.x, kZipLo); o0.y = __builtin_amdgcn_perm(uv.x, y.x, kZipHi);
        o0.z = __builtin_amdgcn_perm(uv.y, y.y, kZipLo); o0.w = __builtin_amdgcn_perm(uv.y, y.y, kZipHi);
        o1.x = __builtin_amdgcn_perm(uv.z, y.z, kZipLo); o1.y = __builtin_amdgcn_perm(uv.z, y.z, kZipHi);
        o1.z = __builtin_amdgcn_perm(uv.w, y.w, kZipLo); o1.w = __builtin_amdgcn_perm(uv.w, y.w, kZipHi);
    } else {                                                 // U0 Y0 V0 Y1 | U1 Y2 V1 Y3: the chroma word is the low one
        o0.x = __builtin_amdgcn_perm(y.x, uv.x, kZipLo); o0.y = __builtin_amdgcn_perm(y.x, uv.x, kZipHi);
        o0.z = __builtin_amdgcn_perm(y.y, uv.y, kZipLo); o0.w = __builtin_amdgcn_perm(y.y, uv.y, kZipHi);
        o1.x = __builtin_amdgcn_perm(y.z, uv.z, kZipLo); o1.y = __builtin_amdgcn_perm(y.z, uv.z, kZipHi);
        o1.z = __builtin_amdgcn_perm(y.w, uv.w, kZipLo); o1.w = __builtin_amdgcn_perm(y.w, uv.w, kZipHi);
    }
    *reinterpret_cast<u32x4*>(p) = o0;
    *reinterpret_cast<u32x4*>(p + 16) = o1;
}

// the 8 U,V pairs of the 16-pixel group at column x0 of a chroma row: `c0r` / `c1r` point at the row's first byte
template <bool PLANAR>
__device__ __forceinline__ u32x4 load_uv16(const uint8_t* c0r, const uint8_t* c1r, int x0)
{
    if (PLANAR) return zip_uv8(*reinterpret_cast<const uint2*>(c0r + (x0 >> 1)), *reinterpret_cast<const uint2*>(c1r + (x0 >> 1)));
    return *reinterpret_cast<const u32x4*>(c0r + x0);
}

// ---------------------------------------------------------------------------------------------
// LUT apply + pack (equalizeHist, MI_K_LUT_APPLY), and with LUT = false the pack alone (MI_K_COLOR: second pass of the CLAHE fallback,
// whose Y planes are the planar CLAHE's output in scratch): the grid, the grid-stride walk and the LDS LUT of nv12_to_bgr_body.
// grid = (B, n_frames), 256 threads.
// vec: a lane owns a 16 x 2 pixel group -- two 16-byte Y loads, one 16-byte UV load (interleaved) or two 8-byte loads + zip_uv8
// (planar), 32 LDS LUT reads through the kCopies table, four 16-byte stores: two per output row, both rows from the same chroma
// registers.  Otherwise a 2 x 2 block: byte loads and one aligned dword store per macropixel per row (the output is 4-aligned by
// contract).  Both paths give the same bytes.  Only the 2*W bytes of each output row are written.
// ---------------------------------------------------------------------------------------------
template <int OFF, bool PLANAR, bool LUT>
__global__ __launch_bounds__(kThreads) void yuv420_to_packed422_kernel(Yuv420P422Job j, const uint8_t* __restrict__ luts)
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
    const uint8_t* c0p = j.c0 + (long long)f * j.c_frame;      // not dereferenced unless copy_uv
    const uint8_t* c1p = j.c1 + (long long)f * j.c_frame;
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
            u32x4 uv = {kChroma128, kChroma128, kChroma128, kChroma128};
            if (j.copy_uv) {
                const long long co = (long long)by * j.c_step;
                uv = load_uv16<PLANAR>(c0p + co, c1p + co, gx << 4);
            }
            if (LUT) { y0 = lut_vec(lut, y0, copy); y1 = lut_vec(lut, y1, copy); }
            uint8_t* d0 = op + (long long)(2 * by) * j.out_step + (gx << 5);
            pack_store16<OFF>(d0, y0, uv);
            pack_store16<OFF>(d0 + j.out_step, y1, uv);
        }
        return;
    }
    // the chroma bytes of a dword: bytes 1 and 3 (OFF = 0) or 0 and 2 (OFF = 1); U is the lower of the two
    constexpr int kUShift = OFF ? 0 : 8, kVShift = kUShift + 16;
    const int bx_n = j.width >> 1;
    const long long blocks = (long long)bx_n * (j.height >> 1);
    for (long long bi = (long long)blockIdx.x * kThreads + t; bi < blocks; bi += (long long)gridDim.x * kThreads) {
        const int by = (int)(bi / bx_n), bx = (int)(bi - (long long)by * bx_n);
        const uint8_t* r0 = yp + (long long)(2 * by) * j.y_step + 2 * bx;
        const uint8_t* r1 = r0 + j.y_step;
        uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 4 * bx;
        uint32_t Y00 = r0[0], Y01 = r0[1], Y10 = r1[0], Y11 = r1[1];
        if (LUT) {
            Y00 = lut[(Y00 << kCopyShift) + copy]; Y01 = lut[(Y01 << kCopyShift) + copy];
            Y10 = lut[(Y10 << kCopyShift) + copy]; Y11 = lut[(Y11 << kCopyShift) + copy];
        }
        uint32_t U = 128, V = 128;
        if (j.copy_uv) {
            const long long co = (long long)by * j.c_step;
            if (PLANAR) { U = c0p[co + bx]; V = c1p[co + bx]; }
            else        { U = c0p[co + 2 * bx]; V = c0p[co + 2 * bx + 1]; }
        }
        const uint32_t cw = (U << kUShift) | (V << kVShift);
        *reinterpret_cast<uint32_t*>(d0) = put_y<OFF>(Y00, Y01) | cw;
        *reinterpret_cast<uint32_t*>(d0 + j.out_step) = put_y<OFF>(Y10, Y11) | cw;
    }
}

// ---------------------------------------------------------------------------------------------
// CLAHE blend + pack: a COPY of nv12_bgr_clahe_interp_kernel (nv12_bgr.hip.h) -- its bands, sub-bands, column segments, f32 pair
// tables and rounding -- with do_row ending in the pack.  A shared body changed that kernel's table fill loop, so it
// keeps its text and this one repeats it: a change there is made here too.  Rows 2r and 2r+1 may belong to different bands (and
// workgroups): each loads its own chroma row y >> 1.  grid = (bands*subs, n_frames, col_segments).
// Taken for the common shape only (host: no REFLECT_101 padding, tile_w % 16 == 0, the alignment of the 16 x 2 groups above,
// tiles_x + 1 <= kMaxPairsLdsF32, no clahe_fp_contract); everything else runs the planar CLAHE into scratch and the pack above.
// ---------------------------------------------------------------------------------------------
template <int OFF, bool PLANAR>
__global__ __launch_bounds__(kThreads) void yuv420_packed422_clahe_interp_kernel(Yuv420P422Job j, ClaheGeom g, const uint8_t* __restrict__ luts, int subs, int groups)
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
    const uint8_t* c0p = j.c0 + (long long)f * j.c_frame;      // not dereferenced unless copy_uv
    const uint8_t* c1p = j.c1 + (long long)f * j.c_frame;
    uint8_t* dst = j.out + (long long)f * j.out_frame + (long long)x0 * 2;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<false>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    auto do_row = [&](int y, const u32x4& yq, const u32x4& uv) {
        const float tyf = tile_coord<false>(y, g.inv_th);
        const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
        const u32x4 yo = clahe_vec16_f32<false>(quadf, yq, poff, xw, ya, ya1);       // the host takes the fallback for ClaheGeom::contract
        pack_store16<OFF>(dst + (long long)y * j.out_step, yo, uv);
    };
    for (int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases; y < ya_hi; y += phases) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(yp + (long long)y * j.y_step);
        u32x4 uv = {kChroma128, kChroma128, kChroma128, kChroma128};
        if (j.copy_uv) {
            const long long co = (long long)(y >> 1) * j.c_step;
            uv = load_uv16<PLANAR>(c0p + co, c1p + co, x0);
        }
        do_row(y, q, uv);
    }
}

// =============================================================================================
// The same two stages on a LIST of frames, each at its own four addresses (mi_*_yuv420_to_packed422_frames_dev: a decoder's surface
// pool in -- separately allocated, pitched Y, U and V (or UV) planes -- a playout or v4l2 buffer pool out).  The {y, c0, c1, out}
// entries travel BY VALUE in the kernel arguments like Yuv420BgrList -- 64 x 32 B = 2 KiB -- and are read with scalar kernarg loads
// indexed by the frame's grid coordinate.  The shape (pitches, width, height, copy_uv) is the launch's Yuv420P422Job, whose y / c0 / c1 /
// out / *_frame a table launch ignores and whose vec says what the SHAPE allows (W % 16 == 0, the Y and output pitches multiples of 16,
// under copy_uv the chroma pitch a multiple of 16 interleaved or 8 planar): whether frame f takes the 16 x 2 groups is then decided by
// its own addresses -- per frame, so uniform for a workgroup.  Interleaved entries carry c1 = nullptr, MI_UV_FILL128 entries c0 = c1 =
// nullptr (the host clears them): they are not dereferenced and decide nothing.
// Both kernels are COPIES of the two above with the frame's addresses read from the table, so that those keep their ISA:
// a change there is made here too.
// =============================================================================================
struct Yuv420P422Frame { const uint8_t* y; const uint8_t* c0; const uint8_t* c1; uint8_t* out; };
struct Yuv420P422List { Yuv420P422Frame f[kFramesPerLaunch]; };
static_assert(sizeof(Yuv420P422Frame) == 32, "four addresses an entry");

// THE rule "does this frame of a list take the 16 x 2 groups": what the shape allows, the frame's own Y and output addresses
// multiples of 16 and, under copy_uv only, its UV address a multiple of 16 (interleaved; c1 is not looked at) or its U and V addresses
// multiples of 8 (planar).  The kernel decides by it and the host counts by it.
__host__ __device__ __forceinline__ bool yuv420_packed422_frame_vec(int shape_vec, int copy_uv, bool planar, const void* y, const void* c0,
                                                                    const void* c1, const void* out)
{
    const uintptr_t c = !copy_uv ? 0 : planar ? (((uintptr_t)c0 | (uintptr_t)c1) & 7) : ((uintptr_t)c0 & 15);
    return shape_vec && ((((uintptr_t)y | (uintptr_t)out) & 15) | c) == 0;
}

// yuv420_to_packed422_kernel on a frame list: both loops are grid-stride, so one grid (sized by the shape alone) serves frames of
// either walk
template <int OFF, bool PLANAR, bool LUT>
__global__ __launch_bounds__(kThreads) void yuv420_to_packed422_frames_kernel(Yuv420P422List l, Yuv420P422Job j, const uint8_t* __restrict__ luts)
{
    __shared__ uint32_t lut[LUT ? 256 * kCopies : 1];
    const int t = threadIdx.x;
    const int f = LUT ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y;      // frame order as yuv420_to_packed422_kernel
    const uint32_t copy = t & (kCopies - 1);
    if (LUT) {
        const uint32_t v = luts[(size_t)f * 256 + t];
#pragma unroll
        for (int k = 0; k < kCopies; ++k) lut[(t << kCopyShift) + ((k + t) & (kCopies - 1))] = v;
        __syncthreads();
    }
    const uint8_t* yp = l.f[f].y;
    const uint8_t* c0p = l.f[f].c0;                            // not dereferenced unless copy_uv
    const uint8_t* c1p = l.f[f].c1;
    uint8_t* op = l.f[f].out;
    if (yuv420_packed422_frame_vec(j.vec, j.copy_uv, PLANAR, yp, c0p, c1p, op)) {
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
            u32x4 uv = {kChroma128, kChroma128, kChroma128, kChroma128};
            if (j.copy_uv) {
                const long long co = (long long)by * j.c_step;
                uv = load_uv16<PLANAR>(c0p + co, c1p + co, gx << 4);
            }
            if (LUT) { y0 = lut_vec(lut, y0, copy); y1 = lut_vec(lut, y1, copy); }
            uint8_t* d0 = op + (long long)(2 * by) * j.out_step + (gx << 5);
            pack_store16<OFF>(d0, y0, uv);
            pack_store16<OFF>(d0 + j.out_step, y1, uv);
        }
        return;
    }
    constexpr int kUShift = OFF ? 0 : 8, kVShift = kUShift + 16;
    const int bx_n = j.width >> 1;
    const long long blocks = (long long)bx_n * (j.height >> 1);
    for (long long bi = (long long)blockIdx.x * kThreads + t; bi < blocks; bi += (long long)gridDim.x * kThreads) {
        const int by = (int)(bi / bx_n), bx = (int)(bi - (long long)by * bx_n);
        const uint8_t* r0 = yp + (long long)(2 * by) * j.y_step + 2 * bx;
        const uint8_t* r1 = r0 + j.y_step;
        uint8_t* d0 = op + (long long)(2 * by) * j.out_step + 4 * bx;
        uint32_t Y00 = r0[0], Y01 = r0[1], Y10 = r1[0], Y11 = r1[1];
        if (LUT) {
            Y00 = lut[(Y00 << kCopyShift) + copy]; Y01 = lut[(Y01 << kCopyShift) + copy];
            Y10 = lut[(Y10 << kCopyShift) + copy]; Y11 = lut[(Y11 << kCopyShift) + copy];
        }
        uint32_t U = 128, V = 128;
        if (j.copy_uv) {
            const long long co = (long long)by * j.c_step;
            if (PLANAR) { U = c0p[co + bx]; V = c1p[co + bx]; }
            else        { U = c0p[co + 2 * bx]; V = c0p[co + 2 * bx + 1]; }
        }
        const uint32_t cw = (U << kUShift) | (V << kVShift);
        *reinterpret_cast<uint32_t*>(d0) = put_y<OFF>(Y00, Y01) | cw;
        *reinterpret_cast<uint32_t*>(d0 + j.out_step) = put_y<OFF>(Y10, Y11) | cw;
    }
}

// yuv420_packed422_clahe_interp_kernel on a frame list.  No byte path: the host takes this kernel only when every frame of the call
// passes yuv420_packed422_frame_vec.
template <int OFF, bool PLANAR>
__global__ __launch_bounds__(kThreads) void yuv420_packed422_clahe_interp_frames_kernel(Yuv420P422List l, Yuv420P422Job j, ClaheGeom g,
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
    const uint8_t* yp = l.f[f].y + x0;
    const uint8_t* c0p = l.f[f].c0;                            // not dereferenced unless copy_uv
    const uint8_t* c1p = l.f[f].c1;
    uint8_t* dst = l.f[f].out + (long long)x0 * 2;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<false>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    auto do_row = [&](int y, const u32x4& yq, const u32x4& uv) {
        const float tyf = tile_coord<false>(y, g.inv_th);
        const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
        const u32x4 yo = clahe_vec16_f32<false>(quadf, yq, poff, xw, ya, ya1);       // the host takes the fallback for ClaheGeom::contract
        pack_store16<OFF>(dst + (long long)y * j.out_step, yo, uv);
    };
    for (int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases; y < ya_hi; y += phases) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(yp + (long long)y * j.y_step);
        u32x4 uv = {kChroma128, kChroma128, kChroma128, kChroma128};
        if (j.copy_uv) {
            const long long co = (long long)(y >> 1) * j.c_step;
            uv = load_uv16<PLANAR>(c0p + co, c1p + co, x0);
        }
        do_row(y, q, uv);
    }
}
// yuv420_packed422_clahe_interp_frames_kernel(l, j, g, luts, subs, groups) is the longer list of the two; 256: the implicit arguments a
// code object carries behind the explicit ones
static_assert(sizeof(Yuv420P422List) == (size_t)kFramesPerLaunch * 32 && sizeof(Yuv420P422List) <= 2048, "the table is at most 2 KiB");
static_assert(sizeof(Yuv420P422List) + sizeof(Yuv420P422Job) + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 2 * sizeof(int) + 8 + 256 <= 4096,
              "the table and the remaining arguments of either *_frames_kernel stay below HIP's 4 KiB of kernel arguments");
static_assert(sizeof(Yuv420P422List) + sizeof(Yuv420P422Job) + sizeof(const uint8_t*) + 8 + 256 <= 4096,
              "yuv420_to_packed422_frames_kernel's arguments");

}  // namespace mi
