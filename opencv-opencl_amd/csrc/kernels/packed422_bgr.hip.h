// packed422_bgr.hip.h -- the pixel-WRITING stages of "packed 4:2:2 in (YUY2 / UYVY), interleaved 8-bit BGR / RGB out": LUT apply, CLAHE
// interpolation and its wide-grid fallback, each with the BT.601 decode behind it.  Part of the gfx950 kernel set of libmi_lumaeq (see
// ../lumaeq_kernels.hip.h for the design notes).
//
// The histogram stages are packed422.hip.h's own, unchanged (they only read).  What is new is what the second pass does with a lane's
// 16 columns: the 16 new luma bytes meet the 8 U,V pairs of the SAME eight dwords -- every row keeps its own chroma, nothing is shared
// or filtered vertically -- go through color.hip.h's integer decode (bt601_uv_terms / bt601_px_bgr: OpenCV 4.4's ITUR_BT_601, shift 20,
// the arithmetic of cvt420_kernel<1>) and leave as 48 bytes.  Here the chroma ORDER matters: OFF = 0 is exactly Y0 U Y1 V, OFF = 1
// exactly U Y0 V Y1 (a YVYU frame would come out with U and V swapped).
// Input rows start at multiples of 4 as in every packed form.  The output has no alignment rule.  `wide` (host: the output pointer, its
// pitch and its frame stride are multiples of 4; in a list, the pitch and the frame's own address): a lane's 48 bytes start at a multiple of 4 and leave as three unaligned-capable
// 16-byte stores, the ragged last group of a row (W % 16 != 0, 3 * n bytes) as dwords and at most one final 2-byte store.  Otherwise
// every byte is stored on its own: slower, the same bytes.  Nothing beyond byte 3 * W of any row is written.
// ORDER 0: B, G, R in memory (MI_ORDER_BGR); 1: R, G, B (MI_ORDER_RGB).
#pragma once
#include "packed422_nv12.hip.h"
#include "color.hip.h"

namespace mi {

// A batch of packed frames in, images out: frame f reads src + f * src_frame and writes out + f * out_frame.
struct Packed422Bgr {
    const uint8_t* src;
    uint8_t* out;
    long long src_step, out_step;
    long long src_frame, out_frame;
    int dwords, rows;                 // macropixels per row (W / 2), rows (H, any value >= 1)
    int wide;                         // 1: out, out_step and out_frame are multiples of 4 -> vector stores; 0: byte stores
                                      // (a table launch: out_step alone, each frame adds its own address -- Table422Bgr::wide_of)
};

// THE rule "does an image at these addresses take the wide stores", for every pixel form of packed input: its address is a multiple of
// 4, and so are the pitch and (a batch; a list passes 0) the frame stride.  The host fills `wide` and counts by it.
__host__ __device__ __forceinline__ bool packed422_image_wide(const void* out, long long out_step, long long out_frame)
{
    return (((uintptr_t)out | (uintptr_t)out_step | (uintptr_t)out_frame) & 3) == 0;
}

// Where frame f lives, and which store path it takes.  The bodies below are templates on such a policy, as packed422_nv12.hip.h's
// are: the batch kernels wrap them with the strided policy, the *_frames_kernel entries with the table.
struct Strided422Bgr {
    const Packed422Bgr& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return p.src + f * p.src_frame; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return p.out + f * p.out_frame; }
    __device__ __forceinline__ bool wide_of(long long) const { return p.wide != 0; }
};
// A list of frames, each at its own addresses (mi_*_packed422_to_bgr_frames_dev: a capture device's buffer pool in, an image pool out).
// An entry is packed422.hip.h's own {in, out} pair, so the table is its Packed422List -- by value in the kernel arguments, read with
// scalar loads indexed by the frame's grid coordinate -- and the chunks are those of the histogram stages.  The shape is the launch's
// Packed422Bgr, whose src / out / *_frame a table launch ignores and whose `wide` says only that out_step is a multiple of 4: each
// frame adds its own address.  The frame index is uniform across a workgroup, so the choice stays a scalar branch.
// clahe_interp422_bgr_frames_kernel(l, p, g, luts, subs, groups, pair_cap) is the longest list; 256: the implicit arguments
static_assert(sizeof(Packed422List) + sizeof(Packed422Bgr) + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 3 * sizeof(int) + 8 + 256 <= 4096,
              "the kernel arguments of a table launch stay within 4 KiB");
struct Table422Bgr {
    const Packed422List& l;
    const Packed422Bgr& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return l.f[f].out; }
    __device__ __forceinline__ bool wide_of(long long f) const { return p.wide != 0 && ((uintptr_t)l.f[f].out & 3) == 0; }
};

// 16 luma bytes (already mapped) and the 8 U,V pairs of the same macropixels -> the 48 bytes of 16 pixels as 12 dwords.  The decode of
// nv12_bgr.hip.h's decode_store16, packed pixel by pixel so that at most one pixel's three channels are live beside the 12 dwords.
template <int ORDER>
__device__ __forceinline__ void decode422_16(const u32x4& y, const u32x4& uv, uint32_t* w)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int ruv, guv, buv;
        bt601_uv_terms(byte_of(uv, 2 * k), byte_of(uv, 2 * k + 1), ruv, guv, buv);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int px = 2 * k + h;
            uint32_t b, g, r;
            bt601_px_bgr(byte_of(y, px), ruv, guv, buv, b, g, r);
            const uint32_t c0 = ORDER == 0 ? b : r, c2 = ORDER == 0 ? r : b;
            w[(3 * px) >> 2] |= c0 << (8 * ((3 * px) & 3));
            w[(3 * px + 1) >> 2] |= g << (8 * ((3 * px + 1) & 3));
            w[(3 * px + 2) >> 2] |= c2 << (8 * ((3 * px + 2) & 3));
        }
    }
}

// The first 3 * n bytes of w (n pixels, n even, 2 <= n <= 16) to p.  wide: p is a multiple of 4.  Every index into w is a compile-time
// constant (the loops are unrolled and predicated), so w stays in registers.
__device__ __forceinline__ void store422_px(uint8_t* p, const uint32_t* w, int n, bool wide)
{
    if (wide) {
        if (n == 16) {
            u32x4_u* dp = reinterpret_cast<u32x4_u*>(p);
            const u32x4 r0 = {w[0], w[1], w[2], w[3]}, r1 = {w[4], w[5], w[6], w[7]}, r2 = {w[8], w[9], w[10], w[11]};
            dp[0] = r0; dp[1] = r1; dp[2] = r2;
            return;
        }
        const int bytes = 3 * n, nd = bytes >> 2;                // bytes is even: whole dwords, then 0 or 2 bytes
#pragma unroll
        for (int k = 0; k < 11; ++k) {                            // n <= 14 here: at most 10 dwords and a half
            if (k < nd) reinterpret_cast<uint32_t*>(p)[k] = w[k];
            else if (k == nd && (bytes & 2)) reinterpret_cast<uint16_t*>(p)[2 * k] = (uint16_t)w[k];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 48; ++i)
        if (i < 3 * n) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// What the LUT-apply and the interpolation body below do with a lane's 16 decoded pixels is a store policy S; they are written once
// for every pixel form (this file's Store422Bgr; a form with another pixel size brings its own block type and policy and wraps the
// same bodies):
//   kPxBytes, kGroupBytes       bytes per pixel and per 16-pixel group of the image
//   group(p, y, uv, n, wide)    16 mapped luma bytes and the 8 U,V pairs of the same macropixels -> the first n pixels at p
// The three-channel policy: 48 bytes a group (decode422_16, store422_px).
template <int ORDER> struct Store422Bgr {
    static constexpr int kPxBytes = 3, kGroupBytes = 48;
    static __device__ __forceinline__ void group(uint8_t* p, const u32x4& y, const u32x4& uv, int n, bool wide)
    {
        uint32_t w[12];
        decode422_16<ORDER>(y, uv, w);
        store422_px(p, w, n, wide);
    }
};

// ---------------------------------------------------------------------------------------------
// K3b  LUT apply + decode, packed -> BGR / RGB.  grid = (B, n_frames).  A workgroup takes a band of rows and walks it as (row,
// 16-column group) items kThreads apart; an item is two 16-byte loads, 16 LUT reads, 8 chroma terms, 16 pixels decoded and 48 bytes
// stored (S::kGroupBytes).  The input is read once: luma and chroma come out of the same two registers quads.  Groups are cut at
// multiples of 16 columns from the row start; the last group of a row may be ragged (nd < 8 dwords).
// ---------------------------------------------------------------------------------------------
template <int OFF, class S, class Block, class Frames>
__device__ __forceinline__ void lut_apply422_bgr_body(const Block& p, const Frames& fr, const uint8_t* __restrict__ luts)
{
    __shared__ uint32_t lut[256 * kCopies];
    // frames last-to-first: the histogram pass streamed the batch first-to-last, its tail is still in the Infinity Cache
    const int t = threadIdx.x, f = (int)gridDim.y - 1 - (int)blockIdx.y;
    {
        const uint32_t v = luts[(size_t)f * 256 + t];
#pragma unroll
        for (int k = 0; k < kCopies; ++k) lut[(t << kCopyShift) + ((k + t) & (kCopies - 1))] = v;
    }
    __syncthreads();
    const uint32_t copy = t & (kCopies - 1);
    const bool wide = fr.wide_of(f);
    const int r0 = (int)((long long)p.rows * blockIdx.x / gridDim.x), r1 = (int)((long long)p.rows * (blockIdx.x + 1) / gridDim.x);
    const uint8_t* src0 = fr.src_of(f) + (long long)r0 * p.src_step;
    uint8_t* out0 = fr.out_of(f) + (long long)r0 * p.out_step;
    const int G = (p.dwords + 7) >> 3;                          // 16-column groups per row, the last one possibly ragged
    const long long items = (long long)(r1 - r0) * G;
    int row = t / G, grp = t - row * G;
    const int drow = kThreads / G, dgrp = kThreads - drow * G;
    for (long long it = t; it < items; it += kThreads) {
        const uint8_t* s = src0 + (long long)row * p.src_step + 32LL * grp;
        uint8_t* d = out0 + (long long)row * p.out_step + (long long)S::kGroupBytes * grp;
        const int nd = min(8, p.dwords - 8 * grp);
        u32x4 a, b;
        if (nd == 8) {
            const u32x4_u* sp = reinterpret_cast<const u32x4_u*>(s);
            a = sp[0]; b = sp[1];
        } else {
            load422_tail(s, nd, a, b);
        }
        const u32x4 o = lut_vec(lut, gather422<OFF>(a, b), copy);
        S::group(d, o, chroma422<OFF>(a, b), 2 * nd, wide);
        row += drow; grp += dgrp;
        if (grp >= G) { grp -= G; ++row; }
    }
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void lut_apply422_bgr_kernel(Packed422Bgr p, const uint8_t* __restrict__ luts)
{
    lut_apply422_bgr_body<OFF, Store422Bgr<ORDER>>(p, Strided422Bgr{p}, luts);
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void lut_apply422_bgr_frames_kernel(Packed422List l, Packed422Bgr p, const uint8_t* __restrict__ luts)
{
    lut_apply422_bgr_body<OFF, Store422Bgr<ORDER>>(p, Table422Bgr{l, p}, luts);
}

// ---------------------------------------------------------------------------------------------
// K6b  CLAHE interpolation + decode, packed -> BGR / RGB: clahe_interp422_kernel's grid, bands, pair tables, column segments and
// blend (interp_stage in clahe.hip.h; all four <FT, FMA> rungs), the 16 blended luma bytes decoded with the chroma of the same two
// loads.  Every row belongs to exactly one band and carries its own chroma, so no lane reads a second row.
// ---------------------------------------------------------------------------------------------
template <bool FT, bool FMA, int OFF, class S, class Block, class Frames>
__device__ __forceinline__ void clahe_interp422_bgr_body(const Block& p, const Frames& fr, const ClaheGeom g,
                                                         const uint8_t* __restrict__ luts, int subs, int groups, int pair_cap)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t quad[];   // [(tiles_x + 1)][256] u32 quads, or f32x4 when FT
    f32x4* quadf = reinterpret_cast<f32x4*>(quad);
    const InterpStage st = interp_stage<FT, FMA>(quad, g, luts, subs, groups, pair_cap);
    const int t = threadIdx.x, f = st.f, ty1u = st.ty1u, p0 = st.p0, npairs = st.npairs, y_lo = st.y_lo, y_hi = st.y_hi;

    const int phases = kThreads / groups;
    const int grp = t % groups, phase = t / groups;
    const int x0 = (blockIdx.z * groups + grp) * kInterpPx;
    if (!(phase < phases && x0 < g.width)) return;
    // column weights, row trim and first row: duplicated in the interpolation bodies, see interp_stage (clahe.hip.h)
    float xa[kInterpPx], xa1[kInterpPx];
    f32x2 xw[kInterpPx];                                       // {xa1, xa} pairs for the packed float-table body
    int poff[kInterpPx];
#pragma unroll
    for (int j = 0; j < kInterpPx; ++j) {
        const float txf = tile_coord<FMA>(x0 + j, g.inv_tw);
        const int tx1 = floor_f32_to_int(txf);
        xa[j] = __fsub_rn(txf, (float)tx1);
        xa1[j] = __fsub_rn(1.0f, xa[j]);
        xw[j].x = xa1[j]; xw[j].y = xa[j];
        int pr = tx1 + 1;                                      // pair index; columns beyond the frame are never used
        pr = pr < 0 ? 0 : (pr > g.tiles_x ? g.tiles_x : pr);
        pr -= p0;                                              // position in this workgroup's table
        pr = pr < 0 ? 0 : (pr >= npairs ? npairs - 1 : pr);
        poff[j] = pr << 8;
    }
    const uint8_t* src = fr.src_of(f) + 2LL * x0;
    uint8_t* dst = fr.out_of(f) + (long long)S::kPxBytes * x0;
    const bool full = x0 + kInterpPx <= g.width;
    const bool wide = fr.wide_of(f);
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<FMA>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases;
    if (full) {
        auto do_row = [&](int yy, const u32x4& a, const u32x4& b) {
            const float tyf = tile_coord<FMA>(yy, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            const u32x4 q = gather422<OFF>(a, b);
            const u32x4 o = FT ? clahe_vec16_f32<FMA>(quadf, q, poff, xw, ya, ya1) : clahe_vec16<FMA>(quad, q, poff, xa, xa1, ya, ya1);
            S::group(dst + (long long)yy * p.out_step, o, chroma422<OFF>(a, b), kInterpPx, wide);
        };
        // two rows in flight per lane, as clahe_interp422_kernel: 64 bytes of loads
        constexpr int kRowsInFlight = 2;
        for (; y + (kRowsInFlight - 1) * phases < ya_hi; y += kRowsInFlight * phases) {
            u32x4 a[kRowsInFlight], b[kRowsInFlight];
#pragma unroll
            for (int k = 0; k < kRowsInFlight; ++k) {
                const u32x4_u* s = reinterpret_cast<const u32x4_u*>(src + (long long)(y + k * phases) * p.src_step);
                a[k] = s[0]; b[k] = s[1];
            }
#pragma unroll
            for (int k = 0; k < kRowsInFlight; ++k) { do_row(y + k * phases, a[k], b[k]); __builtin_amdgcn_sched_barrier(0); }
        }
        for (; y < ya_hi; y += phases) {
            const u32x4_u* s = reinterpret_cast<const u32x4_u*>(src + (long long)y * p.src_step);
            const u32x4 a = s[0], b = s[1];
            do_row(y, a, b);
        }
    } else {                                                   // the last group of a row whose width is not a multiple of 16: dword by dword
        const int nd = (g.width - x0) >> 1;                    // W is even: 1 <= nd <= 7 whole macropixels
        for (; y < ya_hi; y += phases) {
            const float tyf = tile_coord<FMA>(y, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            u32x4 a, b;
            load422_tail(src + (long long)y * p.src_step, nd, a, b);
            const u32x4 q = gather422<OFF>(a, b);
            uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < kInterpPx; ++j)
                if (j < 2 * nd) {
                    const uint32_t v = byte_of(q, j);
                    uint32_t e;
                    if (FT) {
                        const f32x4 fe = quadf[poff[j] + v];
                        e = (uint32_t)fe.x | ((uint32_t)fe.z << 8) | ((uint32_t)fe.y << 16) | ((uint32_t)fe.w << 24);
                    } else {
                        e = quad[poff[j] + v];
                    }
                    o[j >> 2] |= clahe_px<FMA>(e, xa[j], xa1[j], ya, ya1) << (8 * (j & 3));
                }
            const u32x4 ov = {o[0], o[1], o[2], o[3]};
            S::group(dst + (long long)y * p.out_step, ov, chroma422<OFF>(a, b), 2 * nd, wide);
        }
    }
}
template <bool FT, bool FMA, int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgr_kernel(Packed422Bgr p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                      int subs, int groups, int pair_cap)
{
    clahe_interp422_bgr_body<FT, FMA, OFF, Store422Bgr<ORDER>>(p, Strided422Bgr{p}, g, luts, subs, groups, pair_cap);
}
template <bool FT, bool FMA, int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgr_frames_kernel(Packed422List l, Packed422Bgr p, ClaheGeom g,
                                                                             const uint8_t* __restrict__ luts, int subs, int groups, int pair_cap)
{
    clahe_interp422_bgr_body<FT, FMA, OFF, Store422Bgr<ORDER>>(p, Table422Bgr{l, p}, g, luts, subs, groups, pair_cap);
}

// Fallback for tile grids too wide for the LDS pair table (clahe_interp422_global_kernel's arithmetic): one macropixel per thread, the
// LUTs gathered from global memory (L2), two pixels decoded with the macropixel's own U and V: 6 bytes, as three 2-byte stores when the
// row starts at an even address (`wide`), else as bytes.  grid = (ceil(W / 2 / 256), H, n_frames).
// This body is written out for each pixel form (here and in the four-channel file), not shared through the store policy as the two
// bodies above are: every policy shape tried for its 6- or 8-byte store -- one pair(o, ...) function, decode and store apart with the
// pixels in a struct or in a word array, the wide / byte branch inside the policy or kept here -- left the instructions the same and
// turned one of the kernel's two uniform branches round in 12 or 16 of the 16 instantiations (docs/experiments.md).
template <int OFF, int ORDER, class Frames>
__device__ __forceinline__ void clahe_interp422_bgr_global_body(const Packed422Bgr& p, const Frames& fr, const ClaheGeom& g,
                                                                const uint8_t* __restrict__ luts)
{
    const int f = blockIdx.z;
    const int y = blockIdx.y;
    const int d = blockIdx.x * kThreads + threadIdx.x;
    if (d >= p.dwords) return;
    const uint8_t* lf = luts + (size_t)f * g.tiles_x * g.tiles_y * 256;
    const float tyf = tile_coord(y, g.inv_th, g.contract);
    int ty1 = floor_f32_to_int(tyf);
    const float ya = __fsub_rn(tyf, (float)ty1), ya1 = __fsub_rn(1.0f, ya);
    int ty2 = ty1 + 1; ty1 = max(ty1, 0); ty2 = min(ty2, g.tiles_y - 1);
    const uint32_t w = reinterpret_cast<const uint32_t*>(fr.src_of(f) + (long long)y * p.src_step)[d];
    uint32_t e[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float txf = tile_coord(2 * d + b, g.inv_tw, g.contract);
        int tx1 = floor_f32_to_int(txf);
        const float xa = __fsub_rn(txf, (float)tx1), xa1 = __fsub_rn(1.0f, xa);
        int tx2 = tx1 + 1; tx1 = max(tx1, 0); tx2 = min(tx2, g.tiles_x - 1);
        const uint32_t v = b ? y1_of<OFF>(w) : y0_of<OFF>(w);
        const uint32_t q = (uint32_t)lf[((size_t)ty1 * g.tiles_x + tx1) * 256 + v] |
                           ((uint32_t)lf[((size_t)ty1 * g.tiles_x + tx2) * 256 + v] << 8) |
                           ((uint32_t)lf[((size_t)ty2 * g.tiles_x + tx1) * 256 + v] << 16) |
                           ((uint32_t)lf[((size_t)ty2 * g.tiles_x + tx2) * 256 + v] << 24);
        e[b] = g.contract ? clahe_px<true>(q, xa, xa1, ya, ya1) : clahe_px<false>(q, xa, xa1, ya, ya1);
    }
    const uint32_t uv = chroma422_px<OFF>(w);
    int ruv, guv, buv;
    bt601_uv_terms(uv & 0xffu, uv >> 8, ruv, guv, buv);
    uint32_t c[6];                                             // the 6 output bytes in memory order
    constexpr int B = ORDER == 0 ? 0 : 2, R = 2 - B;
    bt601_px_bgr(e[0], ruv, guv, buv, c[B], c[1], c[R]);
    bt601_px_bgr(e[1], ruv, guv, buv, c[3 + B], c[4], c[3 + R]);
    uint8_t* o = fr.out_of(f) + (long long)y * p.out_step + 6LL * d;
    if (fr.wide_of(f)) {
        uint16_t* o2 = reinterpret_cast<uint16_t*>(o);
        o2[0] = (uint16_t)(c[0] | (c[1] << 8)); o2[1] = (uint16_t)(c[2] | (c[3] << 8)); o2[2] = (uint16_t)(c[4] | (c[5] << 8));
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = (uint8_t)c[k];
    }
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgr_global_kernel(Packed422Bgr p, ClaheGeom g, const uint8_t* __restrict__ luts)
{
    clahe_interp422_bgr_global_body<OFF, ORDER>(p, Strided422Bgr{p}, g, luts);
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgr_global_frames_kernel(Packed422List l, Packed422Bgr p, ClaheGeom g,
                                                                                    const uint8_t* __restrict__ luts)
{
    clahe_interp422_bgr_global_body<OFF, ORDER>(p, Table422Bgr{l, p}, g, luts);
}

}  // namespace mi
