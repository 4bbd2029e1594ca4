// packed422_bgra.hip.h -- the pixel-WRITING stages of "packed 4:2:2 in (YUY2 / UYVY), interleaved 8-bit four-channel images out
// (BGRA / RGBA: CV_8UC4, A = 255)": LUT apply, CLAHE interpolation and its wide-grid fallback, each with the BT.601 decode behind it.
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
//
// capture card -> display surface / swap-chain image / interop texture / GUI image.  The bodies are those of packed422_bgr.hip.h --
// same grids, bands, carried walks, column segments and blends, the histogram stages packed422.hip.h's own, every row decoded with its
// own chroma, OFF = 0 exactly Y0 U Y1 V and OFF = 1 exactly U Y0 V Y1 -- with the store of yuv420_bgra.hip.h: every pixel is one dword
// (bgra_dword), so no pixel straddles a dword and none of the 48-byte packing of the three-channel form is needed.  The first three
// bytes of a pixel are the three-channel form's, the fourth is 255.
// Input rows start at multiples of 4 as in every packed form.  The output has no alignment rule; packed422_bgra_frame_wide below says
// which of the two store paths a frame takes.  Nothing beyond byte 4 * W of any row is written.
// ORDER 0: B, G, R, A in memory (MI_ORDER_BGR); 1: R, G, B, A (MI_ORDER_RGB).
#pragma once
#include "packed422_bgr.hip.h"
#include "yuv420_bgra.hip.h"

namespace mi {

// A batch of packed frames in, four-channel images out: frame f reads src + f * src_frame and writes out + f * out_frame.  The fields
// of Packed422Bgr, with rows of 4 * W bytes behind `out`.
struct Packed422Bgra {
    const uint8_t* src;
    uint8_t* out;
    long long src_step, out_step;
    long long src_frame, out_frame;
    int dwords, rows;                 // macropixels per row (W / 2), rows (H, any value >= 1)
    int wide;                         // a batch launch: packed422_bgra_frame_wide(out, out_step, out_frame), decided by the host for the
                                      // whole launch; a table launch does not look at it (every frame has its own address)
};

// THE rule "does a frame at these addresses take the wide stores": its image address is a multiple of 4, and so are the pitch and (a
// batch; a list passes 0) the frame stride.  Wide: a 16-column group leaves as four unaligned-capable 16-byte stores, the ragged last
// group of a row (W % 16 != 0, nd macropixels) as 2 * nd dword stores.  Otherwise every byte is stored on its own: slower, the same
// bytes.  The kernel decides by it and the host counts by it.
__host__ __device__ __forceinline__ bool packed422_bgra_frame_wide(const void* out, long long out_step, long long out_frame)
{
    return (((uintptr_t)out | (uintptr_t)out_step | (uintptr_t)out_frame) & 3) == 0;
}

// Where frame f lives, and which store path it takes: the two policies of packed422_bgr.hip.h.
struct Strided422Bgra {
    const Packed422Bgra& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return p.src + f * p.src_frame; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return p.out + f * p.out_frame; }
    __device__ __forceinline__ bool wide_of(long long) const { return p.wide != 0; }
};
// A list of frames, each at its own addresses (mi_*_packed422_to_bgra_frames_dev: a capture device's buffer pool in, a surface pool
// out).  The table is packed422.hip.h's Packed422List of {in, out} pairs, by value in the kernel arguments; the shape is the launch's
// Packed422Bgra, whose src / out / *_frame / wide a table launch ignores.  The frame index is uniform across a workgroup, so the choice
// of the store path stays a scalar branch.
// clahe_interp422_bgra_frames_kernel(l, p, g, luts, subs, groups, pair_cap) is the longest list; 256: the implicit arguments
static_assert(sizeof(Packed422Bgra) == sizeof(Packed422Bgr), "the block of the three-channel form, with 4 B/px semantics");
static_assert(sizeof(Packed422List) + sizeof(Packed422Bgra) + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 3 * sizeof(int) + 8 + 256 <= 4096,
              "the kernel arguments of a table launch stay within 4 KiB");
struct Table422Bgra {
    const Packed422List& l;
    const Packed422Bgra& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* out_of(long long f) const { return l.f[f].out; }
    __device__ __forceinline__ bool wide_of(long long f) const { return packed422_bgra_frame_wide(l.f[f].out, p.out_step, 0); }
};

// 16 luma bytes (already mapped) and the 8 U,V pairs of the same macropixels -> the first n pixels (n even, 2 <= n <= 16) as 4 * n
// bytes at p.  Four pixels are packed and stored at a time, as decode_store16_4 does, so four output dwords are live beside the inputs,
// not sixteen.  wide (p is a multiple of 4): n == 16 leaves as four 16-byte stores, a ragged group as n dword stores.  Every index is a
// compile-time constant (the loops are unrolled and predicated).
template <int ORDER>
__device__ __forceinline__ void decode422_4(const u32x4& y, const u32x4& uv, int q, uint32_t* w)     // pixels 4q .. 4q + 3
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = 2 * q + h;                              // macropixel k: pixels 2k and 2k + 1
        int ruv, guv, buv;
        bt601_uv_terms(byte_of(uv, 2 * k), byte_of(uv, 2 * k + 1), ruv, guv, buv);
        uint32_t b, g, r;
        bt601_px_bgr(byte_of(y, 2 * k), ruv, guv, buv, b, g, r);     w[2 * h] = bgra_dword<ORDER>(b, g, r);
        bt601_px_bgr(byte_of(y, 2 * k + 1), ruv, guv, buv, b, g, r); w[2 * h + 1] = bgra_dword<ORDER>(b, g, r);
    }
}
// The store path is chosen once, outside the loop over the four quarters: each path is a straight run of decode 4, store 4 (with the
// branch inside the loop the compiler keeps all sixteen dwords live: 184 VGPRs in the float-table interpolation instead of 143).
// gfx950 accepts unaligned vector stores, so the compiler may merge the byte path's neighbouring stores into wider unaligned ones.
template <int ORDER>
__device__ __forceinline__ void decode422_store_bgra(uint8_t* p, const u32x4& y, const u32x4& uv, int n, bool wide)
{
    uint32_t w[4];
    if (wide && n == 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            decode422_4<ORDER>(y, uv, q, w);
            const u32x4 o = {w[0], w[1], w[2], w[3]};
            reinterpret_cast<u32x4_u*>(p)[q] = o;
        }
    } else if (wide) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            decode422_4<ORDER>(y, uv, q, w);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * q + i < n) reinterpret_cast<uint32_t*>(p)[4 * q + i] = w[i];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            decode422_4<ORDER>(y, uv, q, w);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (4 * q + (i >> 2) < n) p[16 * q + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K3c  LUT apply + decode, packed -> BGRA / RGBA.  grid = (B, n_frames): lut_apply422_bgr_body's grid, band and carried (row, group)
// walk.  An item is two 16-byte loads, 16 LUT reads, 8 chroma terms, 16 pixels decoded and 64 bytes stored.
// ---------------------------------------------------------------------------------------------
template <int OFF, int ORDER, class Frames>
__device__ __forceinline__ void lut_apply422_bgra_body(const Packed422Bgra& p, const Frames& fr, const uint8_t* __restrict__ luts)
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
        uint8_t* d = out0 + (long long)row * p.out_step + 64LL * grp;
        const int nd = min(8, p.dwords - 8 * grp);
        u32x4 a, b;
        if (nd == 8) {
            const u32x4_u* sp = reinterpret_cast<const u32x4_u*>(s);
            a = sp[0]; b = sp[1];
        } else {
            load422_tail(s, nd, a, b);
        }
        const u32x4 o = lut_vec(lut, gather422<OFF>(a, b), copy);
        decode422_store_bgra<ORDER>(d, o, chroma422<OFF>(a, b), 2 * nd, wide);
        row += drow; grp += dgrp;
        if (grp >= G) { grp -= G; ++row; }
    }
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void lut_apply422_bgra_kernel(Packed422Bgra p, const uint8_t* __restrict__ luts)
{
    lut_apply422_bgra_body<OFF, ORDER>(p, Strided422Bgra{p}, luts);
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void lut_apply422_bgra_frames_kernel(Packed422List l, Packed422Bgra p, const uint8_t* __restrict__ luts)
{
    lut_apply422_bgra_body<OFF, ORDER>(p, Table422Bgra{l, p}, luts);
}

// ---------------------------------------------------------------------------------------------
// K6c  CLAHE interpolation + decode, packed -> BGRA / RGBA: clahe_interp422_bgr_body's grid, bands, sub-bands, pair tables, column
// segments, two-rows-in-flight loop, ragged last group and blend (interp_stage in clahe.hip.h; all four <FT, FMA> rungs), with
// dst = out + 4 * x0.  Every row belongs to exactly one band and carries its own chroma, so no lane reads a second row.
// ---------------------------------------------------------------------------------------------
template <bool FT, bool FMA, int OFF, int ORDER, class Frames>
__device__ __forceinline__ void clahe_interp422_bgra_body(const Packed422Bgra& p, const Frames& fr, const ClaheGeom g,
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
    uint8_t* dst = fr.out_of(f) + 4LL * x0;
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
            decode422_store_bgra<ORDER>(dst + (long long)yy * p.out_step, o, chroma422<OFF>(a, b), kInterpPx, wide);
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
            decode422_store_bgra<ORDER>(dst + (long long)y * p.out_step, ov, chroma422<OFF>(a, b), 2 * nd, wide);
        }
    }
}
template <bool FT, bool FMA, int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgra_kernel(Packed422Bgra p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                       int subs, int groups, int pair_cap)
{
    clahe_interp422_bgra_body<FT, FMA, OFF, ORDER>(p, Strided422Bgra{p}, g, luts, subs, groups, pair_cap);
}
template <bool FT, bool FMA, int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgra_frames_kernel(Packed422List l, Packed422Bgra p, ClaheGeom g,
                                                                              const uint8_t* __restrict__ luts, int subs, int groups, int pair_cap)
{
    clahe_interp422_bgra_body<FT, FMA, OFF, ORDER>(p, Table422Bgra{l, p}, g, luts, subs, groups, pair_cap);
}

// Fallback for tile grids too wide for the LDS pair table (clahe_interp422_bgr_global_body's arithmetic): one macropixel per thread,
// the LUTs gathered from global memory (L2), two pixels decoded with the macropixel's own U and V: 8 bytes, as one 8-byte store (dword-aligned)
// when the frame is wide, else as bytes.
// grid = (ceil(W / 2 / 256), H, n_frames).
template <int OFF, int ORDER, class Frames>
__device__ __forceinline__ void clahe_interp422_bgra_global_body(const Packed422Bgra& p, const Frames& fr, const ClaheGeom& g,
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
    uint32_t b0, g0, c0, b1, g1, c1;
    bt601_px_bgr(e[0], ruv, guv, buv, b0, g0, c0);
    bt601_px_bgr(e[1], ruv, guv, buv, b1, g1, c1);
    const uint32_t px0 = bgra_dword<ORDER>(b0, g0, c0), px1 = bgra_dword<ORDER>(b1, g1, c1);
    uint8_t* o = fr.out_of(f) + (long long)y * p.out_step + 8LL * d;
    if (fr.wide_of(f)) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        typedef u32x2 u32x2_u __attribute__((aligned(4)));    // o is a multiple of 4, not always of 8
        const u32x2 px = {px0, px1};
        *reinterpret_cast<u32x2_u*>(o) = px;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { o[k] = (uint8_t)(px0 >> (8 * k)); o[4 + k] = (uint8_t)(px1 >> (8 * k)); }
    }
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgra_global_kernel(Packed422Bgra p, ClaheGeom g, const uint8_t* __restrict__ luts)
{
    clahe_interp422_bgra_global_body<OFF, ORDER>(p, Strided422Bgra{p}, g, luts);
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgra_global_frames_kernel(Packed422List l, Packed422Bgra p, ClaheGeom g,
                                                                                     const uint8_t* __restrict__ luts)
{
    clahe_interp422_bgra_global_body<OFF, ORDER>(p, Table422Bgra{l, p}, g, luts);
}

}  // namespace mi
