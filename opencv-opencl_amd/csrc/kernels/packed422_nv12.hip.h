// packed422_nv12.hip.h -- the pixel-WRITING stages of "packed 4:2:2 in (YUY2 / UYVY), NV12 out": LUT apply, CLAHE interpolation and its
// wide-grid fallback.  Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
//
// The histogram stages are packed422.hip.h's own, unchanged (they only read).  What is new is where the second pass puts its bytes:
// the new luma of 16 columns goes to a planar Y row as ONE 16-byte store, and the chroma of a row PAIR -- the odd bytes of the same
// dwords, already U0 V0 U1 V1 ... in NV12's order once gathered -- is halved vertically with the per-byte rounding mean
// (a + b + 1) >> 1 and goes to the interleaved UV row as one 16-byte store.  No horizontal filtering, no change of siting.
// Output rows start at multiples of 4 (pointers and pitches are), a lane's 16 columns at a multiple of 16 inside the row: full groups
// are unaligned-capable 16-byte stores like the interpolation kernels', the ragged last group of a row is written as dwords and, when
// W % 4 == 2, one final 2-byte store.  No byte stores, nothing beyond column W of any row.
#pragma once
#include "packed422.hip.h"

namespace mi {

// A batch of packed frames in, NV12 planes out: frame f reads src + f * src_frame and writes y + f * out_frame / uv + f * out_frame.
struct Packed422Nv12 {
    const uint8_t* src;
    uint8_t* y;
    uint8_t* uv;
    long long src_step, y_step, uv_step;
    long long src_frame, out_frame;
    int dwords, rows;                 // macropixels per row (W / 2), rows (H, even)
    int copy_uv;                      // 1: MI_UV_COPY (row-pair mean of the input chroma), 0: every UV byte 128
};

// Where frame f lives.  The bodies below are templates on such a policy from the start, as packed422.hip.h's are: a frame-list form
// (capture pool in, encoder surface pool out) adds a table policy and *_frames_kernel entries, not new bodies.
struct Strided422Nv12 {
    const Packed422Nv12& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return p.src + f * p.src_frame; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return p.y + f * p.out_frame; }
    __device__ __forceinline__ uint8_t* uv_of(long long f) const { return p.uv + f * p.out_frame; }
};

// A list of such frames, each at its own three addresses (mi_*_packed422_to_nv12_frames_dev: a capture pool in, an encoder's surface
// pool out).  The {in, y, uv} entries travel BY VALUE in the kernel arguments like Packed422List -- 24 B an entry -- and are read with
// scalar kernarg loads indexed by the frame's grid coordinate.  The shape (pitches, dwords, rows, copy_uv) is the launch's
// Packed422Nv12, whose src / y / uv / *_frame a table launch ignores.  128 entries are 3 KiB: with the largest remaining argument list
// (the interpolation kernel's) and the 256 B of implicit arguments a code object carries behind the explicit ones, a launch stays
// inside the 4 KiB of kernel arguments HIP accepts -- and the chunks are those of the histogram stages' Packed422List, so 256 frames
// are two launches per stage.  64 builds too (-DMI_PACKED422_NV12_FRAMES_PER_LAUNCH=64); the host cuts both tables by the smaller one.
#ifndef MI_PACKED422_NV12_FRAMES_PER_LAUNCH
#define MI_PACKED422_NV12_FRAMES_PER_LAUNCH 128
#endif
constexpr int kPacked422Nv12FramesPerLaunch = MI_PACKED422_NV12_FRAMES_PER_LAUNCH;
static_assert(kPacked422Nv12FramesPerLaunch == 64 || kPacked422Nv12FramesPerLaunch == 128, "a table is 1.5 or 3 KiB of kernel arguments");
struct Packed422Nv12Frame { const uint8_t* in; uint8_t* y; uint8_t* uv; };
struct Packed422Nv12List { Packed422Nv12Frame f[kPacked422Nv12FramesPerLaunch]; };
static_assert(sizeof(Packed422Nv12Frame) == 24, "three addresses an entry");
// clahe_interp422_nv12_frames_kernel(l, p, g, luts, subs, groups, pair_cap) is the longest list; 256: the implicit arguments
static_assert(sizeof(Packed422Nv12List) + sizeof(Packed422Nv12) + 8 + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 3 * sizeof(int) + 8 + 256 <= 4096,
              "the table and the largest remaining argument list stay within HIP's 4 KiB of kernel arguments");
struct Table422Nv12 {
    const Packed422Nv12List& l;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return l.f[f].y; }
    __device__ __forceinline__ uint8_t* uv_of(long long f) const { return l.f[f].uv; }
};

// per-byte (a + b + 1) >> 1 of four bytes at once: a | b = (a ^ b) + (a & b) and a + b = (a ^ b) + 2 * (a & b), so the rounded-up mean
// is (a | b) - ((a ^ b) >> 1); masking the shifted difference with 0x7f keeps a neighbour's low bit out of each byte, and the
// subtraction never borrows (each byte of the subtrahend is <= the same byte of a | b).
__device__ __forceinline__ uint32_t mean_up_u8x4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }
__device__ __forceinline__ u32x4 mean_up_u8x16(const u32x4& a, const u32x4& b)
{
    u32x4 m;
    m.x = mean_up_u8x4(a.x, b.x); m.y = mean_up_u8x4(a.y, b.y); m.z = mean_up_u8x4(a.z, b.z); m.w = mean_up_u8x4(a.w, b.w);
    return m;
}
// the 16 chroma bytes of 8 consecutive dwords, U V U V ...: the luma gather of the OTHER byte offset
template <int OFF> __device__ __forceinline__ u32x4 chroma422(const u32x4& a, const u32x4& b) { return gather422<1 - OFF>(a, b); }
// U | V << 8 of one macropixel
template <int OFF> __device__ __forceinline__ uint32_t chroma422_px(uint32_t w) { return y0_of<1 - OFF>(w) | (y1_of<1 - OFF>(w) << 8); }

// The ragged last group of a row: nd < 8 dwords at `row`, the missing ones read as 0 (a, b as two full loads would give them) ...
__device__ __forceinline__ void load422_tail(const uint8_t* row, int nd, u32x4& a, u32x4& b)
{
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row);
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = j < nd ? p[j] : 0u;
    a.x = w[0]; a.y = w[1]; a.z = w[2]; a.w = w[3];
    b.x = w[4]; b.y = w[5]; b.z = w[6]; b.w = w[7];
}
// ... and its 2 * nd output bytes (the first bytes of q) at a 4-byte aligned address: dwords, then one 2-byte store when nd is odd
__device__ __forceinline__ void store_nv12_tail(uint8_t* dst, const u32x4& q, int nd)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (2 * k + 1 < nd) reinterpret_cast<uint32_t*>(dst)[k] = w[k];
        else if (2 * k < nd) reinterpret_cast<uint16_t*>(dst)[2 * k] = (uint16_t)w[k];
    }
}

// ---------------------------------------------------------------------------------------------
// K3n  LUT apply, packed -> NV12.  grid = (B, n_frames).  A workgroup takes a band of ROW PAIRS and walks it as (pair, 16-column group)
// items kThreads apart; an item is four 16-byte loads (two per row, 64 bytes in flight per lane), 32 LUT reads, two 16-byte Y stores and
// one 16-byte UV store.  The input is read once: luma and chroma come out of the same four registers, there is no chroma launch.
// ---------------------------------------------------------------------------------------------
template <int OFF, class Frames>
__device__ __forceinline__ void lut_apply422_nv12_body(const Packed422Nv12& p, const Frames& fr, const uint8_t* __restrict__ luts)
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
    const int pairs = p.rows >> 1;
    const int r0 = (int)((long long)pairs * blockIdx.x / gridDim.x), r1 = (int)((long long)pairs * (blockIdx.x + 1) / gridDim.x);
    const uint8_t* src0 = fr.src_of(f) + 2LL * r0 * p.src_step;
    uint8_t* y0 = fr.y_of(f) + 2LL * r0 * p.y_step;
    uint8_t* uv0 = fr.uv_of(f) + (long long)r0 * p.uv_step;
    const int G = (p.dwords + 7) >> 3;                          // 16-column groups per row, the last one possibly ragged
    const long long items = (long long)(r1 - r0) * G;
    int pr = t / G, grp = t - pr * G;
    const int dpr = kThreads / G, dgrp = kThreads - dpr * G;
    const u32x4 fill = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    for (long long it = t; it < items; it += kThreads) {
        const uint8_t* s = src0 + 2LL * pr * p.src_step + 32LL * grp;
        uint8_t* dy = y0 + 2LL * pr * p.y_step + 16LL * grp;
        uint8_t* duv = uv0 + (long long)pr * p.uv_step + 16LL * grp;
        const int nd = min(8, p.dwords - 8 * grp);
        u32x4 a0, b0, a1, b1;
        if (nd == 8) {
            const u32x4_u* s0 = reinterpret_cast<const u32x4_u*>(s);
            const u32x4_u* s1 = reinterpret_cast<const u32x4_u*>(s + p.src_step);
            a0 = s0[0]; b0 = s0[1]; a1 = s1[0]; b1 = s1[1];
        } else {
            load422_tail(s, nd, a0, b0);
            load422_tail(s + p.src_step, nd, a1, b1);
        }
        const u32x4 o0 = lut_vec(lut, gather422<OFF>(a0, b0), copy);
        const u32x4 o1 = lut_vec(lut, gather422<OFF>(a1, b1), copy);
        const u32x4 m = p.copy_uv ? mean_up_u8x16(chroma422<OFF>(a0, b0), chroma422<OFF>(a1, b1)) : fill;
        if (nd == 8) {
            *reinterpret_cast<u32x4_u*>(dy) = o0;
            *reinterpret_cast<u32x4_u*>(dy + p.y_step) = o1;
            *reinterpret_cast<u32x4_u*>(duv) = m;
        } else {
            store_nv12_tail(dy, o0, nd);
            store_nv12_tail(dy + p.y_step, o1, nd);
            store_nv12_tail(duv, m, nd);
        }
        pr += dpr; grp += dgrp;
        if (grp >= G) { grp -= G; ++pr; }
    }
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void lut_apply422_nv12_kernel(Packed422Nv12 p, const uint8_t* __restrict__ luts)
{
    lut_apply422_nv12_body<OFF>(p, Strided422Nv12{p}, luts);
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void lut_apply422_nv12_frames_kernel(Packed422Nv12List l, Packed422Nv12 p, const uint8_t* __restrict__ luts)
{
    lut_apply422_nv12_body<OFF>(p, Table422Nv12{l}, luts);
}

// ---------------------------------------------------------------------------------------------
// K6n  CLAHE interpolation, packed -> NV12: clahe_interp422_kernel's grid, bands, pair tables, column segments and blend, the luma
// written to the Y plane.  Bands are cut by tile-row coordinate, so the two rows of a chroma pair may belong to different bands (and
// lanes): the lane that owns the EVEN row y of a pair also loads the chroma of row y + 1 (the same 32 bytes its neighbour in phase, or
// the next band's workgroup, reads for the luma: a cache hit at worst an L2 one) and writes UV row y / 2 in the same launch.  Every row
// belongs to exactly one band, so every UV row is written exactly once.  With MI_UV_FILL128 there is no second read.
// ---------------------------------------------------------------------------------------------
template <bool FT, bool FMA, int OFF, class Frames>
__device__ __forceinline__ void clahe_interp422_nv12_body(const Packed422Nv12& p, const Frames& fr, const ClaheGeom g,
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
    // column weights, row trim and first row: duplicated in the five bodies, see interp_stage (clahe.hip.h)
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
    uint8_t* dy = fr.y_of(f) + x0;
    uint8_t* duv = fr.uv_of(f) + x0;
    const bool full = x0 + kInterpPx <= g.width;
    const bool copy_uv = p.copy_uv != 0;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<FMA>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases;
    if (full) {
        const u32x4 fill = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
        // c, d: the dwords of row yy + 1, loaded only where this lane writes the UV row (yy even, MI_UV_COPY)
        auto do_row = [&](int yy, const u32x4& a, const u32x4& b, const u32x4& c, const u32x4& d) {
            const float tyf = tile_coord<FMA>(yy, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            const u32x4 q = gather422<OFF>(a, b);
            const u32x4 o = FT ? clahe_vec16_f32<FMA>(quadf, q, poff, xw, ya, ya1) : clahe_vec16<FMA>(quad, q, poff, xa, xa1, ya, ya1);
            *reinterpret_cast<u32x4_u*>(dy + (long long)yy * p.y_step) = o;
            if (!(yy & 1)) {
                const u32x4 m = copy_uv ? mean_up_u8x16(chroma422<OFF>(a, b), chroma422<OFF>(c, d)) : fill;
                *reinterpret_cast<u32x4_u*>(duv + (long long)(yy >> 1) * p.uv_step) = m;
            }
        };
        auto load_rows = [&](int yy, u32x4& a, u32x4& b, u32x4& c, u32x4& d) {
            const u32x4_u* s = reinterpret_cast<const u32x4_u*>(src + (long long)yy * p.src_step);
            a = s[0]; b = s[1];
            if (copy_uv && !(yy & 1)) {                        // H is even: row yy + 1 exists
                const u32x4_u* s1 = reinterpret_cast<const u32x4_u*>(src + (long long)(yy + 1) * p.src_step);
                c = s1[0]; d = s1[1];
            } else {
                c = fill; d = fill;
            }
        };
        // two rows in flight per lane, as clahe_interp422_kernel: 64 bytes of luma rows, up to 64 more where both rows are even
        constexpr int kRowsInFlight = 2;
        for (; y + (kRowsInFlight - 1) * phases < ya_hi; y += kRowsInFlight * phases) {
            u32x4 a[kRowsInFlight], b[kRowsInFlight], c[kRowsInFlight], d[kRowsInFlight];
#pragma unroll
            for (int k = 0; k < kRowsInFlight; ++k) load_rows(y + k * phases, a[k], b[k], c[k], d[k]);
#pragma unroll
            for (int k = 0; k < kRowsInFlight; ++k) { do_row(y + k * phases, a[k], b[k], c[k], d[k]); __builtin_amdgcn_sched_barrier(0); }
        }
        for (; y < ya_hi; y += phases) {
            u32x4 a, b, c, d;
            load_rows(y, a, b, c, d);
            do_row(y, a, b, c, d);
        }
    } else {                                                   // the last group of a row whose width is not a multiple of 16: dword by dword
        for (; y < ya_hi; y += phases) {
            const float tyf = tile_coord<FMA>(y, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            const uint32_t* sr = reinterpret_cast<const uint32_t*>(src + (long long)y * p.src_step);
            const uint32_t* sr1 = reinterpret_cast<const uint32_t*>(src + (long long)(y + 1) * p.src_step);     // read only when y is even
            uint16_t* yr = reinterpret_cast<uint16_t*>(dy + (long long)y * p.y_step);
            uint16_t* uvr = reinterpret_cast<uint16_t*>(duv + (long long)(y >> 1) * p.uv_step);
#pragma unroll
            for (int dd = 0; dd < kInterpPx / 2; ++dd)
                if (x0 + 2 * dd < g.width) {                   // W is even: both columns of the dword are inside
                    const uint32_t w = sr[dd];
                    uint32_t e[2];
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int j = 2 * dd + b;
                        const uint32_t v = b ? y1_of<OFF>(w) : y0_of<OFF>(w);
                        if (FT) {
                            const f32x4 fe = quadf[poff[j] + v];
                            e[b] = (uint32_t)fe.x | ((uint32_t)fe.z << 8) | ((uint32_t)fe.y << 16) | ((uint32_t)fe.w << 24);
                        } else {
                            e[b] = quad[poff[j] + v];
                        }
                        e[b] = clahe_px<FMA>(e[b], xa[j], xa1[j], ya, ya1);
                    }
                    yr[dd] = (uint16_t)(e[0] | (e[1] << 8));
                    if (!(y & 1))
                        uvr[dd] = (uint16_t)(copy_uv ? mean_up_u8x4(chroma422_px<OFF>(w), chroma422_px<OFF>(sr1[dd])) : 0x8080u);
                }
        }
    }
}
template <bool FT, bool FMA, int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_nv12_kernel(Packed422Nv12 p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                       int subs, int groups, int pair_cap)
{
    clahe_interp422_nv12_body<FT, FMA, OFF>(p, Strided422Nv12{p}, g, luts, subs, groups, pair_cap);
}
template <bool FT, bool FMA, int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_nv12_frames_kernel(Packed422Nv12List l, Packed422Nv12 p, ClaheGeom g,
                                                                              const uint8_t* __restrict__ luts, int subs, int groups, int pair_cap)
{
    clahe_interp422_nv12_body<FT, FMA, OFF>(p, Table422Nv12{l}, g, luts, subs, groups, pair_cap);
}

// Fallback for tile grids too wide for the LDS pair table (clahe_interp422_global_kernel's arithmetic): one macropixel per thread, the
// LUTs gathered from global memory (L2), two luma bytes to the Y plane as one 2-byte store; the thread of an even row also reads the
// macropixel below it and writes the UV pair.  grid = (ceil(W / 2 / 256), H, n_frames).
template <int OFF, class Frames>
__device__ __forceinline__ void clahe_interp422_nv12_global_body(const Packed422Nv12& p, const Frames& fr, const ClaheGeom& g,
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
    const uint8_t* row = fr.src_of(f) + (long long)y * p.src_step;
    const uint32_t w = reinterpret_cast<const uint32_t*>(row)[d];
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
    reinterpret_cast<uint16_t*>(fr.y_of(f) + (long long)y * p.y_step)[d] = (uint16_t)(e[0] | (e[1] << 8));
    if (!(y & 1)) {
        uint32_t m = 0x8080u;
        if (p.copy_uv) m = mean_up_u8x4(chroma422_px<OFF>(w), chroma422_px<OFF>(reinterpret_cast<const uint32_t*>(row + p.src_step)[d]));
        reinterpret_cast<uint16_t*>(fr.uv_of(f) + (long long)(y >> 1) * p.uv_step)[d] = (uint16_t)m;
    }
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_nv12_global_kernel(Packed422Nv12 p, ClaheGeom g, const uint8_t* __restrict__ luts)
{
    clahe_interp422_nv12_global_body<OFF>(p, Strided422Nv12{p}, g, luts);
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_nv12_global_frames_kernel(Packed422Nv12List l, Packed422Nv12 p, ClaheGeom g,
                                                                                     const uint8_t* __restrict__ luts)
{
    clahe_interp422_nv12_global_body<OFF>(p, Table422Nv12{l}, g, luts);
}

}  // namespace mi
