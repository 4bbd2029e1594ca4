// packed422.hip.h -- the four pixel-touching stages on packed 4:2:2 frames (YUY2 / UYVY): histogram partials, LUT apply, CLAHE tile
// histograms, CLAHE interpolation.  Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
//
// A frame is rows of W / 2 macropixels; a macropixel is ONE dword -- Y0 U Y1 V (OFF = 0: luma in bytes 0 and 2) or U Y0 V Y1 (OFF = 1:
// bytes 1 and 3).  Pointers and pitches are multiples of 4, never assumed to be multiples of 16: a row is walked as 16-byte slots cut at
// the row's own 16-byte boundaries, the ragged first and last slot of a row dword by dword (Slot422).  The luma is counted / mapped in
// place in the dword and the output dword assembled from the two new luma bytes and the input's chroma bytes or 0x80: no byte stores.
// Everything that never touches pixels (LUT arithmetic, scans, LDS histogram helpers, the CLAHE blend) is the planar kernels' own code.
#pragma once
#include "common.hip.h"
#include "equalize.hip.h"
#include "clahe.hip.h"

namespace mi {

// A batch of packed frames: frame f at base + f * frame stride, `rows` rows of `dwords` macropixels at `step` bytes.
struct Packed422 {
    const uint8_t* src;
    uint8_t* dst;
    long long src_step, dst_step;
    long long src_frame, dst_frame;
    int dwords, rows;
    uint32_t keep, fill;              // chroma of an output dword: (input & keep) | fill -- copy: keep = chroma mask, fill128: fill = 0x80s
};

// A list of packed frames, each at its own addresses (mi_*_packed422_frames_dev): the {in, out} pairs travel BY VALUE in the kernel
// arguments like common.hip.h's FrameList -- 16 B an entry, half of an NV12 entry -- and are read with scalar kernarg loads indexed by
// the frame's grid coordinate.  The shape (pitches, dwords, rows, keep / fill) is the launch's Packed422, whose src / dst / *_frame a
// table launch ignores.
#ifndef MI_PACKED422_FRAMES_PER_LAUNCH
#define MI_PACKED422_FRAMES_PER_LAUNCH 128      // 64 or 128: docs/experiments.md has the measurement
#endif
constexpr int kPacked422FramesPerLaunch = MI_PACKED422_FRAMES_PER_LAUNCH;
static_assert(kPacked422FramesPerLaunch == 64 || kPacked422FramesPerLaunch == 128, "a table is 1 or 2 KiB of kernel arguments");
struct Packed422Frame { const uint8_t* in; uint8_t* out; };
struct Packed422List { Packed422Frame f[kPacked422FramesPerLaunch]; };

// Where frame f of a launch lives (the two policies of common.hip.h, on packed frames).  The kernel bodies below are templates on
// one of them: the batch kernels wrap them with the strided policy, which refers to the kernel's own Packed422 argument (the
// arithmetic they always had; the tile histograms use common.hip.h's StridedSource on their src_base / frame_stride pair), the
// *_frames_kernel entries with the table.
struct Strided422 {
    const Packed422& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return p.src + f * p.src_frame; }
    __device__ __forceinline__ uint8_t* dst_of(long long f) const { return p.dst + f * p.dst_frame; }
};
// In place is a frame's own business here (in == out): the apply and interpolation stages are element-wise on a frame whose LUTs are
// already final -- a lane reads a dword and writes that same dword -- so an in-place frame next to an out-of-place one needs no
// ownership logic.
struct Table422 {
    const Packed422List& l;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* dst_of(long long f) const { return l.f[f].out; }
};

template <int OFF> __device__ __forceinline__ uint32_t y0_of(uint32_t w) { return OFF ? (w >> 8) & 0xffu : w & 0xffu; }
template <int OFF> __device__ __forceinline__ uint32_t y1_of(uint32_t w) { return OFF ? w >> 24 : (w >> 16) & 0xffu; }
template <int OFF> __device__ __forceinline__ uint32_t put_y(uint32_t a, uint32_t b) { return OFF ? (a << 8) | (b << 24) : a | (b << 16); }

// Slot k of a row of `dwords` dwords starting at `row`: the dwords [hd - 4 + 4k, hd + 4k) that lie inside the row, hd = dwords before the
// row's first 16-byte boundary.  n == 4: one aligned vector; n < 4 (first / last slot of a row only): dword accesses.  A row has at most
// slots422(dwords) slots.
struct Slot422 { int d0, n; };
__device__ __forceinline__ int slots422(int dwords) { return ((dwords + 3) >> 2) + 1; }
__device__ __forceinline__ Slot422 slot422(const uint8_t* row, int dwords, int k)
{
    const int hd = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);
    const int a = max(hd - 4 + 4 * k, 0), b = min(hd + 4 * k, dwords);
    Slot422 s; s.d0 = a; s.n = max(b - a, 0);
    return s;
}
// the slot's dwords in x, y, z, w order (a ragged slot holds its n < 4 dwords in the first n components)
__device__ __forceinline__ u32x4 load422(const uint8_t* row, int d0, int n)
{
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row) + d0;
    if (n == 4) return *reinterpret_cast<const u32x4_u*>(p);
    u32x4 q = {0u, 0u, 0u, 0u};
    if (n > 0) q.x = p[0];
    if (n > 1) q.y = p[1];
    if (n > 2) q.z = p[2];
    return q;
}
__device__ __forceinline__ void store422(uint8_t* row, int d0, int n, u32x4 q)
{
    uint32_t* p = reinterpret_cast<uint32_t*>(row) + d0;
    if (n == 4) { *reinterpret_cast<u32x4_u*>(p) = q; return; }
    if (n > 0) p[0] = q.x;
    if (n > 1) p[1] = q.y;
    if (n > 2) p[2] = q.z;
}

// counts the luma of the first n dwords of q; skip_first / skip_last: the first luma of the first dword / the last luma of the n-th
// dword lies outside the columns being counted (a CLAHE tile that starts or ends on an odd column)
template <int OFF>
__device__ __forceinline__ void hist422_add(uint32_t* h, u32x4 q, int n, bool skip_first, bool skip_last, uint32_t copy)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    if (n == 4 && !skip_first && !skip_last) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lds_inc(h, (y0_of<OFF>(w[j]) << kCopyShift) + copy);
            lds_inc(h, (y1_of<OFF>(w[j]) << kCopyShift) + copy);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) {
            if (!(skip_first && j == 0)) lds_inc(h, (y0_of<OFF>(w[j]) << kCopyShift) + copy);
            if (!(skip_last && j == n - 1)) lds_inc(h, (y1_of<OFF>(w[j]) << kCopyShift) + copy);
        }
}

// ---------------------------------------------------------------------------------------------
// K1p  histogram partials of the luma.  grid = (B, n_frames); partial[f][b][256] as hist_partial_kernel writes them.  A workgroup takes
// a band of rows and walks it as (row, slot) items NT apart, four loads in flight per lane.  Reads the chroma too (same cache lines).
// ---------------------------------------------------------------------------------------------
template <int OFF, class Frames>
__device__ __forceinline__ void hist422_partial_body(const Packed422& p, const Frames& fr, uint32_t* __restrict__ partial)
{
    constexpr int NT = kHistThreads;
    __shared__ uint32_t h[256 * kCopies];
    lds_hist_zero(h);
    const int t = threadIdx.x;
    const uint32_t copy = t & (kCopies - 1);
    const int r0 = (int)((long long)p.rows * blockIdx.x / gridDim.x), r1 = (int)((long long)p.rows * (blockIdx.x + 1) / gridDim.x);
    const uint8_t* row0 = fr.src_of(blockIdx.y) + (long long)r0 * p.src_step;
    const int S = slots422(p.dwords);
    const long long items = (long long)(r1 - r0) * S;
    int row = t / S, slot = t - row * S;
    const int drow = NT / S, dslot = NT - drow * S;
    for (long long it = t; it < items; it += 4 * NT) {
        u32x4 q[4]; int qn[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* rp = row0 + (long long)row * p.src_step;
            const Slot422 s = slot422(rp, p.dwords, slot);
            qn[k] = it + (long long)k * NT < items ? s.n : 0;
            q[k] = load422(rp, s.d0, qn[k]);
            row += drow; slot += dslot;
            if (slot >= S) { slot -= S; ++row; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) hist422_add<OFF>(h, q[k], qn[k], false, false, copy);
    }
    __syncthreads();
    if (t < 256) partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + t] = lds_hist_bin(h, t);
}
template <int OFF>
__global__ __launch_bounds__(kHistThreads) void hist422_partial_kernel(Packed422 p, uint32_t* __restrict__ partial)
{
    hist422_partial_body<OFF>(p, Strided422{p}, partial);
}
template <int OFF>
__global__ __launch_bounds__(kHistThreads) void hist422_partial_frames_kernel(Packed422List l, Packed422 p, uint32_t* __restrict__ partial)
{
    hist422_partial_body<OFF>(p, Table422{l}, partial);
}

// ---------------------------------------------------------------------------------------------
// K3p  LUT apply on the luma, chroma copied or set to 128, one full dword written per macropixel.  grid = (B, n_frames).
// Slots are cut at the DESTINATION row's 16-byte boundaries (aligned vector stores; the source loads take whatever alignment they have).
// ---------------------------------------------------------------------------------------------
template <int OFF>
__device__ __forceinline__ uint32_t lut422_dword(const uint32_t* lut, uint32_t w, uint32_t copy, uint32_t keep, uint32_t fill)
{
    const uint32_t a = lut[(y0_of<OFF>(w) << kCopyShift) + copy];
    const uint32_t b = lut[(y1_of<OFF>(w) << kCopyShift) + copy];
    return put_y<OFF>(a, b) | (w & keep) | fill;
}

template <int OFF, class Frames>
__device__ __forceinline__ void lut_apply422_body(const Packed422& p, const Frames& fr, const uint8_t* __restrict__ luts)
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
    const int r0 = (int)((long long)p.rows * blockIdx.x / gridDim.x), r1 = (int)((long long)p.rows * (blockIdx.x + 1) / gridDim.x);
    const uint8_t* src0 = fr.src_of(f) + (long long)r0 * p.src_step;
    uint8_t* dst0 = fr.dst_of(f) + (long long)r0 * p.dst_step;
    const int S = slots422(p.dwords);
    const long long items = (long long)(r1 - r0) * S;
    int row = t / S, slot = t - row * S;
    const int drow = kThreads / S, dslot = kThreads - drow * S;
    for (long long it = t; it < items; it += 4 * kThreads) {
        u32x4 q[4]; int qn[4], qd[4]; uint8_t* dr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dr[k] = dst0 + (long long)row * p.dst_step;
            const Slot422 s = slot422(dr[k], p.dwords, slot);
            qn[k] = it + (long long)k * kThreads < items ? s.n : 0;
            qd[k] = s.d0;
            q[k] = load422(src0 + (long long)row * p.src_step, s.d0, qn[k]);
            row += drow; slot += dslot;
            if (slot >= S) { slot -= S; ++row; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (qn[k] == 0) continue;
            u32x4 o;
            o.x = lut422_dword<OFF>(lut, q[k].x, copy, p.keep, p.fill); o.y = lut422_dword<OFF>(lut, q[k].y, copy, p.keep, p.fill);
            o.z = lut422_dword<OFF>(lut, q[k].z, copy, p.keep, p.fill); o.w = lut422_dword<OFF>(lut, q[k].w, copy, p.keep, p.fill);
            store422(dr[k], qd[k], qn[k], o);
        }
    }
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void lut_apply422_kernel(Packed422 p, const uint8_t* __restrict__ luts)
{
    lut_apply422_body<OFF>(p, Strided422{p}, luts);
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void lut_apply422_frames_kernel(Packed422List l, Packed422 p, const uint8_t* __restrict__ luts)
{
    lut_apply422_body<OFF>(p, Table422{l}, luts);
}

// ---------------------------------------------------------------------------------------------
// K4p  per-tile luma histograms (tile_hist_kernel's grid, splits, XCD map and LUT fold).  The in-frame columns [x0, x0 + in_w) of a
// tile row are the dwords [x0 / 2, (x0 + in_w + 1) / 2): a tile that starts or ends on an odd column shares its first / last dword with
// its neighbour and counts one luma of it.  Rows beyond the frame by index reflection; reflected columns (right border tiles) byte loads.
// ---------------------------------------------------------------------------------------------
template <int OFF, int NT, class Frames>
__device__ __forceinline__ void tile_hist422_body(const Frames& fr, long long step, const ClaheGeom& g, uint32_t* __restrict__ partial,
                                                  uint8_t* __restrict__ luts, int xcd_map)
{
    __shared__ uint32_t h[256 * kCopies];                       // 32 KiB; the scans reuse h[0..3] once h is folded
    uint32_t* const s_wave = h;
    const int t = threadIdx.x;
    for (int i = t; i < 256 * kCopies; i += NT) h[i] = 0;
    __syncthreads();
    const uint32_t copy = t & (kCopies - 1);
    const int S = gridDim.x, s = blockIdx.x, f = blockIdx.z;
    const int ntiles = gridDim.y;
    const int tile = xcd_map ? ((int)(blockIdx.y & 7) * (ntiles >> 3) + (int)(blockIdx.y >> 3)) : (int)blockIdx.y;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const uint8_t* src = fr.src_of(f);
    const int r0 = (int)((long long)g.tile_h * s / S), r1 = (int)((long long)g.tile_h * (s + 1) / S);
    const int x0 = tx * g.tile_w;
    const int in_w = max(0, min(g.tile_w, g.width - x0));     // columns of this tile that lie inside the frame
    if (in_w > 0) {
        const int dA = x0 >> 1, nd = ((x0 + in_w + 1) >> 1) - dA;
        const bool odd_first = x0 & 1, odd_last = (x0 + in_w) & 1;
        const int RS = slots422(nd);
        const long long items = (long long)(r1 - r0) * RS;
        int row = t / RS, slot = t - row * RS;
        const int drow = NT / RS, dslot = NT - drow * RS;
        for (long long it = t; it < items; it += 4 * NT) {
            u32x4 q[4]; int qn[4]; bool qf[4], ql[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = reflect101(ty * g.tile_h + r0 + row, g.height);
                const uint8_t* rp = src + (long long)y * step + ((long long)dA << 2);
                const Slot422 sl = slot422(rp, nd, slot);
                qn[k] = it + (long long)k * NT < items ? sl.n : 0;
                qf[k] = odd_first && sl.d0 == 0;
                ql[k] = odd_last && sl.d0 + sl.n == nd;
                q[k] = load422(rp, sl.d0, qn[k]);
                row += drow; slot += dslot;
                if (slot >= RS) { slot -= RS; ++row; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) hist422_add<OFF>(h, q[k], qn[k], qf[k], ql[k], copy);
        }
    }
    if (in_w < g.tile_w) {                                      // reflected columns (right border tiles only)
        const int pw = g.tile_w - in_w;
        const long long items = (long long)(r1 - r0) * pw;
        for (long long it = t; it < items; it += NT) {
            const int row = (int)(it / pw), c = (int)(it - (long long)row * pw);
            const int y = reflect101(ty * g.tile_h + r0 + row, g.height);
            const int x = reflect101(x0 + in_w + c, g.width);
            lds_inc(h, ((uint32_t)src[(long long)y * step + 2 * (long long)x + OFF] << kCopyShift) + copy);
        }
    }
    __syncthreads();
    if (NT > kThreads && t >= kThreads) return;                 // the fold and the LUT are 256-thread stages
    const uint32_t bin = lds_hist_bin(h, t);
    __syncthreads();                                            // everybody has folded its bin: h[0..3] becomes the scan scratch
    if (luts) luts[((size_t)f * gridDim.y + tile) * 256 + t] = tile_lut_value(bin, g, s_wave);     // host passes luts only when S == 1
    else partial[(((size_t)f * gridDim.y + tile) * S + s) * 256 + t] = bin;
}
template <int OFF, int NT>
__global__ __launch_bounds__(NT) void tile_hist422_kernel(const uint8_t* __restrict__ src_base, long long step, long long frame_stride,
                                                         ClaheGeom g, uint32_t* __restrict__ partial, uint8_t* __restrict__ luts, int xcd_map)
{
    tile_hist422_body<OFF, NT>(StridedSource{src_base, frame_stride}, step, g, partial, luts, xcd_map);
}
template <int OFF, int NT>
__global__ __launch_bounds__(NT) void tile_hist422_frames_kernel(Packed422List l, long long step, ClaheGeom g, uint32_t* __restrict__ partial,
                                                                uint8_t* __restrict__ luts, int xcd_map)
{
    tile_hist422_body<OFF, NT>(Table422{l}, step, g, partial, luts, xcd_map);
}

// ---------------------------------------------------------------------------------------------
// K6p  bilinear interpolation of the tile LUTs on the luma (clahe_interp_kernel's grid, bands, pair tables and column segments:
// interp_stage in clahe.hip.h).
// A lane owns 16 columns = 8 dwords of a row: two 16-byte loads, the 16 luma bytes gathered into four dwords (v_perm_b32), blended by the
// planar kernel's own clahe_vec16 / clahe_vec16_f32, and scattered back between the chroma bytes (v_perm_b32 again), two 16-byte stores.
// Rows are only dword aligned, so these are unaligned-capable vector accesses, like the planar kernel's stores.
// ---------------------------------------------------------------------------------------------
template <int OFF>
__device__ __forceinline__ u32x4 gather422(const u32x4& a, const u32x4& b)      // 16 luma bytes of 8 consecutive dwords
{
    constexpr uint32_t sel = OFF ? 0x07050301u : 0x06040200u;
    u32x4 y;
    y.x = __builtin_amdgcn_perm(a.y, a.x, sel); y.y = __builtin_amdgcn_perm(a.w, a.z, sel);
    y.z = __builtin_amdgcn_perm(b.y, b.x, sel); y.w = __builtin_amdgcn_perm(b.w, b.z, sel);
    return y;
}
// two output dwords from four new luma bytes `y` and the chroma source dwords c0, c1 (input & keep | fill)
template <int OFF>
__device__ __forceinline__ uint32_t scatter422_lo(uint32_t y, uint32_t c) { return __builtin_amdgcn_perm(c, y, OFF ? 0x01060004u : 0x07010500u); }
template <int OFF>
__device__ __forceinline__ uint32_t scatter422_hi(uint32_t y, uint32_t c) { return __builtin_amdgcn_perm(c, y, OFF ? 0x03060204u : 0x07030502u); }

template <bool FT, bool FMA, int OFF, class Frames>
__device__ __forceinline__ void clahe_interp422_body(const Packed422& p, const Frames& fr, const ClaheGeom g, const uint8_t* __restrict__ luts,
                                                     int subs, int groups, int pair_cap)
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
    uint8_t* dst = fr.dst_of(f) + 2LL * x0;
    const bool full = x0 + kInterpPx <= g.width;
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
            u32x4 oa, ob;
            oa.x = scatter422_lo<OFF>(o.x, (a.x & p.keep) | p.fill); oa.y = scatter422_hi<OFF>(o.x, (a.y & p.keep) | p.fill);
            oa.z = scatter422_lo<OFF>(o.y, (a.z & p.keep) | p.fill); oa.w = scatter422_hi<OFF>(o.y, (a.w & p.keep) | p.fill);
            ob.x = scatter422_lo<OFF>(o.z, (b.x & p.keep) | p.fill); ob.y = scatter422_hi<OFF>(o.z, (b.y & p.keep) | p.fill);
            ob.z = scatter422_lo<OFF>(o.w, (b.z & p.keep) | p.fill); ob.w = scatter422_hi<OFF>(o.w, (b.w & p.keep) | p.fill);
            u32x4_u* d = reinterpret_cast<u32x4_u*>(dst + (long long)yy * p.dst_step);
            d[0] = oa; d[1] = ob;
        };
        // 32 bytes per lane and row: two rows in flight give a lane the planar float-table kernel's 64 bytes in flight
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
        for (; y < ya_hi; y += phases) {
            const float tyf = tile_coord<FMA>(y, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            const uint32_t* sr = reinterpret_cast<const uint32_t*>(src + (long long)y * p.src_step);
            uint32_t* dr = reinterpret_cast<uint32_t*>(dst + (long long)y * p.dst_step);
#pragma unroll
            for (int d = 0; d < kInterpPx / 2; ++d)
                if (x0 + 2 * d < g.width) {                    // W is even: both columns of the dword are inside
                    const uint32_t w = sr[d];
                    uint32_t e[2];
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int j = 2 * d + b;
                        const uint32_t v = b ? y1_of<OFF>(w) : y0_of<OFF>(w);
                        if (FT) {
                            const f32x4 fe = quadf[poff[j] + v];
                            e[b] = (uint32_t)fe.x | ((uint32_t)fe.z << 8) | ((uint32_t)fe.y << 16) | ((uint32_t)fe.w << 24);
                        } else {
                            e[b] = quad[poff[j] + v];
                        }
                        e[b] = clahe_px<FMA>(e[b], xa[j], xa1[j], ya, ya1);
                    }
                    dr[d] = put_y<OFF>(e[0], e[1]) | (w & p.keep) | p.fill;
                }
        }
    }
}
template <bool FT, bool FMA, int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_kernel(Packed422 p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                  int subs, int groups, int pair_cap)
{
    clahe_interp422_body<FT, FMA, OFF>(p, Strided422{p}, g, luts, subs, groups, pair_cap);
}
template <bool FT, bool FMA, int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_frames_kernel(Packed422List l, Packed422 p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                         int subs, int groups, int pair_cap)
{
    clahe_interp422_body<FT, FMA, OFF>(p, Table422{l}, g, luts, subs, groups, pair_cap);
}

// Fallback for tile grids too wide for the LDS pair table (clahe_interp_global_kernel's arithmetic): one macropixel per thread, the LUTs
// gathered from global memory (L2).  grid = (ceil(W / 2 / 256), H, n_frames).
template <int OFF, class Frames>
__device__ __forceinline__ void clahe_interp422_global_body(const Packed422& p, const Frames& fr, const ClaheGeom& g, const uint8_t* __restrict__ luts)
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
    reinterpret_cast<uint32_t*>(fr.dst_of(f) + (long long)y * p.dst_step)[d] = put_y<OFF>(e[0], e[1]) | (w & p.keep) | p.fill;
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_global_kernel(Packed422 p, ClaheGeom g, const uint8_t* __restrict__ luts)
{
    clahe_interp422_global_body<OFF>(p, Strided422{p}, g, luts);
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_global_frames_kernel(Packed422List l, Packed422 p, ClaheGeom g, const uint8_t* __restrict__ luts)
{
    clahe_interp422_global_body<OFF>(p, Table422{l}, g, luts);
}

}  // namespace mi
