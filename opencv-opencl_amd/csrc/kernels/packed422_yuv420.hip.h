// packed422_yuv420.hip.h -- the pixel-WRITING stages of "packed 4:2:2 in (YUY2 / UYVY), planar 4:2:0 out (I420 / YV12)": LUT apply, CLAHE
// interpolation and its wide-grid fallback.  Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
//
// The histogram stages are packed422.hip.h's own, unchanged (they only read), and the walks are packed422_nv12.hip.h's: what differs is
// where the chroma goes.  The 16 chroma bytes U0 V0 U1 V1 ... of a row pair, halved vertically with (a + b + 1) >> 1 (mean_up_u8x16),
// are de-interleaved in registers -- v_perm_b32 with the kEven / kOdd selectors of yuv420.hip.h -- and leave as ONE 8-byte store into
// the U row and ONE into the V row, in the launch that writes the luma: a software encoder's three planes without an NV12 intermediate.
// Chroma rows start at multiples of 4 (pointers and pitches are), a lane's 8 samples at a multiple of 8 inside the row: full groups are
// 8-byte stores at 4-byte aligned addresses, the ragged last group of a row (nd < 8 macropixels) is one dword when nd >= 4, then one
// 2-byte store, then one byte.  Nothing beyond column W of a Y row or column W/2 of a chroma row.
#pragma once
#include "packed422_nv12.hip.h"
#include "yuv420.hip.h"

namespace mi {

// A batch of packed frames in, three planes out: frame f reads src + f * src_frame and writes y / u / v + f * out_frame.
struct Packed422Yuv420 {
    const uint8_t* src;
    uint8_t* y;
    uint8_t* u;
    uint8_t* v;
    long long src_step, y_step, c_step;   // both chroma planes share the pitch
    long long src_frame, out_frame;
    int dwords, rows;                     // macropixels per row (W / 2), rows (H, even)
    int copy_uv;                          // 1: MI_UV_COPY (row-pair mean of the input chroma), 0: every chroma byte 128
};

struct Strided422Yuv420 {
    const Packed422Yuv420& p;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return p.src + f * p.src_frame; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return p.y + f * p.out_frame; }
    __device__ __forceinline__ uint8_t* u_of(long long f) const { return p.u + f * p.out_frame; }
    __device__ __forceinline__ uint8_t* v_of(long long f) const { return p.v + f * p.out_frame; }
};

// A list of such frames, each at its own four addresses (mi_*_packed422_to_yuv420_frames_dev: a capture pool in, a software encoder's
// frame pool out).  The {in, y, c0, c1} entries travel BY VALUE in the kernel arguments -- 32 B an entry, kFramesPerLaunch (64) of them
// are 2 KiB -- and are read with scalar kernarg loads indexed by the frame's grid coordinate.  The shape is the launch's
// Packed422Yuv420, whose src / y / u / v / *_frame a table launch ignores.
struct Packed422Yuv420Frame { const uint8_t* in; uint8_t* y; uint8_t* c0; uint8_t* c1; };
struct Packed422Yuv420List { Packed422Yuv420Frame f[kFramesPerLaunch]; };
static_assert(sizeof(Packed422Yuv420Frame) == 32, "four addresses an entry");
// clahe_interp422_yuv420_frames_kernel(l, p, g, luts, subs, groups, pair_cap) is the longest list; 256: the implicit arguments
static_assert(sizeof(Packed422Yuv420List) + sizeof(Packed422Yuv420) + 8 + sizeof(ClaheGeom) + 8 + sizeof(const uint8_t*) + 3 * sizeof(int) + 8 + 256 <= 4096,
              "the table and the largest remaining argument list stay within HIP's 4 KiB of kernel arguments");
struct Table422Yuv420 {
    const Packed422Yuv420List& l;
    __device__ __forceinline__ const uint8_t* src_of(long long f) const { return l.f[f].in; }
    __device__ __forceinline__ uint8_t* y_of(long long f) const { return l.f[f].y; }
    __device__ __forceinline__ uint8_t* u_of(long long f) const { return l.f[f].c0; }
    __device__ __forceinline__ uint8_t* v_of(long long f) const { return l.f[f].c1; }
};

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));            // a chroma group starts at a multiple of 4, not always of 8

// 16 bytes U0 V0 U1 V1 ... U7 V7 -> U0 .. U7 and V0 .. V7 (unzip_uv's selectors on half its width)
__device__ __forceinline__ void unzip_uv8(const u32x4& m, u32x2& u, u32x2& v)
{
    u.x = __builtin_amdgcn_perm(m.y, m.x, kEven); u.y = __builtin_amdgcn_perm(m.w, m.z, kEven);
    v.x = __builtin_amdgcn_perm(m.y, m.x, kOdd);  v.y = __builtin_amdgcn_perm(m.w, m.z, kOdd);
}
// the first nd < 8 bytes of q at a 4-byte aligned address: one dword if nd >= 4, then one 2-byte store, then one byte
__device__ __forceinline__ void store_c_tail(uint8_t* dst, const u32x2& q, int nd)
{
    uint32_t w = q.x;
    if (nd >= 4) { *reinterpret_cast<uint32_t*>(dst) = w; w = q.y; dst += 4; }
    if (nd & 2) { *reinterpret_cast<uint16_t*>(dst) = (uint16_t)w; w >>= 16; dst += 2; }
    if (nd & 1) *dst = (uint8_t)w;
}

// ---------------------------------------------------------------------------------------------
// K3y  LUT apply, packed -> planar 4:2:0.  lut_apply422_nv12_body's walk: grid = (B, n_frames), a workgroup takes a band of ROW PAIRS
// and walks it as (pair, 16-column group) items kThreads apart; an item is four 16-byte loads, 32 LUT reads, two 16-byte Y stores, one
// 8-byte U store and one 8-byte V store.  The input is read once, there is no chroma launch.
// ---------------------------------------------------------------------------------------------
template <int OFF, class Frames>
__device__ __forceinline__ void lut_apply422_yuv420_body(const Packed422Yuv420& p, const Frames& fr, const uint8_t* __restrict__ luts)
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
    uint8_t* u0 = fr.u_of(f) + (long long)r0 * p.c_step;
    uint8_t* v0 = fr.v_of(f) + (long long)r0 * p.c_step;
    const int G = (p.dwords + 7) >> 3;                          // 16-column groups per row, the last one possibly ragged
    const long long items = (long long)(r1 - r0) * G;
    int pr = t / G, grp = t - pr * G;
    const int dpr = kThreads / G, dgrp = kThreads - dpr * G;
    const u32x4 fill = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    for (long long it = t; it < items; it += kThreads) {
        const uint8_t* s = src0 + 2LL * pr * p.src_step + 32LL * grp;
        uint8_t* dy = y0 + 2LL * pr * p.y_step + 16LL * grp;
        uint8_t* du = u0 + (long long)pr * p.c_step + 8LL * grp;
        uint8_t* dv = v0 + (long long)pr * p.c_step + 8LL * grp;
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
        u32x2 cu, cv;
        unzip_uv8(m, cu, cv);
        if (nd == 8) {
            *reinterpret_cast<u32x4_u*>(dy) = o0;
            *reinterpret_cast<u32x4_u*>(dy + p.y_step) = o1;
            *reinterpret_cast<u32x2_a4*>(du) = cu;
            *reinterpret_cast<u32x2_a4*>(dv) = cv;
        } else {
            store_nv12_tail(dy, o0, nd);
            store_nv12_tail(dy + p.y_step, o1, nd);
            store_c_tail(du, cu, nd);
            store_c_tail(dv, cv, nd);
        }
        pr += dpr; grp += dgrp;
        if (grp >= G) { grp -= G; ++pr; }
    }
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void lut_apply422_yuv420_kernel(Packed422Yuv420 p, const uint8_t* __restrict__ luts)
{
    lut_apply422_yuv420_body<OFF>(p, Strided422Yuv420{p}, luts);
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void lut_apply422_yuv420_frames_kernel(Packed422Yuv420List l, Packed422Yuv420 p, const uint8_t* __restrict__ luts)
{
    lut_apply422_yuv420_body<OFF>(p, Table422Yuv420{l}, luts);
}

// ---------------------------------------------------------------------------------------------
// K6y  CLAHE interpolation, packed -> planar 4:2:0: clahe_interp422_nv12_body's grid, bands, pair tables, column segments and blend.
// Bands are cut by tile-row coordinate, so the two rows of a chroma pair may belong to different bands (and lanes): the lane that owns
// the EVEN row y of a pair also loads the chroma of row y + 1 and writes U row y / 2 and V row y / 2 in the same launch.  Every row
// belongs to exactly one band, so every chroma row is written exactly once.  With MI_UV_FILL128 there is no second read.
// ---------------------------------------------------------------------------------------------
template <bool FT, bool FMA, int OFF, class Frames>
__device__ __forceinline__ void clahe_interp422_yuv420_body(const Packed422Yuv420& p, const Frames& fr, const ClaheGeom g,
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
    uint8_t* dy = fr.y_of(f) + x0;
    uint8_t* du = fr.u_of(f) + (x0 >> 1);
    uint8_t* dv = fr.v_of(f) + (x0 >> 1);
    const bool full = x0 + kInterpPx <= g.width;
    const bool copy_uv = p.copy_uv != 0;
    auto ty1_of = [&](int y) { return floor_f32_to_int(tile_coord<FMA>(y, g.inv_th)); };
    int ya_lo = y_lo, ya_hi = y_hi;
    while (ya_lo < ya_hi && ty1_of(ya_lo) != ty1u) ++ya_lo;
    while (ya_hi > ya_lo && ty1_of(ya_hi - 1) != ty1u) --ya_hi;
    int y = ya_lo + ((phase - (ya_lo - y_lo) % phases) % phases + phases) % phases;
    if (full) {
        const u32x4 fill = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
        // c, d: the dwords of row yy + 1, loaded only where this lane writes the chroma rows (yy even, MI_UV_COPY)
        auto do_row = [&](int yy, const u32x4& a, const u32x4& b, const u32x4& c, const u32x4& d) {
            const float tyf = tile_coord<FMA>(yy, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            const u32x4 q = gather422<OFF>(a, b);
            const u32x4 o = FT ? clahe_vec16_f32<FMA>(quadf, q, poff, xw, ya, ya1) : clahe_vec16<FMA>(quad, q, poff, xa, xa1, ya, ya1);
            *reinterpret_cast<u32x4_u*>(dy + (long long)yy * p.y_step) = o;
            if (!(yy & 1)) {
                const u32x4 m = copy_uv ? mean_up_u8x16(chroma422<OFF>(a, b), chroma422<OFF>(c, d)) : fill;
                u32x2 cu, cv;
                unzip_uv8(m, cu, cv);
                *reinterpret_cast<u32x2_a4*>(du + (long long)(yy >> 1) * p.c_step) = cu;
                *reinterpret_cast<u32x2_a4*>(dv + (long long)(yy >> 1) * p.c_step) = cv;
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
        // two rows in flight per lane, as clahe_interp422_nv12_body
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
        const int nd = (g.width - x0) >> 1;                    // 1 .. 7 macropixels (W is even)
        for (; y < ya_hi; y += phases) {
            const float tyf = tile_coord<FMA>(y, g.inv_th);
            const float ya = __fsub_rn(tyf, (float)ty1u), ya1 = __fsub_rn(1.0f, ya);
            const uint32_t* sr = reinterpret_cast<const uint32_t*>(src + (long long)y * p.src_step);
            const uint32_t* sr1 = reinterpret_cast<const uint32_t*>(src + (long long)(y + 1) * p.src_step);     // read only when y is even
            uint16_t* yr = reinterpret_cast<uint16_t*>(dy + (long long)y * p.y_step);
            const bool chroma_row = !(y & 1);
            u32x2 cu = {0u, 0u}, cv = {0u, 0u};
#pragma unroll
            for (int dd = 0; dd < kInterpPx / 2; ++dd)
                if (dd < nd) {
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
                    if (chroma_row) {
                        const uint32_t m = copy_uv ? mean_up_u8x4(chroma422_px<OFF>(w), chroma422_px<OFF>(sr1[dd])) : 0x8080u;
                        const uint32_t sh = 8u * (dd & 3);
                        if (dd < 4) { cu.x |= (m & 0xffu) << sh; cv.x |= ((m >> 8) & 0xffu) << sh; }
                        else        { cu.y |= (m & 0xffu) << sh; cv.y |= ((m >> 8) & 0xffu) << sh; }
                    }
                }
            if (chroma_row) {
                store_c_tail(du + (long long)(y >> 1) * p.c_step, cu, nd);
                store_c_tail(dv + (long long)(y >> 1) * p.c_step, cv, nd);
            }
        }
    }
}
template <bool FT, bool FMA, int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_yuv420_kernel(Packed422Yuv420 p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                         int subs, int groups, int pair_cap)
{
    clahe_interp422_yuv420_body<FT, FMA, OFF>(p, Strided422Yuv420{p}, g, luts, subs, groups, pair_cap);
}
template <bool FT, bool FMA, int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_yuv420_frames_kernel(Packed422Yuv420List l, Packed422Yuv420 p, ClaheGeom g,
                                                                                const uint8_t* __restrict__ luts, int subs, int groups, int pair_cap)
{
    clahe_interp422_yuv420_body<FT, FMA, OFF>(p, Table422Yuv420{l}, g, luts, subs, groups, pair_cap);
}

// Fallback for tile grids too wide for the LDS pair table (clahe_interp422_nv12_global_body's arithmetic): one macropixel per thread,
// the LUTs gathered from global memory (L2), two luma bytes to the Y plane as one 2-byte store; the thread of an even row also reads the
// macropixel below it and writes one U byte and one V byte.  grid = (ceil(W / 2 / 256), H, n_frames).
template <int OFF, class Frames>
__device__ __forceinline__ void clahe_interp422_yuv420_global_body(const Packed422Yuv420& p, const Frames& fr, const ClaheGeom& g,
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
        (fr.u_of(f) + (long long)(y >> 1) * p.c_step)[d] = (uint8_t)m;
        (fr.v_of(f) + (long long)(y >> 1) * p.c_step)[d] = (uint8_t)(m >> 8);
    }
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_yuv420_global_kernel(Packed422Yuv420 p, ClaheGeom g, const uint8_t* __restrict__ luts)
{
    clahe_interp422_yuv420_global_body<OFF>(p, Strided422Yuv420{p}, g, luts);
}
template <int OFF>
__global__ __launch_bounds__(kThreads) void clahe_interp422_yuv420_global_frames_kernel(Packed422Yuv420List l, Packed422Yuv420 p, ClaheGeom g,
                                                                                       const uint8_t* __restrict__ luts)
{
    clahe_interp422_yuv420_global_body<OFF>(p, Table422Yuv420{l}, g, luts);
}

}  // namespace mi
