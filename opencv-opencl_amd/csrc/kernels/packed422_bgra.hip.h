// packed422_bgra.hip.h -- the pixel-WRITING stages of "packed 4:2:2 in (YUY2 / UYVY), interleaved 8-bit four-channel images out
// (BGRA / RGBA: CV_8UC4, A = 255)": LUT apply, CLAHE interpolation and its wide-grid fallback, each with the BT.601 decode behind it.
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
//
// capture card -> display surface / swap-chain image / interop texture / GUI image.  The bodies ARE those of packed422_bgr.hip.h,
// templates on the block type and a store policy -- same grids, bands, carried walks, column segments and blends, the histogram stages
// packed422.hip.h's own, every row decoded with its own chroma, OFF = 0 exactly Y0 U Y1 V and OFF = 1 exactly U Y0 V Y1 -- and this
// file holds what differs, the store of yuv420_bgra.hip.h (Store422Bgra): every pixel is one dword
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
    return packed422_image_wide(out, out_step, out_frame);
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
// The store policy of the bodies of packed422_bgr.hip.h (lut_apply422_bgr_body, clahe_interp422_bgr_body -- one text for both pixel
// forms: grids, bands, carried walks, column segments, the two-rows-in-flight loop, the ragged last group and the blends) for
// four-byte pixels: 64 bytes a group.
// group: the store path is chosen once, outside the loop over the four quarters: each path is a straight run of decode 4, store 4
// (with the branch inside the loop the compiler keeps all sixteen dwords live: 184 VGPRs in the float-table interpolation instead of
// 143).  gfx950 accepts unaligned vector stores, so the compiler may merge the byte path's neighbouring stores into wider unaligned ones.
template <int ORDER> struct Store422Bgra {
    static constexpr int kPxBytes = 4, kGroupBytes = 64;
    static __device__ __forceinline__ void group(uint8_t* p, const u32x4& y, const u32x4& uv, int n, bool wide)
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
};

// K3c  LUT apply + decode, packed -> BGRA / RGBA.  grid = (B, n_frames).  An item is two 16-byte loads, 16 LUT reads, 8 chroma terms,
// 16 pixels decoded and 64 bytes stored.
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void lut_apply422_bgra_kernel(Packed422Bgra p, const uint8_t* __restrict__ luts)
{
    lut_apply422_bgr_body<OFF, Store422Bgra<ORDER>>(p, Strided422Bgra{p}, luts);
}
template <int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void lut_apply422_bgra_frames_kernel(Packed422List l, Packed422Bgra p, const uint8_t* __restrict__ luts)
{
    lut_apply422_bgr_body<OFF, Store422Bgra<ORDER>>(p, Table422Bgra{l, p}, luts);
}

// K6c  CLAHE interpolation + decode, packed -> BGRA / RGBA (all four <FT, FMA> rungs), with dst = out + 4 * x0.
template <bool FT, bool FMA, int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgra_kernel(Packed422Bgra p, ClaheGeom g, const uint8_t* __restrict__ luts,
                                                                       int subs, int groups, int pair_cap)
{
    clahe_interp422_bgr_body<FT, FMA, OFF, Store422Bgra<ORDER>>(p, Strided422Bgra{p}, g, luts, subs, groups, pair_cap);
}
template <bool FT, bool FMA, int OFF, int ORDER>
__global__ __launch_bounds__(kThreads) void clahe_interp422_bgra_frames_kernel(Packed422List l, Packed422Bgra p, ClaheGeom g,
                                                                              const uint8_t* __restrict__ luts, int subs, int groups, int pair_cap)
{
    clahe_interp422_bgr_body<FT, FMA, OFF, Store422Bgra<ORDER>>(p, Table422Bgra{l, p}, g, luts, subs, groups, pair_cap);
}

// Fallback for tile grids too wide for the LDS pair table (clahe_interp422_bgr_global_body's arithmetic): one macropixel per thread,
// the LUTs gathered from global memory (L2), two pixels decoded with the macropixel's own U and V: 8 bytes, as one 8-byte store (dword-aligned)
// when the frame is wide, else as bytes.
// grid = (ceil(W / 2 / 256), H, n_frames).  Written out beside the three-channel one, not shared: see the note there.
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
