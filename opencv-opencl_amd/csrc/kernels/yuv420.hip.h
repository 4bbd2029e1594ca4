// yuv420.hip.h -- the chroma of 8-bit 4:2:0 frames whose two sides say where their planes lie: interleaved (NV12) or planar (I420 / YV12)
// Part of the gfx950 kernel set of libmi_lumaeq (see ../lumaeq_kernels.hip.h for the design notes).
#pragma once
#include "equalize.hip.h"

namespace mi {
// =============================================================================================
// mi_*_yuv420*: the luma is the planar forms' own (equalize_dev / clahe_dev on the Y planes); this file carries the chroma from the
// input's layout into the output's -- U and V interleaved into one plane of W-byte rows, or two planes of W/2-byte rows -- or fills the
// output's planes with 128.  A pure streaming kernel: no LDS, no arithmetic but the byte shuffle of a layout change, which v_perm_b32
// does in registers (packed422.hip.h's split422 is the precedent).  c0 is always the U plane and c1 the V plane; a YV12 frame is the
// same planes handed over in the other order of addresses, decided by the caller.
// =============================================================================================
struct Yuv420Side {
    uint8_t* c0; uint8_t* c1;                 // interleaved: c0 = UV plane, c1 unused; planar: c0 = U plane, c1 = V plane
    long long step;                           // bytes between chroma rows (both planes of a planar side)
    long long frame;                          // bytes between frames
    int planar;
};
struct Yuv420Job {
    Yuv420Side in, out;                       // in.c0 / in.c1 are only read
    int width;                                // W (even): an interleaved row holds W bytes, a planar row W/2
    int rows;                                 // H/2
    int mode;                                 // 0 = fill 128, 1 = copy
    int vec;                                  // layout change: 1 = W % 32 == 0 and every chroma address, pitch and frame stride a multiple of 16
    int flat;                                 // same layout: 1 = the rows the launch touches are tight on every side it touches
    int skip0, skip1;                         // same-layout copy: the plane is the same plane on both sides (in place), nothing to move
};

// selectors of v_perm_b32(hi, lo, sel): byte k of the result is byte sel[k] of {lo: 0..3, hi: 4..7}
constexpr uint32_t kZipLo = 0x05010400u, kZipHi = 0x07030602u;      // (hi = V word, lo = U word) -> U0 V0 U1 V1 / U2 V2 U3 V3
constexpr uint32_t kEven = 0x06040200u, kOdd = 0x07050301u;         // (hi = second UV word, lo = first) -> U0 U1 U2 U3 / V0 V1 V2 V3

// 16 U and 16 V bytes -> 32 interleaved bytes
__device__ __forceinline__ void zip_uv(const u32x4 u, const u32x4 v, u32x4& lo, u32x4& hi)
{
    lo.x = __builtin_amdgcn_perm(v.x, u.x, kZipLo); lo.y = __builtin_amdgcn_perm(v.x, u.x, kZipHi);
    lo.z = __builtin_amdgcn_perm(v.y, u.y, kZipLo); lo.w = __builtin_amdgcn_perm(v.y, u.y, kZipHi);
    hi.x = __builtin_amdgcn_perm(v.z, u.z, kZipLo); hi.y = __builtin_amdgcn_perm(v.z, u.z, kZipHi);
    hi.z = __builtin_amdgcn_perm(v.w, u.w, kZipLo); hi.w = __builtin_amdgcn_perm(v.w, u.w, kZipHi);
}
// 32 interleaved bytes -> 16 U and 16 V bytes
__device__ __forceinline__ void unzip_uv(const u32x4 lo, const u32x4 hi, u32x4& u, u32x4& v)
{
    u.x = __builtin_amdgcn_perm(lo.y, lo.x, kEven); u.y = __builtin_amdgcn_perm(lo.w, lo.z, kEven);
    u.z = __builtin_amdgcn_perm(hi.y, hi.x, kEven); u.w = __builtin_amdgcn_perm(hi.w, hi.z, kEven);
    v.x = __builtin_amdgcn_perm(lo.y, lo.x, kOdd); v.y = __builtin_amdgcn_perm(lo.w, lo.z, kOdd);
    v.z = __builtin_amdgcn_perm(hi.y, hi.x, kOdd); v.w = __builtin_amdgcn_perm(hi.w, hi.z, kOdd);
}

// A layout change of one frame: `uv` is the interleaved side, (pu, pv) the planar one; TO_PLANAR says which of the two is written.
// vec: an item is one chroma row x 32 output pixels -- two 16-byte loads, the byte shuffle in registers, two 16-byte stores -- four items
// in flight per lane, each predicated on its own bound as in uv_rows; the (row, slot) of a lane's next item is carried (one division per
// lane, none per item).  Otherwise an item is one U, V sample pair moved with byte accesses: any W/2, any address.  Both walks are
// grid-stride over the frame's items: workgroup `part` of `nparts`.
template <bool TO_PLANAR>
__device__ __forceinline__ void yuv420_relayout(uint8_t* uv, long long uv_step, uint8_t* pu, uint8_t* pv, long long p_step,
                                                int width, int rows, int vec, int part, int nparts)
{
    const int t = threadIdx.x;
    const int stride = nparts * kThreads;                           // <= 2048 * 256
    int gi = part * kThreads + t;
    if (vec) {
        const int slots = width >> 5;
        const int items = slots * rows;                             // < 2^25 (W * H < 2^31)
        const int drow = stride / slots, dslot = stride - drow * slots;
        int row = gi / slots, slot = gi - row * slots;
        for (; gi < items; gi += 4 * stride) {
            u32x4 a[4], b[4]; bool qv[4]; long long ouv[4], op[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                qv[k] = gi + k * stride < items;
                ouv[k] = (long long)row * uv_step + ((long long)slot << 5);
                op[k] = (long long)row * p_step + ((long long)slot << 4);
                if (qv[k]) {
                    if (TO_PLANAR) {
                        a[k] = *reinterpret_cast<const u32x4*>(uv + ouv[k]);
                        b[k] = *reinterpret_cast<const u32x4*>(uv + ouv[k] + 16);
                    } else {
                        a[k] = *reinterpret_cast<const u32x4*>(pu + op[k]);
                        b[k] = *reinterpret_cast<const u32x4*>(pv + op[k]);
                    }
                }
                row += drow; slot += dslot;
                if (slot >= slots) { slot -= slots; ++row; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!qv[k]) continue;
                u32x4 x, y;
                if (TO_PLANAR) {
                    unzip_uv(a[k], b[k], x, y);
                    *reinterpret_cast<u32x4*>(pu + op[k]) = x;
                    *reinterpret_cast<u32x4*>(pv + op[k]) = y;
                } else {
                    zip_uv(a[k], b[k], x, y);
                    *reinterpret_cast<u32x4*>(uv + ouv[k]) = x;
                    *reinterpret_cast<u32x4*>(uv + ouv[k] + 16) = y;
                }
            }
        }
    } else {
        const int half = width >> 1;
        const long long pairs = (long long)half * rows;             // < 2^30
        const int drow = stride / half, dx = stride - drow * half;
        int row = gi / half, x = gi - row * half;
        for (long long pi = gi; pi < pairs; pi += stride) {
            const long long ouv = (long long)row * uv_step + 2 * x, op = (long long)row * p_step + x;
            if (TO_PLANAR) { const uint8_t U = uv[ouv], V = uv[ouv + 1]; pu[op] = U; pv[op] = V; }
            else           { const uint8_t U = pu[op], V = pv[op]; uv[ouv] = U; uv[ouv + 1] = V; }
            row += drow; x += dx;
            if (x >= half) { x -= half; ++row; }
        }
    }
}

// One plane of a same-layout move or of a fill: uv_rows / uv_flat as they are (equalize.hip.h), on rows of `row_bytes`.
__device__ __forceinline__ void yuv420_plane(const uint8_t* src, long long src_step, uint8_t* dst, long long dst_step, long long row_bytes,
                                             int rows, int mode, int flat, int part, int nparts)
{
    if (flat) uv_flat(src, dst, row_bytes * rows, mode, part, nparts);
    else uv_rows(src, src_step, dst, dst_step, row_bytes, rows, mode, part, nparts);
}

// grid = (B, frames of the chunk), 256 threads, no LDS.  Every branch below is uniform for the launch (it depends on the job alone).
__global__ __launch_bounds__(kThreads) void yuv420_chroma_kernel(Yuv420Job j)
{
    const long long f = blockIdx.y;
    const int part = blockIdx.x, nparts = gridDim.x;
    uint8_t* o0 = j.out.c0 + f * j.out.frame;
    uint8_t* o1 = j.out.planar ? j.out.c1 + f * j.out.frame : nullptr;
    if (j.mode == 0 || j.in.planar == j.out.planar) {               // fill the output's planes, or move rows between equal layouts
        const uint8_t* i0 = j.mode ? j.in.c0 + f * j.in.frame : nullptr;
        const uint8_t* i1 = j.mode && j.in.planar ? j.in.c1 + f * j.in.frame : nullptr;
        const long long row_bytes = j.out.planar ? j.width >> 1 : j.width;
        if (!j.skip0) yuv420_plane(i0, j.in.step, o0, j.out.step, row_bytes, j.rows, j.mode, j.flat, part, nparts);
        if (j.out.planar && !j.skip1) yuv420_plane(i1, j.in.step, o1, j.out.step, row_bytes, j.rows, j.mode, j.flat, part, nparts);
    } else if (j.out.planar) {
        yuv420_relayout<true>(j.in.c0 + f * j.in.frame, j.in.step, o0, o1, j.out.step, j.width, j.rows, j.vec, part, nparts);
    } else {
        yuv420_relayout<false>(o0, j.out.step, j.in.c0 + f * j.in.frame, j.in.c1 + f * j.in.frame, j.in.step, j.width, j.rows, j.vec,
                               part, nparts);
    }
}

}  // namespace mi
