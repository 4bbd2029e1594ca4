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

// Whether ONE frame of a layout change moves 16 bytes per access: `shape16` says what the call's shape allows (W % 32 == 0 and both
// c_pitch multiples of 16), the rest is the frame's own four chroma addresses (the c1 of an interleaved side is handed over as null).
// The host counts frames with it (host/yuv420_frames.inc.hpp) and the table policy below branches on it: one function, one answer.
__host__ __device__ __forceinline__ bool yuv420_frame_vec(int shape16, const void* c0_in, const void* c1_in, const void* c0_out,
                                                          const void* c1_out)
{
    return shape16 && (((uintptr_t)c0_in | (uintptr_t)c1_in | (uintptr_t)c0_out | (uintptr_t)c1_out) & 15) == 0;
}

// Where the chroma of frame f of a launch lives and which path it takes, as StridedBgrNv12 / TableBgrNv12 (bgr_nv12.hip.h) say it for
// their kernel: the body below is a template on one of these two policies.  The batch entry wraps it with the strided one -- the
// arithmetic it always had, on the kernel's own argument, every decision the host's for the whole launch.
struct StridedYuv420 {
    const Yuv420Job& j;
    __device__ __forceinline__ uint8_t* in0(long long f) const { return j.in.c0 + f * j.in.frame; }
    __device__ __forceinline__ uint8_t* in1(long long f) const { return j.in.c1 + f * j.in.frame; }
    __device__ __forceinline__ uint8_t* out0(long long f) const { return j.out.c0 + f * j.out.frame; }
    __device__ __forceinline__ uint8_t* out1(long long f) const { return j.out.c1 + f * j.out.frame; }
    __device__ __forceinline__ int vec(long long) const { return j.vec; }
    __device__ __forceinline__ int skip0(long long) const { return j.skip0; }
    __device__ __forceinline__ int skip1(long long) const { return j.skip1; }
};

// A list of such frames, each with its own chroma addresses (mi_*_yuv420_frames_dev: a software decoder's frame pool, an encoder's
// surface pool).  The entries travel BY VALUE in the kernel arguments like FrameList -- 64 x 32 B = 2 KiB, read with scalar kernarg
// loads indexed by the frame's grid coordinate; the Y addresses are not in it (the luma kernels have their own FrameList).  The shape
// (pitches, width, rows, mode, layouts, flat) is the launch's Yuv420Job, whose addresses and frame strides a table launch ignores, whose
// vec says what the SHAPE allows and whose skip0 / skip1 are unused: whether frame f moves 16 bytes per access and which of its planes
// are in place (the same address on both sides: nothing to move under MI_UV_COPY) is decided by its own entry -- per frame, so uniform
// for a workgroup.  With MI_UV_FILL128 the host hands over null input addresses: no plane is skipped.
struct Yuv420Frame { uint8_t* c0_in; uint8_t* c1_in; uint8_t* c0_out; uint8_t* c1_out; };      // c0_in / c1_in are only read
struct Yuv420List { Yuv420Frame f[kFramesPerLaunch]; };
static_assert(sizeof(Yuv420Frame) == 32, "four addresses an entry");
struct TableYuv420 {
    const Yuv420List& l;
    const Yuv420Job& j;
    __device__ __forceinline__ uint8_t* in0(long long f) const { return l.f[f].c0_in; }
    __device__ __forceinline__ uint8_t* in1(long long f) const { return l.f[f].c1_in; }
    __device__ __forceinline__ uint8_t* out0(long long f) const { return l.f[f].c0_out; }
    __device__ __forceinline__ uint8_t* out1(long long f) const { return l.f[f].c1_out; }
    __device__ __forceinline__ int vec(long long f) const
    {
        return yuv420_frame_vec(j.vec, l.f[f].c0_in, l.f[f].c1_in, l.f[f].c0_out, l.f[f].c1_out);
    }
    __device__ __forceinline__ int skip0(long long f) const { return l.f[f].c0_in == l.f[f].c0_out; }
    __device__ __forceinline__ int skip1(long long f) const { return l.f[f].c1_in == l.f[f].c1_out; }
};

// grid = (B, frames of the chunk), 256 threads, no LDS.  Every branch below is uniform for a workgroup: it depends on the job and, with
// the table policy, on the frame's entry.
template <class Frames>
__device__ __forceinline__ void yuv420_chroma_body(const Yuv420Job& j, const Frames& fr)
{
    const long long f = blockIdx.y;
    const int part = blockIdx.x, nparts = gridDim.x;
    uint8_t* o0 = fr.out0(f);
    uint8_t* o1 = j.out.planar ? fr.out1(f) : nullptr;
    if (j.mode == 0 || j.in.planar == j.out.planar) {               // fill the output's planes, or move rows between equal layouts
        const uint8_t* i0 = j.mode ? fr.in0(f) : nullptr;
        const uint8_t* i1 = j.mode && j.in.planar ? fr.in1(f) : nullptr;
        const long long row_bytes = j.out.planar ? j.width >> 1 : j.width;
        if (!fr.skip0(f)) yuv420_plane(i0, j.in.step, o0, j.out.step, row_bytes, j.rows, j.mode, j.flat, part, nparts);
        if (j.out.planar && !fr.skip1(f)) yuv420_plane(i1, j.in.step, o1, j.out.step, row_bytes, j.rows, j.mode, j.flat, part, nparts);
    } else if (j.out.planar) {
        yuv420_relayout<true>(fr.in0(f), j.in.step, o0, o1, j.out.step, j.width, j.rows, fr.vec(f), part, nparts);
    } else {
        yuv420_relayout<false>(o0, j.out.step, fr.in0(f), fr.in1(f), j.in.step, j.width, j.rows, fr.vec(f), part, nparts);
    }
}
__global__ __launch_bounds__(kThreads) void yuv420_chroma_kernel(Yuv420Job j)
{
    yuv420_chroma_body(j, StridedYuv420{j});
}
// the same on a frame list: every walk is grid-stride, so one grid (sized by the shape alone) serves frames of either path
__global__ __launch_bounds__(kThreads) void yuv420_chroma_frames_kernel(Yuv420Job j, Yuv420List l)
{
    yuv420_chroma_body(j, TableYuv420{l, j});
}
// 256: the implicit arguments a code object carries behind the explicit ones
static_assert(sizeof(Yuv420Job) + sizeof(Yuv420List) + 256 <= 4096,
              "the table and the job of yuv420_chroma_frames_kernel stay below HIP's 4 KiB of kernel arguments");

}  // namespace mi
