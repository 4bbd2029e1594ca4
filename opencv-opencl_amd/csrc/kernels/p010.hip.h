// p010.hip.h -- chroma half of 16-bit 4:2:0 semi-planar frames (P010 / P012 / P016): copy, or fill with the neutral 0x8000.
//
// A P010 frame is W x H little-endian uint16 luma samples followed by H/2 rows of W interleaved uint16 U, V samples (3*W*H bytes).
// The luma goes through the 16-bit CLAHE kernels (clahe16.hip.h) with Y pitch 2*W and frame stride 3*W*H; this kernel writes the
// chroma half of every frame of a batch: frames over grid.y, each frame's chroma chunked over grid.x, aligned 16-byte stores.
// Not uv_flat (equalize.hip.h): that one is byte-oriented (0x80808080).  Here the fill pattern is per SAMPLE -- bytes 00 80 -- and
// it must stay right on the unaligned head and tail, which begin at an even but not 16-byte-aligned address whenever 3*W*H is not
// a multiple of 16 (1918 x 1078).  Every chroma address is even (frames are 2-byte aligned and 3*W*H is a multiple of 4), so the
// head and the tail are whole samples and are written as uint16; the aligned body as u32x4 of 0x80008000 (little endian: 00 80 00 80).
// p010_uv_frames_kernel does the same for a list of pitched frames (mi_clahe_p010_frames_dev): row by row, or as one flat run when both
// chroma planes are tight.
#pragma once
#include "common.hip.h"

namespace mi {

struct P010UV {
    const uint8_t* src;               // chroma of frame 0 of the input (copy only)
    uint8_t* dst;                     // chroma of frame 0 of the output
    long long frame;                  // bytes between frames (3*W*H, input and output alike)
    long long bytes;                  // chroma bytes per frame (W*H); 0 = nothing to do (in-place copy)
    int mode;                         // 0 = fill 0x8000, 1 = copy
};

// Chroma bytes [dst, dst + bytes) of one frame, shared between `nparts` workgroups; this one is `part`.  src: the copy's source (mode 1).
__device__ __forceinline__ void p010_uv_flat(const uint8_t* src, uint8_t* dst, long long bytes, int mode, int part, int nparts)
{
    const int t = threadIdx.x;
    const Split16 s = split16(dst, bytes);                           // head and tail are even: dst and bytes are
    uint16_t* d16 = reinterpret_cast<uint16_t*>(dst);
    const uint16_t* s16 = reinterpret_cast<const uint16_t*>(src);
    if (part == 0 && 2 * t < s.head) d16[t] = mode ? s16[t] : (uint16_t)0x8000u;
    if (part == nparts - 1 && 2 * t < s.tail) {
        const long long o = ((s.head + (s.nvec << 4)) >> 1) + t;
        d16[o] = mode ? s16[o] : (uint16_t)0x8000u;
    }
    const long long v0 = s.nvec * part / nparts, v1 = s.nvec * (part + 1) / nparts;
    u32x4* dp = reinterpret_cast<u32x4*>(dst + s.head);
    if (mode == 0) {
        const u32x4 g = {0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        for (long long i = v0 + t; i < v1; i += kThreads) dp[i] = g;
    } else {
        const u32x4_u* sp = reinterpret_cast<const u32x4_u*>(src + s.head);   // the source may sit at another alignment
        long long i = v0 + t;
        for (; i + 3 * kThreads < v1; i += 4 * kThreads) {
            const u32x4 a = sp[i], b = sp[i + kThreads], c = sp[i + 2 * kThreads], d = sp[i + 3 * kThreads];
            dp[i] = a; dp[i + kThreads] = b; dp[i + 2 * kThreads] = c; dp[i + 3 * kThreads] = d;
        }
        for (; i < v1; i += kThreads) dp[i] = sp[i];
    }
}

__global__ __launch_bounds__(kThreads) void p010_uv_kernel(P010UV j)
{
    const int f = blockIdx.y;
    p010_uv_flat(j.mode ? j.src + (long long)f * j.frame : nullptr, j.dst + (long long)f * j.frame, j.bytes, j.mode, blockIdx.x, gridDim.x);
}

// Pitched chroma (frame lists): rows [r0, r1) of `rows` rows of row_bytes (2 * W) bytes, this workgroup's share.  Every row has its own
// head: the aligned 16-byte stores of row r start at (16 - (dst_r & 15)) & 15, and what precedes them (the head) and follows the last
// one (the tail) is at most seven whole samples each -- dst_r, the pitch and row_bytes are even.  The copy's source may sit at any other
// even alignment (unaligned 16-byte loads).  Nothing outside the row_bytes of a row is written.
__device__ __forceinline__ void p010_uv_rows(const uint8_t* src, long long src_step, uint8_t* dst, long long dst_step, long long row_bytes,
                                             int rows, int mode, int part, int nparts)
{
    const int t = threadIdx.x;
    const int r0 = (int)((long long)rows * part / nparts), r1 = (int)((long long)rows * (part + 1) / nparts);
    const int slots = (int)(row_bytes >> 4);                          // a row holds at most this many aligned vectors
    if (slots > 0) {
        const u32x4 g = {0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        const int items = (r1 - r0) * slots;
        int row = r0 + t / slots, slot = t % slots;
        const int drow = kThreads / slots, dslot = kThreads - drow * slots;
        for (int it = t; it < items; it += 4 * kThreads) {
            u32x4 q[4]; bool qv[4]; uint8_t* dp[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint8_t* d = dst + (long long)row * dst_step;
                const long long o = (long long)((16 - (int)((uintptr_t)d & 15)) & 15) + ((long long)slot << 4);
                qv[k] = it + k * kThreads < items && o + 16 <= row_bytes;
                dp[k] = d + o;
                q[k] = g;
                if (mode && qv[k]) q[k] = *reinterpret_cast<const u32x4_u*>(src + (long long)row * src_step + o);
                row += drow; slot += dslot;
                if (slot >= slots) { slot -= slots; ++row; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) if (qv[k]) *reinterpret_cast<u32x4*>(dp[k]) = q[k];
        }
    }
    const int items = (r1 - r0) * 14;                                 // sample items per row: c < 7 its head, c >= 7 its tail
    for (int it = t; it < items; it += kThreads) {
        const int row = r0 + it / 14, c = it % 14;
        uint8_t* d = dst + (long long)row * dst_step;
        const long long head = min((long long)((16 - (int)((uintptr_t)d & 15)) & 15), row_bytes);
        const long long o = c < 7 ? 2LL * c : head + ((row_bytes - head) & ~15LL) + 2LL * (c - 7);
        if (c < 7 ? o >= head : o >= row_bytes) continue;
        *reinterpret_cast<uint16_t*>(d + o) = mode ? *reinterpret_cast<const uint16_t*>(src + (long long)row * src_step + o) : (uint16_t)0x8000u;
    }
}

// grid = (parts, frames of the list); the chroma planes and their shape are the FrameList's (uv.row_bytes = 2 * W, or one flat run of
// W * H bytes when both planes are tight).  An in-place copy moves nothing.
__global__ __launch_bounds__(kThreads) void p010_uv_frames_kernel(FrameList l)
{
    const int f = blockIdx.y;
    const UVRows& uv = l.uv;
    if (uv.rows <= 0 || (uv.mode && l.f[f].uv_in == l.f[f].uv_out)) return;
    if (uv.rows == 1) p010_uv_flat(l.f[f].uv_in, l.f[f].uv_out, uv.row_bytes, uv.mode, blockIdx.x, gridDim.x);
    else p010_uv_rows(l.f[f].uv_in, uv.src_step, l.f[f].uv_out, uv.dst_step, uv.row_bytes, uv.rows, uv.mode, blockIdx.x, gridDim.x);
}

}  // namespace mi
