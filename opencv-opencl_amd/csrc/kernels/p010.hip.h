// p010.hip.h -- chroma half of 16-bit 4:2:0 semi-planar frames (P010 / P012 / P016): copy, or fill with the neutral 0x8000.
//
// A P010 frame is W x H little-endian uint16 luma samples followed by H/2 rows of W interleaved uint16 U, V samples (3*W*H bytes).
// The luma goes through the 16-bit CLAHE kernels (clahe16.hip.h) with Y pitch 2*W and frame stride 3*W*H; this kernel writes the
// chroma half of every frame of a batch: frames over grid.y, each frame's chroma chunked over grid.x, aligned 16-byte stores.
// Not uv_flat (equalize.hip.h): that one is byte-oriented (0x80808080).  Here the fill pattern is per SAMPLE -- bytes 00 80 -- and
// it must stay right on the unaligned head and tail, which begin at an even but not 16-byte-aligned address whenever 3*W*H is not
// a multiple of 16 (1918 x 1078).  Every chroma address is even (frames are 2-byte aligned and 3*W*H is a multiple of 4), so the
// head and the tail are whole samples and are written as uint16; the aligned body as u32x4 of 0x80008000 (little endian: 00 80 00 80).
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

__global__ __launch_bounds__(kThreads) void p010_uv_kernel(P010UV j)
{
    const int f = blockIdx.y, t = threadIdx.x, part = blockIdx.x, nparts = gridDim.x;
    uint8_t* dst = j.dst + (long long)f * j.frame;
    const uint8_t* src = j.mode ? j.src + (long long)f * j.frame : nullptr;
    const Split16 s = split16(dst, j.bytes);                           // head and tail are even: dst and bytes are
    uint16_t* d16 = reinterpret_cast<uint16_t*>(dst);
    const uint16_t* s16 = reinterpret_cast<const uint16_t*>(src);
    if (part == 0 && 2 * t < s.head) d16[t] = j.mode ? s16[t] : (uint16_t)0x8000u;
    if (part == nparts - 1 && 2 * t < s.tail) {
        const long long o = ((s.head + (s.nvec << 4)) >> 1) + t;
        d16[o] = j.mode ? s16[o] : (uint16_t)0x8000u;
    }
    const long long v0 = s.nvec * part / nparts, v1 = s.nvec * (part + 1) / nparts;
    u32x4* dp = reinterpret_cast<u32x4*>(dst + s.head);
    if (j.mode == 0) {
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

}  // namespace mi
