// p010_chroma.hpp -- the host's share of a 16-bit 4:2:0 frame (P010 / P012 / P016): its chroma half, filled or copied on the CPU
// while the GPU works on the luma (mi_clahe_p010, and mi_pipe under MI_PIPE_UV_HOST).  The 8-bit forms do the same with
// memset(128) / memmove; here the neutral value is a 16-bit SAMPLE, 0x8000 (bytes 00 80), and the fill is laid down in whole
// samples from the first byte on, whatever the alignment of `dst`.
// Stand-alone on purpose (no HIP header): tests/test_p010_abi.py compiles it under AddressSanitizer.
#ifndef MI_P010_CHROMA_HPP_
#define MI_P010_CHROMA_HPP_
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mi_host {

// mode 0: every sample of the `bytes` bytes at dst becomes 0x8000 (little endian); mode 1: copy them from src (src == dst: nothing
// moves; overlapping ranges are allowed).  `bytes` is the chroma size, W*H for a W x H frame: an even number.
inline void p010_chroma(uint8_t* dst, const uint8_t* src, size_t bytes, int mode)
{
    if (bytes == 0) return;
    if (mode == 1) {
        if (dst != src) memmove(dst, src, bytes);
        return;
    }
    // lay down one cache line of samples, then double the written prefix: memcpy-speed at any alignment, never a byte past `bytes`
    size_t done = bytes < 64 ? bytes : 64;
    for (size_t i = 0; i < done; ++i) dst[i] = (i & 1) ? (uint8_t)0x80 : (uint8_t)0x00;
    while (done < bytes) {
        const size_t n = done < bytes - done ? done : bytes - done;      // `done` is even: the copy keeps the sample phase
        memcpy(dst + done, dst, n);
        done += n;
    }
}

}  // namespace mi_host
#endif
