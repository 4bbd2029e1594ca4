// CPU unit test of the host's share of a P010 frame (opencv-opencl_amd/csrc/host/p010_chroma.hpp): the chroma half filled with the
// 16-bit neutral sample 0x8000 (bytes 00 80) or copied.  Built and run by tests/test_p010_abi.py under AddressSanitizer + UBSan.
// Checks: fill writes 00 80 to every sample; copy is exact; in place is a no-op; any start offset (odd ones included) works; not a
// byte outside [dst, dst + bytes) is touched -- guard bytes on both sides, and exactly sized heap blocks for the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../opencv-opencl_amd/csrc/host/p010_chroma.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                \
    do {                                                                \
        if (!(cond)) { ++failures; std::fprintf(stderr, "FAIL %s:%d ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
    } while (0)

static uint8_t pattern(size_t i, unsigned salt) { return (uint8_t)((i * 131u + salt * 7u + (i >> 8)) & 0xff); }

int main()
{
    const size_t sizes[] = {0, 2, 4, 6, 14, 16, 18, 30, 62, 64, 66, 126, 128, 130, 1000, 2244, 4096 + 2, 1918 * 1078, 3840 * 2160};
    const size_t kGuard = 64;
    unsigned cases = 0;
    for (size_t bytes : sizes) {
        for (size_t off = 0; off < 16; ++off) {
            if (bytes >= 1000000 && off > 3) continue;            // the large frames at a few offsets are enough
            // guard bytes on both sides of the chroma half, at start offset `off` from a 16-byte boundary
            std::vector<uint8_t> buf(kGuard + off + bytes + kGuard), src(bytes + 1);
            for (size_t i = 0; i < buf.size(); ++i) buf[i] = pattern(i, 1);
            for (size_t i = 0; i < src.size(); ++i) src[i] = pattern(i, 2);
            uint8_t* dst = buf.data() + kGuard + off;
            const std::vector<uint8_t> before = buf;
            // fill
            mi_host::p010_chroma(dst, src.data() + (off & 1), bytes, 0);
            for (size_t i = 0; i < bytes; ++i) CHECK(dst[i] == ((i & 1) ? 0x80 : 0x00), "fill bytes=%zu off=%zu i=%zu: %02x", bytes, off, i, dst[i]);
            for (size_t i = 0; i < kGuard + off; ++i) CHECK(buf[i] == before[i], "fill touched the leading guard (bytes=%zu off=%zu i=%zu)", bytes, off, i);
            for (size_t i = kGuard + off + bytes; i < buf.size(); ++i) CHECK(buf[i] == before[i], "fill touched the trailing guard (bytes=%zu off=%zu)", bytes, off);
            // copy, from a source at another alignment
            buf = before;
            dst = buf.data() + kGuard + off;
            const uint8_t* s = src.data() + (off & 1);
            mi_host::p010_chroma(dst, s, bytes, 1);
            CHECK(bytes == 0 || std::memcmp(dst, s, bytes) == 0, "copy bytes=%zu off=%zu", bytes, off);
            for (size_t i = 0; i < kGuard + off; ++i) CHECK(buf[i] == before[i], "copy touched the leading guard (bytes=%zu off=%zu)", bytes, off);
            for (size_t i = kGuard + off + bytes; i < buf.size(); ++i) CHECK(buf[i] == before[i], "copy touched the trailing guard (bytes=%zu off=%zu)", bytes, off);
            // copy in place: nothing moves
            buf = before;
            dst = buf.data() + kGuard + off;
            mi_host::p010_chroma(dst, dst, bytes, 1);
            CHECK(buf == before, "in-place copy changed bytes (bytes=%zu off=%zu)", bytes, off);
            ++cases;
        }
        // exactly sized heap blocks: the sanitizer reports any access one byte outside
        if (bytes > 0) {
            uint8_t* d = new uint8_t[bytes];
            uint8_t* q = new uint8_t[bytes];
            for (size_t i = 0; i < bytes; ++i) q[i] = pattern(i, 3);
            mi_host::p010_chroma(d, q, bytes, 0);
            for (size_t i = 0; i < bytes; ++i) CHECK(d[i] == ((i & 1) ? 0x80 : 0x00), "heap fill bytes=%zu i=%zu", bytes, i);
            mi_host::p010_chroma(d, q, bytes, 1);
            CHECK(std::memcmp(d, q, bytes) == 0, "heap copy bytes=%zu", bytes);
            delete[] d;
            delete[] q;
        }
    }
    if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    std::printf("p010_chroma: %u cases ok\n", cases);
    return 0;
}
