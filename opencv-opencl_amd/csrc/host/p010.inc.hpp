// p010.inc.hpp -- CLAHE on 16-bit 4:2:0 semi-planar frames (P010 / P012 / P016): launcher + extern "C" entry points
// Included by ../mi_lumaeq.hip (one translation unit; not a stand-alone header).
//
// The luma is the 16-bit path (clahe16_dev) on the CV_16UC1 view of the Y plane: pitch 2*W, frame stride 3*W*H -- bit-identical to
// mi_clahe_u16_batch_dev on that plane.  When the stride is a multiple of 16 (4K, 1080p) the vector tile histogram and the 12-bit
// bet still apply; otherwise the careful path runs (slower, same bytes).  The chroma half is written by p010_uv_kernel
// (kernels/p010.hip.h) on the device, or by mi_host::p010_chroma (host/p010_chroma.hpp) for host frames.

namespace {

size_t p010_frame_bytes(int width, int height) { return (size_t)width * height * 3; }

// Launches the chroma kernel for `n_frames` frames; nothing for an in-place copy.  Charged to MI_K_LUT_APPLY like the 8-bit uv_kernel.
mi_status p010_uv_dev(mi_ctx* c, hipStream_t s, const uint8_t* in, uint8_t* out, int width, int height, int n_frames, mi_uv_mode mode)
{
    const long long ybytes = 2LL * width * height, uvbytes = (long long)width * height;
    P010UV j;
    j.src = in + ybytes; j.dst = out + ybytes;
    j.frame = 3LL * width * height;
    j.bytes = (mode == MI_UV_COPY && in == out) ? 0 : uvbytes;
    j.mode = mode == MI_UV_COPY ? 1 : 0;
    if (j.bytes == 0) return MI_OK;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxGridY) {
        const int nf = std::min(kMaxGridY, n_frames - f0);
        P010UV jf = j;
        jf.src += (long long)f0 * j.frame; jf.dst += (long long)f0 * j.frame;
        const int B = blocks_per_frame(c, uvbytes, 1, nf, 2048);
        LAUNCH(c, s, MI_K_LUT_APPLY, p010_uv_kernel, dim3(B, nf), dim3(kThreads), 0, jf);
    }
    return MI_OK;
}

// Argument rules of the P010 forms: those of the 16-bit and NV12 forms, plus even W and H.
mi_status check_p010(mi_ctx* c, const void* in, const void* out, int width, int height, int n_frames, mi_uv_mode uv_mode,
                     int tiles_x, int tiles_y)
{
    if (uv_mode != MI_UV_FILL128 && uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (width < 0 || height < 0 || n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if (tiles_x <= 0 || tiles_y <= 0) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (width == 0 || height == 0 || n_frames == 0) return MI_OK;
    if ((width & 1) || (height & 1)) return fail(c, MI_ERR_BAD_ARG, "P010 frames have even width and height");
    return check_u16(c, in, (size_t)width * 2, out, (size_t)width * 2, width, height, n_frames, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_clahe_p010_batch_dev(mi_ctx* c, const void* d_in, void* d_out, int width, int height, int n_frames,
                                  mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    mi_status st = check_p010(c, d_in, d_out, width, height, n_frames, uv_mode, tiles_x, tiles_y);
    if (st || width == 0 || height == 0 || n_frames == 0) return st;
    hipStream_t s = pick_stream(c, stream);
    const size_t frame = p010_frame_bytes(width, height);
    st = clahe16_dev(c, s, (const uint8_t*)d_in, (size_t)width * 2, frame, (uint8_t*)d_out, (size_t)width * 2, frame,
                     width, height, n_frames, clip_limit, tiles_x, tiles_y);
    if (st) return st;
    return p010_uv_dev(c, s, (const uint8_t*)d_in, (uint8_t*)d_out, width, height, n_frames, uv_mode);
}

// Host frame: only the Y plane crosses PCIe (stage_in / stage_out, or directly when the frame is pinned, like mi_clahe_u16); the
// chroma half is written on the host while the GPU works on Y (like mi_clahe_nv12).
mi_status mi_clahe_p010(mi_ctx* c, const uint16_t* in, uint16_t* out, int width, int height, mi_uv_mode uv_mode,
                        double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    mi_status st = check_p010(c, in, out, width, height, 1, uv_mode, tiles_x, tiles_y);
    if (st || width == 0 || height == 0) return st;
    const size_t row = (size_t)width * 2, ybytes = row * height;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    if ((st = stage_in(c, s, (const uint8_t*)in, row, row, (size_t)height, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, ybytes))) return st;
    st = clahe16_dev(c, s, c->d_stage_in, row, ybytes, c->d_stage_out, row, ybytes, width, height, 1, clip_limit, tiles_x, tiles_y);
    if (st) return st;
    mi_host::p010_chroma((uint8_t*)out + ybytes, (const uint8_t*)in + ybytes, (size_t)width * height, uv_mode == MI_UV_COPY ? 1 : 0);
    return stage_out(c, s, (uint8_t*)out, row, row, (size_t)height, drain);
}

}  // extern "C"
