// packed422_nv12.inc.hpp -- packed 4:2:2 frames in (YUY2 / UYVY), NV12 frames out: checks, launch sequences, extern "C" entry points
// Included by ../mi_lumaeq.hip after packed422.inc.hpp (one translation unit; not a stand-alone header).
//
// capture -> equalize -> encoder without a format conversion of its own.  The stage sequences are packed422.inc.hpp's own (one
// MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch per chunk; tile histograms -> interpolation): same scratch, same chunks, same
// grids and splits.  Only the writer differs: the pixel-writing kernels of kernels/packed422_nv12.hip.h put the new luma into a Y plane
// and the chroma of each row pair, halved vertically, into an interleaved UV plane -- in the launch that writes the luma, there is no
// chroma launch.  Never the fused kernel and never hist_lut_kernel, as the packed forms.

namespace {

struct P422Nv12Args {
    P422Args in;                      // the input side (in.out* mirror the input: only check_packed422 and the read-only stages look at them)
    uint8_t* y; size_t y_pitch;
    uint8_t* uv; size_t uv_pitch;
    size_t out_frame;
};

P422Nv12Args p422_nv12_args(const void* d_in, size_t in_pitch, size_t in_frame, void* d_y, size_t y_pitch, void* d_uv, size_t uv_pitch,
                            size_t out_frame, int width, int height, int n_frames, int format, mi_uv_mode uv_mode)
{
    P422Nv12Args a;
    a.in = P422Args{(const uint8_t*)d_in, in_pitch, in_frame, (uint8_t*)const_cast<void*>(d_in), in_pitch, in_frame,
                    width, height, n_frames, format, uv_mode};
    a.y = (uint8_t*)d_y; a.y_pitch = y_pitch; a.uv = (uint8_t*)d_uv; a.uv_pitch = uv_pitch; a.out_frame = out_frame;
    return a;
}

// Everything is checked before anything is enqueued.  The input side, the shape and the modes are check_packed422's own checks (run on
// the input alone); the NV12 side adds the even height and the two planes.  *work = false: MI_OK with nothing to do.
mi_status check_packed422_nv12(mi_ctx* c, const P422Nv12Args& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.in.height > 0 && (a.in.height & 1)) return fail(c, MI_ERR_BAD_ARG, "NV12 frames have an even height");
    bool in_work = false;
    const mi_status st = check_packed422(c, a.in, is_clahe, tiles_x, tiles_y, &in_work);
    if (st || !in_work) return st;
    if (!a.y || !a.uv) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
    if (a.y_pitch < (size_t)a.in.width || a.uv_pitch < (size_t)a.in.width) return fail(c, MI_ERR_BAD_ARG, "NV12 pitch < width");
    if (((uintptr_t)a.y | (uintptr_t)a.uv | a.y_pitch | a.uv_pitch | a.out_frame) & 3)
        return fail(c, MI_ERR_BAD_ARG, "NV12 plane pointers, pitches and the frame stride are multiples of 4 here (pad the pitch when W % 4 == 2)");
    if (a.y == a.in.in || a.uv == a.in.in) return fail(c, MI_ERR_BAD_ARG, "packed in, NV12 out has no in-place form");
    *work = true;
    return MI_OK;
}

Packed422Nv12 packed422_nv12_batch(const P422Nv12Args& a, int f0)
{
    Packed422Nv12 p;
    p.src = a.in.in + (size_t)f0 * a.in.in_frame;
    p.y = a.y + (size_t)f0 * a.out_frame; p.uv = a.uv + (size_t)f0 * a.out_frame;
    p.src_step = (long long)a.in.in_pitch; p.y_step = (long long)a.y_pitch; p.uv_step = (long long)a.uv_pitch;
    p.src_frame = (long long)a.in.in_frame; p.out_frame = (long long)a.out_frame;
    p.dwords = a.in.width / 2; p.rows = a.in.height;
    p.copy_uv = a.in.uv_mode == MI_UV_COPY ? 1 : 0;
    return p;
}

// The writer of the stage sequences of packed422.inc.hpp that puts the new luma into a Y plane and the chroma into a UV plane
struct Nv12Out {
    using Args = P422Nv12Args;
    using Block = Packed422Nv12;
    using List = Packed422Nv12List;
    static const P422Args& input(const Args& a) { return a.in; }
    static Block cut(const Args& a, int f0) { return packed422_nv12_batch(a, f0); }
    static int apply_rows(int height) { return height / 2; }                 // bands of row pairs
    template <int OFF> struct K {
        static constexpr KernelPair apply{lut_apply422_nv12_frames_kernel<OFF>, lut_apply422_nv12_kernel<OFF>};
        static constexpr KernelPair interp_global{clahe_interp422_nv12_global_frames_kernel<OFF>, clahe_interp422_nv12_global_kernel<OFF>};
        template <bool FT, bool FMA>
        static constexpr KernelPair interp{clahe_interp422_nv12_frames_kernel<FT, FMA, OFF>, clahe_interp422_nv12_kernel<FT, FMA, OFF>};
    };
};

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_nv12_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                       void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
                                                       int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Nv12Args a = p422_nv12_args(d_in, in_pitch, in_frame_stride, d_y_out, y_pitch, d_uv_out, uv_pitch, out_frame_stride,
                                          width, height, n_frames, format, uv_mode);
    bool work = false;
    const mi_status st = check_packed422_nv12(c, a, false, 0, 0, &work);
    return (st || !work) ? st : packed422_dev<Nv12Out>(c, pick_stream(c, stream), a, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_nv12_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
                                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Nv12Args a = p422_nv12_args(d_in, in_pitch, in_frame_stride, d_y_out, y_pitch, d_uv_out, uv_pitch, out_frame_stride,
                                          width, height, n_frames, format, uv_mode);
    bool work = false;
    const mi_status st = check_packed422_nv12(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_dev<Nv12Out>(c, pick_stream(c, stream), a, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
