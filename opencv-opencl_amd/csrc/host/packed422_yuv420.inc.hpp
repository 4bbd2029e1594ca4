// packed422_yuv420.inc.hpp -- packed 4:2:2 frames in (YUY2 / UYVY), 4:2:0 frames described by mi_yuv420_planes out (I420 / YV12, or NV12):
// checks, the interleaved hand-over, the writer, extern "C" batch entry points
// Included by ../mi_lumaeq.hip after packed422_nv12_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// capture -> equalize -> software encoder (three pitched planes: data[0..2] / linesize[0..2]) without an NV12 intermediate and without
// a de-interleave outside the library.  An INTERLEAVED output is the NV12 form's own: check_packed422_nv12 and packed422_dev<Nv12Out>
// (packed422_nv12.inc.hpp) with d_uv_out = c0.  A PLANAR output runs the same stage sequences -- packed422.inc.hpp's own: same scratch,
// same chunks, same grids and splits, the same launches per chunk -- with one more writer: the pixel-writing kernels of
// kernels/packed422_yuv420.hip.h put the new luma into the Y plane and the chroma of each row pair, halved vertically and
// de-interleaved in registers, into a U and a V plane, in the launch that writes the luma.  There is no chroma launch.  Never the
// fused kernel and never hist_lut_kernel, as the packed forms.

namespace {

struct P422Yuv420Args {
    P422Args in;                      // the input side (in.out* mirror the input: only check_packed422 and the read-only stages look at them)
    uint8_t* y; size_t y_pitch;
    uint8_t* u; uint8_t* v; size_t c_pitch;      // c0 is always U, c1 always V
    size_t out_frame;
};

P422Yuv420Args p422_yuv420_args(const void* d_in, size_t in_pitch, size_t in_frame, void* y, size_t y_pitch, void* u, void* v, size_t c_pitch,
                                size_t out_frame, int width, int height, int n_frames, int format, mi_uv_mode uv_mode)
{
    P422Yuv420Args a;
    a.in = P422Args{(const uint8_t*)d_in, in_pitch, in_frame, (uint8_t*)const_cast<void*>(d_in), in_pitch, in_frame,
                    width, height, n_frames, format, uv_mode};
    a.y = (uint8_t*)y; a.y_pitch = y_pitch; a.u = (uint8_t*)u; a.v = (uint8_t*)v; a.c_pitch = c_pitch; a.out_frame = out_frame;
    return a;
}

struct P422Yuv420FramesShape {
    int width, height;
    size_t in_pitch, y_pitch, c_pitch;
    int format;
    mi_uv_mode uv_mode;
};

// There is no in-place form (the layouts differ): the rows of a frame's planes may not meet its input's rows, and the Y rows neither
// chroma plane's.  U and V are compared by address only: their rows may lie side by side in one pitched plane.
mi_status check_p422_yuv420_disjoint(mi_ctx* c, const void* in, const void* y, const void* u, const void* v, const P422Yuv420FramesShape& s)
{
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    const Span si(in, s.in_pitch, 2 * w, rows), sy(y, s.y_pitch, w, rows);
    const Span su(u, s.c_pitch, w / 2, rows / 2), sv(v, s.c_pitch, w / 2, rows / 2);
    if (y == u || y == v || u == v) return fail(c, MI_ERR_BAD_ARG, "two output planes at one address");
    if (sy.meets(si) || su.meets(si) || sv.meets(si))
        return fail(c, MI_ERR_BAD_ARG, "packed in, 4:2:0 out has no in-place form: an output plane overlaps its own input frame");
    if (sy.meets(su) || sy.meets(sv)) return fail(c, MI_ERR_BAD_ARG, "the Y plane of a frame overlaps a chroma plane of its own");
    return MI_OK;
}

// Everything is checked before anything is enqueued.  The input side, the shape and the modes are check_packed422's own checks (run on
// the input alone); the planar side adds the even height and the three planes.  *work = false: MI_OK with nothing to do.
// disjoint: also compare every frame's planes with its own input (the device batch form; the list and host forms do it per frame on
// the caller's addresses).
mi_status check_packed422_yuv420(mi_ctx* c, const P422Yuv420Args& a, bool is_clahe, int tiles_x, int tiles_y, bool disjoint, bool* work)
{
    *work = false;
    if (a.in.height > 0 && (a.in.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even height");
    bool in_work = false;
    const mi_status st = check_packed422(c, a.in, is_clahe, tiles_x, tiles_y, &in_work);
    if (st || !in_work) return st;
    if (!a.y || !a.u || !a.v) return fail(c, MI_ERR_BAD_ARG, "null frame or plane pointer");
    if (a.y_pitch < (size_t)a.in.width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (a.c_pitch < (size_t)a.in.width / 2) return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width / 2 planar)");
    if (((uintptr_t)a.y | (uintptr_t)a.u | (uintptr_t)a.v | a.y_pitch | a.c_pitch | a.out_frame) & 3)
        return fail(c, MI_ERR_BAD_ARG, "4:2:0 plane pointers, pitches and the frame stride are multiples of 4 here (pad the chroma pitch when W % 8 != 0)");
    if (disjoint) {
        const P422Yuv420FramesShape s{a.in.width, a.in.height, a.in.in_pitch, a.y_pitch, a.c_pitch, a.in.format, a.in.uv_mode};
        for (int f = 0; f < a.in.n_frames; ++f) {
            const size_t o = (size_t)f * a.out_frame;
            if (mi_status d = check_p422_yuv420_disjoint(c, a.in.in + (size_t)f * a.in.in_frame, a.y + o, a.u + o, a.v + o, s)) return d;
        }
    }
    *work = true;
    return MI_OK;
}

Packed422Yuv420 packed422_yuv420_batch(const P422Yuv420Args& a, int f0)
{
    Packed422Yuv420 p;
    p.src = a.in.in + (size_t)f0 * a.in.in_frame;
    p.y = a.y + (size_t)f0 * a.out_frame; p.u = a.u + (size_t)f0 * a.out_frame; p.v = a.v + (size_t)f0 * a.out_frame;
    p.src_step = (long long)a.in.in_pitch; p.y_step = (long long)a.y_pitch; p.c_step = (long long)a.c_pitch;
    p.src_frame = (long long)a.in.in_frame; p.out_frame = (long long)a.out_frame;
    p.dwords = a.in.width / 2; p.rows = a.in.height;
    p.copy_uv = a.in.uv_mode == MI_UV_COPY ? 1 : 0;
    return p;
}

// The writer of the stage sequences of packed422.inc.hpp that puts the new luma into a Y plane and the chroma into a U and a V plane
struct Yuv420PlanarOut {
    using Args = P422Yuv420Args;
    using Block = Packed422Yuv420;
    using List = Packed422Yuv420List;
    static const P422Args& input(const Args& a) { return a.in; }
    static Block cut(const Args& a, int f0) { return packed422_yuv420_batch(a, f0); }
    static int apply_rows(int height) { return height / 2; }                 // bands of row pairs
    template <int OFF> struct K {
        static constexpr KernelPair apply{lut_apply422_yuv420_frames_kernel<OFF>, lut_apply422_yuv420_kernel<OFF>};
        static constexpr KernelPair interp_global{clahe_interp422_yuv420_global_frames_kernel<OFF>, clahe_interp422_yuv420_global_kernel<OFF>};
        template <bool FT, bool FMA>
        static constexpr KernelPair interp{clahe_interp422_yuv420_frames_kernel<FT, FMA, OFF>, clahe_interp422_yuv420_kernel<FT, FMA, OFF>};
    };
};

// the descriptor's chroma value: one of the two, or the call is refused
mi_status check_chroma_value(mi_ctx* c, int chroma)
{
    if (chroma != MI_CHROMA_INTERLEAVED && chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status packed422_yuv420_batch_entry(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame, const mi_yuv420_planes* out, int width,
                                       int height, int n_frames, int format, mi_uv_mode uv_mode, int op, double clip_limit, int tiles_x,
                                       int tiles_y, void* stream)
{
    if (!out) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (mi_status st = check_chroma_value(c, out->chroma)) return st;
    bool work = false;
    if (out->chroma == MI_CHROMA_INTERLEAVED) {             // the NV12 form's own checks and launch path on {y, c0}; c1 is ignored
        const P422Nv12Args n = p422_nv12_args(d_in, in_pitch, in_frame, out->y, out->y_pitch, out->c0, out->c_pitch, out->frame_stride,
                                              width, height, n_frames, format, uv_mode);
        const mi_status st = check_packed422_nv12(c, n, op != 0, tiles_x, tiles_y, &work);
        return (st || !work) ? st : packed422_dev<Nv12Out>(c, pick_stream(c, stream), n, op, clip_limit, tiles_x, tiles_y);
    }
    const P422Yuv420Args a = p422_yuv420_args(d_in, in_pitch, in_frame, out->y, out->y_pitch, out->c0, out->c1, out->c_pitch, out->frame_stride,
                                              width, height, n_frames, format, uv_mode);
    const mi_status st = check_packed422_yuv420(c, a, op != 0, tiles_x, tiles_y, true, &work);
    return (st || !work) ? st : packed422_dev<Yuv420PlanarOut>(c, pick_stream(c, stream), a, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_yuv420_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                         const mi_yuv420_planes* out, int width, int height, int n_frames, int format,
                                                         mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return packed422_yuv420_batch_entry(c, d_in, in_pitch, in_frame_stride, out, width, height, n_frames, format, uv_mode, 0, 0.0, 0, 0, stream);
}

mi_status mi_clahe_packed422_to_yuv420_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                 const mi_yuv420_planes* out, int width, int height, int n_frames, int format,
                                                 mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return packed422_yuv420_batch_entry(c, d_in, in_pitch, in_frame_stride, out, width, height, n_frames, format, uv_mode, 1, clip_limit,
                                        tiles_x, tiles_y, stream);
}

}  // extern "C"
