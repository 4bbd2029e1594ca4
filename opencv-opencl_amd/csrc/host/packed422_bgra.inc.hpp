// packed422_bgra.inc.hpp -- packed 4:2:2 frames in (YUY2 / UYVY), interleaved 8-bit four-channel images out (BGRA / RGBA: CV_8UC4,
// A = 255): the four-channel pixel form and the extern "C" entry points
// Included by ../mi_lumaeq.hip after yuv420_bgra_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// capture -> equalize -> display surface / swap-chain image / interop texture / GUI image without a three-channel image in scratch and
// a widen to four channels outside the library.  The checks, the block, the writer of packed422_dev<W>, the host frame and the list
// form are packed422_bgr.inc.hpp's and packed422_bgr_frames.inc.hpp's templates, instantiated here on Bgra422Image: the arguments
// (P422BgrArgs), the stage sequences, scratch, chunks, grids and splits are the three-channel form's, the pixel-writing kernels are
// those of kernels/packed422_bgra.hip.h (4 bytes per pixel).  The frame-list entry points are packed422_bgra_frames.inc.hpp's.

namespace {

// The four-channel form: B, G, R, 255 or R, G, B, 255, 4 bytes per pixel.  The store-path rule both forms' blocks and counts go by is
// packed422_bgra_frame_wide's (kernels/packed422_bgra.hip.h forwards to packed422_image_wide).  It counts batch and host calls
// ("packed422_bgra_wide" / "packed422_bgra_bytes") and, apart from them, the frames of list calls.
struct Bgra422Image {
    static constexpr int kPx = 4;
    using Block = Packed422Bgra;
    template <int OFF, int ORDER> struct K {
        static constexpr KernelPair apply{lut_apply422_bgra_frames_kernel<OFF, ORDER>, lut_apply422_bgra_kernel<OFF, ORDER>};
        static constexpr KernelPair interp_global{clahe_interp422_bgra_global_frames_kernel<OFF, ORDER>, clahe_interp422_bgra_global_kernel<OFF, ORDER>};
        template <bool FT, bool FMA>
        static constexpr KernelPair interp{clahe_interp422_bgra_frames_kernel<FT, FMA, OFF, ORDER>, clahe_interp422_bgra_kernel<FT, FMA, OFF, ORDER>};
    };
    static constexpr const char* kOutPitch = "out_pitch < 4 * width";
    static constexpr const char* kOutStep = "out_step < 4 * width";
    static constexpr const char* kInPlace = "packed in, BGRA out has no in-place form";
    static constexpr const char* kHostOverlap = "packed in, BGRA out has no in-place form: the image overlaps the input frame";
    static constexpr const char* kListOverlap = "packed in, BGRA out has no in-place form: an image overlaps its own input frame";
    static void count_call(mi_ctx* c, bool wide) { ++(wide ? c->packed422_bgra_wide : c->packed422_bgra_bytes); }
    static void count_list(mi_ctx* c, int n_frames, unsigned long long n_wide)
    {
        c->packed422_bgra_list_frames_wide += n_wide;
        c->packed422_bgra_list_frames_bytes += (unsigned long long)n_frames - n_wide;
    }
};

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_bgra_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                       void* d_out, size_t out_pitch, size_t out_frame_stride,
                                                       int width, int height, int n_frames, int format, int order, void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs a = p422_bgr_args(d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr<Bgra422Image>(c, a, false, 0, 0, &work);
    return (st || !work) ? st : packed422_bgr_call<Bgra422Image>(c, pick_stream(c, stream), a, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_bgra_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_out, size_t out_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int format, int order,
                                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs a = p422_bgr_args(d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr<Bgra422Image>(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_bgr_call<Bgra422Image>(c, pick_stream(c, stream), a, 1, clip_limit, tiles_x, tiles_y);
}

mi_status mi_equalize_hist_packed422_to_bgra(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
                                             int width, int height, int format, int order)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs h = p422_bgr_args(in, in_pitch, 0, out, out_step, 0, width, height, 1, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr_host<Bgra422Image>(c, h, false, 0, 0, &work);
    return (st || !work) ? st : packed422_bgr_host<Bgra422Image>(c, h, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_bgra(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
                                     int width, int height, int format, int order, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs h = p422_bgr_args(in, in_pitch, 0, out, out_step, 0, width, height, 1, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr_host<Bgra422Image>(c, h, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_bgr_host<Bgra422Image>(c, h, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
