// bgra_packed422.inc.hpp -- interleaved 8-bit four-channel images (BGRA / BGRX, RGBA / RGBX: CV_8UC4) in, pitched packed 4:2:2 frames
// (YUY2 / UYVY) out with the luma equalized: the four-channel pixel form and the extern "C" entry points
// Included by ../mi_lumaeq.hip behind packed422_bgra_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// render target / swap-chain image / screen or window capture / interop buffer -> equalize -> playout card, v4l2 output or loopback
// device, virtual camera in one pass over the 4 B/px surface, without a slice-and-copy to three channels outside the library and
// without an NV12 intermediate (which has dropped every second chroma row).  The checks, the launch of stage 1, the two stage
// sequences, the host form and the entry are bgr_packed422.inc.hpp's templates, instantiated here on BgraTo422: stage 1
// (kernels/bgra_packed422.hip.h) converts into the caller's packed frame and, for equalizeHist, counts the luma it writes into the
// partials equalize_lut_kernel reads; stage 2 is that file's -- the packed form's own kernels IN PLACE on the output frame, the chroma
// kept, no MI_K_HIST launch.  The arguments are its BgrP422Args with a row of 4*W bytes in, the host form's W*H limit 0x7fffffff / 4.
// The frame-list entry points (mi_*_bgra_to_packed422_frames_dev) are bgra_packed422_frames.inc.hpp's.
// (What tests and notes of earlier rounds call launch_bgra_to_packed422 / check_bgra_packed422 is launch_bgr_to_packed422<BgraTo422> /
// check_bgr_packed422<BgraTo422>: the same rules, the grid on BgraTo422::grid_bytes.)

namespace {

// The four-channel form: B, G, R, X or R, G, B, X, 4 bytes per pixel in; stage 1 is kernels/bgra_packed422.hip.h.  The byte basis of
// its grid is half of what it reads and writes, (4 + 2) / 2 = 3 bytes per pixel where the three-channel form takes 5/2.
struct BgraTo422 {
    static constexpr int kPx = 4;
    using Job = BgraPacked422Job;
    template <int ORDER, int OFF, int UVMODE, bool HIST> static constexpr auto kernel = bgra_to_packed422_hist_kernel<ORDER, OFF, UVMODE, HIST>;
    template <int ORDER, int OFF, int UVMODE, bool HIST>
    static constexpr auto frames_kernel = bgra_to_packed422_hist_frames_kernel<ORDER, OFF, UVMODE, HIST>;
    static long long grid_bytes(long long px) { return px * 3; }
    static bool frame_vec(bool shape_vec, const void* in, const void* out) { return bgra_packed422_frame_vec(shape_vec, in, out); }
    static void count_call(mi_ctx* c, bool vec) { ++(vec ? c->bgra_packed422_vec : c->bgra_packed422_bytes); }
    static void count_list(mi_ctx* c, int n_frames, unsigned long long n_vec)
    {
        c->bgra_packed422_list_frames_vec += n_vec;
        c->bgra_packed422_list_frames_bytes += (unsigned long long)n_frames - n_vec;
    }
    static constexpr const char* kInPitch = "in_pitch < 4 * width";
    static constexpr const char* kInPlace = "BGRA in, packed 4:2:2 out has no in-place form";
    static constexpr const char* kListOverlap = "BGRA in, packed 4:2:2 out has no in-place form: an image overlaps its own output frame";
};

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgra_to_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                       void* d_out, size_t out_pitch, size_t out_frame_stride,
                                                       int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
                                                       void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgraTo422>(c, d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames,
                                          order, format, uv_mode, false, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_bgra_to_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_out, size_t out_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
                                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgraTo422>(c, d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames,
                                          order, format, uv_mode, false, true, clip_limit, tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_bgra_to_packed422(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
                                             int width, int height, int order, int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgraTo422>(c, in, in_step, 0, out, out_pitch, 0, width, height, 1, order, format, uv_mode, true, false, 0.0,
                                          0, 0, nullptr);
}

mi_status mi_clahe_bgra_to_packed422(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
                                     int width, int height, int order, int format, mi_uv_mode uv_mode,
                                     double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgraTo422>(c, in, in_step, 0, out, out_pitch, 0, width, height, 1, order, format, uv_mode, true, true,
                                          clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
