// bgra_packed422_frames.inc.hpp -- four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 (YUY2 / UYVY) out on frames given as a LIST of
// addresses (mi_*_bgra_to_packed422_frames_dev): extern "C"
// Included by ../mi_lumaeq.hip after bgra_packed422.inc.hpp (one translation unit; not a stand-alone header).
//
// A renderer, a compositor or a capture API hands out a pool of four-byte surfaces; a playout card, a v4l2 output queue or a virtual
// camera hands out a buffer pool: every packed frame its own allocation, padded to bytesperline, at whatever alignment the driver
// chose.  The checks, the chunk loop (kPacked422FramesPerLaunch frames a chunk) and the entry are bgr_packed422_frames.inc.hpp's
// templates on BgraTo422; the entry struct (mi_bgr_packed422_frame_dev) and the shape (BgrP422FramesShape) are the three-channel
// form's.  Each frame takes the 16 x 1 groups or the macropixels of stage 1 by its own two addresses (bgra_packed422_frame_vec, the
// kernel's own rule, through BgraTo422::frame_vec) and is counted by it in BgraTo422::count_list; stage 2 has always decided per row.

extern "C" {

mi_status mi_equalize_hist_bgra_to_packed422_frames_dev(mi_ctx* c, const mi_bgr_packed422_frame_dev* frames, int n_frames,
                                                        int width, int height, size_t in_pitch, size_t out_pitch, int order, int format,
                                                        mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrP422FramesShape sh{width, height, in_pitch, out_pitch, order, format, uv_mode};
    return bgr_packed422_frames_entry<BgraTo422>(c, frames, n_frames, sh, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_bgra_to_packed422_frames_dev(mi_ctx* c, const mi_bgr_packed422_frame_dev* frames, int n_frames,
                                                int width, int height, size_t in_pitch, size_t out_pitch, int order, int format,
                                                mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrP422FramesShape sh{width, height, in_pitch, out_pitch, order, format, uv_mode};
    return bgr_packed422_frames_entry<BgraTo422>(c, frames, n_frames, sh, true, clip_limit, tiles_x, tiles_y, stream);
}

}  // extern "C"
