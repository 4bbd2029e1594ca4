// packed422_bgra_frames.inc.hpp -- packed 4:2:2 in (YUY2 / UYVY), four-channel BGRA / RGBA (CV_8UC4, A = 255) out on a LIST of device
// frames (mi_*_packed422_to_bgra_frames_dev): extern "C"
// Included by ../mi_lumaeq.hip after packed422_bgra.inc.hpp (one translation unit; not a stand-alone header).
//
// Neither end of a capture -> display pipeline is one allocation at a fixed frame stride: the capture card hands out a buffer pool
// (packed422_frames.inc.hpp), the images are a swap chain's or a pool of surfaces, textures or cv::Mats.  The checks and the chunk
// loop (f0 += kPacked422FramesPerLaunch) are packed422_bgr_frames.inc.hpp's templates on Bgra422Image; the entry type
// (mi_packed422_bgr_frame_dev) and the shape (P422BgrFramesShape, with an out_pitch of at least 4 * W) are the three-channel form's.
// Each frame takes the wide or the byte store path by its own address (packed422_bgra_frame_wide, as Table422Bgra::wide_of calls it),
// and is counted by it in Bgra422Image::count_list.

extern "C" {

mi_status mi_equalize_hist_packed422_to_bgra_frames_dev(mi_ctx* c, const mi_packed422_bgr_frame_dev* frames, int n_frames,
                                                        int width, int height, size_t in_pitch, size_t out_pitch, int format, int order,
                                                        void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrFramesShape sh{width, height, in_pitch, out_pitch, format, order};
    bool work = false;
    const mi_status st = check_packed422_bgr_frames<Bgra422Image>(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : packed422_bgr_frames_dev<Bgra422Image>(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_bgra_frames_dev(mi_ctx* c, const mi_packed422_bgr_frame_dev* frames, int n_frames,
                                                int width, int height, size_t in_pitch, size_t out_pitch, int format, int order,
                                                double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrFramesShape sh{width, height, in_pitch, out_pitch, format, order};
    bool work = false;
    const mi_status st = check_packed422_bgr_frames<Bgra422Image>(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_bgr_frames_dev<Bgra422Image>(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
