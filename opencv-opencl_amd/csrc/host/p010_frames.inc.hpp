// p010_frames.inc.hpp -- P010 / P012 / P016 frames given as a list of plane addresses (mi_clahe_p010_frames_dev): chunking, extern "C"
// Included by ../mi_lumaeq.hip after nv12_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// The 16-bit counterpart of mi_clahe_nv12_frames_dev: decoder surfaces from a pool, each with its own pitched Y and UV plane.  The
// checks are nv12_frames.inc.hpp's (check_frames with 2-byte samples: rows of 2 * W bytes, even pitches, 2-byte aligned planes).  The
// call is cut into chunks of kFramesPerLaunch frames; each chunk's plane addresses travel by value in the kernel arguments (FrameList)
// through clahe16_dev, which picks the *_frames_kernel entries of the 16-bit kernels -- same grids, same bytes as the tight batch --
// and then p010_uv_frames_kernel writes the chroma, charged to MI_K_LUT_APPLY like p010_uv_kernel.
//
// In place is decided PER FRAME (y_out == y_in): the kernels ask TableFrames::in_place(f) where the batch forms compare the two base
// pointers once per call, so one list may mix in-place and out-of-place frames (kernels/clahe16.hip.h, "OWNERSHIP INVARIANT").

namespace {

mi_status p010_frames_dev(mi_ctx* c, hipStream_t s, const mi_nv12_frame_dev* frames, int n_frames, const FramesShape& sh,
                          double clip_limit, int tiles_x, int tiles_y)
{
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        PlaneArgs a;
        const FrameList l = frame_chunk(frames + f0, nf, sh, &a);
        mi_status st = clahe16_dev(c, s, a.src, sh.y_in_pitch, 0, a.dst, sh.y_out_pitch, 0, sh.width, sh.height, nf, clip_limit,
                                   tiles_x, tiles_y, &l);
        if (st) return st;
        bool uv_work = l.uv.mode == 0;                               // an in-place copy moves nothing (as p010_uv_dev)
        for (int k = 0; k < nf && !uv_work; ++k) uv_work = l.f[k].uv_in != l.f[k].uv_out;
        if (!uv_work) continue;
        const long long uv_bytes = l.uv.row_bytes * l.uv.rows;
        const int B = blocks_per_frame(c, uv_bytes, l.uv.rows, nf, 2048);
        LAUNCH(c, s, MI_K_LUT_APPLY, p010_uv_frames_kernel, dim3(B, nf), dim3(kThreads), 0, l);
    }
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_clahe_p010_frames_dev(mi_ctx* c, const mi_nv12_frame_dev* frames, int n_frames, int width, int height,
                                   size_t y_in_pitch, size_t uv_in_pitch, size_t y_out_pitch, size_t uv_out_pitch,
                                   mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    if (tiles_x <= 0 || tiles_y <= 0) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    FramesShape sh{width, height, y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch, uv_mode};
    sh.sample_bytes = 2;
    bool work = false;
    mi_status st = check_frames(c, frames, n_frames, sh, &work);
    if (st || !work) return st;
    return p010_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
