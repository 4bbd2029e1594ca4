// bgr_nv12_frames.inc.hpp -- interleaved BGR / RGB in, NV12 out on frames given as a list of addresses (mi_*_bgr_to_nv12_frames_dev):
// checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip after bgr_nv12.inc.hpp (one translation unit; not a stand-alone header).
//
// A hardware encoder hands out a surface pool: every NV12 surface its own allocation with a pitched Y and a pitched UV plane; renderers,
// models and image readers hand over one image per frame.  The call is cut into chunks of kFramesPerLaunch frames.  A chunk's
// {in, y, uv} triples travel to stage 1 as a BgrNv12List, its Y planes to stage 2 as a FrameList with y_in == y_out and no chroma job,
// both by value in the kernel arguments, through launch_bgr_to_nv12 and the planar launchers (launch_apply / clahe_dev, as
// nv12_frames.inc.hpp uses them in place) -- same grids, same partials, same bytes as the batch form.  Each frame takes the 16 x 2
// groups or the 2 x 2 blocks of stage 1 by its own alignment; stage 2 has always decided per plane.

namespace {

struct BgrNv12FramesShape {
    int width, height;
    size_t in_pitch, y_pitch, uv_pitch;
    int order;
    mi_uv_mode uv_mode;
};

// the shape as check_bgr_nv12 and launch_bgr_to_nv12 take it: stand-in addresses that pass the pointer checks and are multiples of 16,
// frame strides 0, so BgrNv12Job::vec comes out as what the shape allows
BgrNv12Args bgr_nv12_frames_shape_args(const BgrNv12FramesShape& s, int n_frames)
{
    return BgrNv12Args{(const uint8_t*)16, s.in_pitch, 0, (uint8_t*)32, s.y_pitch, (uint8_t*)48, s.uv_pitch, 0,
                       s.width, s.height, n_frames, s.order, s.uv_mode};
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_bgr_nv12_frames(mi_ctx* c, const mi_bgr_nv12_frame_dev* frames, int n_frames, const BgrNv12FramesShape& s,
                                bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_bgr_nv12's own answers (order, uv_mode, sizes, even width and height, tiles, pitches, the planar forms' limits)
    bool any = false;
    const mi_status st = check_bgr_nv12(c, bgr_nv12_frames_shape_args(s, n_frames), is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_bgr_nv12_frame_dev& f = frames[k];
        if (!f.in || !f.y || !f.uv) return fail(c, MI_ERR_BAD_ARG, "null image or plane pointer");
        // there is no in-place form (3 bytes per pixel in, 1 and 1/2 out): the image's rows may meet neither plane of its own frame,
        // and the two planes not each other
        const Span si(f.in, s.in_pitch, 3 * w, rows), sy(f.y, s.y_pitch, w, rows), su(f.uv, s.uv_pitch, w, rows / 2);
        if (si.meets(sy) || si.meets(su))
            return fail(c, MI_ERR_BAD_ARG, "BGR in, NV12 out has no in-place form: an image overlaps a plane of its own frame");
        if (sy.meets(su)) return fail(c, MI_ERR_BAD_ARG, "the Y plane of a frame overlaps its own UV plane");
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE.  Per chunk: one MI_K_COLOR (convert, and count for equalizeHist), then one MI_K_EQ_LUT and one
// MI_K_LUT_APPLY, or what mi_clahe_nv12_frames_dev launches in place on the same Y planes.
mi_status bgr_nv12_frames_dev(mi_ctx* c, hipStream_t s, const mi_bgr_nv12_frame_dev* frames, int n_frames, const BgrNv12FramesShape& sh,
                              int op, double clip_limit, int tiles_x, int tiles_y)
{
    mi_status st;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        BgrNv12List io{};                                            // the three addresses of a frame for stage 1
        FrameList ys{};                                              // this chunk's Y planes for stage 2, in place (uv.rows = 0: no UV work)
        for (int k = 0; k < nf; ++k) {
            const mi_bgr_nv12_frame_dev& f = frames[f0 + k];
            io.f[k] = BgrNv12Frame{(const uint8_t*)f.in, (uint8_t*)f.y, (uint8_t*)f.uv};
            ys.f[k] = FramePlanes{(const uint8_t*)f.y, nullptr, (uint8_t*)f.y, nullptr};
        }
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{ys.f[0].y_in, sh.y_pitch, 0, ys.f[0].y_out, sh.y_pitch, 0, sh.width, sh.height, nf};
        const BgrNv12Args shape = bgr_nv12_frames_shape_args(sh, nf);
        if (!op) {
            int nparts = 0;
            if ((st = launch_bgr_to_nv12(c, s, shape, 0, nf, true, &nparts, &io))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            if ((st = launch_apply(c, s, ya, 0, nf, c->d_luts, nullptr, &ys))) return st;
        } else {
            if ((st = launch_bgr_to_nv12(c, s, shape, 0, nf, false, nullptr, &io))) return st;
            if ((st = clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &ys))) return st;
        }
    }
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgr_to_nv12_frames_dev(mi_ctx* c, const mi_bgr_nv12_frame_dev* frames, int n_frames, int width, int height,
                                                  size_t in_pitch, size_t y_pitch, size_t uv_pitch, int order, mi_uv_mode uv_mode,
                                                  void* stream)
{
    ENTER_COMPUTE(c);
    const BgrNv12FramesShape sh{width, height, in_pitch, y_pitch, uv_pitch, order, uv_mode};
    bool work = false;
    const mi_status st = check_bgr_nv12_frames(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : bgr_nv12_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_bgr_to_nv12_frames_dev(mi_ctx* c, const mi_bgr_nv12_frame_dev* frames, int n_frames, int width, int height,
                                          size_t in_pitch, size_t y_pitch, size_t uv_pitch, int order, mi_uv_mode uv_mode,
                                          double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrNv12FramesShape sh{width, height, in_pitch, y_pitch, uv_pitch, order, uv_mode};
    bool work = false;
    const mi_status st = check_bgr_nv12_frames(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : bgr_nv12_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
