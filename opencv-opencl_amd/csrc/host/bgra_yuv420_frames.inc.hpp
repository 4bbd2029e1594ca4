// bgra_yuv420_frames.inc.hpp -- four-channel BGRA / RGBA (CV_8UC4) in, planar 4:2:0 (I420 / YV12) or NV12 out on frames given as a list
// of addresses (mi_*_bgra_to_yuv420_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip behind bgra_yuv420.inc.hpp (one translation unit; not a stand-alone header).
//
// A renderer, a compositor or a capture API hands out a pool of four-byte surfaces; an encoder hands out a frame pool: every frame
// separately allocated, pitched planes (NV12: a Y and a UV plane; I420 / YV12: data[0..2], linesize[0..2]).  The structure is
// bgr_yuv420_frames.inc.hpp's, but BOTH chroma layouts are this form's own kernels and counters: an INTERLEAVED list is not handed to
// another form.  The call is cut into chunks of kFramesPerLaunch frames.  A chunk's {in, y, c0, c1} entries travel to stage 1 as a
// BgraYuv420List, its Y planes to stage 2 as a FrameList with y_in == y_out and no chroma job, both by value in the kernel arguments,
// through launch_bgra_to_yuv420 and the planar launchers (launch_apply / clahe_dev, as nv12_frames.inc.hpp uses them in place) -- same
// grids, same partials, same bytes as the batch form.  Each frame takes the 16 x 2 groups or the 2 x 2 blocks of stage 1 by its own
// alignment (bgra_yuv420_frame_vec, the kernel's own rule); stage 2 has always decided per plane.

namespace {

struct BgraYuv420FramesShape {
    int width, height;
    size_t in_pitch, y_pitch, c_pitch;
    int order;
    mi_uv_mode uv_mode;
    bool planar;
};

// the shape as check_bgra_yuv420 and launch_bgra_to_yuv420 take it: stand-in addresses that pass the pointer checks and are multiples
// of 16, frame strides 0, so BgraYuv420Job::vec comes out as what the shape allows
BgraYuv420Args bgra_yuv420_frames_shape_args(const BgraYuv420FramesShape& s, int n_frames)
{
    return BgraYuv420Args{(const uint8_t*)16, s.in_pitch, 0, (uint8_t*)32, s.y_pitch, (uint8_t*)48, s.planar ? (uint8_t*)64 : nullptr,
                          s.c_pitch, 0, s.width, s.height, n_frames, s.order, s.uv_mode, s.planar};
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_bgra_yuv420_frames(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, const BgraYuv420FramesShape& s,
                                   bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_bgra_yuv420's own answers (order, uv_mode, sizes, even width and height, tiles, pitches, the planar forms' limits)
    bool any = false;
    const mi_status st = check_bgra_yuv420(c, bgra_yuv420_frames_shape_args(s, n_frames), is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_bgr_yuv420_frame_dev& f = frames[k];
        if (!f.in || !f.y || !f.c0 || (s.planar && !f.c1)) return fail(c, MI_ERR_BAD_ARG, "null image or plane pointer");
        // there is no in-place form (4 bytes per pixel in, 1 and 1/2 out): the image's rows may meet no plane of its own frame, and the
        // Y plane no chroma plane.  U and V are compared by address only: their rows may lie side by side in one pitched plane.
        const Span si(f.in, s.in_pitch, 4 * w, rows), sy(f.y, s.y_pitch, w, rows);
        if (si.meets(sy)) return fail(c, MI_ERR_BAD_ARG, "BGRA in, 4:2:0 out has no in-place form: an image overlaps a plane of its own frame");
        if (s.planar) {
            const Span su(f.c0, s.c_pitch, w / 2, rows / 2), sv(f.c1, s.c_pitch, w / 2, rows / 2);
            if (si.meets(su) || si.meets(sv))
                return fail(c, MI_ERR_BAD_ARG, "BGRA in, 4:2:0 out has no in-place form: an image overlaps a plane of its own frame");
            if (sy.meets(su) || sy.meets(sv)) return fail(c, MI_ERR_BAD_ARG, "the Y plane of a frame overlaps a chroma plane of its own");
            if (f.c0 == f.c1) return fail(c, MI_ERR_BAD_ARG, "the U and the V plane of a frame at one address");
        } else {
            const Span su(f.c0, s.c_pitch, w, rows / 2);
            if (si.meets(su)) return fail(c, MI_ERR_BAD_ARG, "BGRA in, 4:2:0 out has no in-place form: an image overlaps a plane of its own frame");
            if (sy.meets(su)) return fail(c, MI_ERR_BAD_ARG, "the Y plane of a frame overlaps its own UV plane");
        }
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE.  Per chunk: one MI_K_COLOR (convert, and count for equalizeHist), then one MI_K_EQ_LUT and one
// MI_K_LUT_APPLY, or what mi_clahe_nv12_frames_dev launches in place on the same Y planes.  The FRAMES are counted by the walk their
// stage-1 kernel took, once the whole call is enqueued.
mi_status bgra_yuv420_frames_dev(mi_ctx* c, hipStream_t s, const mi_bgr_yuv420_frame_dev* frames, int n_frames, const BgraYuv420FramesShape& sh,
                                 int op, double clip_limit, int tiles_x, int tiles_y)
{
    mi_status st;
    unsigned long long n_vec = 0;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        BgraYuv420List io{};                                         // the four addresses of a frame for stage 1 (c1 null on an interleaved list)
        FrameList ys{};                                              // this chunk's Y planes for stage 2, in place (uv.rows = 0: no UV work)
        for (int k = 0; k < nf; ++k) {
            const mi_bgr_yuv420_frame_dev& f = frames[f0 + k];
            io.f[k] = BgraYuv420Frame{(const uint8_t*)f.in, (uint8_t*)f.y, (uint8_t*)f.c0, sh.planar ? (uint8_t*)f.c1 : nullptr};
            ys.f[k] = FramePlanes{(const uint8_t*)f.y, nullptr, (uint8_t*)f.y, nullptr};
        }
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{ys.f[0].y_in, sh.y_pitch, 0, ys.f[0].y_out, sh.y_pitch, 0, sh.width, sh.height, nf};
        const BgraYuv420Args shape = bgra_yuv420_frames_shape_args(sh, nf);
        bool shape_vec = false;
        if (!op) {
            int nparts = 0;
            if ((st = launch_bgra_to_yuv420(c, s, shape, 0, nf, true, &nparts, &shape_vec, &io))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            if ((st = launch_apply(c, s, ya, 0, nf, c->d_luts, nullptr, &ys))) return st;
        } else {
            if ((st = launch_bgra_to_yuv420(c, s, shape, 0, nf, false, nullptr, &shape_vec, &io))) return st;
            if ((st = clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &ys))) return st;
        }
        for (int k = 0; k < nf; ++k) n_vec += bgra_yuv420_frame_vec(shape_vec, sh.planar, io.f[k].in, io.f[k].y, io.f[k].c0, io.f[k].c1);
    }
    c->bgra_yuv420_list_frames_vec += n_vec;
    c->bgra_yuv420_list_frames_bytes += (unsigned long long)n_frames - n_vec;
    return MI_OK;
}

mi_status bgra_yuv420_frames_entry(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height, size_t in_pitch,
                                   size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode, int op, double clip_limit,
                                   int tiles_x, int tiles_y, void* stream)
{
    if (chroma != MI_CHROMA_INTERLEAVED && chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const BgraYuv420FramesShape sh{width, height, in_pitch, y_pitch, c_pitch, order, uv_mode, chroma == MI_CHROMA_PLANAR};
    bool work = false;
    const mi_status st = check_bgra_yuv420_frames(c, frames, n_frames, sh, op != 0, tiles_x, tiles_y, &work);
    return (st || !work) ? st : bgra_yuv420_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgra_to_yuv420_frames_dev(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                                     size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order,
                                                     mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return bgra_yuv420_frames_entry(c, frames, n_frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order, uv_mode, 0, 0.0, 0, 0,
                                    stream);
}

mi_status mi_clahe_bgra_to_yuv420_frames_dev(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                             size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode,
                                             double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgra_yuv420_frames_entry(c, frames, n_frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order, uv_mode, 1, clip_limit,
                                    tiles_x, tiles_y, stream);
}

}  // extern "C"
