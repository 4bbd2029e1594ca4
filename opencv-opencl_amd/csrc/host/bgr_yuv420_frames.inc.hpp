// bgr_yuv420_frames.inc.hpp -- interleaved BGR / RGB in, planar 4:2:0 (I420 / YV12) or NV12 out on frames given as a list of addresses
// (mi_*_bgr_to_yuv420_frames_dev): checks, the interleaved hand-over, chunking, extern "C"
// Included by ../mi_lumaeq.hip behind bgr_yuv420.inc.hpp (one translation unit; not a stand-alone header).
//
// A software encoder hands out a frame pool: every frame three separately allocated, pitched planes (data[0..2], linesize[0..2]);
// renderers, models and image readers hand over one image per frame.  An INTERLEAVED list is the NV12 list form's own: its checks, its
// kernels (bgr_nv12_frames.inc.hpp) on {in, y, c0}.  A PLANAR list has that form's structure: the call is cut into chunks of
// kFramesPerLaunch frames.  A chunk's {in, y, u, v} entries travel to stage 1 as a BgrYuv420List, its Y planes to stage 2 as a FrameList
// with y_in == y_out and no chroma job, both by value in the kernel arguments, through launch_bgr_to_yuv420 and the planar launchers
// (launch_apply / clahe_dev, as nv12_frames.inc.hpp uses them in place) -- same grids, same partials, same bytes as the batch form.
// Each frame takes the 16 x 2 groups or the 2 x 2 blocks of stage 1 by its own alignment (bgr_yuv420_frame_vec, the kernel's own
// rule); stage 2 has always decided per plane.

namespace {

struct BgrYuv420FramesShape {
    int width, height;
    size_t in_pitch, y_pitch, c_pitch;
    int order;
    mi_uv_mode uv_mode;
};

// the shape as check_bgr_yuv420 and launch_bgr_to_yuv420 take it (PLANAR): stand-in addresses that pass the pointer checks and are
// multiples of 16, frame strides 0, so BgrYuv420Job::vec comes out as what the shape allows
BgrYuv420Args bgr_yuv420_frames_shape_args(const BgrYuv420FramesShape& s, int n_frames)
{
    return BgrYuv420Args{(const uint8_t*)16, s.in_pitch, 0, (uint8_t*)32, s.y_pitch, (uint8_t*)48, (uint8_t*)64, s.c_pitch, 0,
                         s.width, s.height, n_frames, s.order, s.uv_mode, true};
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
// PLANAR lists only (an INTERLEAVED one goes through check_bgr_nv12_frames).
mi_status check_bgr_yuv420_frames(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, const BgrYuv420FramesShape& s,
                                  bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_bgr_yuv420's own answers (order, uv_mode, sizes, even width and height, tiles, pitches, the planar forms' limits)
    bool any = false;
    const mi_status st = check_bgr_yuv420(c, bgr_yuv420_frames_shape_args(s, n_frames), is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_bgr_yuv420_frame_dev& f = frames[k];
        if (!f.in || !f.y || !f.c0 || !f.c1) return fail(c, MI_ERR_BAD_ARG, "null image or plane pointer");
        // there is no in-place form (3 bytes per pixel in, 1 and 2 x 1/4 out): the image's rows may meet no plane of its own frame, and
        // the Y plane neither chroma plane.  U and V are compared by address only: their rows may lie side by side in one pitched plane.
        const Span si(f.in, s.in_pitch, 3 * w, rows), sy(f.y, s.y_pitch, w, rows);
        const Span su(f.c0, s.c_pitch, w / 2, rows / 2), sv(f.c1, s.c_pitch, w / 2, rows / 2);
        if (si.meets(sy) || si.meets(su) || si.meets(sv))
            return fail(c, MI_ERR_BAD_ARG, "BGR in, 4:2:0 out has no in-place form: an image overlaps a plane of its own frame");
        if (sy.meets(su) || sy.meets(sv)) return fail(c, MI_ERR_BAD_ARG, "the Y plane of a frame overlaps a chroma plane of its own");
        if (f.c0 == f.c1) return fail(c, MI_ERR_BAD_ARG, "the U and the V plane of a frame at one address");
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE.  Per chunk: one MI_K_COLOR (convert, and count for equalizeHist), then one MI_K_EQ_LUT and one
// MI_K_LUT_APPLY, or what mi_clahe_nv12_frames_dev launches in place on the same Y planes.  The FRAMES are counted by the walk their
// stage-1 kernel took, once the whole call is enqueued.
mi_status bgr_yuv420_frames_dev(mi_ctx* c, hipStream_t s, const mi_bgr_yuv420_frame_dev* frames, int n_frames, const BgrYuv420FramesShape& sh,
                                int op, double clip_limit, int tiles_x, int tiles_y)
{
    mi_status st;
    unsigned long long n_vec = 0;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        BgrYuv420List io{};                                          // the four addresses of a frame for stage 1
        FrameList ys{};                                              // this chunk's Y planes for stage 2, in place (uv.rows = 0: no UV work)
        for (int k = 0; k < nf; ++k) {
            const mi_bgr_yuv420_frame_dev& f = frames[f0 + k];
            io.f[k] = BgrYuv420Frame{(const uint8_t*)f.in, (uint8_t*)f.y, (uint8_t*)f.c0, (uint8_t*)f.c1};
            ys.f[k] = FramePlanes{(const uint8_t*)f.y, nullptr, (uint8_t*)f.y, nullptr};
        }
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{ys.f[0].y_in, sh.y_pitch, 0, ys.f[0].y_out, sh.y_pitch, 0, sh.width, sh.height, nf};
        const BgrYuv420Args shape = bgr_yuv420_frames_shape_args(sh, nf);
        bool shape_vec = false;
        if (!op) {
            int nparts = 0;
            if ((st = launch_bgr_to_yuv420(c, s, shape, 0, nf, true, &nparts, &shape_vec, &io))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            if ((st = launch_apply(c, s, ya, 0, nf, c->d_luts, nullptr, &ys))) return st;
        } else {
            if ((st = launch_bgr_to_yuv420(c, s, shape, 0, nf, false, nullptr, &shape_vec, &io))) return st;
            if ((st = clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &ys))) return st;
        }
        for (int k = 0; k < nf; ++k) n_vec += bgr_yuv420_frame_vec(shape_vec, io.f[k].in, io.f[k].y, io.f[k].u, io.f[k].v);
    }
    c->bgr_yuv420_list_frames_vec += n_vec;
    c->bgr_yuv420_list_frames_bytes += (unsigned long long)n_frames - n_vec;
    return MI_OK;
}

mi_status bgr_yuv420_frames_entry(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height, size_t in_pitch,
                                  size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode, int op, double clip_limit,
                                  int tiles_x, int tiles_y, void* stream)
{
    if (chroma != MI_CHROMA_INTERLEAVED && chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    bool work = false;
    if (chroma == MI_CHROMA_INTERLEAVED) {                  // the NV12 list form's own path on {in, y, c0}: its checks, its kernels, no counter here
        std::vector<mi_bgr_nv12_frame_dev> nv;
        if (frames && n_frames > 0) {
            nv.resize((size_t)n_frames);
            for (int k = 0; k < n_frames; ++k) nv[k] = mi_bgr_nv12_frame_dev{frames[k].in, frames[k].y, frames[k].c0};
        }
        const BgrNv12FramesShape sh{width, height, in_pitch, y_pitch, c_pitch, order, uv_mode};
        const mi_status st = check_bgr_nv12_frames(c, nv.empty() ? nullptr : nv.data(), n_frames, sh, op != 0, tiles_x, tiles_y, &work);
        return (st || !work) ? st : bgr_nv12_frames_dev(c, pick_stream(c, stream), nv.data(), n_frames, sh, op, clip_limit, tiles_x, tiles_y);
    }
    const BgrYuv420FramesShape sh{width, height, in_pitch, y_pitch, c_pitch, order, uv_mode};
    const mi_status st = check_bgr_yuv420_frames(c, frames, n_frames, sh, op != 0, tiles_x, tiles_y, &work);
    return (st || !work) ? st : bgr_yuv420_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgr_to_yuv420_frames_dev(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                                    size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order,
                                                    mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_yuv420_frames_entry(c, frames, n_frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order, uv_mode, 0, 0.0, 0, 0,
                                   stream);
}

mi_status mi_clahe_bgr_to_yuv420_frames_dev(mi_ctx* c, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                            size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode,
                                            double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_yuv420_frames_entry(c, frames, n_frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order, uv_mode, 1, clip_limit,
                                   tiles_x, tiles_y, stream);
}

}  // extern "C"
