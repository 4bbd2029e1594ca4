// bgr_packed422_frames.inc.hpp -- interleaved BGR / RGB in, packed 4:2:2 (YUY2 / UYVY) out on frames given as a LIST of addresses
// (mi_*_bgr_to_packed422_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip after bgr_packed422.inc.hpp (one translation unit; not a stand-alone header).
//
// A playout card, a v4l2 output queue or a virtual camera hands out a buffer pool: every packed frame its own allocation, padded to
// bytesperline, at whatever alignment the driver chose; renderers, models and image readers hand over one image per frame.  The call is
// cut into chunks of kPacked422FramesPerLaunch frames -- the capacity of stage 2's table, so one chunk size serves both stages.  A
// chunk's {image, frame} pairs travel to stage 1 as a Packed422List, its output frames to stage 2 as a second Packed422List with
// in == out, both by value in the kernel arguments, through launch_bgr_to_packed422 and the packed form's own launchers (launch_pair on
// PackedOut's apply / clahe422_dev, as packed422_frames.inc.hpp uses them in place) -- same grids, same partials, same bytes as the
// batch form.  Each frame takes the 16 x 1 groups or the macropixels of stage 1 by its own two addresses; stage 2 has always decided
// per row.  The check, the chunk loop and the entry are templates on the pixel form F of bgr_packed422.inc.hpp, written once for every
// form.

namespace {

struct BgrP422FramesShape {
    int width, height;
    size_t in_pitch, out_pitch;
    int order, format;
    mi_uv_mode uv_mode;
};

// the shape as check_bgr_packed422 and launch_bgr_to_packed422 take it: stand-in addresses that pass the pointer checks and are
// multiples of 16, frame strides 0, so BgrPacked422Job::vec comes out as what the shape allows
BgrP422Args bgr_packed422_frames_shape_args(const BgrP422FramesShape& s, int n_frames)
{
    return BgrP422Args{(const uint8_t*)16, s.in_pitch, 0, (uint8_t*)32, s.out_pitch, 0, s.width, s.height, n_frames, s.order, s.format,
                       s.uv_mode};
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
template <class F>
mi_status check_bgr_packed422_frames(mi_ctx* c, const mi_bgr_packed422_frame_dev* frames, int n_frames, const BgrP422FramesShape& s,
                                     bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_bgr_packed422's own answers (order, format, uv_mode, sizes, even width, tiles, the pitches, the limits of the
    // packed and planar forms)
    bool any = false;
    const mi_status st = check_bgr_packed422<F>(c, bgr_packed422_frames_shape_args(s, n_frames), false, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_bgr_packed422_frame_dev& f = frames[k];
        if (!f.in || !f.out) return fail(c, MI_ERR_BAD_ARG, "null image or frame pointer");
        if ((uintptr_t)f.out & 3) return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 frame addresses are multiples of 4");
        // there is no in-place form (kPx bytes per pixel in, 2 out): the image's rows may not meet the rows of its own output frame
        if (Span(f.in, s.in_pitch, F::kPx * w, rows).meets(Span(f.out, s.out_pitch, 2 * w, rows)))
            return fail(c, MI_ERR_BAD_ARG, F::kListOverlap);
    }
    *work = true;
    return MI_OK;
}

// Per chunk: one MI_K_COLOR (convert, and count for equalizeHist), then one MI_K_EQ_LUT and one MI_K_LUT_APPLY, or what
// mi_clahe_packed422_frames_dev launches in place on the same output frames.  No MI_K_HIST.
template <class F, int OFF>
mi_status bgr_packed422_frames_dev(mi_ctx* c, hipStream_t s, const mi_bgr_packed422_frame_dev* frames, int n_frames,
                                   const BgrP422FramesShape& sh, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    mi_status st;
    unsigned long long n_vec = 0;
    const long long frame_bytes = 2LL * sh.width * sh.height;
    for (int f0 = 0; f0 < n_frames; f0 += kPacked422FramesPerLaunch) {
        const int nf = std::min(kPacked422FramesPerLaunch, n_frames - f0);
        Packed422List io{};                                          // this chunk's {image, frame} pairs for stage 1, from index 0
        Packed422List fr{};                                          // its output frames for stage 2, in place
        for (int k = 0; k < nf; ++k) {
            const mi_bgr_packed422_frame_dev& f = frames[f0 + k];
            io.f[k] = Packed422Frame{(const uint8_t*)f.in, (uint8_t*)f.out};
            fr.f[k] = Packed422Frame{(const uint8_t*)f.out, (uint8_t*)f.out};
        }
        const BgrP422Args shape = bgr_packed422_frames_shape_args(sh, nf);
        // the frames as the packed form's stages take them with a list: the chunk's first frame, frame strides 0, the chroma kept
        const P422Args pa{fr.f[0].in, sh.out_pitch, 0, fr.f[0].out, sh.out_pitch, 0, sh.width, sh.height, nf, sh.format, MI_UV_COPY};
        bool shape_vec = false;
        if (!is_clahe) {
            int nparts = 0;
            if ((st = launch_bgr_to_packed422<F>(c, s, shape, 0, nf, true, &nparts, &shape_vec, &io))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            const int BA = blocks_per_frame(c, frame_bytes, PackedOut::apply_rows(sh.height), nf, 2048);
            if ((st = launch_pair(c, s, MI_K_LUT_APPLY, PackedOut::K<OFF>::apply, &fr, dim3(BA, nf), dim3(kThreads), 0,
                                  PackedOut::cut(pa, 0), (const uint8_t*)c->d_luts))) return st;
        } else {
            if ((st = launch_bgr_to_packed422<F>(c, s, shape, 0, nf, false, nullptr, &shape_vec, &io))) return st;
            if ((st = clahe422_dev<PackedOut, OFF>(c, s, pa, clip_limit, tiles_x, tiles_y, &fr, &fr))) return st;
        }
        // the walk of each frame: the kernel's own rule (bgr_packed422_frame_vec for three channels), shape_vec being the launch's j.vec
        for (int k = 0; k < nf; ++k) n_vec += F::frame_vec(shape_vec, io.f[k].in, io.f[k].out);
    }
    // the FRAMES by the walk their stage-1 kernel took, once the whole call is enqueued
    F::count_list(c, n_frames, n_vec);
    return MI_OK;
}

template <class F>
mi_status bgr_packed422_frames_entry(mi_ctx* c, const mi_bgr_packed422_frame_dev* frames, int n_frames, const BgrP422FramesShape& sh,
                                     bool is_clahe, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    bool work = false;
    const mi_status st = check_bgr_packed422_frames<F>(c, frames, n_frames, sh, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    hipStream_t s = pick_stream(c, stream);
    return sh.format == MI_FMT_UYVY ? bgr_packed422_frames_dev<F, 1>(c, s, frames, n_frames, sh, is_clahe, clip_limit, tiles_x, tiles_y)
                                    : bgr_packed422_frames_dev<F, 0>(c, s, frames, n_frames, sh, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgr_to_packed422_frames_dev(mi_ctx* c, const mi_bgr_packed422_frame_dev* frames, int n_frames,
                                                       int width, int height, size_t in_pitch, size_t out_pitch, int order, int format,
                                                       mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrP422FramesShape sh{width, height, in_pitch, out_pitch, order, format, uv_mode};
    return bgr_packed422_frames_entry<BgrTo422>(c, frames, n_frames, sh, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_bgr_to_packed422_frames_dev(mi_ctx* c, const mi_bgr_packed422_frame_dev* frames, int n_frames,
                                               int width, int height, size_t in_pitch, size_t out_pitch, int order, int format,
                                               mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrP422FramesShape sh{width, height, in_pitch, out_pitch, order, format, uv_mode};
    return bgr_packed422_frames_entry<BgrTo422>(c, frames, n_frames, sh, true, clip_limit, tiles_x, tiles_y, stream);
}

}  // extern "C"
