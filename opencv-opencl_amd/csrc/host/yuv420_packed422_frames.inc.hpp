// yuv420_packed422_frames.inc.hpp -- 4:2:0 (NV12, or planar I420 / YV12) in, pitched packed 4:2:2 (YUY2 / UYVY) out on frames given as a
// list of addresses (mi_*_yuv420_to_packed422_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip behind yuv420_packed422.inc.hpp (one translation unit; not a stand-alone header).
//
// Both real sides of this form are pools: a decoder hands out surfaces whose Y, U and V (or UV) planes are separate pitched allocations
// (data[0..2], linesize[0..2]), and a playout card, a v4l2 output queue or a virtual camera hands out one buffer per frame, padded to
// bytesperline.  The structure is that of yuv420_bgr_frames.inc.hpp: the call is cut into chunks of kFramesPerLaunch frames; a chunk's
// Y planes travel to the histogram stages as a FrameList (the planar launchers: same scratch, same grids), its {y, c0, c1, out}
// entries to the pixel-writing stage as a Yuv420P422List, both by value in the kernel arguments, through the launchers of
// yuv420_packed422.inc.hpp -- same grids, same bands and segments, same bytes as the batch form.  Unlike that sibling an INTERLEAVED
// list is not handed to another form: the kernels carry the chroma layout as a template parameter, so one pair of entry points and one
// set of counters serves both layouts.
// equalizeHist maps and packs in one kernel whatever the addresses are: each frame takes the 16 x 2 groups or the 2 x 2 blocks by its
// own alignment (yuv420_packed422_frame_vec, the kernel's own rule).  The CLAHE blend + pack kernel has no byte path, so CLAHE is
// one-pass only when the shape is the batch form's one-pass shape, the shape allows the groups AND every frame of the call passes the
// address rule; otherwise the whole call runs the planar CLAHE (clahe_dev on the list) into the context's scratch planes and the pack
// alone from there, chunk by chunk.  Under MI_UV_FILL128 the chroma addresses and the chroma pitch are cleared before anything looks
// at them: they are not read and decide nothing.

namespace {

struct Yuv420P422FramesShape {
    int width, height;
    size_t y_pitch, c_pitch, out_pitch;      // c_pitch: 0 under MI_UV_FILL128
    int format;
    mi_uv_mode uv_mode;
    bool planar;
};

// the addresses of entry f as the kernels and the rule see them: c1 of an interleaved list and both chroma addresses under
// MI_UV_FILL128 are dropped
Yuv420P422Frame yuv420_packed422_entry_of(const mi_yuv420_packed422_frame_dev& f, const Yuv420P422FramesShape& s)
{
    const bool copy = s.uv_mode == MI_UV_COPY;
    return Yuv420P422Frame{(const uint8_t*)f.y, copy ? (const uint8_t*)f.c0 : nullptr, copy && s.planar ? (const uint8_t*)f.c1 : nullptr,
                           (uint8_t*)f.out};
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_yuv420_packed422_frames(mi_ctx* c, const mi_yuv420_packed422_frame_dev* frames, int n_frames, const Yuv420P422FramesShape& s,
                                        bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    const bool copy = s.uv_mode == MI_UV_COPY;
    // the shape: check_yuv420_packed422's own answers (format, uv_mode, sizes, even width and height, tiles, pitches, the multiple of 4
    // of out_pitch, the planar forms' limits), on stand-in addresses that pass its pointer checks
    const Yuv420P422Args shape{(const uint8_t*)16, s.y_pitch, copy ? (const uint8_t*)32 : nullptr, copy && s.planar ? (const uint8_t*)48 : nullptr,
                               s.c_pitch, 0, (uint8_t*)64, s.out_pitch, 0, s.width, s.height, n_frames, s.format, s.uv_mode, s.planar};
    bool any = false;
    const mi_status st = check_yuv420_packed422(c, shape, false, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const Yuv420P422Frame f = yuv420_packed422_entry_of(frames[k], s);
        if (!f.y || !f.out) return fail(c, MI_ERR_BAD_ARG, "null plane or frame pointer");
        if (copy && (!f.c0 || (s.planar && !f.c1))) return fail(c, MI_ERR_BAD_ARG, "MI_UV_COPY needs the input chroma planes");
        if ((uintptr_t)f.out & 3) return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 pointers are multiples of 4");
        // there is no in-place form (1.5 bytes per pixel in, 2 out): the frame's rows may meet no plane of its own frame that the call
        // reads.  The input planes are not compared with each other: U and V rows may lie side by side in one pitched plane.
        const Span so(f.out, s.out_pitch, 2 * w, rows), sy(f.y, s.y_pitch, w, rows);
        bool meets = so.meets(sy);
        if (copy && s.planar) meets = meets || so.meets(Span(f.c0, s.c_pitch, w / 2, rows / 2)) || so.meets(Span(f.c1, s.c_pitch, w / 2, rows / 2));
        else if (copy)        meets = meets || so.meets(Span(f.c0, s.c_pitch, w, rows / 2));
        if (meets) return fail(c, MI_ERR_BAD_ARG, "4:2:0 in, packed 4:2:2 out has no in-place form: a frame overlaps a plane of its own input");
    }
    *work = true;
    return MI_OK;
}

// what the shape allows (Yuv420P422Job::vec of a table launch); the kernel adds each frame's own addresses
bool yuv420_packed422_frames_shape_vec(const Yuv420P422FramesShape& s)
{
    return s.width % 16 == 0 && ((s.y_pitch | s.out_pitch) & 15) == 0 && (s.c_pitch & (s.planar ? 7 : 15)) == 0;
}

// the shape of a table launch; y_pitch: the caller's, or that of the scratch planes
Yuv420P422Job yuv420_packed422_frames_job(const Yuv420P422FramesShape& s, size_t y_pitch)
{
    Yuv420P422Job j{};
    j.y_step = (long long)y_pitch; j.c_step = (long long)s.c_pitch; j.out_step = (long long)s.out_pitch;
    j.width = s.width; j.height = s.height;
    j.vec = yuv420_packed422_frames_shape_vec(s) && (y_pitch & 15) == 0;
    j.copy_uv = s.uv_mode == MI_UV_COPY;
    return j;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status yuv420_packed422_frames_dev(mi_ctx* c, hipStream_t s, const mi_yuv420_packed422_frame_dev* frames, int n_frames,
                                      const Yuv420P422FramesShape& sh, int op, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g{};
    mi_status st;
    bool onepass = true;
    const int copy = sh.uv_mode == MI_UV_COPY;
    const size_t plane = ((size_t)sh.width * sh.height + 15) & ~(size_t)15;      // a tight scratch Y plane, 16-byte aligned
    if (op) {
        if ((st = clahe_geometry(c, sh.width, sh.height, clip_limit, tiles_x, tiles_y, &g))) return st;
        onepass = nv12_bgr_onepass_shape(g, sh.width, sh.height, tiles_x, tiles_y) && yuv420_packed422_frames_shape_vec(sh);
        for (int k = 0; onepass && k < n_frames; ++k) {
            const Yuv420P422Frame f = yuv420_packed422_entry_of(frames[k], sh);
            onepass = yuv420_packed422_frame_vec(1, copy, sh.planar, f.y, f.c0, f.c1, f.out);
        }
        if (!onepass && (st = grow_dev(c, &c->d_planes, &c->planes_bytes, plane * (size_t)std::min(kFramesPerLaunch, n_frames)))) return st;
    }
    const int tiles = tiles_x * tiles_y;
    // the shape of the pixel-writing launch: the luma comes from the caller's planes, or from the scratch planes of the fallback
    const Yuv420P422Job j = yuv420_packed422_frames_job(sh, onepass ? sh.y_pitch : (size_t)sh.width);
    unsigned long long n_vec = 0;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        FrameList in{};                                              // this chunk's Y planes for the planar stages (uv.rows = 0: no UV work)
        Yuv420P422List io{};                                         // the four addresses of a frame for the stage that writes pixels
        for (int k = 0; k < nf; ++k) {
            Yuv420P422Frame f = yuv420_packed422_entry_of(frames[f0 + k], sh);
            uint8_t* y_out = onepass ? nullptr : c->d_planes + (size_t)k * plane;
            in.f[k] = FramePlanes{f.y, nullptr, y_out, nullptr};
            if (!onepass) f.y = y_out;
            io.f[k] = f;
            n_vec += yuv420_packed422_frame_vec(j.vec, copy, sh.planar, f.y, f.c0, f.c1, f.out);
        }
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{in.f[0].y_in, sh.y_pitch, 0, in.f[0].y_out, onepass ? 0 : (size_t)sh.width, 0, sh.width, sh.height, nf};
        if (!op) {
            int nparts = 0;
            if ((st = launch_hist_partials(c, s, ya, 0, nf, &nparts, &in))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            if ((st = launch_yuv420_to_packed422(c, s, j, nf, sh.format, sh.planar, c->d_luts, &io))) return st;
        } else if (onepass) {
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, 0, nf, c->d_luts, &in))) return st;
            if ((st = launch_yuv420_packed422_interp(c, s, j, g, nf, sh.format, sh.planar, c->d_luts, &io))) return st;
        } else {
            if ((st = clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &in))) return st;
            if ((st = launch_yuv420_to_packed422(c, s, j, nf, sh.format, sh.planar, nullptr, &io))) return st;
        }
    }
    // one count per call; the FRAMES by the walk their pixel-writing kernel took (the one-pass CLAHE kernel has the 16-pixel walk only,
    // and is taken only when the rule holds for every frame)
    ++(onepass ? c->yuv420_packed422_onepass : c->yuv420_packed422_twopass);
    c->yuv420_packed422_list_frames_vec += n_vec;
    c->yuv420_packed422_list_frames_bytes += (unsigned long long)n_frames - n_vec;
    return MI_OK;
}

mi_status yuv420_packed422_frames_entry(mi_ctx* c, const mi_yuv420_packed422_frame_dev* frames, int n_frames, int width, int height,
                                        size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int format, mi_uv_mode uv_mode, int op,
                                        double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    if (chroma != MI_CHROMA_INTERLEAVED && chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    // with MI_UV_FILL128 the input's chroma is not read and c_pitch is ignored
    const Yuv420P422FramesShape sh{width, height, y_pitch, uv_mode == MI_UV_COPY ? c_pitch : 0, out_pitch, format, uv_mode,
                                   chroma == MI_CHROMA_PLANAR};
    bool work = false;
    const mi_status st = check_yuv420_packed422_frames(c, frames, n_frames, sh, op != 0, tiles_x, tiles_y, &work);
    return (st || !work) ? st : yuv420_packed422_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_to_packed422_frames_dev(mi_ctx* c, const mi_yuv420_packed422_frame_dev* frames, int n_frames, int width,
                                                          int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int format,
                                                          mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_packed422_frames_entry(c, frames, n_frames, width, height, y_pitch, c_pitch, chroma, out_pitch, format, uv_mode, 0, 0.0, 0, 0,
                                         stream);
}

mi_status mi_clahe_yuv420_to_packed422_frames_dev(mi_ctx* c, const mi_yuv420_packed422_frame_dev* frames, int n_frames, int width, int height,
                                                  size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int format, mi_uv_mode uv_mode,
                                                  double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_packed422_frames_entry(c, frames, n_frames, width, height, y_pitch, c_pitch, chroma, out_pitch, format, uv_mode, 1, clip_limit,
                                         tiles_x, tiles_y, stream);
}

}  // extern "C"
