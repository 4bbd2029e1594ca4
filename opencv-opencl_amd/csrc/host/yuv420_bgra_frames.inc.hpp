// yuv420_bgra_frames.inc.hpp -- planar 4:2:0 (I420 / YV12) or NV12 in, interleaved four-channel BGRA / RGBA (CV_8UC4, A = 255) out on
// frames given as a list of addresses (mi_*_yuv420_to_bgra_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip behind yuv420_bgra.inc.hpp (one translation unit; not a stand-alone header).
//
// A decoder hands out a frame pool -- a software decoder three separately allocated, pitched planes a frame (data[0..2],
// linesize[0..2]), a hardware decoder a Y and a UV plane a surface -- and the images go to a pool of display surfaces or textures.
// Unlike yuv420_bgr_frames.inc.hpp an INTERLEAVED list is not handed to another form: both layouts are this form's own kernels and
// counters (c1 of an entry is ignored and may be null then).  The call is cut into chunks of kFramesPerLaunch frames; a chunk's Y
// planes travel to the histogram stages as a FrameList (the planar launchers: same scratch, same grids), its {y, c0, c1, out} entries
// to the pixel-writing stage as a Yuv420BgraList, both by value in the kernel arguments, through the launchers of yuv420_bgra.inc.hpp
// -- same grids, same bands and segments, same bytes as the batch form.
// equalizeHist maps and decodes in one kernel whatever the addresses are: each frame takes the 16 x 2 groups or the 2 x 2 blocks by
// its own alignment (yuv420_bgra_frame_vec, the kernel's own rule).  The CLAHE blend + decode kernel has no byte path, so CLAHE is
// one-pass only when the shape is the batch form's one-pass shape, the shape allows the groups AND every frame of the call passes the
// address rule; otherwise the whole call runs the planar CLAHE (clahe_dev on the list) into the context's scratch planes and the decode
// alone from there, chunk by chunk.

namespace {

struct Yuv420BgraFramesShape {
    int width, height;
    size_t y_pitch, c_pitch, out_pitch;
    int order;
    bool planar;
};

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_yuv420_bgra_frames(mi_ctx* c, const mi_yuv420_bgr_frame_dev* frames, int n_frames, const Yuv420BgraFramesShape& s,
                                   bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_yuv420_bgra's own answers (order, sizes, even width and height, tiles, pitches, the planar forms' limits), on
    // stand-in addresses that pass its pointer checks
    const Yuv420BgraArgs shape{(const uint8_t*)16, s.y_pitch, (const uint8_t*)32, s.planar ? (const uint8_t*)48 : nullptr, s.c_pitch, 0,
                               (uint8_t*)64, s.out_pitch, 0, s.width, s.height, n_frames, s.order, s.planar};
    bool any = false;
    const mi_status st = check_yuv420_bgra(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_yuv420_bgr_frame_dev& f = frames[k];
        if (!f.y || !f.c0 || (s.planar && !f.c1) || !f.out) return fail(c, MI_ERR_BAD_ARG, "null plane pointer");
        // there is no in-place form (1 or 1/4 byte per pixel in, 4 out): the image's rows may meet no plane of its own frame.  The
        // input planes are not compared with each other: U and V rows may lie side by side in one pitched plane.
        const Span so(f.out, s.out_pitch, 4 * w, rows), sy(f.y, s.y_pitch, w, rows);
        bool meets = so.meets(sy);
        if (s.planar) {
            const Span su(f.c0, s.c_pitch, w / 2, rows / 2), sv(f.c1, s.c_pitch, w / 2, rows / 2);
            meets = meets || so.meets(su) || so.meets(sv);
        } else {
            meets = meets || so.meets(Span(f.c0, s.c_pitch, w, rows / 2));
        }
        if (meets) return fail(c, MI_ERR_BAD_ARG, "4:2:0 in, BGRA out has no in-place form: an image overlaps a plane of its own frame");
    }
    *work = true;
    return MI_OK;
}

// what the shape allows (Yuv420BgraJob::vec of a table launch); the kernel adds each frame's own addresses
bool yuv420_bgra_frames_shape_vec(const Yuv420BgraFramesShape& s)
{
    return s.width % 16 == 0 && ((s.y_pitch | s.out_pitch) & 15) == 0 && (s.c_pitch & (s.planar ? 7 : 15)) == 0;
}

// the shape of a table launch; y_pitch: the caller's, or that of the scratch planes
Yuv420BgraJob yuv420_bgra_frames_job(const Yuv420BgraFramesShape& s, size_t y_pitch)
{
    Yuv420BgraJob j{};
    j.y_step = (long long)y_pitch; j.c_step = (long long)s.c_pitch; j.out_step = (long long)s.out_pitch;
    j.width = s.width; j.height = s.height;
    j.vec = yuv420_bgra_frames_shape_vec(s) && (y_pitch & 15) == 0;
    return j;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status yuv420_bgra_frames_dev(mi_ctx* c, hipStream_t s, const mi_yuv420_bgr_frame_dev* frames, int n_frames, const Yuv420BgraFramesShape& sh,
                                 int op, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g{};
    mi_status st;
    bool onepass = true;
    const size_t plane = ((size_t)sh.width * sh.height + 15) & ~(size_t)15;      // a tight scratch Y plane, 16-byte aligned
    if (op) {
        if ((st = clahe_geometry(c, sh.width, sh.height, clip_limit, tiles_x, tiles_y, &g))) return st;
        onepass = nv12_bgr_onepass_shape(g, sh.width, sh.height, tiles_x, tiles_y) && yuv420_bgra_frames_shape_vec(sh);
        for (int k = 0; onepass && k < n_frames; ++k)
            onepass = yuv420_bgra_frame_vec(1, sh.planar, frames[k].y, frames[k].c0, frames[k].c1, frames[k].out);
        if (!onepass && (st = grow_dev(c, &c->d_planes, &c->planes_bytes, plane * (size_t)std::min(kFramesPerLaunch, n_frames)))) return st;
    }
    const int tiles = tiles_x * tiles_y;
    // the shape of the pixel-writing launch: the luma comes from the caller's planes, or from the scratch planes of the fallback
    const Yuv420BgraJob j = yuv420_bgra_frames_job(sh, onepass ? sh.y_pitch : (size_t)sh.width);
    unsigned long long n_vec = 0;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        FrameList in{};                                              // this chunk's Y planes for the planar stages (uv.rows = 0: no UV work)
        Yuv420BgraList io{};                                         // the four addresses of a frame for the stage that writes pixels (c1 null on an interleaved list)
        for (int k = 0; k < nf; ++k) {
            const mi_yuv420_bgr_frame_dev& f = frames[f0 + k];
            uint8_t* y_out = onepass ? nullptr : c->d_planes + (size_t)k * plane;
            in.f[k] = FramePlanes{(const uint8_t*)f.y, nullptr, y_out, nullptr};
            io.f[k] = Yuv420BgraFrame{onepass ? (const uint8_t*)f.y : y_out, (const uint8_t*)f.c0, sh.planar ? (const uint8_t*)f.c1 : nullptr,
                                      (uint8_t*)f.out};
            n_vec += yuv420_bgra_frame_vec(j.vec, sh.planar, io.f[k].y, io.f[k].c0, io.f[k].c1, io.f[k].out);
        }
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{in.f[0].y_in, sh.y_pitch, 0, in.f[0].y_out, onepass ? 0 : (size_t)sh.width, 0, sh.width, sh.height, nf};
        if (!op) {
            int nparts = 0;
            if ((st = launch_hist_partials(c, s, ya, 0, nf, &nparts, &in))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            if ((st = launch_yuv420_to_bgra(c, s, j, nf, sh.order, sh.planar, c->d_luts, &io))) return st;
        } else if (onepass) {
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, 0, nf, c->d_luts, &in))) return st;
            if ((st = launch_yuv420_bgra_interp(c, s, j, g, nf, sh.order, sh.planar, c->d_luts, &io))) return st;
        } else {
            if ((st = clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &in))) return st;
            if ((st = launch_yuv420_to_bgra(c, s, j, nf, sh.order, sh.planar, nullptr, &io))) return st;
        }
    }
    // one count per call; the FRAMES by the walk their pixel-writing kernel took (the one-pass CLAHE kernel has the 16-pixel walk only,
    // and is taken only when the rule holds for every frame)
    ++(onepass ? c->yuv420_bgra_onepass : c->yuv420_bgra_twopass);
    c->yuv420_bgra_list_frames_vec += n_vec;
    c->yuv420_bgra_list_frames_bytes += (unsigned long long)n_frames - n_vec;
    return MI_OK;
}

mi_status yuv420_bgra_frames_entry(mi_ctx* c, const mi_yuv420_bgr_frame_dev* frames, int n_frames, int width, int height, size_t y_pitch,
                                   size_t c_pitch, int chroma, size_t out_pitch, int order, int op, double clip_limit, int tiles_x,
                                   int tiles_y, void* stream)
{
    if (chroma != MI_CHROMA_INTERLEAVED && chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const Yuv420BgraFramesShape sh{width, height, y_pitch, c_pitch, out_pitch, order, chroma == MI_CHROMA_PLANAR};
    bool work = false;
    const mi_status st = check_yuv420_bgra_frames(c, frames, n_frames, sh, op != 0, tiles_x, tiles_y, &work);
    return (st || !work) ? st : yuv420_bgra_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_to_bgra_frames_dev(mi_ctx* c, const mi_yuv420_bgr_frame_dev* frames, int n_frames, int width, int height,
                                                     size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_bgra_frames_entry(c, frames, n_frames, width, height, y_pitch, c_pitch, chroma, out_pitch, order, 0, 0.0, 0, 0, stream);
}

mi_status mi_clahe_yuv420_to_bgra_frames_dev(mi_ctx* c, const mi_yuv420_bgr_frame_dev* frames, int n_frames, int width, int height,
                                             size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order,
                                             double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_bgra_frames_entry(c, frames, n_frames, width, height, y_pitch, c_pitch, chroma, out_pitch, order, 1, clip_limit, tiles_x,
                                    tiles_y, stream);
}

}  // extern "C"
