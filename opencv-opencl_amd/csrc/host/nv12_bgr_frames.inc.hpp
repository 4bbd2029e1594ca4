// nv12_bgr_frames.inc.hpp -- NV12 in, interleaved BGR / RGB out on frames given as a list of addresses (mi_*_nv12_to_bgr_frames_dev):
// checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip after nv12_bgr.inc.hpp (one translation unit; not a stand-alone header).
//
// A hardware decoder hands out a surface pool: every frame its own allocation with a pitched Y and a pitched UV plane, and the images
// go to a pool of their own.  The call is cut into chunks of kFramesPerLaunch frames.  A chunk's Y planes travel to the histogram
// stages as a FrameList (the planar launchers, as nv12_frames.inc.hpp uses them: same scratch, same grids), its {y, uv, out} triples
// to the pixel-writing stage as an Nv12BgrList, both by value in the kernel arguments, through the launchers of nv12_bgr.inc.hpp --
// same grids, same bands and segments, same bytes as the batch form.
// equalizeHist maps and decodes in one kernel whatever the addresses are: each frame takes the 16 x 2 groups or the 2 x 2 blocks by
// its own alignment.  The CLAHE blend + decode kernel has no byte path, so CLAHE is one-pass only when the shape is the batch form's
// one-pass shape AND every address of every frame of the call is a multiple of 16; otherwise the whole call runs the planar CLAHE
// (clahe_dev on the list) into the context's scratch planes and the decode alone from there, chunk by chunk.

namespace {

struct Nv12BgrFramesShape {
    int width, height;
    size_t y_pitch, uv_pitch, out_pitch;
    int order;
};

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_nv12_bgr_frames(mi_ctx* c, const mi_nv12_bgr_frame_dev* frames, int n_frames, const Nv12BgrFramesShape& s,
                                bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_nv12_bgr's own answers (order, sizes, even width and height, tiles, pitches, the planar forms' limits), on
    // stand-in addresses that pass its pointer checks
    const Nv12BgrArgs shape{(const uint8_t*)16, s.y_pitch, (const uint8_t*)32, s.uv_pitch, 0, (uint8_t*)48, s.out_pitch, 0,
                            s.width, s.height, n_frames, s.order};
    bool any = false;
    const mi_status st = check_nv12_bgr(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_nv12_bgr_frame_dev& f = frames[k];
        if (!f.y || !f.uv || !f.out) return fail(c, MI_ERR_BAD_ARG, "null plane pointer");
        // there is no in-place form (1 or 1/2 byte per pixel in, 3 out): the image's rows may meet neither plane of its own frame
        const Span so(f.out, s.out_pitch, 3 * w, rows), sy(f.y, s.y_pitch, w, rows), su(f.uv, s.uv_pitch, w, rows / 2);
        if (so.meets(sy) || so.meets(su))
            return fail(c, MI_ERR_BAD_ARG, "NV12 in, BGR out has no in-place form: an image overlaps a plane of its own frame");
    }
    *work = true;
    return MI_OK;
}

// what the shape allows (Nv12BgrJob::vec of a table launch); the kernel adds each frame's own addresses
bool nv12_bgr_frames_shape16(const Nv12BgrFramesShape& s)
{
    return s.width % 16 == 0 && ((s.y_pitch | s.uv_pitch | s.out_pitch) & 15) == 0;
}

// the shape of a table launch; y_pitch: the caller's, or that of the scratch planes
Nv12BgrJob nv12_bgr_frames_job(const Nv12BgrFramesShape& s, size_t y_pitch)
{
    Nv12BgrJob j{};
    j.y_step = (long long)y_pitch; j.uv_step = (long long)s.uv_pitch; j.out_step = (long long)s.out_pitch;
    j.width = s.width; j.height = s.height;
    j.vec = nv12_bgr_frames_shape16(s) && (y_pitch & 15) == 0;
    return j;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status nv12_bgr_frames_dev(mi_ctx* c, hipStream_t s, const mi_nv12_bgr_frame_dev* frames, int n_frames, const Nv12BgrFramesShape& sh,
                              int op, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g{};
    mi_status st;
    bool onepass = true;
    const size_t plane = ((size_t)sh.width * sh.height + 15) & ~(size_t)15;      // a tight scratch Y plane, 16-byte aligned
    if (op) {
        if ((st = clahe_geometry(c, sh.width, sh.height, clip_limit, tiles_x, tiles_y, &g))) return st;
        uintptr_t bits = 0;
        for (int k = 0; k < n_frames; ++k) bits |= (uintptr_t)frames[k].y | (uintptr_t)frames[k].uv | (uintptr_t)frames[k].out;
        onepass = nv12_bgr_onepass_shape(g, sh.width, sh.height, tiles_x, tiles_y) && nv12_bgr_frames_shape16(sh) && (bits & 15) == 0;
        if (!onepass && (st = grow_dev(c, &c->d_planes, &c->planes_bytes, plane * (size_t)std::min(kFramesPerLaunch, n_frames)))) return st;
    }
    const int tiles = tiles_x * tiles_y;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        FrameList in{};                                              // this chunk's Y planes for the planar stages (uv.rows = 0: no UV work)
        Nv12BgrList io{};                                            // the three addresses of a frame for the stage that writes pixels
        for (int k = 0; k < nf; ++k) {
            const mi_nv12_bgr_frame_dev& f = frames[f0 + k];
            uint8_t* y_out = onepass ? nullptr : c->d_planes + (size_t)k * plane;
            in.f[k] = FramePlanes{(const uint8_t*)f.y, nullptr, y_out, nullptr};
            io.f[k] = Nv12BgrFrame{onepass ? (const uint8_t*)f.y : y_out, (const uint8_t*)f.uv, (uint8_t*)f.out};
        }
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{in.f[0].y_in, sh.y_pitch, 0, in.f[0].y_out, onepass ? 0 : (size_t)sh.width, 0, sh.width, sh.height, nf};
        if (!op) {
            int nparts = 0;
            if ((st = launch_hist_partials(c, s, ya, 0, nf, &nparts, &in))) return st;
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
            LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
                   (const uint32_t*)c->d_partial, nparts, (int)((long long)sh.width * sh.height), c->d_luts, (int32_t*)nullptr);
            if ((st = launch_nv12_to_bgr(c, s, nv12_bgr_frames_job(sh, sh.y_pitch), nf, sh.order, c->d_luts, &io))) return st;
        } else if (onepass) {
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, 0, nf, c->d_luts, &in))) return st;
            if ((st = launch_nv12_bgr_interp(c, s, nv12_bgr_frames_job(sh, sh.y_pitch), g, nf, sh.order, c->d_luts, &io))) return st;
        } else {
            if ((st = clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &in))) return st;
            if ((st = launch_nv12_to_bgr(c, s, nv12_bgr_frames_job(sh, (size_t)sh.width), nf, sh.order, nullptr, &io))) return st;
        }
    }
    ++(onepass ? c->nv12_bgr_onepass : c->nv12_bgr_twopass);
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_nv12_to_bgr_frames_dev(mi_ctx* c, const mi_nv12_bgr_frame_dev* frames, int n_frames, int width, int height,
                                                  size_t y_pitch, size_t uv_pitch, size_t out_pitch, int order, void* stream)
{
    ENTER_COMPUTE(c);
    const Nv12BgrFramesShape sh{width, height, y_pitch, uv_pitch, out_pitch, order};
    bool work = false;
    const mi_status st = check_nv12_bgr_frames(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : nv12_bgr_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_nv12_to_bgr_frames_dev(mi_ctx* c, const mi_nv12_bgr_frame_dev* frames, int n_frames, int width, int height,
                                          size_t y_pitch, size_t uv_pitch, size_t out_pitch, int order,
                                          double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const Nv12BgrFramesShape sh{width, height, y_pitch, uv_pitch, out_pitch, order};
    bool work = false;
    const mi_status st = check_nv12_bgr_frames(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : nv12_bgr_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
