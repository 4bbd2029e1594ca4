// yuv420_bgr.inc.hpp -- 4:2:0 frames described by mi_yuv420_planes (I420 / YV12, or NV12) in, interleaved 8-bit BGR / RGB out in the pass
// that maps the luma: checks, the interleaved hand-over, the planar launch sequences, the host form, extern "C"
// Included by ../mi_lumaeq.hip behind yuv420_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// software decoder (three planes) -> equalize -> display / image writer / model without an interleave of U and V and without an NV12
// intermediate.  An INTERLEAVED input is the NV12 form's own: equalize_nv12_bgr_dev / clahe_nv12_bgr_dev (nv12_bgr.inc.hpp) with their
// kernels and their counters.  A PLANAR input runs the same two sequences -- the planar forms' histogram stages on the Y planes, then
// the pixel-writing kernel -- on the kernels of kernels/yuv420_bgr.hip.h, which load the chroma from two planes.  Never the fused
// kernel and never hist_lut_kernel.  CLAHE shapes the one-pass interpolation kernel does not take run the planar CLAHE into scratch Y
// planes and then the decode alone: the same bytes in one more pass.

namespace {

struct Yuv420BgrArgs {
    const uint8_t* y; size_t y_pitch;
    const uint8_t* u; const uint8_t* v; size_t c_pitch;     // planar: U and V planes; interleaved: u = the UV plane, v unused
    size_t in_frame;
    uint8_t* out; size_t out_pitch, out_frame;
    int width, height, n_frames, order;
    bool planar;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  `a` has been filled from a non-null
// descriptor whose chroma is one of the two values.
mi_status check_yuv420_bgr(mi_ctx* c, const Yuv420BgrArgs& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.y || !a.u || !a.out || (a.planar && !a.v)) return fail(c, MI_ERR_BAD_ARG, "null plane pointer");
    if (a.y_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (a.c_pitch < (a.planar ? (size_t)a.width / 2 : (size_t)a.width))
        return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width interleaved, width / 2 planar)");
    if (a.out_pitch < 3 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "out_pitch < 3 * width");
    if (a.out == a.y || a.out == a.u || (a.planar && a.out == a.v)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 in, BGR out has no in-place form");
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    *work = true;
    return MI_OK;
}

Nv12BgrArgs yuv420_bgr_as_nv12(const Yuv420BgrArgs& a)
{
    return Nv12BgrArgs{a.y, a.y_pitch, a.u, a.c_pitch, a.in_frame, a.out, a.out_pitch, a.out_frame, a.width, a.height, a.n_frames, a.order};
}

// the rule of the 16 x 2 pixel groups without its W % 16 == 0 term: the Y and output terms multiples of 16, the chroma terms of 8 (a
// lane loads 8 bytes from each chroma plane; in_frame steps the chroma planes too, 16 covers them)
bool yuv420_bgr_aligned(const Yuv420BgrArgs& a)
{
    return (((uintptr_t)a.y | (uintptr_t)a.out | a.y_pitch | a.out_pitch | a.in_frame | a.out_frame) & 15) == 0 &&
           (((uintptr_t)a.u | (uintptr_t)a.v | a.c_pitch) & 7) == 0;
}

// the job of frames f0.. of the call; y / y_pitch / y_frame say where the luma comes from (the caller's planes, or scratch)
Yuv420BgrJob yuv420_bgr_job(const Yuv420BgrArgs& a, int f0, const uint8_t* y, size_t y_pitch, size_t y_frame)
{
    Yuv420BgrJob j{};
    j.y = y; j.u = a.u + (size_t)f0 * a.in_frame; j.v = a.v + (size_t)f0 * a.in_frame; j.out = a.out + (size_t)f0 * a.out_frame;
    j.y_step = (long long)y_pitch; j.c_step = (long long)a.c_pitch; j.out_step = (long long)a.out_pitch;
    j.y_frame = (long long)y_frame; j.c_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = a.width % 16 == 0 && yuv420_bgr_aligned(a) && (((uintptr_t)y | y_pitch | y_frame) & 15) == 0;
    return j;
}

// LUT apply + decode (luts != nullptr, MI_K_LUT_APPLY) or the decode alone (MI_K_COLOR): the grid of launch_nv12_to_bgr.  `fl`: a
// chunk of a frame list (at most kFramesPerLaunch frames, yuv420_bgr_frames.inc.hpp): the same grid on the *_frames_kernel entry; `j`
// then carries the shape, and j.vec what the shape allows.
mi_status launch_yuv420_to_bgr(mi_ctx* c, hipStream_t s, const Yuv420BgrJob& j, int nf, int order, const uint8_t* luts,
                               const Yuv420BgrList* fl = nullptr)
{
    const long long px = (long long)j.width * j.height;
    int B = blocks_per_frame(c, px * 9 / 4, j.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    const dim3 grid(B, nf), block(kThreads);
    if (fl && luts) {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_bgr_frames_kernel<1, true>), grid, block, 0, *fl, j, luts);
        else                       LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_bgr_frames_kernel<0, true>), grid, block, 0, *fl, j, luts);
    } else if (fl) {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_COLOR, (yuv420_to_bgr_frames_kernel<1, false>), grid, block, 0, *fl, j, luts);
        else                       LAUNCH(c, s, MI_K_COLOR, (yuv420_to_bgr_frames_kernel<0, false>), grid, block, 0, *fl, j, luts);
    } else if (luts) {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_bgr_kernel<1, true>), grid, block, 0, j, luts);
        else                       LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_bgr_kernel<0, true>), grid, block, 0, j, luts);
    } else {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_COLOR, (yuv420_to_bgr_kernel<1, false>), grid, block, 0, j, luts);
        else                       LAUNCH(c, s, MI_K_COLOR, (yuv420_to_bgr_kernel<0, false>), grid, block, 0, j, luts);
    }
    return MI_OK;
}

// CLAHE blend + decode of nf frames whose tile LUTs are in `luts`: the grid of launch_nv12_bgr_interp.  `fl`: as for
// launch_yuv420_to_bgr.
mi_status launch_yuv420_bgr_interp(mi_ctx* c, hipStream_t s, const Yuv420BgrJob& j, const ClaheGeom& g, int nf, int order, const uint8_t* luts,
                                   const Yuv420BgrList* fl = nullptr)
{
    const int ngroups = j.width / kInterpPx;
    const int groups = std::min(ngroups, kThreads);
    const int segs = (ngroups + groups - 1) / groups;
    const int bands = g.tiles_y + 1;
    const long long want = ((long long)c->cu_count * 8 + (long long)bands * nf * segs - 1) / ((long long)bands * nf * segs);
    const int subs = (int)std::max<long long>(1, std::min<long long>({want, (long long)std::max(1, (g.tile_h + 2 * kBandMargin) / 8), 64LL}));
    const dim3 grid(bands * subs, nf, segs);
    const size_t lds = (size_t)(g.tiles_x + 1) * 256 * 4 * sizeof(float);
    if (fl) {
        if (order == MI_ORDER_RGB)
            LAUNCH(c, s, MI_K_CLAHE_INTERP, yuv420_bgr_clahe_interp_frames_kernel<1>, grid, dim3(kThreads), lds, *fl, j, g, luts, subs, groups);
        else
            LAUNCH(c, s, MI_K_CLAHE_INTERP, yuv420_bgr_clahe_interp_frames_kernel<0>, grid, dim3(kThreads), lds, *fl, j, g, luts, subs, groups);
        return MI_OK;
    }
    if (order == MI_ORDER_RGB)
        LAUNCH(c, s, MI_K_CLAHE_INTERP, yuv420_bgr_clahe_interp_kernel<1>, grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    else
        LAUNCH(c, s, MI_K_CLAHE_INTERP, yuv420_bgr_clahe_interp_kernel<0>, grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    return MI_OK;
}

PlaneArgs yuv420_bgr_y_plane(const Yuv420BgrArgs& a)
{
    return PlaneArgs{a.y, a.y_pitch, a.in_frame, nullptr, 0, 0, a.width, a.height, a.n_frames};
}

// one count per call, by the walk its pixel-writing kernel took
void yuv420_bgr_count(mi_ctx* c, bool onepass, bool vec)
{
    ++(onepass ? c->yuv420_bgr_onepass : c->yuv420_bgr_twopass);
    ++(vec ? c->yuv420_bgr_vec : c->yuv420_bgr_bytes);
}

// equalize_nv12_bgr_dev on planar chroma
mi_status equalize_yuv420_bgr_dev(mi_ctx* c, hipStream_t s, const Yuv420BgrArgs& a)
{
    const PlaneArgs ya = yuv420_bgr_y_plane(a);
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_hist_partials(c, s, ya, f0, nf, &nparts);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        const Yuv420BgrJob j = yuv420_bgr_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
        if ((st = launch_yuv420_to_bgr(c, s, j, nf, a.order, c->d_luts))) return st;
        vec = j.vec != 0;
    }
    yuv420_bgr_count(c, true, vec);
    return MI_OK;
}

// clahe_nv12_bgr_dev on planar chroma
mi_status clahe_yuv420_bgr_dev(mi_ctx* c, hipStream_t s, const Yuv420BgrArgs& a, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g;
    mi_status st = clahe_geometry(c, a.width, a.height, clip_limit, tiles_x, tiles_y, &g);
    if (st) return st;
    const int tiles = tiles_x * tiles_y;
    const bool onepass = nv12_bgr_onepass_shape(g, a.width, a.height, tiles_x, tiles_y) && yuv420_bgr_aligned(a);
    const PlaneArgs ya = yuv420_bgr_y_plane(a);
    if (onepass) {
        for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
            const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, f0, nf, c->d_luts))) return st;
            const Yuv420BgrJob j = yuv420_bgr_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
            if ((st = launch_yuv420_bgr_interp(c, s, j, g, nf, a.order, c->d_luts))) return st;
        }
        yuv420_bgr_count(c, true, true);       // the one-pass kernel has the 16-pixel walk only
        return MI_OK;
    }
    // fallback: the planar CLAHE into tight scratch Y planes (each 16-byte aligned), then the decode alone
    const size_t plane = ((size_t)a.width * a.height + 15) & ~(size_t)15;
    const int chunk = std::min(kNv12BgrFramesPerLaunch, a.n_frames);
    if ((st = grow_dev(c, &c->d_planes, &c->planes_bytes, plane * (size_t)chunk))) return st;
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        const PlaneArgs pa{a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame, c->d_planes, (size_t)a.width, plane, a.width, a.height, nf};
        if ((st = clahe_dev(c, s, pa, clip_limit, tiles_x, tiles_y, nullptr))) return st;
        const Yuv420BgrJob j = yuv420_bgr_job(a, f0, c->d_planes, (size_t)a.width, plane);
        if ((st = launch_yuv420_to_bgr(c, s, j, nf, a.order, nullptr))) return st;
        vec = j.vec != 0;
    }
    yuv420_bgr_count(c, false, vec);
    return MI_OK;
}

mi_status yuv420_bgr_dev(mi_ctx* c, hipStream_t s, const Yuv420BgrArgs& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if (!a.planar) {                                    // the NV12 form's own path: its kernels, its counters
        const Nv12BgrArgs n = yuv420_bgr_as_nv12(a);
        return is_clahe ? clahe_nv12_bgr_dev(c, s, n, clip_limit, tiles_x, tiles_y) : equalize_nv12_bgr_dev(c, s, n);
    }
    return is_clahe ? clahe_yuv420_bgr_dev(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_yuv420_bgr_dev(c, s, a);
}

// One host frame up plane by plane (yuv420_plane_in: pinned tight planes are DMA'd as they are, everything else goes through the
// context's pinned staging), one CV_8UC3 image back as nv12_bgr_host returns it.  On the device the frame is tight with every plane at
// a 16-byte aligned offset, so a W % 16 == 0 frame takes the 16 x 2 groups whatever the caller's addresses are.  `h` holds the
// caller's pointers and pitches; it has passed the checks.
mi_status yuv420_bgr_host(mi_ctx* c, const Yuv420BgrArgs& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if ((long long)h.width * h.height > 0x7fffffffLL / 3) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    const size_t w = (size_t)h.width, rows = (size_t)h.height, ysz = w * rows, csz = ysz / 4;
    const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o0 = up16(ysz), o1 = up16(o0 + csz);                      // planar: U at o0, V at o1; interleaved: UV at o0
    const size_t frame = up16(h.planar ? o1 + csz : o0 + 2 * csz);
    const size_t row = 3 * w, out_bytes = row * rows;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = grow_dev(c, &c->d_stage_in, &c->stage_in_bytes, frame))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    if ((st = grow_pinned(c, &c->h_pin_in, &c->pin_in_bytes, frame))) return st;
    uint8_t* const di = c->d_stage_in;
    if ((st = yuv420_plane_in(c, s, h.y, h.y_pitch, w, rows, di, c->h_pin_in, drain))) return st;
    if (h.planar) {
        if ((st = yuv420_plane_in(c, s, h.u, h.c_pitch, w / 2, rows / 2, di + o0, c->h_pin_in + o0, drain))) return st;
        if ((st = yuv420_plane_in(c, s, h.v, h.c_pitch, w / 2, rows / 2, di + o1, c->h_pin_in + o1, drain))) return st;
    } else {
        if ((st = yuv420_plane_in(c, s, h.u, h.c_pitch, w, rows / 2, di + o0, c->h_pin_in + o0, drain))) return st;
    }
    const Yuv420BgrArgs d{di, w, di + o0, h.planar ? di + o1 : nullptr, h.planar ? w / 2 : w, frame, c->d_stage_out, row, up16(out_bytes),
                          h.width, h.height, 1, h.order, h.planar};
    if ((st = yuv420_bgr_dev(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, row, rows, drain);
}

mi_status yuv420_bgr_entry(mi_ctx* c, const mi_yuv420_planes* in, void* out, size_t out_pitch, size_t out_frame, int width, int height,
                           int n_frames, int order, bool host, bool is_clahe, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    if (!in) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (in->chroma != MI_CHROMA_INTERLEAVED && in->chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const bool planar = in->chroma == MI_CHROMA_PLANAR;
    const Yuv420BgrArgs a{(const uint8_t*)in->y, in->y_pitch, (const uint8_t*)in->c0, planar ? (const uint8_t*)in->c1 : nullptr, in->c_pitch,
                          host ? 0 : in->frame_stride, (uint8_t*)out, out_pitch, out_frame, width, height, n_frames, order, planar};
    bool work = false;
    const mi_status st = check_yuv420_bgr(c, a, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? yuv420_bgr_host(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : yuv420_bgr_dev(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_to_bgr_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
                                                   size_t out_frame_stride, int width, int height, int n_frames, int order, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_bgr_entry(c, in, d_out, out_pitch, out_frame_stride, width, height, n_frames, order, false, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_yuv420_to_bgr_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
                                           size_t out_frame_stride, int width, int height, int n_frames, int order,
                                           double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_bgr_entry(c, in, d_out, out_pitch, out_frame_stride, width, height, n_frames, order, false, true, clip_limit, tiles_x,
                            tiles_y, stream);
}

mi_status mi_equalize_hist_yuv420_to_bgr(mi_ctx* c, const mi_yuv420_planes* in, uint8_t* out, size_t out_step, int width, int height,
                                         int order)
{
    ENTER_COMPUTE(c);
    return yuv420_bgr_entry(c, in, out, out_step, 0, width, height, 1, order, true, false, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_yuv420_to_bgr(mi_ctx* c, const mi_yuv420_planes* in, uint8_t* out, size_t out_step, int width, int height, int order,
                                 double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return yuv420_bgr_entry(c, in, out, out_step, 0, width, height, 1, order, true, true, clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
