// yuv420_bgra.inc.hpp -- 4:2:0 frames described by mi_yuv420_planes (I420 / YV12, or NV12) in, interleaved 8-bit four-channel images
// (BGRA / RGBA: CV_8UC4, A = 255) out in the pass that maps the luma: checks, the job builder, the two launchers, the two launch
// sequences, the host form, extern "C"
// Included by ../mi_lumaeq.hip behind bgra_yuv420_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// decoder (NV12 surfaces, or a software decoder's three planes) -> equalize -> display surface / swap-chain image / interop texture /
// GUI image in one pass, without a three-channel image in scratch and a widen to four channels outside the library.  The structure is
// yuv420_bgr.inc.hpp's, but BOTH chroma layouts are this form's own kernels (kernels/yuv420_bgra.hip.h): an INTERLEAVED input is not
// handed to the NV12 form and counts like a planar one.  The histogram stages are the planar forms' on the Y planes, then the
// pixel-writing kernel.  Never the fused kernel and never hist_lut_kernel.  CLAHE shapes the one-pass interpolation kernel does not
// take run the planar CLAHE into scratch Y planes and then the decode alone: the same bytes in one more pass.

namespace {

struct Yuv420BgraArgs {
    const uint8_t* y; size_t y_pitch;
    const uint8_t* c0; const uint8_t* c1; size_t c_pitch;   // planar: the U and the V plane; interleaved: c0 = the UV plane, c1 unused (null)
    size_t in_frame;
    uint8_t* out; size_t out_pitch, out_frame;
    int width, height, n_frames, order;
    bool planar;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  `a` has been filled from a non-null
// descriptor whose chroma is one of the two values (c1 = null on an interleaved one).  The rules and their order are
// check_yuv420_bgr's, with a row of 4*W bytes.
mi_status check_yuv420_bgra(mi_ctx* c, const Yuv420BgraArgs& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.y || !a.c0 || !a.out || (a.planar && !a.c1)) return fail(c, MI_ERR_BAD_ARG, "null plane pointer");
    if (a.y_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (a.c_pitch < (a.planar ? (size_t)a.width / 2 : (size_t)a.width))
        return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width interleaved, width / 2 planar)");
    if (a.out_pitch < 4 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "out_pitch < 4 * width");
    if (a.out == a.y || a.out == a.c0 || (a.planar && a.out == a.c1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 in, BGRA out has no in-place form");
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    *work = true;
    return MI_OK;
}

// THE rule of the header for a call without its W % 16 == 0 term: the Y and output terms multiples of 16, the chroma terms of 16 for
// interleaved chroma (one 16-byte UV load) and of 8 for planar chroma (an 8-byte U and an 8-byte V load; in_frame steps the chroma
// planes too, 16 covers them)
bool yuv420_bgra_aligned(const Yuv420BgraArgs& a)
{
    const uintptr_t chroma = a.planar ? (((uintptr_t)a.c0 | (uintptr_t)a.c1 | a.c_pitch) & 7) : (((uintptr_t)a.c0 | a.c_pitch) & 15);
    return (((uintptr_t)a.y | (uintptr_t)a.out | a.y_pitch | a.out_pitch | a.in_frame | a.out_frame) & 15) == 0 && chroma == 0;
}

// the job of frames f0.. of the call; y / y_pitch / y_frame say where the luma comes from (the caller's planes, or scratch)
Yuv420BgraJob yuv420_bgra_job(const Yuv420BgraArgs& a, int f0, const uint8_t* y, size_t y_pitch, size_t y_frame)
{
    Yuv420BgraJob j{};
    j.y = y; j.c0 = a.c0 + (size_t)f0 * a.in_frame; j.c1 = a.planar ? a.c1 + (size_t)f0 * a.in_frame : nullptr;
    j.out = a.out + (size_t)f0 * a.out_frame;
    j.y_step = (long long)y_pitch; j.c_step = (long long)a.c_pitch; j.out_step = (long long)a.out_pitch;
    j.y_frame = (long long)y_frame; j.c_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = a.width % 16 == 0 && yuv420_bgra_aligned(a) && (((uintptr_t)y | y_pitch | y_frame) & 15) == 0;
    return j;
}

// LUT apply + decode (luts != nullptr, MI_K_LUT_APPLY) or the decode alone (MI_K_COLOR).  The grid is launch_yuv420_to_bgr's rule on
// this form's own byte basis: half of what the launch moves, (1 + 0.5 + 4) / 2 = 11/4 bytes per pixel, where the three-channel form
// takes 9/4; the same cap of 2048, and never more workgroups than there are items for (16 x 2 groups: a workgroup pass covers 8192
// pixels; 2 x 2 blocks: 1024).  `fl`: a chunk of a frame list (at most kFramesPerLaunch frames, yuv420_bgra_frames.inc.hpp): the same
// grid on the *_frames_kernel entry; `j` then carries the shape, and j.vec what the shape allows.
mi_status launch_yuv420_to_bgra(mi_ctx* c, hipStream_t s, const Yuv420BgraJob& j, int nf, int order, bool planar, const uint8_t* luts,
                                const Yuv420BgraList* fl = nullptr)
{
    const long long px = (long long)j.width * j.height;
    int B = blocks_per_frame(c, px * 11 / 4, j.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    const dim3 grid(B, nf), block(kThreads);
    const bool rgb = order == MI_ORDER_RGB;
#define MI_YUV420_BGRA_LAUNCH(O, C)                                                                                          \
    do {                                                                                                                     \
        if (fl && luts) LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_bgra_frames_kernel<O, C, true>), grid, block, 0, *fl, j, luts); \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (yuv420_to_bgra_frames_kernel<O, C, false>), grid, block, 0, *fl, j, luts);    \
        else if (luts)  LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_bgra_kernel<O, C, true>), grid, block, 0, j, luts);             \
        else            LAUNCH(c, s, MI_K_COLOR, (yuv420_to_bgra_kernel<O, C, false>), grid, block, 0, j, luts);                \
    } while (0)
    if (planar) { if (rgb) MI_YUV420_BGRA_LAUNCH(1, 1); else MI_YUV420_BGRA_LAUNCH(0, 1); }
    else        { if (rgb) MI_YUV420_BGRA_LAUNCH(1, 0); else MI_YUV420_BGRA_LAUNCH(0, 0); }
#undef MI_YUV420_BGRA_LAUNCH
    return MI_OK;
}

// CLAHE blend + decode of nf frames whose tile LUTs are in `luts`: the geometry of launch_yuv420_bgr_interp.  `fl`: as for
// launch_yuv420_to_bgra.
mi_status launch_yuv420_bgra_interp(mi_ctx* c, hipStream_t s, const Yuv420BgraJob& j, const ClaheGeom& g, int nf, int order, bool planar,
                                    const uint8_t* luts, const Yuv420BgraList* fl = nullptr)
{
    const int ngroups = j.width / kInterpPx;
    const int groups = std::min(ngroups, kThreads);
    const int segs = (ngroups + groups - 1) / groups;
    const int bands = g.tiles_y + 1;
    const long long want = ((long long)c->cu_count * 8 + (long long)bands * nf * segs - 1) / ((long long)bands * nf * segs);
    const int subs = (int)std::max<long long>(1, std::min<long long>({want, (long long)std::max(1, (g.tile_h + 2 * kBandMargin) / 8), 64LL}));
    const dim3 grid(bands * subs, nf, segs);
    const size_t lds = (size_t)(g.tiles_x + 1) * 256 * 4 * sizeof(float);
    const bool rgb = order == MI_ORDER_RGB;
#define MI_YUV420_BGRA_INTERP(O, C)                                                                                                          \
    do {                                                                                                                                     \
        if (fl) LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_bgra_clahe_interp_frames_kernel<O, C>), grid, dim3(kThreads), lds, *fl, j, g, luts, subs, groups); \
        else    LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_bgra_clahe_interp_kernel<O, C>), grid, dim3(kThreads), lds, j, g, luts, subs, groups);  \
    } while (0)
    if (planar) { if (rgb) MI_YUV420_BGRA_INTERP(1, 1); else MI_YUV420_BGRA_INTERP(0, 1); }
    else        { if (rgb) MI_YUV420_BGRA_INTERP(1, 0); else MI_YUV420_BGRA_INTERP(0, 0); }
#undef MI_YUV420_BGRA_INTERP
    return MI_OK;
}

PlaneArgs yuv420_bgra_y_plane(const Yuv420BgraArgs& a)
{
    return PlaneArgs{a.y, a.y_pitch, a.in_frame, nullptr, 0, 0, a.width, a.height, a.n_frames};
}

// one count per call, by the walk its pixel-writing kernel took
void yuv420_bgra_count(mi_ctx* c, bool onepass, bool vec)
{
    ++(onepass ? c->yuv420_bgra_onepass : c->yuv420_bgra_twopass);
    ++(vec ? c->yuv420_bgra_vec : c->yuv420_bgra_bytes);
}

// Per chunk: MI_K_HIST, MI_K_EQ_LUT, then one MI_K_LUT_APPLY launch that maps and decodes
mi_status equalize_yuv420_bgra_dev(mi_ctx* c, hipStream_t s, const Yuv420BgraArgs& a)
{
    const PlaneArgs ya = yuv420_bgra_y_plane(a);
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_hist_partials(c, s, ya, f0, nf, &nparts);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        const Yuv420BgraJob j = yuv420_bgra_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
        if ((st = launch_yuv420_to_bgra(c, s, j, nf, a.order, a.planar, c->d_luts))) return st;
        vec = j.vec != 0;
    }
    yuv420_bgra_count(c, true, vec);
    return MI_OK;
}

// One pass (tile LUTs, then blend + decode) when the shape is the one-pass shape and the alignment rule holds; otherwise the planar
// CLAHE into scratch and the decode alone
mi_status clahe_yuv420_bgra_dev(mi_ctx* c, hipStream_t s, const Yuv420BgraArgs& a, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g;
    mi_status st = clahe_geometry(c, a.width, a.height, clip_limit, tiles_x, tiles_y, &g);
    if (st) return st;
    const int tiles = tiles_x * tiles_y;
    const bool onepass = nv12_bgr_onepass_shape(g, a.width, a.height, tiles_x, tiles_y) && yuv420_bgra_aligned(a);
    const PlaneArgs ya = yuv420_bgra_y_plane(a);
    if (onepass) {
        for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
            const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, f0, nf, c->d_luts))) return st;
            const Yuv420BgraJob j = yuv420_bgra_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
            if ((st = launch_yuv420_bgra_interp(c, s, j, g, nf, a.order, a.planar, c->d_luts))) return st;
        }
        yuv420_bgra_count(c, true, true);       // the one-pass kernel has the 16-pixel walk only
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
        const Yuv420BgraJob j = yuv420_bgra_job(a, f0, c->d_planes, (size_t)a.width, plane);
        if ((st = launch_yuv420_to_bgra(c, s, j, nf, a.order, a.planar, nullptr))) return st;
        vec = j.vec != 0;
    }
    yuv420_bgra_count(c, false, vec);
    return MI_OK;
}

mi_status yuv420_bgra_dev(mi_ctx* c, hipStream_t s, const Yuv420BgraArgs& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    return is_clahe ? clahe_yuv420_bgra_dev(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_yuv420_bgra_dev(c, s, a);
}

// One host frame up plane by plane as yuv420_bgr_host stages it (yuv420_plane_in: pinned tight planes are DMA'd as they are,
// everything else goes through the context's pinned staging), one CV_8UC4 image back through stage_out at a row of 4*W bytes.  On the
// device the frame is tight with every plane at a 16-byte aligned offset, so a W % 16 == 0 frame takes the 16 x 2 groups whatever the
// caller's addresses are.  `h` holds the caller's pointers and pitches; it has passed the checks.
mi_status yuv420_bgra_host(mi_ctx* c, const Yuv420BgraArgs& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if ((long long)h.width * h.height > 0x7fffffffLL / 4) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    const size_t w = (size_t)h.width, rows = (size_t)h.height, ysz = w * rows, csz = ysz / 4;
    const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o0 = up16(ysz), o1 = up16(o0 + csz);                      // planar: U at o0, V at o1; interleaved: UV at o0
    const size_t frame = up16(h.planar ? o1 + csz : o0 + 2 * csz);
    const size_t row = 4 * w, out_bytes = row * rows;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = grow_dev(c, &c->d_stage_in, &c->stage_in_bytes, frame))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    if ((st = grow_pinned(c, &c->h_pin_in, &c->pin_in_bytes, frame))) return st;
    uint8_t* const di = c->d_stage_in;
    if ((st = yuv420_plane_in(c, s, h.y, h.y_pitch, w, rows, di, c->h_pin_in, drain))) return st;
    if (h.planar) {
        if ((st = yuv420_plane_in(c, s, h.c0, h.c_pitch, w / 2, rows / 2, di + o0, c->h_pin_in + o0, drain))) return st;
        if ((st = yuv420_plane_in(c, s, h.c1, h.c_pitch, w / 2, rows / 2, di + o1, c->h_pin_in + o1, drain))) return st;
    } else {
        if ((st = yuv420_plane_in(c, s, h.c0, h.c_pitch, w, rows / 2, di + o0, c->h_pin_in + o0, drain))) return st;
    }
    const Yuv420BgraArgs d{di, w, di + o0, h.planar ? di + o1 : nullptr, h.planar ? w / 2 : w, frame, c->d_stage_out, row, up16(out_bytes),
                           h.width, h.height, 1, h.order, h.planar};
    if ((st = yuv420_bgra_dev(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, row, rows, drain);
}

mi_status yuv420_bgra_entry(mi_ctx* c, const mi_yuv420_planes* in, void* out, size_t out_pitch, size_t out_frame, int width, int height,
                            int n_frames, int order, bool host, bool is_clahe, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    if (!in) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (in->chroma != MI_CHROMA_INTERLEAVED && in->chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const bool planar = in->chroma == MI_CHROMA_PLANAR;
    const Yuv420BgraArgs a{(const uint8_t*)in->y, in->y_pitch, (const uint8_t*)in->c0, planar ? (const uint8_t*)in->c1 : nullptr, in->c_pitch,
                           host ? 0 : in->frame_stride, (uint8_t*)out, out_pitch, host ? 0 : out_frame, width, height, n_frames, order, planar};
    bool work = false;
    const mi_status st = check_yuv420_bgra(c, a, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? yuv420_bgra_host(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : yuv420_bgra_dev(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_to_bgra_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
                                                    size_t out_frame_stride, int width, int height, int n_frames, int order, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_bgra_entry(c, in, d_out, out_pitch, out_frame_stride, width, height, n_frames, order, false, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_yuv420_to_bgra_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
                                            size_t out_frame_stride, int width, int height, int n_frames, int order,
                                            double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_bgra_entry(c, in, d_out, out_pitch, out_frame_stride, width, height, n_frames, order, false, true, clip_limit, tiles_x,
                             tiles_y, stream);
}

mi_status mi_equalize_hist_yuv420_to_bgra(mi_ctx* c, const mi_yuv420_planes* in, uint8_t* out, size_t out_step, int width, int height,
                                          int order)
{
    ENTER_COMPUTE(c);
    return yuv420_bgra_entry(c, in, out, out_step, 0, width, height, 1, order, true, false, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_yuv420_to_bgra(mi_ctx* c, const mi_yuv420_planes* in, uint8_t* out, size_t out_step, int width, int height, int order,
                                  double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return yuv420_bgra_entry(c, in, out, out_step, 0, width, height, 1, order, true, true, clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
