// yuv420_packed422.inc.hpp -- 4:2:0 frames described by mi_yuv420_planes (NV12, or I420 / YV12) in, pitched packed 4:2:2 frames (YUY2 /
// UYVY) out in the pass that maps the luma: checks, launch sequences, the host form, extern "C"
// Included by ../mi_lumaeq.hip behind bgr_packed422_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// hardware decoder (NV12) or software decoder (three planes) -> equalize -> playout card, v4l2 output or loopback device, virtual
// camera, without an NV12 intermediate and a scatter of Y and row-repeated UV outside the library.  The order of yuv420_bgr.inc.hpp:
// the planar forms' histogram stages on the Y planes, then the pixel-writing kernel of kernels/yuv420_packed422.hip.h, which has
// both chroma layouts as a template parameter -- there is no hand-over to another form, and one pair of counters serves both.  Never
// the fused kernel and never hist_lut_kernel: option two_kernel_max_frames does not apply.  CLAHE shapes the one-pass interpolation
// kernel does not take run the planar CLAHE into scratch Y planes and then the pack alone: the same bytes in one more pass.

namespace {

struct Yuv420P422Args {
    const uint8_t* y; size_t y_pitch;
    const uint8_t* c0; const uint8_t* c1; size_t c_pitch;   // planar: U and V planes; interleaved: c0 = the UV plane, c1 = nullptr.  MI_UV_FILL128: both nullptr, c_pitch 0
    size_t in_frame;
    uint8_t* out; size_t out_pitch, out_frame;
    int width, height, n_frames, format;
    mi_uv_mode uv_mode;
    bool planar;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  host: the output is host memory the
// kernels never see -- any address and pitch.  `a` has been filled from a non-null descriptor whose chroma is one of the two values;
// under MI_UV_FILL128 its chroma fields have been cleared (they are not read).
mi_status check_yuv420_packed422(mi_ctx* c, const Yuv420P422Args& a, bool host, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    const bool copy = a.uv_mode == MI_UV_COPY;
    if (a.format != MI_FMT_YUY2 && a.format != MI_FMT_UYVY) return fail(c, MI_ERR_BAD_ARG, "format must be MI_FMT_YUY2 or MI_FMT_UYVY");
    if (a.uv_mode != MI_UV_FILL128 && a.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.y || !a.out) return fail(c, MI_ERR_BAD_ARG, "null plane or frame pointer");
    if (copy && (!a.c0 || (a.planar && !a.c1))) return fail(c, MI_ERR_BAD_ARG, "MI_UV_COPY needs the input chroma planes");
    if (a.y_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (copy && a.c_pitch < (a.planar ? (size_t)a.width / 2 : (size_t)a.width))
        return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width interleaved, width / 2 planar)");
    if (a.out_pitch < 2 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "out_pitch < 2 * width");
    if (!host && (((uintptr_t)a.out | a.out_pitch | a.out_frame) & 3))
        return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 pointers, pitches and frame strides are multiples of 4");
    if (a.out == a.y || a.out == a.c0 || a.out == a.c1) return fail(c, MI_ERR_BAD_ARG, "4:2:0 in, packed 4:2:2 out has no in-place form");
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    if (host && (long long)a.width * a.height > 0x7fffffffLL / 2) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    *work = true;
    return MI_OK;
}

// the rule of the 16 x 2 pixel groups without its W % 16 == 0 term: the Y and output terms multiples of 16, the chroma terms of 16
// (interleaved: a lane loads 16 bytes) or of 8 (planar: 8 bytes from each plane; in_frame steps the chroma planes too, 16 covers
// them).  Under MI_UV_FILL128 the chroma terms are zero: they are not read and decide nothing.
bool yuv420_packed422_aligned(const Yuv420P422Args& a)
{
    return (((uintptr_t)a.y | (uintptr_t)a.out | a.y_pitch | a.out_pitch | a.in_frame | a.out_frame) & 15) == 0 &&
           (((uintptr_t)a.c0 | (uintptr_t)a.c1 | a.c_pitch) & (a.planar ? 7 : 15)) == 0;
}

// the job of frames f0.. of the call; y / y_pitch / y_frame say where the luma comes from (the caller's planes, or scratch)
Yuv420P422Job yuv420_packed422_job(const Yuv420P422Args& a, int f0, const uint8_t* y, size_t y_pitch, size_t y_frame)
{
    const bool copy = a.uv_mode == MI_UV_COPY;
    Yuv420P422Job j{};
    j.y = y; j.out = a.out + (size_t)f0 * a.out_frame;
    j.c0 = copy ? a.c0 + (size_t)f0 * a.in_frame : nullptr;
    j.c1 = copy && a.planar ? a.c1 + (size_t)f0 * a.in_frame : nullptr;
    j.y_step = (long long)y_pitch; j.c_step = (long long)a.c_pitch; j.out_step = (long long)a.out_pitch;
    j.y_frame = (long long)y_frame; j.c_frame = copy ? (long long)a.in_frame : 0; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = a.width % 16 == 0 && yuv420_packed422_aligned(a) && (((uintptr_t)y | y_pitch | y_frame) & 15) == 0;
    j.copy_uv = copy;
    return j;
}

// LUT apply + pack (luts != nullptr, MI_K_LUT_APPLY) or the pack alone (MI_K_COLOR).  The grid rule is launch_nv12_to_bgr's on this
// form's bytes: half of what is read and written (1.5 + 2 B/px) as the byte basis, one row unit per pair of rows, the cap 2048; in
// 16 x 2 groups a workgroup pass covers 8192 pixels, in 2 x 2 blocks 1024.  `fl`: a chunk of a frame list (at most kFramesPerLaunch
// frames, yuv420_packed422_frames.inc.hpp): the same grid on the *_frames_kernel entry; `j` then carries the shape, and j.vec what
// the shape allows.
mi_status launch_yuv420_to_packed422(mi_ctx* c, hipStream_t s, const Yuv420P422Job& j, int nf, int format, bool planar, const uint8_t* luts,
                                     const Yuv420P422List* fl = nullptr)
{
    const long long px = (long long)j.width * j.height;
    int B = blocks_per_frame(c, px * 7 / 4, j.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    const dim3 grid(B, nf), block(kThreads);
#define MI_YUV420_P422_LAUNCH(F, P)                                                                                                  \
    do {                                                                                                                             \
        if (fl && luts) LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_packed422_frames_kernel<F, P, true>), grid, block, 0, *fl, j, luts); \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (yuv420_to_packed422_frames_kernel<F, P, false>), grid, block, 0, *fl, j, luts);    \
        else if (luts)  LAUNCH(c, s, MI_K_LUT_APPLY, (yuv420_to_packed422_kernel<F, P, true>), grid, block, 0, j, luts);             \
        else            LAUNCH(c, s, MI_K_COLOR, (yuv420_to_packed422_kernel<F, P, false>), grid, block, 0, j, luts);                \
    } while (0)
    const bool uyvy = format == MI_FMT_UYVY;
    if (uyvy && planar) MI_YUV420_P422_LAUNCH(1, true);
    else if (uyvy)      MI_YUV420_P422_LAUNCH(1, false);
    else if (planar)    MI_YUV420_P422_LAUNCH(0, true);
    else                MI_YUV420_P422_LAUNCH(0, false);
#undef MI_YUV420_P422_LAUNCH
    return MI_OK;
}

// CLAHE blend + pack of nf frames whose tile LUTs are in `luts`: the grid of launch_nv12_bgr_interp.  `fl`: as for
// launch_yuv420_to_packed422.
mi_status launch_yuv420_packed422_interp(mi_ctx* c, hipStream_t s, const Yuv420P422Job& j, const ClaheGeom& g, int nf, int format, bool planar,
                                         const uint8_t* luts, const Yuv420P422List* fl = nullptr)
{
    const int ngroups = j.width / kInterpPx;
    const int groups = std::min(ngroups, kThreads);
    const int segs = (ngroups + groups - 1) / groups;
    const int bands = g.tiles_y + 1;
    const long long want = ((long long)c->cu_count * 8 + (long long)bands * nf * segs - 1) / ((long long)bands * nf * segs);
    const int subs = (int)std::max<long long>(1, std::min<long long>({want, (long long)std::max(1, (g.tile_h + 2 * kBandMargin) / 8), 64LL}));
    const dim3 grid(bands * subs, nf, segs);
    const size_t lds = (size_t)(g.tiles_x + 1) * 256 * 4 * sizeof(float);
    const bool uyvy = format == MI_FMT_UYVY;
#define MI_YUV420_P422_INTERP_FRAMES(F, P)                                                                                           \
    LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_packed422_clahe_interp_frames_kernel<F, P>), grid, dim3(kThreads), lds, *fl, j, g, luts, subs, groups)
    if (fl) {
        if (uyvy && planar) MI_YUV420_P422_INTERP_FRAMES(1, true);
        else if (uyvy)      MI_YUV420_P422_INTERP_FRAMES(1, false);
        else if (planar)    MI_YUV420_P422_INTERP_FRAMES(0, true);
        else                MI_YUV420_P422_INTERP_FRAMES(0, false);
        return MI_OK;
    }
#undef MI_YUV420_P422_INTERP_FRAMES
    if (uyvy && planar) LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_packed422_clahe_interp_kernel<1, true>), grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    else if (uyvy)      LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_packed422_clahe_interp_kernel<1, false>), grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    else if (planar)    LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_packed422_clahe_interp_kernel<0, true>), grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    else                LAUNCH(c, s, MI_K_CLAHE_INTERP, (yuv420_packed422_clahe_interp_kernel<0, false>), grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    return MI_OK;
}

PlaneArgs yuv420_packed422_y_plane(const Yuv420P422Args& a)
{
    return PlaneArgs{a.y, a.y_pitch, a.in_frame, nullptr, 0, 0, a.width, a.height, a.n_frames};
}

// one count of each pair per call, by the passes it ran and by the walk its pixel-writing kernel took
void yuv420_packed422_count(mi_ctx* c, bool onepass, bool vec)
{
    ++(onepass ? c->yuv420_packed422_onepass : c->yuv420_packed422_twopass);
    ++(vec ? c->yuv420_packed422_vec : c->yuv420_packed422_bytes);
}

// per chunk: one MI_K_HIST, one MI_K_EQ_LUT, one MI_K_LUT_APPLY (apply + pack), for either uv_mode
mi_status equalize_yuv420_packed422_dev(mi_ctx* c, hipStream_t s, const Yuv420P422Args& a)
{
    const PlaneArgs ya = yuv420_packed422_y_plane(a);
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_hist_partials(c, s, ya, f0, nf, &nparts);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        const Yuv420P422Job j = yuv420_packed422_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
        if ((st = launch_yuv420_to_packed422(c, s, j, nf, a.format, a.planar, c->d_luts))) return st;
        vec = j.vec != 0;
    }
    yuv420_packed422_count(c, true, vec);
    return MI_OK;
}

mi_status clahe_yuv420_packed422_dev(mi_ctx* c, hipStream_t s, const Yuv420P422Args& a, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g;
    mi_status st = clahe_geometry(c, a.width, a.height, clip_limit, tiles_x, tiles_y, &g);
    if (st) return st;
    const int tiles = tiles_x * tiles_y;
    const bool onepass = nv12_bgr_onepass_shape(g, a.width, a.height, tiles_x, tiles_y) && yuv420_packed422_aligned(a);
    const PlaneArgs ya = yuv420_packed422_y_plane(a);
    if (onepass) {
        for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
            const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, f0, nf, c->d_luts))) return st;
            const Yuv420P422Job j = yuv420_packed422_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
            if ((st = launch_yuv420_packed422_interp(c, s, j, g, nf, a.format, a.planar, c->d_luts))) return st;
        }
        yuv420_packed422_count(c, true, true);       // the one-pass kernel has the 16-pixel walk only
        return MI_OK;
    }
    // fallback: the planar CLAHE into tight scratch Y planes (each 16-byte aligned), then the pack alone
    const size_t plane = ((size_t)a.width * a.height + 15) & ~(size_t)15;
    const int chunk = std::min(kNv12BgrFramesPerLaunch, a.n_frames);
    if ((st = grow_dev(c, &c->d_planes, &c->planes_bytes, plane * (size_t)chunk))) return st;
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        const PlaneArgs pa{a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame, c->d_planes, (size_t)a.width, plane, a.width, a.height, nf};
        if ((st = clahe_dev(c, s, pa, clip_limit, tiles_x, tiles_y, nullptr))) return st;
        const Yuv420P422Job j = yuv420_packed422_job(a, f0, c->d_planes, (size_t)a.width, plane);
        if ((st = launch_yuv420_to_packed422(c, s, j, nf, a.format, a.planar, nullptr))) return st;
        vec = j.vec != 0;
    }
    yuv420_packed422_count(c, false, vec);
    return MI_OK;
}

mi_status yuv420_packed422_dev(mi_ctx* c, hipStream_t s, const Yuv420P422Args& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    return is_clahe ? clahe_yuv420_packed422_dev(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_yuv420_packed422_dev(c, s, a);
}

// One host frame up plane by plane as yuv420_bgr_host stages it (yuv420_plane_in: pinned tight planes are DMA'd as they are,
// everything else goes through the context's pinned staging; under MI_UV_FILL128 only the Y plane travels), one packed frame back as
// bgr_packed422_host returns it (stage_out, 2 B/px).  On the device the frame is tight with every plane at a 16-byte aligned offset,
// so a W % 16 == 0 frame takes the 16 x 2 groups whatever the caller's addresses are.  `h` holds the caller's pointers and pitches;
// it has passed the checks.  Every error exit after the first copy on caller memory drains the stream first.
mi_status yuv420_packed422_host(mi_ctx* c, const Yuv420P422Args& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    const bool copy = h.uv_mode == MI_UV_COPY;
    const size_t w = (size_t)h.width, rows = (size_t)h.height, ysz = w * rows, csz = ysz / 4;
    const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o0 = up16(ysz), o1 = up16(o0 + csz);                      // planar: U at o0, V at o1; interleaved: UV at o0
    const size_t frame = !copy ? o0 : up16(h.planar ? o1 + csz : o0 + 2 * csz);
    const size_t row = 2 * w, out_bytes = row * rows;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = grow_dev(c, &c->d_stage_in, &c->stage_in_bytes, frame))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    if ((st = grow_pinned(c, &c->h_pin_in, &c->pin_in_bytes, frame))) return st;
    uint8_t* const di = c->d_stage_in;
    if ((st = yuv420_plane_in(c, s, h.y, h.y_pitch, w, rows, di, c->h_pin_in, drain))) return st;
    if (copy && h.planar) {
        if ((st = yuv420_plane_in(c, s, h.c0, h.c_pitch, w / 2, rows / 2, di + o0, c->h_pin_in + o0, drain))) return st;
        if ((st = yuv420_plane_in(c, s, h.c1, h.c_pitch, w / 2, rows / 2, di + o1, c->h_pin_in + o1, drain))) return st;
    } else if (copy) {
        if ((st = yuv420_plane_in(c, s, h.c0, h.c_pitch, w, rows / 2, di + o0, c->h_pin_in + o0, drain))) return st;
    }
    const Yuv420P422Args d{di, w, copy ? di + o0 : nullptr, copy && h.planar ? di + o1 : nullptr, !copy ? 0 : h.planar ? w / 2 : w, frame,
                           c->d_stage_out, row, up16(out_bytes), h.width, h.height, 1, h.format, h.uv_mode, h.planar};
    if ((st = yuv420_packed422_dev(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, row, rows, drain);
}

mi_status yuv420_packed422_entry(mi_ctx* c, const mi_yuv420_planes* in, void* out, size_t out_pitch, size_t out_frame, int width, int height,
                                 int n_frames, int format, mi_uv_mode uv_mode, bool host, bool is_clahe, double clip_limit, int tiles_x,
                                 int tiles_y, void* stream)
{
    if (!in) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (in->chroma != MI_CHROMA_INTERLEAVED && in->chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const bool planar = in->chroma == MI_CHROMA_PLANAR, copy = uv_mode == MI_UV_COPY;
    // with MI_UV_FILL128 the input's chroma is not read and its descriptor fields are ignored
    const Yuv420P422Args a{(const uint8_t*)in->y, in->y_pitch, copy ? (const uint8_t*)in->c0 : nullptr,
                           copy && planar ? (const uint8_t*)in->c1 : nullptr, copy ? in->c_pitch : 0, host ? 0 : in->frame_stride,
                           (uint8_t*)out, out_pitch, out_frame, width, height, n_frames, format, uv_mode, planar};
    bool work = false;
    const mi_status st = check_yuv420_packed422(c, a, host, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? yuv420_packed422_host(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : yuv420_packed422_dev(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_to_packed422_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
                                                         size_t out_frame_stride, int width, int height, int n_frames, int format,
                                                         mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_packed422_entry(c, in, d_out, out_pitch, out_frame_stride, width, height, n_frames, format, uv_mode, false, false, 0.0, 0, 0,
                                  stream);
}

mi_status mi_clahe_yuv420_to_packed422_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, void* d_out, size_t out_pitch,
                                                 size_t out_frame_stride, int width, int height, int n_frames, int format,
                                                 mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_packed422_entry(c, in, d_out, out_pitch, out_frame_stride, width, height, n_frames, format, uv_mode, false, true, clip_limit,
                                  tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_yuv420_to_packed422(mi_ctx* c, const mi_yuv420_planes* in, uint8_t* out, size_t out_pitch, int width, int height,
                                               int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return yuv420_packed422_entry(c, in, out, out_pitch, 0, width, height, 1, format, uv_mode, true, false, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_yuv420_to_packed422(mi_ctx* c, const mi_yuv420_planes* in, uint8_t* out, size_t out_pitch, int width, int height,
                                       int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return yuv420_packed422_entry(c, in, out, out_pitch, 0, width, height, 1, format, uv_mode, true, true, clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
