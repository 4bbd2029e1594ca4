// bgr_yuv420.inc.hpp -- interleaved 8-bit BGR / RGB images in, 4:2:0 frames described by mi_yuv420_planes (I420 / YV12, or NV12) out with the
// luma equalized: checks, the interleaved hand-over, the planar launch sequences, the host form, extern "C"
// Included by ../mi_lumaeq.hip behind yuv420_bgr_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// renderer / model output / image reader -> equalize -> software encoder (three pitched planes: data[0..2] / linesize[0..2]) without an
// NV12 intermediate and without plane copies outside the library.  An INTERLEAVED output is the NV12 form's own: check_bgr_nv12 /
// equalize_bgr_nv12_dev / clahe_bgr_nv12_dev (bgr_nv12.inc.hpp) with their kernels.  A PLANAR output runs the same two stages on the
// kernel of kernels/bgr_yuv420.hip.h, which stores the chroma into two planes: stage 1 converts into the caller's pitched planes and,
// for equalizeHist, counts the luma it writes into the partials equalize_lut_kernel reads; stage 2 is the planar forms' own in place
// on the output Y plane (launch_apply / clahe_dev with src == dst and no chroma job).  Never the fused kernel and never
// hist_lut_kernel: option two_kernel_max_frames does not apply.

namespace {

struct BgrYuv420Args {
    const uint8_t* in; size_t in_pitch, in_frame;
    uint8_t* y; size_t y_pitch;
    uint8_t* u; uint8_t* v; size_t c_pitch;             // planar: U and V planes; interleaved: u = the UV plane, v unused
    size_t out_frame;
    int width, height, n_frames, order;
    mi_uv_mode uv_mode;
    bool planar;
};

BgrNv12Args bgr_yuv420_as_nv12(const BgrYuv420Args& a)
{
    return BgrNv12Args{a.in, a.in_pitch, a.in_frame, a.y, a.y_pitch, a.u, a.c_pitch, a.out_frame, a.width, a.height, a.n_frames, a.order,
                       a.uv_mode};
}

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  `a` has been filled from a non-null
// descriptor whose chroma is one of the two values.  An INTERLEAVED output has the NV12 form's checks.
mi_status check_bgr_yuv420(mi_ctx* c, const BgrYuv420Args& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    if (!a.planar) return check_bgr_nv12(c, bgr_yuv420_as_nv12(a), is_clahe, tiles_x, tiles_y, work);
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.uv_mode != MI_UV_FILL128 && a.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.in || !a.y || !a.u || !a.v) return fail(c, MI_ERR_BAD_ARG, "null image or plane pointer");
    if (a.in_pitch < 3 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "in_pitch < 3 * width");
    if (a.y_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (a.c_pitch < (size_t)a.width / 2) return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width / 2 planar)");
    if (a.y == a.u || a.y == a.v || a.u == a.v) return fail(c, MI_ERR_BAD_ARG, "two output planes at one address");
    if (a.y == a.in || a.u == a.in || a.v == a.in) return fail(c, MI_ERR_BAD_ARG, "BGR in, 4:2:0 out has no in-place form");
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    *work = true;
    return MI_OK;
}

// Stage 1 on frames f0 .. f0 + nf of a PLANAR call (MI_K_COLOR).  hist: count the luma into c->d_partial, *nparts_out workgroups a
// frame.  *vec_out: the walk the kernel takes.  The grid is launch_bgr_to_nv12's: the same byte basis, the same cap.
// With a frame table (fl: one chunk of at most kFramesPerLaunch frames, bgr_yuv420_frames.inc.hpp): the same grid on the
// *_frames_kernel entry; `a` then carries the shape, its base pointers (stand-ins for the vec rule) and frame strides are not used by
// the kernel, and j.vec (*vec_out) says what the shape allows -- a byte-path frame of such a launch simply takes more grid-stride steps.
mi_status launch_bgr_to_yuv420(mi_ctx* c, hipStream_t s, const BgrYuv420Args& a, int f0, int nf, bool hist, int* nparts_out, bool* vec_out,
                               const BgrYuv420List* fl = nullptr)
{
    BgrYuv420Job j{};
    j.in = a.in + (size_t)f0 * a.in_frame; j.y = a.y + (size_t)f0 * a.out_frame;
    j.u = a.u + (size_t)f0 * a.out_frame; j.v = a.v + (size_t)f0 * a.out_frame;
    j.in_step = (long long)a.in_pitch; j.y_step = (long long)a.y_pitch; j.c_step = (long long)a.c_pitch;
    j.in_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    // the image and Y terms multiples of 16, the chroma terms of 8 (a lane stores 8 bytes into each chroma plane; out_frame steps the
    // chroma planes too, 16 covers them)
    j.vec = a.width % 16 == 0 &&
            (((uintptr_t)a.in | (uintptr_t)a.y | a.in_pitch | a.y_pitch | a.in_frame | a.out_frame) & 15) == 0 &&
            (((uintptr_t)a.u | (uintptr_t)a.v | a.c_pitch) & 7) == 0;
    const long long px = (long long)a.width * a.height;
    int B = blocks_per_frame(c, px * 9 / 4, a.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    if (hist) {
        if (mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t))) return st;
    }
    const dim3 grid(B, nf), block(kThreads);
    const bool rgb = a.order == MI_ORDER_RGB, cp = a.uv_mode == MI_UV_COPY;
#define MI_BGR_YUV420_LAUNCH(O, U)                                                                                                   \
    do {                                                                                                                             \
        if (fl && hist) LAUNCH(c, s, MI_K_COLOR, (bgr_to_yuv420_hist_frames_kernel<O, U, true>), grid, block, 0, j, *fl, c->d_partial);  \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (bgr_to_yuv420_hist_frames_kernel<O, U, false>), grid, block, 0, j, *fl, (uint32_t*)nullptr); \
        else if (hist)  LAUNCH(c, s, MI_K_COLOR, (bgr_to_yuv420_hist_kernel<O, U, true>), grid, block, 0, j, c->d_partial);            \
        else            LAUNCH(c, s, MI_K_COLOR, (bgr_to_yuv420_hist_kernel<O, U, false>), grid, block, 0, j, (uint32_t*)nullptr);     \
    } while (0)
    if (rgb && cp) MI_BGR_YUV420_LAUNCH(1, 1);
    else if (rgb)  MI_BGR_YUV420_LAUNCH(1, 0);
    else if (cp)   MI_BGR_YUV420_LAUNCH(0, 1);
    else           MI_BGR_YUV420_LAUNCH(0, 0);
#undef MI_BGR_YUV420_LAUNCH
    if (nparts_out) *nparts_out = B;
    *vec_out = j.vec != 0;
    return MI_OK;
}

// The output Y plane as the planar stage launchers see it: source and destination at once
PlaneArgs bgr_yuv420_y_plane(const BgrYuv420Args& a, int f0, int nf)
{
    uint8_t* y = a.y + (size_t)f0 * a.out_frame;
    return PlaneArgs{y, a.y_pitch, a.out_frame, y, a.y_pitch, a.out_frame, a.width, a.height, nf};
}

// equalize_bgr_nv12_dev on planar chroma.  Per chunk: one MI_K_COLOR (convert + count), one MI_K_EQ_LUT, one MI_K_LUT_APPLY (in place
// on Y); no MI_K_HIST.  One count per call, by the walk the conversion kernel took.
mi_status equalize_bgr_yuv420_dev(mi_ctx* c, hipStream_t s, const BgrYuv420Args& a)
{
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_bgr_to_yuv420(c, s, a, f0, nf, true, &nparts, &vec);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        if ((st = launch_apply(c, s, bgr_yuv420_y_plane(a, f0, nf), 0, nf, c->d_luts, nullptr))) return st;
    }
    ++(vec ? c->bgr_yuv420_vec : c->bgr_yuv420_bytes);
    return MI_OK;
}

// clahe_bgr_nv12_dev on planar chroma.  Per chunk: one MI_K_COLOR (convert), then what mi_clahe_u8_batch_dev launches for the same
// plane, in place.
mi_status clahe_bgr_yuv420_dev(mi_ctx* c, hipStream_t s, const BgrYuv420Args& a, double clip_limit, int tiles_x, int tiles_y)
{
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        mi_status st = launch_bgr_to_yuv420(c, s, a, f0, nf, false, nullptr, &vec);
        if (st) return st;
        if ((st = clahe_dev(c, s, bgr_yuv420_y_plane(a, f0, nf), clip_limit, tiles_x, tiles_y, nullptr))) return st;
    }
    ++(vec ? c->bgr_yuv420_vec : c->bgr_yuv420_bytes);
    return MI_OK;
}

mi_status bgr_yuv420_dev(mi_ctx* c, hipStream_t s, const BgrYuv420Args& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if (!a.planar) {                                    // the NV12 form's own path: its kernels, none of the counters above
        const BgrNv12Args n = bgr_yuv420_as_nv12(a);
        return is_clahe ? clahe_bgr_nv12_dev(c, s, n, clip_limit, tiles_x, tiles_y) : equalize_bgr_nv12_dev(c, s, n);
    }
    return is_clahe ? clahe_bgr_yuv420_dev(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_bgr_yuv420_dev(c, s, a);
}

// One CV_8UC3 host image up as bgr_nv12_host stages it (stage_in), the planes back one by one as yuv420_host returns them (PlaneOut:
// pinned tight planes are DMA'd as they are, everything else goes through the context's pinned staging).  On the device the frame is
// tight with every plane at a 16-byte aligned offset, so a W % 16 == 0 frame takes the 16 x 2 groups whatever the caller's addresses
// are.  `h` holds the caller's pointers and pitches; it has passed the checks.  Every error exit after the first copy on caller
// memory drains the stream first.
mi_status bgr_yuv420_host(mi_ctx* c, const BgrYuv420Args& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if ((long long)h.width * h.height > 0x7fffffffLL / 3) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    const size_t w = (size_t)h.width, rows = (size_t)h.height, ysz = w * rows, csz = ysz / 4, row = 3 * w;
    const auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o0 = up16(ysz), o1 = up16(o0 + csz);                      // planar: U at o0, V at o1; interleaved: UV at o0
    const size_t frame = up16(h.planar ? o1 + csz : o0 + 2 * csz);
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = stage_in(c, s, h.in, h.in_pitch, row, rows, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, frame))) return st;
    if ((st = grow_pinned(c, &c->h_pin_out, &c->pin_out_bytes, frame))) return st;
    uint8_t* const dout = c->d_stage_out;
    const BgrYuv420Args d{c->d_stage_in, row, up16(row * rows), dout, w, dout + o0, h.planar ? dout + o1 : nullptr, h.planar ? w / 2 : w,
                          frame, h.width, h.height, 1, h.order, h.uv_mode, h.planar};
    if ((st = bgr_yuv420_dev(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    const PlaneOut py(c, h.y, h.y_pitch, w, w, rows);
    const PlaneOut p0 = h.planar ? PlaneOut(c, h.u, h.c_pitch, w / 2, w / 2, rows / 2) : PlaneOut(c, h.u, h.c_pitch, w, w, rows / 2);
    const PlaneOut p1 = h.planar ? PlaneOut(c, h.v, h.c_pitch, w / 2, w / 2, rows / 2) : p0;       // planar outputs only
    drain.watch(s);
    if ((st = enqueue_plane_out(c, s, dout, c->h_pin_out, py))) return st;
    if ((st = enqueue_plane_out(c, s, dout + o0, c->h_pin_out + o0, p0))) return st;
    if (h.planar && (st = enqueue_plane_out(c, s, dout + o1, c->h_pin_out + o1, p1))) return st;
    HIPCHK(c, hipStreamSynchronize(s));
    drain.done();
    copy_plane_out(py, c->h_pin_out);
    copy_plane_out(p0, c->h_pin_out + o0);
    if (h.planar) copy_plane_out(p1, c->h_pin_out + o1);
    return MI_OK;
}

mi_status bgr_yuv420_entry(mi_ctx* c, const void* in, size_t in_pitch, size_t in_frame, const mi_yuv420_planes* out, int width, int height,
                           int n_frames, int order, mi_uv_mode uv_mode, bool host, bool is_clahe, double clip_limit, int tiles_x,
                           int tiles_y, void* stream)
{
    if (!out) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (out->chroma != MI_CHROMA_INTERLEAVED && out->chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const bool planar = out->chroma == MI_CHROMA_PLANAR;
    const BgrYuv420Args a{(const uint8_t*)in, in_pitch, host ? 0 : in_frame, (uint8_t*)out->y, out->y_pitch, (uint8_t*)out->c0,
                          planar ? (uint8_t*)out->c1 : nullptr, out->c_pitch, host ? 0 : out->frame_stride, width, height, n_frames, order,
                          uv_mode, planar};
    bool work = false;
    const mi_status st = check_bgr_yuv420(c, a, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? bgr_yuv420_host(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : bgr_yuv420_dev(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgr_to_yuv420_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                   const mi_yuv420_planes* out, int width, int height, int n_frames, int order,
                                                   mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_yuv420_entry(c, d_in, in_pitch, in_frame_stride, out, width, height, n_frames, order, uv_mode, false, false, 0.0, 0, 0,
                            stream);
}

mi_status mi_clahe_bgr_to_yuv420_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                           const mi_yuv420_planes* out, int width, int height, int n_frames, int order,
                                           mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_yuv420_entry(c, d_in, in_pitch, in_frame_stride, out, width, height, n_frames, order, uv_mode, false, true, clip_limit,
                            tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_bgr_to_yuv420(mi_ctx* c, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out, int width, int height,
                                         int order, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return bgr_yuv420_entry(c, in, in_step, 0, out, width, height, 1, order, uv_mode, true, false, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_bgr_to_yuv420(mi_ctx* c, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out, int width, int height,
                                 int order, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return bgr_yuv420_entry(c, in, in_step, 0, out, width, height, 1, order, uv_mode, true, true, clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
