// bgra_yuv420.inc.hpp -- interleaved 8-bit four-channel images (BGRA / BGRX, RGBA / RGBX: CV_8UC4) in, 4:2:0 frames described by
// mi_yuv420_planes (I420 / YV12, or NV12) out with the luma equalized: checks, the launch of stage 1, the two stage sequences, the host
// form, extern "C"
// Included by ../mi_lumaeq.hip behind yuv420_packed422_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// render target / swap-chain image / screen capture / interop buffer -> equalize -> hardware encoder (NV12) or software encoder (three
// pitched planes) in one pass over the 4 B/px surface, without a slice-and-copy to three channels outside the library.  The structure
// is bgr_yuv420.inc.hpp's, but BOTH chroma layouts are this form's own kernels (kernels/bgra_yuv420.hip.h): an INTERLEAVED output is not
// handed to another form and counts like a planar one.  Stage 1 converts into the caller's pitched planes and, for equalizeHist, counts
// the luma it writes into the partials equalize_lut_kernel reads; stage 2 is the planar forms' own in place on the output Y plane
// (launch_apply / clahe_dev with src == dst and no chroma job).  Never the fused kernel and never hist_lut_kernel: option
// two_kernel_max_frames does not apply.

namespace {

// frames per launch sequence, as kBgrNv12FramesPerLaunch: bounds the grids and the partials of a sequence
constexpr int kBgraYuv420FramesPerLaunch = 256;

struct BgraYuv420Args {
    const uint8_t* in; size_t in_pitch, in_frame;
    uint8_t* y; size_t y_pitch;
    uint8_t* c0; uint8_t* c1; size_t c_pitch;           // planar: the U and the V plane; interleaved: c0 = the UV plane, c1 unused (null)
    size_t out_frame;
    int width, height, n_frames, order;
    mi_uv_mode uv_mode;
    bool planar;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  `a` has been filled from a non-null
// descriptor whose chroma is one of the two values (c1 = null on an interleaved one).  The rules and their order are check_bgr_yuv420's
// and check_bgr_nv12's, with a row of 4*W bytes.
mi_status check_bgra_yuv420(mi_ctx* c, const BgraYuv420Args& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.uv_mode != MI_UV_FILL128 && a.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.in || !a.y || !a.c0 || (a.planar && !a.c1)) return fail(c, MI_ERR_BAD_ARG, "null image or plane pointer");
    if (a.in_pitch < 4 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "in_pitch < 4 * width");
    if (a.y_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (a.c_pitch < (a.planar ? (size_t)a.width / 2 : (size_t)a.width))
        return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width interleaved, width / 2 planar)");
    if (a.y == a.c0 || (a.planar && (a.y == a.c1 || a.c0 == a.c1))) return fail(c, MI_ERR_BAD_ARG, "two output planes at one address");
    if (a.y == a.in || a.c0 == a.in || (a.planar && a.c1 == a.in)) return fail(c, MI_ERR_BAD_ARG, "BGRA in, 4:2:0 out has no in-place form");
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    *work = true;
    return MI_OK;
}

// THE rule of the header for a call (and, with stand-in addresses and frame strides 0, for the shape of a list): W % 16 == 0, the image
// and Y terms multiples of 16, the chroma terms of 16 for interleaved chroma (one 16-byte UV store) and of 8 for planar chroma (an
// 8-byte U and an 8-byte V store; out_frame steps the chroma planes too, 16 covers them)
bool bgra_yuv420_call_vec(const BgraYuv420Args& a)
{
    const uintptr_t chroma = a.planar ? (((uintptr_t)a.c0 | (uintptr_t)a.c1 | a.c_pitch) & 7) : (((uintptr_t)a.c0 | a.c_pitch) & 15);
    return a.width % 16 == 0 &&
           (((uintptr_t)a.in | (uintptr_t)a.y | a.in_pitch | a.y_pitch | a.in_frame | a.out_frame) & 15) == 0 && chroma == 0;
}

// Stage 1 on frames f0 .. f0 + nf of the call (MI_K_COLOR).  hist: count the luma into c->d_partial, *nparts_out workgroups a frame.
// *vec_out: the walk the kernel takes (a list: what the shape allows).
// The grid is the siblings' rule (launch_bgr_to_nv12) on this form's own byte basis: half of what stage 1 reads and writes,
// (4 + 1.5) / 2 = 11/4 bytes per pixel, where the three-channel forms take 9/4; the same cap of 2048, and never more workgroups than
// there are items for (16 x 2 groups: a workgroup pass covers 8192 pixels; 2 x 2 blocks: 1024).
// With a frame table (fl: one chunk of at most kFramesPerLaunch frames, bgra_yuv420_frames.inc.hpp): the same grid on the
// *_frames_kernel entry; `a` then carries the shape, its base pointers (stand-ins for the vec rule) and frame strides are not used by
// the kernel, and j.vec says what the shape allows -- a byte-path frame of such a launch simply takes more grid-stride steps.
mi_status launch_bgra_to_yuv420(mi_ctx* c, hipStream_t s, const BgraYuv420Args& a, int f0, int nf, bool hist, int* nparts_out, bool* vec_out,
                                const BgraYuv420List* fl = nullptr)
{
    BgraYuv420Job j{};
    j.in = a.in + (size_t)f0 * a.in_frame; j.y = a.y + (size_t)f0 * a.out_frame;
    j.c0 = a.c0 + (size_t)f0 * a.out_frame; j.c1 = a.planar ? a.c1 + (size_t)f0 * a.out_frame : nullptr;
    j.in_step = (long long)a.in_pitch; j.y_step = (long long)a.y_pitch; j.c_step = (long long)a.c_pitch;
    j.in_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = bgra_yuv420_call_vec(a);
    const long long px = (long long)a.width * a.height;
    int B = blocks_per_frame(c, px * 11 / 4, a.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    if (hist) {
        if (mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t))) return st;
    }
    const dim3 grid(B, nf), block(kThreads);
    const bool rgb = a.order == MI_ORDER_RGB, cp = a.uv_mode == MI_UV_COPY;
#define MI_BGRA_YUV420_LAUNCH(O, C, U)                                                                                               \
    do {                                                                                                                             \
        if (fl && hist) LAUNCH(c, s, MI_K_COLOR, (bgra_to_yuv420_hist_frames_kernel<O, C, U, true>), grid, block, 0, j, *fl, c->d_partial);   \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (bgra_to_yuv420_hist_frames_kernel<O, C, U, false>), grid, block, 0, j, *fl, (uint32_t*)nullptr); \
        else if (hist)  LAUNCH(c, s, MI_K_COLOR, (bgra_to_yuv420_hist_kernel<O, C, U, true>), grid, block, 0, j, c->d_partial);        \
        else            LAUNCH(c, s, MI_K_COLOR, (bgra_to_yuv420_hist_kernel<O, C, U, false>), grid, block, 0, j, (uint32_t*)nullptr); \
    } while (0)
#define MI_BGRA_YUV420_LAUNCH_C(C)                                                                                                   \
    do {                                                                                                                             \
        if (rgb && cp) MI_BGRA_YUV420_LAUNCH(1, C, 1);                                                                               \
        else if (rgb)  MI_BGRA_YUV420_LAUNCH(1, C, 0);                                                                               \
        else if (cp)   MI_BGRA_YUV420_LAUNCH(0, C, 1);                                                                               \
        else           MI_BGRA_YUV420_LAUNCH(0, C, 0);                                                                               \
    } while (0)
    if (a.planar) MI_BGRA_YUV420_LAUNCH_C(1);
    else          MI_BGRA_YUV420_LAUNCH_C(0);
#undef MI_BGRA_YUV420_LAUNCH_C
#undef MI_BGRA_YUV420_LAUNCH
    if (nparts_out) *nparts_out = B;
    *vec_out = j.vec != 0;
    return MI_OK;
}

// The output Y plane as the planar stage launchers see it: source and destination at once
PlaneArgs bgra_yuv420_y_plane(const BgraYuv420Args& a, int f0, int nf)
{
    uint8_t* y = a.y + (size_t)f0 * a.out_frame;
    return PlaneArgs{y, a.y_pitch, a.out_frame, y, a.y_pitch, a.out_frame, a.width, a.height, nf};
}

// Per chunk: one MI_K_COLOR (convert + count), one MI_K_EQ_LUT, one MI_K_LUT_APPLY (in place on Y); no MI_K_HIST.  One count per call,
// by the walk the conversion kernel took.
mi_status equalize_bgra_yuv420_dev(mi_ctx* c, hipStream_t s, const BgraYuv420Args& a)
{
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgraYuv420FramesPerLaunch) {
        const int nf = std::min(kBgraYuv420FramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_bgra_to_yuv420(c, s, a, f0, nf, true, &nparts, &vec);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        if ((st = launch_apply(c, s, bgra_yuv420_y_plane(a, f0, nf), 0, nf, c->d_luts, nullptr))) return st;
    }
    ++(vec ? c->bgra_yuv420_vec : c->bgra_yuv420_bytes);
    return MI_OK;
}

// Per chunk: one MI_K_COLOR (convert), then what mi_clahe_u8_batch_dev launches for the same plane, in place.
mi_status clahe_bgra_yuv420_dev(mi_ctx* c, hipStream_t s, const BgraYuv420Args& a, double clip_limit, int tiles_x, int tiles_y)
{
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgraYuv420FramesPerLaunch) {
        const int nf = std::min(kBgraYuv420FramesPerLaunch, a.n_frames - f0);
        mi_status st = launch_bgra_to_yuv420(c, s, a, f0, nf, false, nullptr, &vec);
        if (st) return st;
        if ((st = clahe_dev(c, s, bgra_yuv420_y_plane(a, f0, nf), clip_limit, tiles_x, tiles_y, nullptr))) return st;
    }
    ++(vec ? c->bgra_yuv420_vec : c->bgra_yuv420_bytes);
    return MI_OK;
}

mi_status bgra_yuv420_dev(mi_ctx* c, hipStream_t s, const BgraYuv420Args& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    return is_clahe ? clahe_bgra_yuv420_dev(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_bgra_yuv420_dev(c, s, a);
}

// One CV_8UC4 host image up as bgr_yuv420_host stages its CV_8UC3 one (stage_in, a row of 4*W bytes), the planes back one by one as
// yuv420_host returns them (PlaneOut: pinned tight planes are DMA'd as they are, everything else goes through the context's pinned
// staging).  On the device the frame is tight with every plane at a 16-byte aligned offset, so a W % 16 == 0 frame takes the 16 x 2
// groups whatever the caller's addresses are.  `h` holds the caller's pointers and pitches; it has passed the checks.  Every error exit
// after the first copy on caller memory drains the stream first.
mi_status bgra_yuv420_host(mi_ctx* c, const BgraYuv420Args& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if ((long long)h.width * h.height > 0x7fffffffLL / 4) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    const size_t w = (size_t)h.width, rows = (size_t)h.height, ysz = w * rows, csz = ysz / 4, row = 4 * w;
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
    const BgraYuv420Args d{c->d_stage_in, row, up16(row * rows), dout, w, dout + o0, h.planar ? dout + o1 : nullptr, h.planar ? w / 2 : w,
                           frame, h.width, h.height, 1, h.order, h.uv_mode, h.planar};
    if ((st = bgra_yuv420_dev(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    const PlaneOut py(c, h.y, h.y_pitch, w, w, rows);
    const PlaneOut p0 = h.planar ? PlaneOut(c, h.c0, h.c_pitch, w / 2, w / 2, rows / 2) : PlaneOut(c, h.c0, h.c_pitch, w, w, rows / 2);
    const PlaneOut p1 = h.planar ? PlaneOut(c, h.c1, h.c_pitch, w / 2, w / 2, rows / 2) : p0;      // planar outputs only
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

mi_status bgra_yuv420_entry(mi_ctx* c, const void* in, size_t in_pitch, size_t in_frame, const mi_yuv420_planes* out, int width, int height,
                            int n_frames, int order, mi_uv_mode uv_mode, bool host, bool is_clahe, double clip_limit, int tiles_x,
                            int tiles_y, void* stream)
{
    if (!out) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (out->chroma != MI_CHROMA_INTERLEAVED && out->chroma != MI_CHROMA_PLANAR)
        return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    const bool planar = out->chroma == MI_CHROMA_PLANAR;
    const BgraYuv420Args a{(const uint8_t*)in, in_pitch, host ? 0 : in_frame, (uint8_t*)out->y, out->y_pitch, (uint8_t*)out->c0,
                           planar ? (uint8_t*)out->c1 : nullptr, out->c_pitch, host ? 0 : out->frame_stride, width, height, n_frames, order,
                           uv_mode, planar};
    bool work = false;
    const mi_status st = check_bgra_yuv420(c, a, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? bgra_yuv420_host(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : bgra_yuv420_dev(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgra_to_yuv420_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                    const mi_yuv420_planes* out, int width, int height, int n_frames, int order,
                                                    mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return bgra_yuv420_entry(c, d_in, in_pitch, in_frame_stride, out, width, height, n_frames, order, uv_mode, false, false, 0.0, 0, 0,
                             stream);
}

mi_status mi_clahe_bgra_to_yuv420_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                            const mi_yuv420_planes* out, int width, int height, int n_frames, int order,
                                            mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgra_yuv420_entry(c, d_in, in_pitch, in_frame_stride, out, width, height, n_frames, order, uv_mode, false, true, clip_limit,
                             tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_bgra_to_yuv420(mi_ctx* c, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out, int width, int height,
                                          int order, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return bgra_yuv420_entry(c, in, in_step, 0, out, width, height, 1, order, uv_mode, true, false, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_bgra_to_yuv420(mi_ctx* c, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out, int width, int height,
                                  int order, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return bgra_yuv420_entry(c, in, in_step, 0, out, width, height, 1, order, uv_mode, true, true, clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
