// bgra_packed422.inc.hpp -- interleaved 8-bit four-channel images (BGRA / BGRX, RGBA / RGBX: CV_8UC4) in, pitched packed 4:2:2 frames
// (YUY2 / UYVY) out with the luma equalized: checks, the launch of stage 1, the two stage sequences, the host form, extern "C"
// Included by ../mi_lumaeq.hip behind packed422_bgra_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// render target / swap-chain image / screen or window capture / interop buffer -> equalize -> playout card, v4l2 output or loopback
// device, virtual camera in one pass over the 4 B/px surface, without a slice-and-copy to three channels outside the library and
// without an NV12 intermediate (which has dropped every second chroma row).  The structure is bgr_packed422.inc.hpp's: stage 1
// (kernels/bgra_packed422.hip.h) converts into the caller's packed frame and, for equalizeHist, counts the luma it writes into the
// partials equalize_lut_kernel reads; stage 2 is exactly that form's -- bgr_packed422_in_place + the packed form's own kernels
// (packed422.inc.hpp: PackedOut / clahe422_dev) IN PLACE on the output frame, the chroma kept.  Never the fused kernel and never
// hist_lut_kernel: option two_kernel_max_frames does not apply.  Every CLAHE shape runs in one pass.
// The frame-list form (mi_*_bgra_to_packed422_frames_dev) is bgra_packed422_frames.inc.hpp: the same stage 1 on its *_frames_kernel
// entry (launch_bgra_to_packed422 with a Packed422List), the same stage 2 with the list.
// The arguments are bgr_packed422.inc.hpp's BgrP422Args with a row of 4*W bytes in.

namespace {

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  host: the output is host memory the
// kernels never see -- any address and pitch.  The rules and their order are check_bgr_packed422's, with a row of 4*W bytes in and
// the host form's W*H limit that of bgra_yuv420_host.
mi_status check_bgra_packed422(mi_ctx* c, const BgrP422Args& a, bool host, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.format != MI_FMT_YUY2 && a.format != MI_FMT_UYVY) return fail(c, MI_ERR_BAD_ARG, "format must be MI_FMT_YUY2 or MI_FMT_UYVY");
    if (a.uv_mode != MI_UV_FILL128 && a.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width & 1) return fail(c, MI_ERR_BAD_ARG, "4:2:2 frames have an even width");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.in || !a.out) return fail(c, MI_ERR_BAD_ARG, "null image or frame pointer");
    if (a.in_pitch < 4 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "in_pitch < 4 * width");
    if (a.out_pitch < 2 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "out_pitch < 2 * width");
    if (!host && (((uintptr_t)a.out | a.out_pitch | a.out_frame) & 3))
        return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 pointers, pitches and frame strides are multiples of 4");
    if (a.out == a.in) return fail(c, MI_ERR_BAD_ARG, "BGRA in, packed 4:2:2 out has no in-place form");
    // the limits of the packed and planar forms, and the tile grids and heights the stage sequences would refuse only after stage 1
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    if (host && (long long)a.width * a.height > 0x7fffffffLL / 4) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    *work = true;
    return MI_OK;
}

// THE rule of the header for a call (and, with stand-in addresses and frame strides 0, for the shape of a list): W % 16 == 0 and the
// image and frame bases, pitches and frame strides multiples of 16
bool bgra_packed422_call_vec(const BgrP422Args& a)
{
    return a.width % 16 == 0 &&
           (((uintptr_t)a.in | (uintptr_t)a.out | a.in_pitch | a.out_pitch | a.in_frame | a.out_frame) & 15) == 0;
}

// Stage 1 on frames f0 .. f0 + nf of the call (MI_K_COLOR).  hist: count the luma into c->d_partial, *nparts_out workgroups a frame.
// *vec_out: the walk the kernel takes (a list: what the shape allows).
// The grid is launch_bgr_to_packed422's rule on this form's own byte basis: half of what stage 1 reads and writes, (4 + 2) / 2 = 3
// bytes per pixel where the three-channel form takes 5/2; one row unit per image row, the same cap of 2048, and never more workgroups
// than there are items for (16 x 1 groups: a workgroup pass covers 4096 pixels; macropixels: 512).
// With a frame table (fl: one chunk of at most kPacked422FramesPerLaunch frames, bgra_packed422_frames.inc.hpp): the same grid on the
// *_frames_kernel entry; `a` then carries the shape, its base pointers (stand-ins for the vec rule) and frame strides are not used by
// the kernel, and j.vec says what the shape allows -- a byte-walk frame of such a launch simply takes more grid-stride steps.
mi_status launch_bgra_to_packed422(mi_ctx* c, hipStream_t s, const BgrP422Args& a, int f0, int nf, bool hist, int* nparts_out, bool* vec_out,
                                   const Packed422List* fl = nullptr)
{
    BgraPacked422Job j{};
    j.in = a.in + (size_t)f0 * a.in_frame; j.out = a.out + (size_t)f0 * a.out_frame;
    j.in_step = (long long)a.in_pitch; j.out_step = (long long)a.out_pitch;
    j.in_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = bgra_packed422_call_vec(a);
    const long long px = (long long)a.width * a.height;
    int B = blocks_per_frame(c, px * 3, a.height, nf, 2048);
    const long long items = j.vec ? px / 16 : px / 2;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    if (hist) {
        if (mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t))) return st;
    }
    const dim3 grid(B, nf), block(kThreads);
    const bool rgb = a.order == MI_ORDER_RGB, uyvy = a.format == MI_FMT_UYVY, cp = a.uv_mode == MI_UV_COPY;
#define MI_BGRA_P422_LAUNCH(O, F, U)                                                                                                 \
    do {                                                                                                                             \
        if (fl && hist) LAUNCH(c, s, MI_K_COLOR, (bgra_to_packed422_hist_frames_kernel<O, F, U, true>), grid, block, 0, j, *fl, c->d_partial); \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (bgra_to_packed422_hist_frames_kernel<O, F, U, false>), grid, block, 0, j, *fl, (uint32_t*)nullptr); \
        else if (hist)  LAUNCH(c, s, MI_K_COLOR, (bgra_to_packed422_hist_kernel<O, F, U, true>), grid, block, 0, j, c->d_partial);     \
        else            LAUNCH(c, s, MI_K_COLOR, (bgra_to_packed422_hist_kernel<O, F, U, false>), grid, block, 0, j, (uint32_t*)nullptr); \
    } while (0)
#define MI_BGRA_P422_LAUNCH_OF(O, F)                                                                                                 \
    do {                                                                                                                             \
        if (cp) MI_BGRA_P422_LAUNCH(O, F, 1);                                                                                        \
        else    MI_BGRA_P422_LAUNCH(O, F, 0);                                                                                        \
    } while (0)
    if (rgb && uyvy) MI_BGRA_P422_LAUNCH_OF(1, 1);
    else if (rgb)    MI_BGRA_P422_LAUNCH_OF(1, 0);
    else if (uyvy)   MI_BGRA_P422_LAUNCH_OF(0, 1);
    else             MI_BGRA_P422_LAUNCH_OF(0, 0);
#undef MI_BGRA_P422_LAUNCH_OF
#undef MI_BGRA_P422_LAUNCH
    if (nparts_out) *nparts_out = B;
    *vec_out = j.vec != 0;
    return MI_OK;
}

// per chunk: one MI_K_COLOR (convert + count), one MI_K_EQ_LUT, one MI_K_LUT_APPLY (the packed form's, in place); no MI_K_HIST.
// One count per call, by the walk the conversion kernel took.
template <int OFF>
mi_status equalize_bgra_packed422_dev(mi_ctx* c, hipStream_t s, const BgrP422Args& a)
{
    bool vec = false;
    const long long frame_bytes = 2LL * a.width * a.height;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_bgra_to_packed422(c, s, a, f0, nf, true, &nparts, &vec);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        const int BA = blocks_per_frame(c, frame_bytes, PackedOut::apply_rows(a.height), nf, 2048);
        if ((st = launch_pair(c, s, MI_K_LUT_APPLY, PackedOut::K<OFF>::apply, (const Packed422List*)nullptr, dim3(BA, nf), dim3(kThreads), 0,
                              PackedOut::cut(bgr_packed422_in_place(a, f0, nf), 0), (const uint8_t*)c->d_luts))) return st;
    }
    ++(vec ? c->bgra_packed422_vec : c->bgra_packed422_bytes);
    return MI_OK;
}

// per chunk: one MI_K_COLOR (convert), then what mi_clahe_packed422_batch_dev launches for the same frames in place
template <int OFF>
mi_status clahe_bgra_packed422_dev(mi_ctx* c, hipStream_t s, const BgrP422Args& a, double clip_limit, int tiles_x, int tiles_y)
{
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        mi_status st = launch_bgra_to_packed422(c, s, a, f0, nf, false, nullptr, &vec);
        if (st) return st;
        if ((st = clahe422_dev<PackedOut, OFF>(c, s, bgr_packed422_in_place(a, f0, nf), clip_limit, tiles_x, tiles_y, nullptr, nullptr))) return st;
    }
    ++(vec ? c->bgra_packed422_vec : c->bgra_packed422_bytes);
    return MI_OK;
}

mi_status bgra_packed422_dev(mi_ctx* c, hipStream_t s, const BgrP422Args& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if (a.format == MI_FMT_UYVY)
        return is_clahe ? clahe_bgra_packed422_dev<1>(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_bgra_packed422_dev<1>(c, s, a);
    return is_clahe ? clahe_bgra_packed422_dev<0>(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_bgra_packed422_dev<0>(c, s, a);
}

// One CV_8UC4 host image up as bgra_yuv420_host stages it (stage_in, a row of 4*W bytes), one packed frame back as bgr_packed422_host
// returns it (stage_out, 2 B/px: pinned tight frames are DMA'd as they are, anything else goes through the context's pinned staging).
// On the device the frame is tight and 16-byte aligned, so a W % 16 == 0 image takes the 16 x 1 groups whatever the caller's
// addresses are.  `h` holds the caller's pointers and pitches; it has passed the checks.  Every error exit after the first copy on
// caller memory drains the stream first.
mi_status bgra_packed422_host(mi_ctx* c, const BgrP422Args& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    const size_t rows = (size_t)h.height, in_row = 4 * (size_t)h.width, out_row = 2 * (size_t)h.width, out_bytes = out_row * rows;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = stage_in(c, s, h.in, h.in_pitch, in_row, rows, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    const BgrP422Args d{c->d_stage_in, in_row, in_row * rows, c->d_stage_out, out_row, out_bytes, h.width, h.height, 1, h.order, h.format,
                        h.uv_mode};
    if ((st = bgra_packed422_dev(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, out_row, rows, drain);
}

mi_status bgra_packed422_entry(mi_ctx* c, const void* in, size_t in_pitch, size_t in_frame, void* out, size_t out_pitch, size_t out_frame,
                               int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode, bool host, bool is_clahe,
                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    const BgrP422Args a{(const uint8_t*)in, in_pitch, in_frame, (uint8_t*)out, out_pitch, out_frame, width, height, n_frames, order, format,
                        uv_mode};
    bool work = false;
    const mi_status st = check_bgra_packed422(c, a, host, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? bgra_packed422_host(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : bgra_packed422_dev(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgra_to_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                       void* d_out, size_t out_pitch, size_t out_frame_stride,
                                                       int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
                                                       void* stream)
{
    ENTER_COMPUTE(c);
    return bgra_packed422_entry(c, d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, order,
                                format, uv_mode, false, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_bgra_to_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_out, size_t out_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
                                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgra_packed422_entry(c, d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, order,
                                format, uv_mode, false, true, clip_limit, tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_bgra_to_packed422(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
                                             int width, int height, int order, int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return bgra_packed422_entry(c, in, in_step, 0, out, out_pitch, 0, width, height, 1, order, format, uv_mode, true, false, 0.0, 0, 0,
                                nullptr);
}

mi_status mi_clahe_bgra_to_packed422(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
                                     int width, int height, int order, int format, mi_uv_mode uv_mode,
                                     double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return bgra_packed422_entry(c, in, in_step, 0, out, out_pitch, 0, width, height, 1, order, format, uv_mode, true, true, clip_limit,
                                tiles_x, tiles_y, nullptr);
}

}  // extern "C"
