// bgr_packed422.inc.hpp -- interleaved 8-bit BGR / RGB images in, pitched packed 4:2:2 frames (YUY2 / UYVY) out with the luma equalized:
// checks, launch sequences, the host form, extern "C"
// Included by ../mi_lumaeq.hip behind bgr_yuv420_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// renderer / model output / image reader -> equalize -> playout card, v4l2 output or loopback device, virtual camera, without an NV12
// intermediate (which has dropped every second chroma row) and without an interleave outside the library.  The order of
// bgr_nv12.inc.hpp: stage 1 (kernels/bgr_packed422.hip.h) converts into the caller's packed frame and, for equalizeHist, counts the
// luma it writes into the partials equalize_lut_kernel reads; stage 2 is the packed form's own kernels (packed422.inc.hpp: PackedOut)
// IN PLACE on the output frame with keep = the chroma mask and fill = 0, whatever uv_mode is -- stage 1 has written the chroma.  Never
// the fused kernel and never hist_lut_kernel: option two_kernel_max_frames does not apply.  Every CLAHE shape runs in one pass.
// The frame-list form (mi_*_bgr_to_packed422_frames_dev) is bgr_packed422_frames.inc.hpp: the same stage 1 on its *_frames_kernel
// entry (launch_bgr_to_packed422 with a Packed422List), the same stage 2 with the list.
//
// Everything between the arguments and the extern "C" entry points is written ONCE, as templates on a pixel form F (BgrTo422 below; a
// form with another number of channels is such a struct in its own file, behind this one in the translation unit).  A form supplies
//   kPx                            bytes per pixel of the image
//   Job                            the argument block of its stage-1 kernels
//   kernel / frames_kernel<ORDER, OFF, UVMODE, HIST>   stage 1, batch and list entry
//   grid_bytes(px)                 the byte basis of stage 1's grid: half of what it reads and writes
//   frame_vec(shape_vec, in, out)  the walk of one frame of a list, the kernel's own rule
//   count_call, count_list         its counters: calls by the walk of their conversion kernel, frames of list calls
//   kInPitch, kInPlace, kListOverlap   its refusal texts, whole literals (fail() keeps the pointer)

namespace {

struct BgrP422Args {
    const uint8_t* in; size_t in_pitch, in_frame;
    uint8_t* out; size_t out_pitch, out_frame;
    int width, height, n_frames, order, format;
    mi_uv_mode uv_mode;
};

// The three-channel form: B, G, R or R, G, B, 3 bytes per pixel in; stage 1 is kernels/bgr_packed422.hip.h.
struct BgrTo422 {
    static constexpr int kPx = 3;
    using Job = BgrPacked422Job;
    template <int ORDER, int OFF, int UVMODE, bool HIST> static constexpr auto kernel = bgr_to_packed422_hist_kernel<ORDER, OFF, UVMODE, HIST>;
    template <int ORDER, int OFF, int UVMODE, bool HIST>
    static constexpr auto frames_kernel = bgr_to_packed422_hist_frames_kernel<ORDER, OFF, UVMODE, HIST>;
    static long long grid_bytes(long long px) { return px * 5 / 2; }           // (3 + 2) / 2 bytes per pixel
    static bool frame_vec(bool shape_vec, const void* in, const void* out) { return bgr_packed422_frame_vec(shape_vec, in, out); }
    static void count_call(mi_ctx* c, bool vec) { ++(vec ? c->bgr_packed422_vec : c->bgr_packed422_bytes); }
    static void count_list(mi_ctx* c, int n_frames, unsigned long long n_vec)
    {
        c->bgr_packed422_list_frames_vec += n_vec;
        c->bgr_packed422_list_frames_bytes += (unsigned long long)n_frames - n_vec;
    }
    static constexpr const char* kInPitch = "in_pitch < 3 * width";
    static constexpr const char* kInPlace = "BGR in, packed 4:2:2 out has no in-place form";
    static constexpr const char* kListOverlap = "BGR in, packed 4:2:2 out has no in-place form: an image overlaps its own output frame";
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  host: the output is host memory the
// kernels never see -- any address and pitch.
template <class F>
mi_status check_bgr_packed422(mi_ctx* c, const BgrP422Args& a, bool host, bool is_clahe, int tiles_x, int tiles_y, bool* work)
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
    if (a.in_pitch < F::kPx * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, F::kInPitch);
    if (a.out_pitch < 2 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "out_pitch < 2 * width");
    if (!host && (((uintptr_t)a.out | a.out_pitch | a.out_frame) & 3))
        return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 pointers, pitches and frame strides are multiples of 4");
    if (a.out == a.in) return fail(c, MI_ERR_BAD_ARG, F::kInPlace);
    // the limits of the packed and planar forms, and the tile grids and heights the stage sequences would refuse only after stage 1
    if (mi_status st = check_yuv420_limits(c, a.width, a.height, is_clahe, tiles_x, tiles_y)) return st;
    if (host && (long long)a.width * a.height > 0x7fffffffLL / F::kPx) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    *work = true;
    return MI_OK;
}

// THE rule of the header for a call (and, with stand-in addresses and frame strides 0, for the shape of a list): W % 16 == 0 and the
// image and frame bases, pitches and frame strides multiples of 16
bool bgr_packed422_call_vec(const BgrP422Args& a)
{
    return a.width % 16 == 0 &&
           (((uintptr_t)a.in | (uintptr_t)a.out | a.in_pitch | a.out_pitch | a.in_frame | a.out_frame) & 15) == 0;
}

// Stage 1 on frames f0 .. f0 + nf of the call (MI_K_COLOR).  hist: count the luma into c->d_partial, *nparts_out workgroups a frame.
// *vec_out: the walk the kernel takes.  The grid rule is launch_bgr_to_nv12's on the form's bytes: half of what is read and written
// (F::grid_bytes: 3 + 2 or 4 + 2 B/px) as the byte basis, one row unit per image row, the cap 2048, and never more workgroups than
// there are items for; a workgroup pass covers 4096 pixels in 16 x 1 groups, 512 in macropixels.
// With a frame table (fl: one chunk of at most kPacked422FramesPerLaunch frames, bgr_packed422_frames.inc.hpp): the same grid on the
// *_frames_kernel entry; `a` then carries the shape, its base pointers (stand-ins for the vec rule) and frame strides are not used by
// the kernel, and j.vec -- *vec_out -- says what the shape allows: a byte-walk frame of such a launch simply takes more grid-stride steps.
template <class F>
mi_status launch_bgr_to_packed422(mi_ctx* c, hipStream_t s, const BgrP422Args& a, int f0, int nf, bool hist, int* nparts_out, bool* vec_out,
                                  const Packed422List* fl = nullptr)
{
    typename F::Job j{};
    j.in = a.in + (size_t)f0 * a.in_frame; j.out = a.out + (size_t)f0 * a.out_frame;
    j.in_step = (long long)a.in_pitch; j.out_step = (long long)a.out_pitch;
    j.in_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = bgr_packed422_call_vec(a);
    const long long px = (long long)a.width * a.height;
    int B = blocks_per_frame(c, F::grid_bytes(px), a.height, nf, 2048);
    const long long items = j.vec ? px / 16 : px / 2;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    if (hist) {
        if (mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t))) return st;
    }
    const dim3 grid(B, nf), block(kThreads);
    const bool rgb = a.order == MI_ORDER_RGB, uyvy = a.format == MI_FMT_UYVY, cp = a.uv_mode == MI_UV_COPY;
#define MI_BGR_P422_LAUNCH(O, FMT, U)                                                                                                \
    do {                                                                                                                             \
        if (fl && hist) LAUNCH(c, s, MI_K_COLOR, (F::template frames_kernel<O, FMT, U, true>), grid, block, 0, j, *fl, c->d_partial); \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (F::template frames_kernel<O, FMT, U, false>), grid, block, 0, j, *fl, (uint32_t*)nullptr); \
        else if (hist)  LAUNCH(c, s, MI_K_COLOR, (F::template kernel<O, FMT, U, true>), grid, block, 0, j, c->d_partial);        \
        else            LAUNCH(c, s, MI_K_COLOR, (F::template kernel<O, FMT, U, false>), grid, block, 0, j, (uint32_t*)nullptr); \
    } while (0)
#define MI_BGR_P422_LAUNCH_OF(O, FMT)                                                                                                \
    do {                                                                                                                             \
        if (cp) MI_BGR_P422_LAUNCH(O, FMT, 1);                                                                                       \
        else    MI_BGR_P422_LAUNCH(O, FMT, 0);                                                                                       \
    } while (0)
    if (rgb && uyvy) MI_BGR_P422_LAUNCH_OF(1, 1);
    else if (rgb)    MI_BGR_P422_LAUNCH_OF(1, 0);
    else if (uyvy)   MI_BGR_P422_LAUNCH_OF(0, 1);
    else             MI_BGR_P422_LAUNCH_OF(0, 0);
#undef MI_BGR_P422_LAUNCH_OF
#undef MI_BGR_P422_LAUNCH
    if (nparts_out) *nparts_out = B;
    *vec_out = j.vec != 0;
    return MI_OK;
}

// Frames f0 .. f0 + nf of the output as the packed form's stages see them: source and destination at once, the chroma kept
P422Args bgr_packed422_in_place(const BgrP422Args& a, int f0, int nf)
{
    uint8_t* p = a.out + (size_t)f0 * a.out_frame;
    return P422Args{p, a.out_pitch, a.out_frame, p, a.out_pitch, a.out_frame, a.width, a.height, nf, a.format, MI_UV_COPY};
}

// per chunk: one MI_K_COLOR (convert + count), one MI_K_EQ_LUT, one MI_K_LUT_APPLY (the packed form's, in place); no MI_K_HIST.
// One count per call, by the walk the conversion kernel took.
template <class F, int OFF>
mi_status equalize_bgr_packed422_dev(mi_ctx* c, hipStream_t s, const BgrP422Args& a)
{
    bool vec = false;
    const long long frame_bytes = 2LL * a.width * a.height;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_bgr_to_packed422<F>(c, s, a, f0, nf, true, &nparts, &vec);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        const int BA = blocks_per_frame(c, frame_bytes, PackedOut::apply_rows(a.height), nf, 2048);
        if ((st = launch_pair(c, s, MI_K_LUT_APPLY, PackedOut::K<OFF>::apply, (const Packed422List*)nullptr, dim3(BA, nf), dim3(kThreads), 0,
                              PackedOut::cut(bgr_packed422_in_place(a, f0, nf), 0), (const uint8_t*)c->d_luts))) return st;
    }
    F::count_call(c, vec);
    return MI_OK;
}

// per chunk: one MI_K_COLOR (convert), then what mi_clahe_packed422_batch_dev launches for the same frames in place
template <class F, int OFF>
mi_status clahe_bgr_packed422_dev(mi_ctx* c, hipStream_t s, const BgrP422Args& a, double clip_limit, int tiles_x, int tiles_y)
{
    bool vec = false;
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        mi_status st = launch_bgr_to_packed422<F>(c, s, a, f0, nf, false, nullptr, &vec);
        if (st) return st;
        if ((st = clahe422_dev<PackedOut, OFF>(c, s, bgr_packed422_in_place(a, f0, nf), clip_limit, tiles_x, tiles_y, nullptr, nullptr))) return st;
    }
    F::count_call(c, vec);
    return MI_OK;
}

template <class F>
mi_status bgr_packed422_dev(mi_ctx* c, hipStream_t s, const BgrP422Args& a, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    if (a.format == MI_FMT_UYVY)
        return is_clahe ? clahe_bgr_packed422_dev<F, 1>(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_bgr_packed422_dev<F, 1>(c, s, a);
    return is_clahe ? clahe_bgr_packed422_dev<F, 0>(c, s, a, clip_limit, tiles_x, tiles_y) : equalize_bgr_packed422_dev<F, 0>(c, s, a);
}

// One host image up as bgr_yuv420_host stages it (stage_in, a row of kPx * W bytes), one packed frame back as packed422_host returns it
// (stage_out, 2 B/px: pinned tight frames are DMA'd as they are, anything else goes through the context's pinned staging).  On the
// device the frame is tight and 16-byte aligned, so a W % 16 == 0 image takes the 16 x 1 groups whatever the caller's addresses are.
// `h` holds the caller's pointers and pitches; it has passed the checks.  Every error exit after the first copy on caller memory
// drains the stream first.
template <class F>
mi_status bgr_packed422_host(mi_ctx* c, const BgrP422Args& h, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    const size_t rows = (size_t)h.height, in_row = F::kPx * (size_t)h.width, out_row = 2 * (size_t)h.width, out_bytes = out_row * rows;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = stage_in(c, s, h.in, h.in_pitch, in_row, rows, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    const BgrP422Args d{c->d_stage_in, in_row, in_row * rows, c->d_stage_out, out_row, out_bytes, h.width, h.height, 1, h.order, h.format,
                        h.uv_mode};
    if ((st = bgr_packed422_dev<F>(c, s, d, is_clahe, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, out_row, rows, drain);
}

template <class F>
mi_status bgr_packed422_entry(mi_ctx* c, const void* in, size_t in_pitch, size_t in_frame, void* out, size_t out_pitch, size_t out_frame,
                              int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode, bool host, bool is_clahe,
                              double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    const BgrP422Args a{(const uint8_t*)in, in_pitch, in_frame, (uint8_t*)out, out_pitch, out_frame, width, height, n_frames, order, format,
                        uv_mode};
    bool work = false;
    const mi_status st = check_bgr_packed422<F>(c, a, host, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    return host ? bgr_packed422_host<F>(c, a, is_clahe, clip_limit, tiles_x, tiles_y)
                : bgr_packed422_dev<F>(c, pick_stream(c, stream), a, is_clahe, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgr_to_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                      void* d_out, size_t out_pitch, size_t out_frame_stride,
                                                      int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
                                                      void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgrTo422>(c, d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, order, format,
                               uv_mode, false, false, 0.0, 0, 0, stream);
}

mi_status mi_clahe_bgr_to_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                              void* d_out, size_t out_pitch, size_t out_frame_stride,
                                              int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode,
                                              double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgrTo422>(c, d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, order, format,
                               uv_mode, false, true, clip_limit, tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_bgr_to_packed422(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
                                            int width, int height, int order, int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgrTo422>(c, in, in_step, 0, out, out_pitch, 0, width, height, 1, order, format, uv_mode, true, false, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_bgr_to_packed422(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch,
                                    int width, int height, int order, int format, mi_uv_mode uv_mode,
                                    double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return bgr_packed422_entry<BgrTo422>(c, in, in_step, 0, out, out_pitch, 0, width, height, 1, order, format, uv_mode, true, true, clip_limit,
                               tiles_x, tiles_y, nullptr);
}

}  // extern "C"
