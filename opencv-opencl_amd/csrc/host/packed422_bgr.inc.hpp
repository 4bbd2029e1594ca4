// packed422_bgr.inc.hpp -- packed 4:2:2 frames in (YUY2 / UYVY), interleaved 8-bit BGR / RGB images out: checks, writer, host frame,
// extern "C" entry points
// Included by ../mi_lumaeq.hip after packed422_nv12_frames.inc.hpp and nv12_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// capture -> equalize -> display / image writer / model without an NV12 intermediate and without losing the chroma of every second
// row.  The stage sequences are packed422.inc.hpp's own (one MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch per chunk; tile
// histograms -> interpolation): same scratch, same chunks, same grids and splits, every shape in one pass.  Only the writer differs:
// the pixel-writing kernels of kernels/packed422_bgr.hip.h decode the new luma with the row's own chroma and write 3 bytes per pixel.
// Never the fused kernel and never hist_lut_kernel, as the packed forms.  The frame-list form is packed422_bgr_frames.inc.hpp's.
//
// Everything between the arguments and the extern "C" entry points is written ONCE, as templates on a pixel form F (Bgr422Image below;
// a form with another number of channels is such a struct in its own file, behind this one in the translation unit).  A form supplies
//   kPx                         bytes per pixel of the image
//   Block                       the argument block of its pixel-writing kernels
//   K<OFF, ORDER>               their six KernelPairs: apply, interp_global, interp<FT, FMA>
//   kOutPitch ... kListOverlap  its refusal texts, whole literals (fail() keeps the pointer)
//   count_call, count_list      how a finished batch / host call and the frames of a finished list call are counted

namespace {

struct P422BgrArgs {
    P422Args in;                      // the input side (in.out* mirror the input: only check_packed422 and the read-only stages look at them)
    uint8_t* out; size_t out_pitch, out_frame;
    int order;
};

P422BgrArgs p422_bgr_args(const void* d_in, size_t in_pitch, size_t in_frame, void* d_out, size_t out_pitch, size_t out_frame,
                          int width, int height, int n_frames, int format, int order)
{
    P422BgrArgs a;
    a.in = P422Args{(const uint8_t*)d_in, in_pitch, in_frame, (uint8_t*)const_cast<void*>(d_in), in_pitch, in_frame,
                    width, height, n_frames, format, MI_UV_COPY};
    a.out = (uint8_t*)d_out; a.out_pitch = out_pitch; a.out_frame = out_frame; a.order = order;
    return a;
}

// The three-channel form: B, G, R or R, G, B, 3 bytes per pixel.  It counts the frames of list calls only.
struct Bgr422Image {
    static constexpr int kPx = 3;
    using Block = Packed422Bgr;
    template <int OFF, int ORDER> struct K {
        static constexpr KernelPair apply{lut_apply422_bgr_frames_kernel<OFF, ORDER>, lut_apply422_bgr_kernel<OFF, ORDER>};
        static constexpr KernelPair interp_global{clahe_interp422_bgr_global_frames_kernel<OFF, ORDER>, clahe_interp422_bgr_global_kernel<OFF, ORDER>};
        template <bool FT, bool FMA>
        static constexpr KernelPair interp{clahe_interp422_bgr_frames_kernel<FT, FMA, OFF, ORDER>, clahe_interp422_bgr_kernel<FT, FMA, OFF, ORDER>};
    };
    static constexpr const char* kOutPitch = "out_pitch < 3 * width";
    static constexpr const char* kOutStep = "out_step < 3 * width";
    static constexpr const char* kInPlace = "packed in, BGR out has no in-place form";
    static constexpr const char* kHostOverlap = "packed in, BGR out has no in-place form: the image overlaps the input frame";
    static constexpr const char* kListOverlap = "packed in, BGR out has no in-place form: an image overlaps its own input frame";
    static void count_call(mi_ctx*, bool) {}
    static void count_list(mi_ctx* c, int n_frames, unsigned long long n_wide)
    {
        c->packed422_bgr_list_frames_wide += n_wide;
        c->packed422_bgr_list_frames_bytes += (unsigned long long)n_frames - n_wide;
    }
};

// Everything is checked before anything is enqueued.  The input side, the shape and the format are check_packed422's own checks (run on
// the input alone); the image side adds the order, the pitch and -- as check_nv12_bgr does -- the tile grids and heights the stage
// sequences would refuse only after their first launch.  No alignment rule on the image side.  *work = false: MI_OK with nothing to do.
template <class F>
mi_status check_packed422_bgr(mi_ctx* c, const P422BgrArgs& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    bool in_work = false;
    const mi_status st = check_packed422(c, a.in, is_clahe, tiles_x, tiles_y, &in_work);
    if (st || !in_work) return st;
    if (!a.out) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
    if (a.out_pitch < F::kPx * (size_t)a.in.width) return fail(c, MI_ERR_BAD_ARG, F::kOutPitch);
    if (a.out == a.in.in) return fail(c, MI_ERR_BAD_ARG, F::kInPlace);
    if (is_clahe) {
        ClaheGeom g;
        if (mi_status gs = clahe_geometry(c, a.in.width, a.in.height, 0.0, tiles_x, tiles_y, &g)) return gs;
        if (tiles_x * tiles_y > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "more than 65535 tiles per frame");
        if (tiles_x + 1 > kMaxPairsLds && a.in.height > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "height > 65535 with tiles_x > 62");
    }
    *work = true;
    return MI_OK;
}

// `wide`: the one store-path rule of both image forms (packed422_image_wide, kernels/packed422_bgr.hip.h) on the block's own numbers;
// a table launch comes with a null image base and frame stride 0, which leave it to out_pitch % 4 == 0, and every frame adds its own
// address in the kernel
template <class F>
typename F::Block packed422_bgr_batch(const P422BgrArgs& a, int f0)
{
    typename F::Block p;
    p.src = a.in.in + (size_t)f0 * a.in.in_frame; p.out = a.out + (size_t)f0 * a.out_frame;
    p.src_step = (long long)a.in.in_pitch; p.out_step = (long long)a.out_pitch;
    p.src_frame = (long long)a.in.in_frame; p.out_frame = (long long)a.out_frame;
    p.dwords = a.in.width / 2; p.rows = a.in.height;
    p.wide = packed422_image_wide(a.out, p.out_step, p.out_frame) ? 1 : 0;
    return p;
}

// The writer of the stage sequences of packed422.inc.hpp that decodes the new luma with the row's own chroma into the pixels of form
// F, first channel B (ORDER 0) or R (ORDER 1).  Its frame list is the packed forms' own {in, out} table (packed422_bgr_frames.inc.hpp
// fills it).
template <class F, int ORDER> struct BgrOut {
    using Args = P422BgrArgs;
    using Block = typename F::Block;
    using List = Packed422List;
    static const P422Args& input(const Args& a) { return a.in; }
    static Block cut(const Args& a, int f0) { return packed422_bgr_batch<F>(a, f0); }
    static int apply_rows(int height) { return height; }
    template <int OFF> using K = typename F::template K<OFF, ORDER>;
};

// fl_in / fl_out: a chunk of a frame list (both or neither, see packed422.inc.hpp)
template <class F>
mi_status packed422_bgr_dev(mi_ctx* c, hipStream_t s, const P422BgrArgs& a, int op, double clip_limit, int tiles_x, int tiles_y,
                            const Packed422List* fl_in = nullptr, const Packed422List* fl_out = nullptr)
{
    return a.order == MI_ORDER_RGB ? packed422_dev<BgrOut<F, 1>>(c, s, a, op, clip_limit, tiles_x, tiles_y, fl_in, fl_out)
                                   : packed422_dev<BgrOut<F, 0>>(c, s, a, op, clip_limit, tiles_x, tiles_y, fl_in, fl_out);
}

// A batch (or the host form's device frame): enqueue, then the form's count of the call by the store path of its launches
template <class F>
mi_status packed422_bgr_call(mi_ctx* c, hipStream_t s, const P422BgrArgs& a, int op, double clip_limit, int tiles_x, int tiles_y)
{
    const mi_status st = packed422_bgr_dev<F>(c, s, a, op, clip_limit, tiles_x, tiles_y);
    if (st) return st;
    F::count_call(c, packed422_image_wide(a.out, (long long)a.out_pitch, (long long)a.out_frame));
    return MI_OK;
}

// The host form's checks: the input side and the shape are the device form's (on the caller's input and a stand-in image); the output
// side is host memory the kernels never see -- any address, any out_step >= kPx * W -- whose rows may not meet the input's.
template <class F>
mi_status check_packed422_bgr_host(mi_ctx* c, const P422BgrArgs& h, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    P422BgrArgs shape = h;
    shape.out = h.out ? (uint8_t*)16 : nullptr;
    shape.out_pitch = F::kPx * (size_t)std::max(h.in.width, 0); shape.out_frame = 0;
    bool any = false;
    const mi_status st = check_packed422_bgr<F>(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)h.in.width, rows = (size_t)h.in.height;
    if (h.out_pitch < F::kPx * w) return fail(c, MI_ERR_BAD_ARG, F::kOutStep);
    if ((long long)h.in.width * h.in.height > 0x7fffffffLL / F::kPx) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    if (Span(h.out, h.out_pitch, F::kPx * w, rows).meets(Span(h.in.in, h.in.in_pitch, 2 * w, rows)))
        return fail(c, MI_ERR_BAD_ARG, F::kHostOverlap);
    *work = true;
    return MI_OK;
}

// Host frame: the packed frame goes up tight (2 B/px), the image comes back tight (kPx B/px); pinned tight buffers are DMA'd as they
// are, anything else goes through the context's pinned staging (stage_in / stage_out, which drain the stream on every error exit).
// Only the 2 * W bytes of each input row are read and the kPx * W bytes of each output row written.  The device image is tight at an
// aligned allocation: with 4 B/px always the wide store path, whatever the caller's address and out_step are.
template <class F>
mi_status packed422_bgr_host(mi_ctx* c, const P422BgrArgs& h, int op, double clip_limit, int tiles_x, int tiles_y)
{
    const size_t w = (size_t)h.in.width, rows = (size_t)h.in.height;
    const size_t in_row = 2 * w, in_bytes = in_row * rows, out_row = F::kPx * w, out_bytes = out_row * rows;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = stage_in(c, s, h.in.in, h.in.in_pitch, in_row, rows, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    const P422BgrArgs d = p422_bgr_args(c->d_stage_in, in_row, in_bytes, c->d_stage_out, out_row, out_bytes,
                                        h.in.width, h.in.height, 1, h.in.format, h.order);
    if ((st = packed422_bgr_call<F>(c, s, d, op, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, out_row, rows, drain);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_bgr_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                      void* d_out, size_t out_pitch, size_t out_frame_stride,
                                                      int width, int height, int n_frames, int format, int order, void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs a = p422_bgr_args(d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr<Bgr422Image>(c, a, false, 0, 0, &work);
    return (st || !work) ? st : packed422_bgr_call<Bgr422Image>(c, pick_stream(c, stream), a, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_bgr_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                              void* d_out, size_t out_pitch, size_t out_frame_stride,
                                              int width, int height, int n_frames, int format, int order,
                                              double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs a = p422_bgr_args(d_in, in_pitch, in_frame_stride, d_out, out_pitch, out_frame_stride, width, height, n_frames, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr<Bgr422Image>(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_bgr_call<Bgr422Image>(c, pick_stream(c, stream), a, 1, clip_limit, tiles_x, tiles_y);
}

mi_status mi_equalize_hist_packed422_to_bgr(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
                                            int width, int height, int format, int order)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs h = p422_bgr_args(in, in_pitch, 0, out, out_step, 0, width, height, 1, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr_host<Bgr422Image>(c, h, false, 0, 0, &work);
    return (st || !work) ? st : packed422_bgr_host<Bgr422Image>(c, h, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_bgr(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step,
                                    int width, int height, int format, int order, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    const P422BgrArgs h = p422_bgr_args(in, in_pitch, 0, out, out_step, 0, width, height, 1, format, order);
    bool work = false;
    const mi_status st = check_packed422_bgr_host<Bgr422Image>(c, h, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_bgr_host<Bgr422Image>(c, h, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
