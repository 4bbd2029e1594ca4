// bgr_nv12.inc.hpp -- interleaved 8-bit BGR / RGB images in, pitched NV12 frames out with the luma equalized: checks, launch sequences, extern "C"
// Included by ../mi_lumaeq.hip (one translation unit; not a stand-alone header).
//
// renderer / model output / image reader -> equalize -> encoder without an I420 intermediate and without an interleave outside the
// library.  Y is not in the input, so the order of nv12_bgr.inc.hpp is turned round: stage 1 (kernels/bgr_nv12.hip.h) converts into the
// caller's pitched planes and, for equalizeHist, counts the luma it writes into the partials equalize_lut_kernel reads; stage 2 is the
// planar forms' own in place on the output Y plane (launch_apply / clahe_dev with src == dst and no chroma job).  Never the fused kernel
// and never hist_lut_kernel: option two_kernel_max_frames does not apply.  CLAHE has no one-pass / two-pass split and no scratch plane:
// every shape the planar form takes runs the planar form's kernels.

namespace {

// frames per launch sequence, as kNv12BgrFramesPerLaunch: bounds the grids and the partials of a sequence
constexpr int kBgrNv12FramesPerLaunch = 256;

struct BgrNv12Args {
    const uint8_t* in; size_t in_pitch, in_frame;
    uint8_t* y; size_t y_pitch;
    uint8_t* uv; size_t uv_pitch;
    size_t out_frame;
    int width, height, n_frames, order;
    mi_uv_mode uv_mode;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.
mi_status check_bgr_nv12(mi_ctx* c, const BgrNv12Args& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.uv_mode != MI_UV_FILL128 && a.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "NV12 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.in || !a.y || !a.uv) return fail(c, MI_ERR_BAD_ARG, "null image or plane pointer");
    if (a.in_pitch < 3 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "in_pitch < 3 * width");
    if (a.y_pitch < (size_t)a.width || a.uv_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "NV12 pitch < width");
    if (a.y == a.in || a.uv == a.in || a.y == a.uv) return fail(c, MI_ERR_BAD_ARG, "BGR in, NV12 out has no in-place form");
    // the planar forms' limits (check_plane), with their status
    if ((long long)a.width * a.height > 0x7fffffffLL) return fail(c, MI_ERR_UNSUPPORTED, "width*height must be < 2^31 (OpenCV: int total)");
    if (a.width > (1 << 24) || a.height > (1 << 24)) return fail(c, MI_ERR_UNSUPPORTED, "width/height must be <= 2^24");
    if (is_clahe) {
        ClaheGeom g;
        if (mi_status st = clahe_geometry(c, a.width, a.height, 0.0, tiles_x, tiles_y, &g)) return st;
        if (tiles_x * tiles_y > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "more than 65535 tiles per frame");
        if (tiles_x + 1 > kMaxPairsLds && a.height > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "height > 65535 with tiles_x > 62");
    }
    *work = true;
    return MI_OK;
}

// Stage 1 on frames f0 .. f0 + nf of the call (MI_K_COLOR).  hist: count the luma into c->d_partial, *nparts_out workgroups a frame.
// With a frame table (fl: one chunk of at most kFramesPerLaunch frames, bgr_nv12_frames.inc.hpp): the same grid on the
// *_frames_kernel entry; `a` then carries the shape, its base pointers (stand-ins for the vec rule) and frame strides are not used by
// the kernel, and j.vec says what the shape allows -- a byte-path frame of such a launch simply takes more grid-stride steps.
mi_status launch_bgr_to_nv12(mi_ctx* c, hipStream_t s, const BgrNv12Args& a, int f0, int nf, bool hist, int* nparts_out,
                             const BgrNv12List* fl = nullptr)
{
    BgrNv12Job j{};
    j.in = a.in + (size_t)f0 * a.in_frame; j.y = a.y + (size_t)f0 * a.out_frame; j.uv = a.uv + (size_t)f0 * a.out_frame;
    j.in_step = (long long)a.in_pitch; j.y_step = (long long)a.y_pitch; j.uv_step = (long long)a.uv_pitch;
    j.in_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = a.width % 16 == 0 &&
            (((uintptr_t)a.in | (uintptr_t)a.y | (uintptr_t)a.uv | a.in_pitch | a.y_pitch | a.uv_pitch | a.in_frame | a.out_frame) & 15) == 0;
    const long long px = (long long)a.width * a.height;
    // the byte basis and the cap of launch_nv12_to_bgr: half of what is read and written (3 + 1.5 B/px); in 16 x 2 groups a workgroup
    // pass covers 8192 pixels, in 2 x 2 blocks 1024
    int B = blocks_per_frame(c, px * 9 / 4, a.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    if (hist) {
        if (mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t))) return st;
    }
    const dim3 grid(B, nf), block(kThreads);
    const bool rgb = a.order == MI_ORDER_RGB, cp = a.uv_mode == MI_UV_COPY;
#define MI_BGR_NV12_LAUNCH(O, U)                                                                                                     \
    do {                                                                                                                             \
        if (fl && hist) LAUNCH(c, s, MI_K_COLOR, (bgr_to_nv12_hist_frames_kernel<O, U, true>), grid, block, 0, j, *fl, c->d_partial);   \
        else if (fl)    LAUNCH(c, s, MI_K_COLOR, (bgr_to_nv12_hist_frames_kernel<O, U, false>), grid, block, 0, j, *fl, (uint32_t*)nullptr); \
        else if (hist)  LAUNCH(c, s, MI_K_COLOR, (bgr_to_nv12_hist_kernel<O, U, true>), grid, block, 0, j, c->d_partial);              \
        else            LAUNCH(c, s, MI_K_COLOR, (bgr_to_nv12_hist_kernel<O, U, false>), grid, block, 0, j, (uint32_t*)nullptr);       \
    } while (0)
    if (rgb && cp) MI_BGR_NV12_LAUNCH(1, 1);
    else if (rgb)  MI_BGR_NV12_LAUNCH(1, 0);
    else if (cp)   MI_BGR_NV12_LAUNCH(0, 1);
    else           MI_BGR_NV12_LAUNCH(0, 0);
#undef MI_BGR_NV12_LAUNCH
    if (nparts_out) *nparts_out = B;
    return MI_OK;
}

// The output Y plane as the planar stage launchers see it: source and destination at once
PlaneArgs bgr_nv12_y_plane(const BgrNv12Args& a, int f0, int nf)
{
    uint8_t* y = a.y + (size_t)f0 * a.out_frame;
    return PlaneArgs{y, a.y_pitch, a.out_frame, y, a.y_pitch, a.out_frame, a.width, a.height, nf};
}

// per chunk: one MI_K_COLOR (convert + count), one MI_K_EQ_LUT, one MI_K_LUT_APPLY (in place on Y); no MI_K_HIST
mi_status equalize_bgr_nv12_dev(mi_ctx* c, hipStream_t s, const BgrNv12Args& a)
{
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_bgr_to_nv12(c, s, a, f0, nf, true, &nparts);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        if ((st = launch_apply(c, s, bgr_nv12_y_plane(a, f0, nf), 0, nf, c->d_luts, nullptr))) return st;
    }
    return MI_OK;
}

// per chunk: one MI_K_COLOR (convert), then what mi_clahe_u8_batch_dev launches for the same plane, in place
mi_status clahe_bgr_nv12_dev(mi_ctx* c, hipStream_t s, const BgrNv12Args& a, double clip_limit, int tiles_x, int tiles_y)
{
    for (int f0 = 0; f0 < a.n_frames; f0 += kBgrNv12FramesPerLaunch) {
        const int nf = std::min(kBgrNv12FramesPerLaunch, a.n_frames - f0);
        mi_status st = launch_bgr_to_nv12(c, s, a, f0, nf, false, nullptr);
        if (st) return st;
        if ((st = clahe_dev(c, s, bgr_nv12_y_plane(a, f0, nf), clip_limit, tiles_x, tiles_y, nullptr))) return st;
    }
    return MI_OK;
}

// One CV_8UC3 host image up (3 B/px), one tight NV12 frame back (1.5 B/px), staged as nv12_bgr_host stages its two: stage_in takes the
// pitched image, the device form writes a tight frame into d_stage_out, stage_out copies it as ONE row of W*H*3/2 bytes; every error
// exit after the first copy on caller memory drains the stream first.
mi_status bgr_nv12_host(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* nv12_out, int width, int height, int order,
                        mi_uv_mode uv_mode, bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    // (the output is one tight frame: its Y plane stands for the frame in the checks, the UV plane is never null with it)
    const size_t wz = (size_t)std::max(width, 0), ysz_chk = wz * (size_t)std::max(height, 0);
    const BgrNv12Args a{in, in_step, 0, nv12_out, wz, nv12_out ? nv12_out + ysz_chk : nullptr, wz, 0, width, height, 1, order, uv_mode};
    bool work = false;
    mi_status st = check_bgr_nv12(c, a, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    if ((long long)width * height > 0x7fffffffLL / 3) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    const size_t ysz = (size_t)width * height, row = 3 * (size_t)width, out_bytes = ysz * 3 / 2;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    if ((st = stage_in(c, s, in, in_step, row, (size_t)height, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    const BgrNv12Args d{c->d_stage_in, row, row * height, c->d_stage_out, (size_t)width, c->d_stage_out + ysz, (size_t)width, out_bytes,
                        width, height, 1, order, uv_mode};
    st = is_clahe ? clahe_bgr_nv12_dev(c, s, d, clip_limit, tiles_x, tiles_y) : equalize_bgr_nv12_dev(c, s, d);
    if (st) return st;
    return stage_out(c, s, nv12_out, out_bytes, out_bytes, 1, drain);
}

BgrNv12Args bgr_nv12_args(const void* d_in, size_t in_pitch, size_t in_frame, void* d_y, size_t y_pitch, void* d_uv, size_t uv_pitch,
                          size_t out_frame, int width, int height, int n_frames, int order, mi_uv_mode uv_mode)
{
    return BgrNv12Args{(const uint8_t*)d_in, in_pitch, in_frame, (uint8_t*)d_y, y_pitch, (uint8_t*)d_uv, uv_pitch, out_frame,
                       width, height, n_frames, order, uv_mode};
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_bgr_to_nv12_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                 void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
                                                 int width, int height, int n_frames, int order, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrNv12Args a = bgr_nv12_args(d_in, in_pitch, in_frame_stride, d_y_out, y_pitch, d_uv_out, uv_pitch, out_frame_stride,
                                        width, height, n_frames, order, uv_mode);
    bool work = false;
    const mi_status st = check_bgr_nv12(c, a, false, 0, 0, &work);
    return (st || !work) ? st : equalize_bgr_nv12_dev(c, pick_stream(c, stream), a);
}

mi_status mi_clahe_bgr_to_nv12_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                         void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
                                         int width, int height, int n_frames, int order, mi_uv_mode uv_mode,
                                         double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const BgrNv12Args a = bgr_nv12_args(d_in, in_pitch, in_frame_stride, d_y_out, y_pitch, d_uv_out, uv_pitch, out_frame_stride,
                                        width, height, n_frames, order, uv_mode);
    bool work = false;
    const mi_status st = check_bgr_nv12(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : clahe_bgr_nv12_dev(c, pick_stream(c, stream), a, clip_limit, tiles_x, tiles_y);
}

mi_status mi_equalize_hist_bgr_to_nv12(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* nv12_out,
                                       int width, int height, int order, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return bgr_nv12_host(c, in, in_step, nv12_out, width, height, order, uv_mode, false, 0.0, 0, 0);
}

mi_status mi_clahe_bgr_to_nv12(mi_ctx* c, const uint8_t* in, size_t in_step, uint8_t* nv12_out,
                               int width, int height, int order, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return bgr_nv12_host(c, in, in_step, nv12_out, width, height, order, uv_mode, true, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
