// yuv420.inc.hpp -- 8-bit 4:2:0 frames whose sides say where their planes lie (mi_*_yuv420*): I420 / YV12 / NV12 in, any of them out:
// checks, chunking, the two device entry points and the two host forms, extern "C"  (the frame-list form: yuv420_frames.inc.hpp)
// Included by ../mi_lumaeq.hip behind bgr_nv12_frames.inc.hpp (one translation unit; not a stand-alone header).
//
// software decoder (three planes, linesize[3]) -> equalize -> hardware encoder surface (NV12), or the other way round, without plane
// copies or an interleave outside the library.  The luma is the planar forms' own: equalize_dev / clahe_dev on the Y planes, with
// whatever path they choose for the batch.  The chroma is one launch of yuv420_chroma_kernel (kernels/yuv420.hip.h) per chunk of
// kYuv420FramesPerLaunch frames, charged to MI_K_LUT_APPLY like uv_kernel and p010_uv_kernel.

namespace {

// frames per chroma launch, as kBgrNv12FramesPerLaunch: bounds the grid of a launch
constexpr int kYuv420FramesPerLaunch = 256;

struct Yuv420Args {
    mi_yuv420_planes in, out;
    int width, height, n_frames;
    mi_uv_mode uv_mode;
};

inline size_t yuv420_chroma_row(const mi_yuv420_planes& p, int width)
{
    return p.chroma == MI_CHROMA_PLANAR ? (size_t)width / 2 : (size_t)width;
}

// check_yuv420 in its three parts, in the order it applies them; the list form (yuv420_frames.inc.hpp) applies the first and the last
// once per call and the middle one per frame.
// 1. What does not depend on where the planes lie.  *any = false: MI_OK with nothing to do.
mi_status check_yuv420_call(mi_ctx* c, int in_chroma, int out_chroma, int width, int height, int n_frames, mi_uv_mode uv_mode,
                            bool is_clahe, int tiles_x, int tiles_y, bool* any)
{
    *any = false;
    for (const int chroma : {in_chroma, out_chroma})
        if (chroma != MI_CHROMA_INTERLEAVED && chroma != MI_CHROMA_PLANAR)
            return fail(c, MI_ERR_BAD_ARG, "chroma must be MI_CHROMA_INTERLEAVED or MI_CHROMA_PLANAR");
    if (uv_mode != MI_UV_FILL128 && uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (width < 0 || height < 0 || n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((width & 1) || (height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    *any = width != 0 && height != 0 && n_frames != 0;
    return MI_OK;
}

// 2. The planes of one frame (of every frame of a batch): pointers, pitches, the planes that may not share an address.
// same_stride: both sides step from frame to frame alike (host frames, list entries: there is no frame stride).
mi_status check_yuv420_planes(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out, int width, mi_uv_mode uv_mode,
                              bool same_stride)
{
    const bool copy = uv_mode == MI_UV_COPY, in_planar = in->chroma == MI_CHROMA_PLANAR, out_planar = out->chroma == MI_CHROMA_PLANAR;
    if (!in->y || !out->y) return fail(c, MI_ERR_BAD_ARG, "null Y plane pointer");
    if (!out->c0 || (out_planar && !out->c1)) return fail(c, MI_ERR_BAD_ARG, "null output chroma plane pointer");
    if (copy && (!in->c0 || (in_planar && !in->c1))) return fail(c, MI_ERR_BAD_ARG, "MI_UV_COPY needs the input chroma planes");
    if (in->y_pitch < (size_t)width || out->y_pitch < (size_t)width) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (out->c_pitch < yuv420_chroma_row(*out, width) || (copy && in->c_pitch < yuv420_chroma_row(*in, width)))
        return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width interleaved, width / 2 planar)");
    // the planes that take part in the call: with MI_UV_FILL128 the input's chroma is not read and its descriptor fields are ignored
    const void* ip[3] = {in->y, copy ? in->c0 : nullptr, copy && in_planar ? in->c1 : nullptr};
    const void* op[3] = {out->y, out->c0, out_planar ? out->c1 : nullptr};
    if (op[0] == op[1] || (op[2] && (op[2] == op[0] || op[2] == op[1]))) return fail(c, MI_ERR_BAD_ARG, "two output planes at one address");
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < 3; ++i) {
            if (!op[o] || op[o] != ip[i]) continue;
            // in place: exactly the same plane on both sides
            const bool same = o == i && same_stride &&
                              (o == 0 ? in->y_pitch == out->y_pitch : in->chroma == out->chroma && in->c_pitch == out->c_pitch);
            if (!same) return fail(c, MI_ERR_BAD_ARG, "an output plane at the address of an input plane that is not exactly the same plane");
        }
    return MI_OK;
}

// 3. The planar forms' limits (check_plane), with their status.
mi_status check_yuv420_limits(mi_ctx* c, int width, int height, bool is_clahe, int tiles_x, int tiles_y)
{
    if ((long long)width * height > 0x7fffffffLL) return fail(c, MI_ERR_UNSUPPORTED, "width*height must be < 2^31 (OpenCV: int total)");
    if (width > (1 << 24) || height > (1 << 24)) return fail(c, MI_ERR_UNSUPPORTED, "width/height must be <= 2^24");
    if (is_clahe) {
        ClaheGeom g;
        if (mi_status st = clahe_geometry(c, width, height, 0.0, tiles_x, tiles_y, &g)) return st;
        if (tiles_x * tiles_y > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "more than 65535 tiles per frame");
        if (tiles_x + 1 > kMaxPairsLds && height > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "height > 65535 with tiles_x > 62");
    }
    return MI_OK;
}

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.  host: one frame, frame_stride ignored.
mi_status check_yuv420(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out, int width, int height, int n_frames,
                       mi_uv_mode uv_mode, bool host, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (!in || !out) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    bool any = false;
    mi_status st = check_yuv420_call(c, in->chroma, out->chroma, width, height, n_frames, uv_mode, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    if ((st = check_yuv420_planes(c, in, out, width, uv_mode, host || in->frame_stride == out->frame_stride))) return st;
    if ((st = check_yuv420_limits(c, width, height, is_clahe, tiles_x, tiles_y))) return st;
    *work = true;
    return MI_OK;
}

// The chroma of the call's frames: one launch per chunk (MI_K_LUT_APPLY); none at all when every chroma plane is copied in place.
mi_status yuv420_chroma_dev(mi_ctx* c, hipStream_t s, const Yuv420Args& a)
{
    const bool copy = a.uv_mode == MI_UV_COPY, in_planar = a.in.chroma == MI_CHROMA_PLANAR, out_planar = a.out.chroma == MI_CHROMA_PLANAR;
    Yuv420Job j{};
    j.out = Yuv420Side{(uint8_t*)a.out.c0, out_planar ? (uint8_t*)a.out.c1 : nullptr, (long long)a.out.c_pitch, (long long)a.out.frame_stride,
                       out_planar ? 1 : 0};
    if (copy) j.in = Yuv420Side{(uint8_t*)a.in.c0, in_planar ? (uint8_t*)a.in.c1 : nullptr, (long long)a.in.c_pitch,
                                (long long)a.in.frame_stride, in_planar ? 1 : 0};
    j.width = a.width; j.rows = a.height / 2; j.mode = copy ? 1 : 0;
    const bool relayout = copy && in_planar != out_planar;
    const size_t row = yuv420_chroma_row(a.out, a.width);
    if (relayout) {
        const uintptr_t bits = (uintptr_t)j.in.c0 | (uintptr_t)j.in.c1 | (uintptr_t)j.out.c0 | (uintptr_t)j.out.c1 |
                               a.in.c_pitch | a.out.c_pitch | a.in.frame_stride | a.out.frame_stride;
        j.vec = a.width % 32 == 0 && (bits & 15) == 0;
    } else {
        j.flat = j.rows == 1 || (a.out.c_pitch == row && (!copy || a.in.c_pitch == row));
        if (copy) {                                                  // check_yuv420: an equal address is exactly the same plane
            j.skip0 = j.in.c0 == j.out.c0;
            j.skip1 = out_planar && j.in.c1 == j.out.c1;
            if (j.skip0 && (j.skip1 || !out_planar)) return MI_OK;
        }
    }
    const long long bytes = (long long)a.width * j.rows * (copy ? 2 : 1);       // read + written per frame
    for (int f0 = 0; f0 < a.n_frames; f0 += kYuv420FramesPerLaunch) {
        const int nf = std::min(kYuv420FramesPerLaunch, a.n_frames - f0);
        Yuv420Job k = j;
        for (Yuv420Side* sd : {&k.in, &k.out}) {
            if (sd->c0) sd->c0 += (long long)f0 * sd->frame;
            if (sd->c1) sd->c1 += (long long)f0 * sd->frame;
        }
        const int B = blocks_per_frame(c, bytes, j.rows, nf, 2048);
        LAUNCH(c, s, MI_K_LUT_APPLY, yuv420_chroma_kernel, dim3(B, nf), dim3(kThreads), 0, k);
    }
    ++((relayout && !j.vec) ? c->yuv420_chroma_bytes : c->yuv420_chroma_vec);
    return MI_OK;
}

PlaneArgs yuv420_y_plane(const Yuv420Args& a)
{
    return PlaneArgs{(const uint8_t*)a.in.y, a.in.y_pitch, a.in.frame_stride, (uint8_t*)a.out.y, a.out.y_pitch, a.out.frame_stride,
                     a.width, a.height, a.n_frames};
}

// op: 0 equalizeHist, 1 CLAHE.  The luma exactly as mi_*_u8_batch_dev enqueues it for the Y planes, then the chroma.
mi_status yuv420_dev(mi_ctx* c, hipStream_t s, const Yuv420Args& a, int op, double clip_limit, int tiles_x, int tiles_y)
{
    const PlaneArgs y = yuv420_y_plane(a);
    const mi_status st = op ? clahe_dev(c, s, y, clip_limit, tiles_x, tiles_y, nullptr) : equalize_dev(c, s, y, nullptr);
    return st ? st : yuv420_chroma_dev(c, s, a);
}

// One plane of the caller's frame up into the staged device frame at d_dst (tight rows): a pinned tight plane is DMA'd as it is,
// anything else is packed into the context's pinned staging at h_stage first.  (h_pin_in has been grown for the whole frame.)
mi_status yuv420_plane_in(mi_ctx* c, hipStream_t s, const void* src, size_t pitch, size_t w, size_t rows, uint8_t* d_dst,
                          uint8_t* h_stage, StreamDrain& drain)
{
    const bool direct = (pitch == w || rows == 1) && host_range_pinned(src, w * rows, &c->pin_neg);
    ++(direct ? c->planes_direct : c->planes_staged);
    if (!direct) copy_rows(h_stage, w, (const uint8_t*)src, pitch, (int)w, (int)rows);
    drain.watch(s);
    HIPCHK(c, hipMemcpyAsync(d_dst, direct ? src : h_stage, w * rows, hipMemcpyHostToDevice, s));
    return MI_OK;
}

// Host frame: every plane goes up tight into d_stage_in (Y, then the chroma planes in the input's layout; no chroma with
// MI_UV_FILL128), the device form runs on tight frames -- the kernels' own pitches, so W % 32 == 0 takes the 16-byte chroma path
// whatever the caller's addresses are -- and the planes of the output's layout come back from d_stage_out as PlaneOut
// (packed422_nv12_frames.inc.hpp) carries them.  `h` holds the caller's pointers and pitches; it has passed the checks.
mi_status yuv420_host(mi_ctx* c, const Yuv420Args& h, int op, double clip_limit, int tiles_x, int tiles_y)
{
    if ((long long)h.width * h.height > 0x7fffffffLL / 3) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    const size_t w = (size_t)h.width, rows = (size_t)h.height, ysz = w * rows, frame = ysz * 3 / 2, csz = ysz / 4;
    const bool copy = h.uv_mode == MI_UV_COPY, in_planar = h.in.chroma == MI_CHROMA_PLANAR, out_planar = h.out.chroma == MI_CHROMA_PLANAR;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = grow_dev(c, &c->d_stage_in, &c->stage_in_bytes, frame))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, frame))) return st;
    if ((st = grow_pinned(c, &c->h_pin_in, &c->pin_in_bytes, frame))) return st;
    if ((st = grow_pinned(c, &c->h_pin_out, &c->pin_out_bytes, frame))) return st;
    uint8_t* const di = c->d_stage_in; uint8_t* const dout = c->d_stage_out;
    if ((st = yuv420_plane_in(c, s, h.in.y, h.in.y_pitch, w, rows, di, c->h_pin_in, drain))) return st;
    if (copy && in_planar) {
        if ((st = yuv420_plane_in(c, s, h.in.c0, h.in.c_pitch, w / 2, rows / 2, di + ysz, c->h_pin_in + ysz, drain))) return st;
        if ((st = yuv420_plane_in(c, s, h.in.c1, h.in.c_pitch, w / 2, rows / 2, di + ysz + csz, c->h_pin_in + ysz + csz, drain))) return st;
    } else if (copy) {
        if ((st = yuv420_plane_in(c, s, h.in.c0, h.in.c_pitch, w, rows / 2, di + ysz, c->h_pin_in + ysz, drain))) return st;
    }
    Yuv420Args d = h;
    d.n_frames = 1;
    d.in = mi_yuv420_planes{di, w, copy ? di + ysz : nullptr, copy && in_planar ? di + ysz + csz : nullptr, in_planar ? w / 2 : w, frame,
                            h.in.chroma};
    d.out = mi_yuv420_planes{dout, w, dout + ysz, out_planar ? dout + ysz + csz : nullptr, out_planar ? w / 2 : w, frame, h.out.chroma};
    if ((st = yuv420_dev(c, s, d, op, clip_limit, tiles_x, tiles_y))) return st;
    const PlaneOut py(c, (uint8_t*)h.out.y, h.out.y_pitch, w, w, rows);
    const PlaneOut p0 = out_planar ? PlaneOut(c, (uint8_t*)h.out.c0, h.out.c_pitch, w / 2, w / 2, rows / 2)
                                   : PlaneOut(c, (uint8_t*)h.out.c0, h.out.c_pitch, w, w, rows / 2);
    const PlaneOut p1 = out_planar ? PlaneOut(c, (uint8_t*)h.out.c1, h.out.c_pitch, w / 2, w / 2, rows / 2) : p0;   // planar outputs only
    drain.watch(s);
    if ((st = enqueue_plane_out(c, s, dout, c->h_pin_out, py))) return st;
    if ((st = enqueue_plane_out(c, s, dout + ysz, c->h_pin_out + ysz, p0))) return st;
    if (out_planar && (st = enqueue_plane_out(c, s, dout + ysz + csz, c->h_pin_out + ysz + csz, p1))) return st;
    HIPCHK(c, hipStreamSynchronize(s));
    drain.done();
    copy_plane_out(py, c->h_pin_out);
    copy_plane_out(p0, c->h_pin_out + ysz);
    if (out_planar) copy_plane_out(p1, c->h_pin_out + ysz + csz);
    return MI_OK;
}

mi_status yuv420_entry(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out, int width, int height, int n_frames,
                       mi_uv_mode uv_mode, bool host, int op, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    bool work = false;
    const mi_status st = check_yuv420(c, in, out, width, height, n_frames, uv_mode, host, op != 0, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    const Yuv420Args a{*in, *out, width, height, n_frames, uv_mode};
    return host ? yuv420_host(c, a, op, clip_limit, tiles_x, tiles_y)
                : yuv420_dev(c, pick_stream(c, stream), a, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
                                            int width, int height, int n_frames, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_entry(c, in, out, width, height, n_frames, uv_mode, false, 0, 0.0, 0, 0, stream);
}

mi_status mi_clahe_yuv420_batch_dev(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
                                    int width, int height, int n_frames, mi_uv_mode uv_mode,
                                    double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return yuv420_entry(c, in, out, width, height, n_frames, uv_mode, false, 1, clip_limit, tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_yuv420(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
                                  int width, int height, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return yuv420_entry(c, in, out, width, height, 1, uv_mode, true, 0, 0.0, 0, 0, nullptr);
}

mi_status mi_clahe_yuv420(mi_ctx* c, const mi_yuv420_planes* in, const mi_yuv420_planes* out,
                          int width, int height, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return yuv420_entry(c, in, out, width, height, 1, uv_mode, true, 1, clip_limit, tiles_x, tiles_y, nullptr);
}

}  // extern "C"
