// packed422_nv12_frames.inc.hpp -- packed 4:2:2 in, NV12 out on frames given one by one: a LIST of device frames
// (mi_*_packed422_to_nv12_frames_dev) and ONE host frame (mi_*_packed422_to_nv12): checks, chunking, staging, extern "C"
// Included by ../mi_lumaeq.hip after packed422_nv12.inc.hpp (one translation unit; not a stand-alone header).
//
// Neither end of a capture -> encoder pipeline is one allocation at a fixed frame stride: the capture card hands out a buffer pool
// (packed422_frames.inc.hpp), the encoder takes a surface pool whose surfaces have a pitched Y and UV plane each
// (nv12_frames.inc.hpp).  The list form joins the two: the call is cut into chunks of at most kPacked422FramesPerLaunch and
// kPacked422Nv12FramesPerLaunch frames; a chunk's inputs travel to the histogram stages as a Packed422List, its {in, y, uv} triples to
// the writers as a Packed422Nv12List, both by value in the kernel arguments, through the stage sequences of packed422_nv12.inc.hpp --
// same grids, same tile splits, same bytes as the batch form.
// The host form stages one frame through the context's buffers (2 B/px up, 1.5 B/px back) around the same sequences.

namespace {

struct P422Nv12FramesShape {
    int width, height;
    size_t in_pitch, y_pitch, uv_pitch;
    int format;
    mi_uv_mode uv_mode;
};

// all stages of a chunk see the same frames: both tables are cut by the smaller one
constexpr int kP422Nv12Chunk = kPacked422FramesPerLaunch < kPacked422Nv12FramesPerLaunch ? kPacked422FramesPerLaunch : kPacked422Nv12FramesPerLaunch;

// There is no in-place form (the layouts differ): the rows of a frame's planes may meet neither its input's rows nor each other's.
mi_status check_p422_nv12_disjoint(mi_ctx* c, const void* in, const void* y, const void* uv, const P422Nv12FramesShape& s)
{
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    const Span si(in, s.in_pitch, 2 * w, rows), sy(y, s.y_pitch, w, rows), su(uv, s.uv_pitch, w, rows / 2);
    if (sy.meets(si) || su.meets(si)) return fail(c, MI_ERR_BAD_ARG, "packed in, NV12 out has no in-place form: an output plane overlaps its own input frame");
    if (sy.meets(su)) return fail(c, MI_ERR_BAD_ARG, "the Y plane and the UV plane of a frame overlap");
    return MI_OK;
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_packed422_nv12_frames(mi_ctx* c, const mi_packed422_nv12_frame_dev* frames, int n_frames, const P422Nv12FramesShape& s,
                                      bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_packed422_nv12's own answers (even width and height, format, uv_mode, sizes, tiles, pitches and their multiples
    // of 4, the planar forms' size limits), on stand-in addresses that pass its pointer checks
    const P422Nv12Args shape = p422_nv12_args((const void*)16, s.in_pitch, 0, (void*)32, s.y_pitch, (void*)48, s.uv_pitch, 0,
                                              s.width, s.height, n_frames, s.format, s.uv_mode);
    bool any = false;
    const mi_status st = check_packed422_nv12(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    for (int k = 0; k < n_frames; ++k) {
        const mi_packed422_nv12_frame_dev& f = frames[k];
        if (!f.in || !f.y_out || !f.uv_out) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
        if (((uintptr_t)f.in | (uintptr_t)f.y_out | (uintptr_t)f.uv_out) & 3)
            return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 frame and NV12 plane addresses are multiples of 4");
        if (mi_status d = check_p422_nv12_disjoint(c, f.in, f.y_out, f.uv_out, s)) return d;
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status packed422_nv12_frames_dev(mi_ctx* c, hipStream_t s, const mi_packed422_nv12_frame_dev* frames, int n_frames,
                                    const P422Nv12FramesShape& sh, int op, double clip_limit, int tiles_x, int tiles_y)
{
    for (int f0 = 0; f0 < n_frames; f0 += kP422Nv12Chunk) {
        const int nf = std::min(kP422Nv12Chunk, n_frames - f0);
        Packed422List in{};                                          // this chunk's frames of the list, from index 0: the inputs for the
        Packed422Nv12List io{};                                      // histogram stages, the three addresses of a frame for the writers
        for (int k = 0; k < nf; ++k) {
            const mi_packed422_nv12_frame_dev& f = frames[f0 + k];
            in.f[k] = Packed422Frame{(const uint8_t*)f.in, (uint8_t*)const_cast<void*>(f.in)};         // read-only stages: out mirrors in
            io.f[k] = Packed422Nv12Frame{(const uint8_t*)f.in, (uint8_t*)f.y_out, (uint8_t*)f.uv_out};
        }
        const P422Nv12Args a = p422_nv12_args(io.f[0].in, sh.in_pitch, 0, io.f[0].y, sh.y_pitch, io.f[0].uv, sh.uv_pitch, 0,
                                              sh.width, sh.height, nf, sh.format, sh.uv_mode);
        const mi_status st = packed422_dev<Nv12Out>(c, s, a, op, clip_limit, tiles_x, tiles_y, &in, &io);
        if (st) return st;
    }
    return MI_OK;
}

// One plane of the staged NV12 frame back to the caller: `rows` rows of `w` bytes, on the device at pitch `dev_pitch` from `d_src`.
// A pinned tight plane whose device rows are tight too (W % 4 == 0) is DMA'd as it is; anything else lands in the context's pinned
// staging at `h_stage` and copy_plane_out() moves the rows once the stream has been waited for.
struct PlaneOut {
    uint8_t* dst; size_t pitch;
    size_t dev_pitch, w, rows;
    bool direct;
    PlaneOut(mi_ctx* c, uint8_t* dst_, size_t pitch_, size_t dev_pitch_, size_t w_, size_t rows_)
        : dst(dst_), pitch(pitch_), dev_pitch(dev_pitch_), w(w_), rows(rows_),
          direct(dev_pitch_ == w_ && (pitch_ == w_ || rows_ == 1) && host_range_pinned(dst_, w_ * rows_, &c->pin_neg)) {}
};
mi_status enqueue_plane_out(mi_ctx* c, hipStream_t s, const uint8_t* d_src, uint8_t* h_stage, const PlaneOut& p)
{
    ++(p.direct ? c->planes_direct : c->planes_staged);
    HIPCHK(c, hipMemcpyAsync(p.direct ? p.dst : h_stage, d_src, p.dev_pitch * p.rows, hipMemcpyDeviceToHost, s));
    return MI_OK;
}
void copy_plane_out(const PlaneOut& p, const uint8_t* h_stage)
{
    if (!p.direct) copy_rows(p.dst, p.pitch, h_stage, p.dev_pitch, (int)p.w, (int)p.rows);
}

// Host frame: the packed frame goes up tight (stage_in: pinned tight frames as they are, anything else through the pinned staging),
// the two planes come back from a device NV12 frame at pitch align4(W) -- the kernels' rule, not the caller's: host outputs may lie at
// any address and pitch, a tight W % 4 == 2 frame included.  `h` carries the caller's pointers and pitches; it has passed the checks.
mi_status packed422_nv12_host(mi_ctx* c, const P422Nv12Args& h, int op, double clip_limit, int tiles_x, int tiles_y)
{
    const size_t w = (size_t)h.in.width, rows = (size_t)h.in.height;
    const size_t row = 2 * w, bytes = row * rows;
    const size_t P = (w + 3) & ~(size_t)3, ybytes = P * rows, uvbytes = P * (rows / 2);
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    ++(((h.in.in_pitch == row || rows == 1) && host_range_pinned(h.in.in, bytes, &c->pin_neg)) ? c->planes_direct : c->planes_staged);
    if ((st = stage_in(c, s, h.in.in, h.in.in_pitch, row, rows, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, ybytes + uvbytes))) return st;
    const PlaneOut py(c, h.y, h.y_pitch, P, w, rows), puv(c, h.uv, h.uv_pitch, P, w, rows / 2);
    if (!(py.direct && puv.direct) && (st = grow_pinned(c, &c->h_pin_out, &c->pin_out_bytes, ybytes + uvbytes))) return st;
    const P422Nv12Args d = p422_nv12_args(c->d_stage_in, row, bytes, c->d_stage_out, P, c->d_stage_out + ybytes, P, ybytes + uvbytes,
                                          h.in.width, h.in.height, 1, h.in.format, h.in.uv_mode);
    if ((st = packed422_dev<Nv12Out>(c, s, d, op, clip_limit, tiles_x, tiles_y))) return st;
    drain.watch(s);
    if ((st = enqueue_plane_out(c, s, c->d_stage_out, c->h_pin_out, py))) return st;
    if ((st = enqueue_plane_out(c, s, c->d_stage_out + ybytes, c->h_pin_out + ybytes, puv))) return st;
    HIPCHK(c, hipStreamSynchronize(s));
    drain.done();
    copy_plane_out(py, c->h_pin_out);
    copy_plane_out(puv, c->h_pin_out + ybytes);
    return MI_OK;
}

// The host form's checks: the input side and the shape are the device form's (check_packed422_nv12 on the caller's input and on
// stand-in planes at pitch align4(W)); the output side is host memory the kernels never see -- any address, any pitch >= W.
mi_status check_packed422_nv12_host(mi_ctx* c, const P422Nv12Args& h, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    const size_t P = ((size_t)std::max(h.in.width, 0) + 3) & ~(size_t)3;
    const P422Nv12Args shape = p422_nv12_args(h.in.in, h.in.in_pitch, 0, h.y ? (void*)32 : nullptr, P, h.uv ? (void*)48 : nullptr, P, 0,
                                              h.in.width, h.in.height, 1, h.in.format, h.in.uv_mode);
    bool any = false;
    const mi_status st = check_packed422_nv12(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    if (h.y_pitch < (size_t)h.in.width || h.uv_pitch < (size_t)h.in.width) return fail(c, MI_ERR_BAD_ARG, "NV12 pitch < width");
    const P422Nv12FramesShape s{h.in.width, h.in.height, h.in.in_pitch, h.y_pitch, h.uv_pitch, h.in.format, h.in.uv_mode};
    if (mi_status d = check_p422_nv12_disjoint(c, h.in.in, h.y, h.uv, s)) return d;
    *work = true;
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_nv12_frames_dev(mi_ctx* c, const mi_packed422_nv12_frame_dev* frames, int n_frames,
                                                        int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch,
                                                        int format, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Nv12FramesShape sh{width, height, in_pitch, y_pitch, uv_pitch, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422_nv12_frames(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : packed422_nv12_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_nv12_frames_dev(mi_ctx* c, const mi_packed422_nv12_frame_dev* frames, int n_frames,
                                                int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch,
                                                int format, mi_uv_mode uv_mode,
                                                double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Nv12FramesShape sh{width, height, in_pitch, y_pitch, uv_pitch, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422_nv12_frames(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_nv12_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

mi_status mi_equalize_hist_packed422_to_nv12(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* y_out, size_t y_pitch,
                                             uint8_t* uv_out, size_t uv_pitch, int width, int height, int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    const P422Nv12Args h = p422_nv12_args(in, in_pitch, 0, y_out, y_pitch, uv_out, uv_pitch, 0, width, height, 1, format, uv_mode);
    bool work = false;
    const mi_status st = check_packed422_nv12_host(c, h, false, 0, 0, &work);
    return (st || !work) ? st : packed422_nv12_host(c, h, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_nv12(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* y_out, size_t y_pitch,
                                     uint8_t* uv_out, size_t uv_pitch, int width, int height, int format, mi_uv_mode uv_mode,
                                     double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    const P422Nv12Args h = p422_nv12_args(in, in_pitch, 0, y_out, y_pitch, uv_out, uv_pitch, 0, width, height, 1, format, uv_mode);
    bool work = false;
    const mi_status st = check_packed422_nv12_host(c, h, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_nv12_host(c, h, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
