// packed422_yuv420_frames.inc.hpp -- packed 4:2:2 in, planar 4:2:0 (I420 / YV12) or NV12 out on frames given one by one: a LIST of device
// frames (mi_*_packed422_to_yuv420_frames_dev) and ONE host frame (mi_*_packed422_to_yuv420): checks, chunking, staging, extern "C"
// Included by ../mi_lumaeq.hip after packed422_yuv420.inc.hpp (one translation unit; not a stand-alone header).
//
// The capture card hands out a buffer pool (packed422_frames.inc.hpp), a software encoder a frame pool whose frames have three
// separately allocated, pitched planes.  An INTERLEAVED list or host frame is the NV12 form's own (packed422_nv12_frames.inc.hpp) on
// {in, y, c0}.  A PLANAR list is cut into chunks of at most kFramesPerLaunch and kPacked422FramesPerLaunch frames; a chunk's inputs
// travel to the histogram stages as a Packed422List, its {in, y, c0, c1} entries to the writers as a Packed422Yuv420List, both by value
// in the kernel arguments, through the stage sequences of packed422.inc.hpp -- same grids, same tile splits, same bytes as the batch form.
// The host form stages one frame through the context's buffers (2 B/px up, 1.5 B/px back in three planes) around the same sequences.

namespace {

// all stages of a chunk see the same frames: both tables are cut by the smaller one
constexpr int kP422Yuv420Chunk = kPacked422FramesPerLaunch < kFramesPerLaunch ? kPacked422FramesPerLaunch : kFramesPerLaunch;

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
// PLANAR lists only (an INTERLEAVED one goes through check_packed422_nv12_frames).
mi_status check_packed422_yuv420_frames(mi_ctx* c, const mi_packed422_yuv420_frame_dev* frames, int n_frames, const P422Yuv420FramesShape& s,
                                        bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_packed422_yuv420's own answers (even width and height, format, uv_mode, sizes, tiles, pitches and their
    // multiples of 4, the planar forms' size limits), on stand-in addresses that pass its pointer checks
    const P422Yuv420Args shape = p422_yuv420_args((const void*)16, s.in_pitch, 0, (void*)32, s.y_pitch, (void*)48, (void*)64, s.c_pitch, 0,
                                                  s.width, s.height, n_frames, s.format, s.uv_mode);
    bool any = false;
    const mi_status st = check_packed422_yuv420(c, shape, is_clahe, tiles_x, tiles_y, false, &any);
    if (st || !any) return st;
    for (int k = 0; k < n_frames; ++k) {
        const mi_packed422_yuv420_frame_dev& f = frames[k];
        if (!f.in || !f.y || !f.c0 || !f.c1) return fail(c, MI_ERR_BAD_ARG, "null frame or plane pointer");
        if (((uintptr_t)f.in | (uintptr_t)f.y | (uintptr_t)f.c0 | (uintptr_t)f.c1) & 3)
            return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 frame and 4:2:0 plane addresses are multiples of 4");
        if (mi_status d = check_p422_yuv420_disjoint(c, f.in, f.y, f.c0, f.c1, s)) return d;
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status packed422_yuv420_frames_dev(mi_ctx* c, hipStream_t s, const mi_packed422_yuv420_frame_dev* frames, int n_frames,
                                      const P422Yuv420FramesShape& sh, int op, double clip_limit, int tiles_x, int tiles_y)
{
    for (int f0 = 0; f0 < n_frames; f0 += kP422Yuv420Chunk) {
        const int nf = std::min(kP422Yuv420Chunk, n_frames - f0);
        Packed422List in{};                                          // this chunk's frames of the list, from index 0: the inputs for the
        Packed422Yuv420List io{};                                    // histogram stages, the four addresses of a frame for the writers
        for (int k = 0; k < nf; ++k) {
            const mi_packed422_yuv420_frame_dev& f = frames[f0 + k];
            in.f[k] = Packed422Frame{(const uint8_t*)f.in, (uint8_t*)const_cast<void*>(f.in)};         // read-only stages: out mirrors in
            io.f[k] = Packed422Yuv420Frame{(const uint8_t*)f.in, (uint8_t*)f.y, (uint8_t*)f.c0, (uint8_t*)f.c1};
        }
        const P422Yuv420Args a = p422_yuv420_args(io.f[0].in, sh.in_pitch, 0, io.f[0].y, sh.y_pitch, io.f[0].c0, io.f[0].c1, sh.c_pitch, 0,
                                                  sh.width, sh.height, nf, sh.format, sh.uv_mode);
        const mi_status st = packed422_dev<Yuv420PlanarOut>(c, s, a, op, clip_limit, tiles_x, tiles_y, &in, &io);
        if (st) return st;
    }
    return MI_OK;
}

mi_status packed422_yuv420_frames_entry(mi_ctx* c, const mi_packed422_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                        size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int format, mi_uv_mode uv_mode, int op,
                                        double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    if (mi_status st = check_chroma_value(c, chroma)) return st;
    bool work = false;
    if (chroma == MI_CHROMA_INTERLEAVED) {                  // the NV12 list form's own path on {in, y, c0}: its checks, its kernels
        std::vector<mi_packed422_nv12_frame_dev> nv;
        if (frames && n_frames > 0) {
            nv.resize((size_t)n_frames);
            for (int k = 0; k < n_frames; ++k) nv[k] = mi_packed422_nv12_frame_dev{frames[k].in, frames[k].y, frames[k].c0};
        }
        const P422Nv12FramesShape sh{width, height, in_pitch, y_pitch, c_pitch, format, uv_mode};
        const mi_status st = check_packed422_nv12_frames(c, nv.empty() ? nullptr : nv.data(), n_frames, sh, op != 0, tiles_x, tiles_y, &work);
        return (st || !work) ? st : packed422_nv12_frames_dev(c, pick_stream(c, stream), nv.data(), n_frames, sh, op, clip_limit, tiles_x, tiles_y);
    }
    const P422Yuv420FramesShape sh{width, height, in_pitch, y_pitch, c_pitch, format, uv_mode};
    const mi_status st = check_packed422_yuv420_frames(c, frames, n_frames, sh, op != 0, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_yuv420_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, op, clip_limit, tiles_x, tiles_y);
}

// Host frame: the packed frame goes up tight (stage_in: pinned tight frames as they are, anything else through the pinned staging),
// the three planes come back from a device frame whose Y rows lie at pitch align4(W) and whose chroma rows at align4(W / 2) -- the
// kernels' rule, not the caller's: host outputs may lie at any address and pitch, a tight W % 8 != 0 frame included.  `h` carries the
// caller's pointers and pitches; it has passed the checks.
mi_status packed422_yuv420_host(mi_ctx* c, const P422Yuv420Args& h, int op, double clip_limit, int tiles_x, int tiles_y)
{
    const size_t w = (size_t)h.in.width, rows = (size_t)h.in.height;
    const size_t row = 2 * w, bytes = row * rows;
    const size_t PY = (w + 3) & ~(size_t)3, PC = (w / 2 + 3) & ~(size_t)3, ybytes = PY * rows, cbytes = PC * (rows / 2);
    const size_t frame = ybytes + 2 * cbytes;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    ++(((h.in.in_pitch == row || rows == 1) && host_range_pinned(h.in.in, bytes, &c->pin_neg)) ? c->planes_direct : c->planes_staged);
    if ((st = stage_in(c, s, h.in.in, h.in.in_pitch, row, rows, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, frame))) return st;
    const PlaneOut py(c, h.y, h.y_pitch, PY, w, rows), pu(c, h.u, h.c_pitch, PC, w / 2, rows / 2), pv(c, h.v, h.c_pitch, PC, w / 2, rows / 2);
    if (!(py.direct && pu.direct && pv.direct) && (st = grow_pinned(c, &c->h_pin_out, &c->pin_out_bytes, frame))) return st;
    uint8_t* const dout = c->d_stage_out;
    const P422Yuv420Args d = p422_yuv420_args(c->d_stage_in, row, bytes, dout, PY, dout + ybytes, dout + ybytes + cbytes, PC, frame,
                                              h.in.width, h.in.height, 1, h.in.format, h.in.uv_mode);
    if ((st = packed422_dev<Yuv420PlanarOut>(c, s, d, op, clip_limit, tiles_x, tiles_y))) return st;
    drain.watch(s);
    if ((st = enqueue_plane_out(c, s, dout, c->h_pin_out, py))) return st;
    if ((st = enqueue_plane_out(c, s, dout + ybytes, c->h_pin_out + ybytes, pu))) return st;
    if ((st = enqueue_plane_out(c, s, dout + ybytes + cbytes, c->h_pin_out + ybytes + cbytes, pv))) return st;
    HIPCHK(c, hipStreamSynchronize(s));
    drain.done();
    copy_plane_out(py, c->h_pin_out);
    copy_plane_out(pu, c->h_pin_out + ybytes);
    copy_plane_out(pv, c->h_pin_out + ybytes + cbytes);
    return MI_OK;
}

// The host form's checks (PLANAR): the input side and the shape are the device form's (check_packed422_yuv420 on the caller's input and
// on stand-in planes at the device pitches); the output side is host memory the kernels never see -- any address, any pitch >= its row.
mi_status check_packed422_yuv420_host(mi_ctx* c, const P422Yuv420Args& h, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    const size_t w = (size_t)std::max(h.in.width, 0);
    const size_t PY = (w + 3) & ~(size_t)3, PC = (w / 2 + 3) & ~(size_t)3;
    const P422Yuv420Args shape = p422_yuv420_args(h.in.in, h.in.in_pitch, 0, h.y ? (void*)32 : nullptr, PY, h.u ? (void*)48 : nullptr,
                                                  h.v ? (void*)64 : nullptr, PC, 0, h.in.width, h.in.height, 1, h.in.format, h.in.uv_mode);
    bool any = false;
    const mi_status st = check_packed422_yuv420(c, shape, is_clahe, tiles_x, tiles_y, false, &any);
    if (st || !any) return st;
    if (h.y_pitch < w) return fail(c, MI_ERR_BAD_ARG, "y_pitch < width");
    if (h.c_pitch < w / 2) return fail(c, MI_ERR_BAD_ARG, "c_pitch below its row (width / 2 planar)");
    const P422Yuv420FramesShape s{h.in.width, h.in.height, h.in.in_pitch, h.y_pitch, h.c_pitch, h.in.format, h.in.uv_mode};
    if (mi_status d = check_p422_yuv420_disjoint(c, h.in.in, h.y, h.u, h.v, s)) return d;
    *work = true;
    return MI_OK;
}

mi_status packed422_yuv420_host_entry(mi_ctx* c, const uint8_t* in, size_t in_pitch, const mi_yuv420_planes* out, int width, int height,
                                      int format, mi_uv_mode uv_mode, int op, double clip_limit, int tiles_x, int tiles_y)
{
    if (!out) return fail(c, MI_ERR_BAD_ARG, "null plane descriptor");
    if (mi_status st = check_chroma_value(c, out->chroma)) return st;
    bool work = false;
    if (out->chroma == MI_CHROMA_INTERLEAVED) {             // the NV12 host form's own checks and staging on {y, c0}; c1 is ignored
        const P422Nv12Args n = p422_nv12_args(in, in_pitch, 0, out->y, out->y_pitch, out->c0, out->c_pitch, 0, width, height, 1, format, uv_mode);
        const mi_status st = check_packed422_nv12_host(c, n, op != 0, tiles_x, tiles_y, &work);
        return (st || !work) ? st : packed422_nv12_host(c, n, op, clip_limit, tiles_x, tiles_y);
    }
    const P422Yuv420Args h = p422_yuv420_args(in, in_pitch, 0, out->y, out->y_pitch, out->c0, out->c1, out->c_pitch, 0, width, height, 1,
                                              format, uv_mode);
    const mi_status st = check_packed422_yuv420_host(c, h, op != 0, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_yuv420_host(c, h, op, clip_limit, tiles_x, tiles_y);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_yuv420_frames_dev(mi_ctx* c, const mi_packed422_yuv420_frame_dev* frames, int n_frames,
                                                          int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch,
                                                          int out_chroma, int format, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    return packed422_yuv420_frames_entry(c, frames, n_frames, width, height, in_pitch, y_pitch, c_pitch, out_chroma, format, uv_mode, 0, 0.0,
                                         0, 0, stream);
}

mi_status mi_clahe_packed422_to_yuv420_frames_dev(mi_ctx* c, const mi_packed422_yuv420_frame_dev* frames, int n_frames,
                                                  int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch,
                                                  int out_chroma, int format, mi_uv_mode uv_mode,
                                                  double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    return packed422_yuv420_frames_entry(c, frames, n_frames, width, height, in_pitch, y_pitch, c_pitch, out_chroma, format, uv_mode, 1,
                                         clip_limit, tiles_x, tiles_y, stream);
}

mi_status mi_equalize_hist_packed422_to_yuv420(mi_ctx* c, const uint8_t* in, size_t in_pitch, const mi_yuv420_planes* out,
                                               int width, int height, int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    return packed422_yuv420_host_entry(c, in, in_pitch, out, width, height, format, uv_mode, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_yuv420(mi_ctx* c, const uint8_t* in, size_t in_pitch, const mi_yuv420_planes* out,
                                       int width, int height, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return packed422_yuv420_host_entry(c, in, in_pitch, out, width, height, format, uv_mode, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
