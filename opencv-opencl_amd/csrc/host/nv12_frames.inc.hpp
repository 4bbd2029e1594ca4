// nv12_frames.inc.hpp -- NV12 frames given as a list of plane addresses (mi_*_nv12_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip (one translation unit; not a stand-alone header).
//
// Decoder surfaces and tensor lists are not one allocation at a fixed frame stride, and their planes are pitched.  The call is cut
// into chunks of kFramesPerLaunch frames; each chunk's plane addresses travel by value in the kernel arguments (FrameList), and the
// chunk runs the stage sequence of equalize_dev (without the fused kernel) or clahe_dev through the same launch helpers, which pick
// the *_frames_kernel entries.  Same grids, same tile splits, same bytes as the contiguous forms.

namespace {

struct FramesShape {
    int width, height;
    size_t y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch;
    mi_uv_mode uv_mode;
    int sample_bytes = 1;             // 2: P010 frames (mi_clahe_p010_frames_dev, host/p010_frames.inc.hpp): rows of 2 * W bytes
};

// The bytes a plane's rows span: [p, p + (rows - 1) * pitch + row_bytes).  Planes are compared as such address ranges.
struct Span {
    uintptr_t lo, hi;
    Span(const void* p, size_t pitch, size_t row_bytes, size_t rows) : lo((uintptr_t)p), hi((uintptr_t)p + (rows - 1) * pitch + row_bytes) {}
    bool meets(const Span& o) const { return lo < o.hi && o.lo < hi; }
};

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
// Rows are W * sample_bytes bytes; 16-bit frames also need even pitches and 2-byte aligned planes, and keep to mi_clahe_u16's sizes.
mi_status check_frames(mi_ctx* c, const mi_nv12_frame_dev* frames, int n_frames, const FramesShape& s, bool* work)
{
    *work = false;
    if (n_frames < 0 || s.width < 0 || s.height < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    if (s.uv_mode != MI_UV_FILL128 && s.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if ((s.width & 1) || (s.height & 1)) return fail(c, MI_ERR_BAD_ARG, "4:2:0 frames have even width and height");
    const size_t w = (size_t)s.width * (size_t)s.sample_bytes;        // bytes per row
    const bool copy = s.uv_mode == MI_UV_COPY;
    if (s.y_in_pitch < w || s.y_out_pitch < w || s.uv_out_pitch < w || (copy && s.uv_in_pitch < w))
        return fail(c, MI_ERR_BAD_ARG, "pitch < width");
    const size_t odd = s.sample_bytes - 1;                             // address bits a 16-bit sample may not have
    if ((s.y_in_pitch | s.y_out_pitch | s.uv_out_pitch | (copy ? s.uv_in_pitch : 0)) & odd)
        return fail(c, MI_ERR_BAD_ARG, "16-bit planes need even pitches");
    if (n_frames == 0 || s.width == 0 || s.height == 0) return MI_OK;
    if (s.sample_bytes == 2 && (long long)s.width * s.height > 0x3fffffffLL) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    if ((long long)s.width * s.height > 0x7fffffffLL) return fail(c, MI_ERR_UNSUPPORTED, "width*height must be < 2^31 (OpenCV: int total)");
    if (s.width > (1 << 24) || s.height > (1 << 24)) return fail(c, MI_ERR_UNSUPPORTED, "width/height must be <= 2^24");
    const size_t yrows = (size_t)s.height, uvrows = yrows / 2;
    for (int k = 0; k < n_frames; ++k) {
        const mi_nv12_frame_dev& f = frames[k];
        if (!f.y_in || !f.y_out || !f.uv_out) return fail(c, MI_ERR_BAD_ARG, "null plane pointer");
        if (copy && !f.uv_in) return fail(c, MI_ERR_BAD_ARG, "null uv_in with MI_UV_COPY");
        if (((uintptr_t)f.y_in | (uintptr_t)f.y_out | (uintptr_t)f.uv_out | (copy ? (uintptr_t)f.uv_in : 0)) & odd)
            return fail(c, MI_ERR_BAD_ARG, "16-bit planes must be 2-byte aligned");
        // each output plane against each plane the call reads (Y in; UV in when copying): disjoint, or the very same plane (in place)
        const Span yi(f.y_in, s.y_in_pitch, w, yrows), yo(f.y_out, s.y_out_pitch, w, yrows), uo(f.uv_out, s.uv_out_pitch, w, uvrows);
        const bool y_in_place = f.y_out == f.y_in && s.y_out_pitch == s.y_in_pitch;
        bool bad = (!y_in_place && yo.meets(yi)) || uo.meets(yi);
        if (copy) {
            const Span ui(f.uv_in, s.uv_in_pitch, w, uvrows);
            const bool uv_in_place = f.uv_out == f.uv_in && s.uv_out_pitch == s.uv_in_pitch;
            bad = bad || (!uv_in_place && uo.meets(ui)) || yo.meets(ui);
        }
        if (bad) return fail(c, MI_ERR_BAD_ARG, "an output plane partly overlaps an input plane of the same frame");
    }
    *work = true;
    return MI_OK;
}

// Chunk k of the list as the kernels see it.  The Y shape goes through PlaneArgs (a.src / a.dst: the chunk's first frame, frame
// strides 0, so make_plane sees the real pitches); the chroma is one flat run when both UV planes are tight.
FrameList frame_chunk(const mi_nv12_frame_dev* frames, int nf, const FramesShape& s, PlaneArgs* a)
{
    FrameList l{};
    for (int k = 0; k < nf; ++k)
        l.f[k] = FramePlanes{(const uint8_t*)frames[k].y_in, s.uv_mode == MI_UV_COPY ? (const uint8_t*)frames[k].uv_in : nullptr,
                             (uint8_t*)frames[k].y_out, (uint8_t*)frames[k].uv_out};
    const long long w = (long long)s.width * s.sample_bytes, uvrows = s.height / 2;
    l.uv.mode = s.uv_mode == MI_UV_COPY ? 1 : 0;
    l.uv.src_step = (long long)s.uv_in_pitch; l.uv.dst_step = (long long)s.uv_out_pitch;
    const bool tight = s.uv_out_pitch == (size_t)w && (l.uv.mode == 0 || s.uv_in_pitch == (size_t)w);
    if (tight || uvrows == 1) { l.uv.rows = 1; l.uv.row_bytes = w * uvrows; }
    else { l.uv.rows = (int)uvrows; l.uv.row_bytes = w; }
    *a = PlaneArgs{(const uint8_t*)frames[0].y_in, s.y_in_pitch, 0, (uint8_t*)frames[0].y_out, s.y_out_pitch, 0, s.width, s.height, nf};
    return l;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status nv12_frames_dev(mi_ctx* c, hipStream_t s, const mi_nv12_frame_dev* frames, int n_frames, const FramesShape& sh, int op,
                          double clip_limit, int tiles_x, int tiles_y)
{
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        PlaneArgs a;
        const FrameList l = frame_chunk(frames + f0, nf, sh, &a);
        const mi_status st = op ? clahe_dev(c, s, a, clip_limit, tiles_x, tiles_y, nullptr, &l) : equalize_dev(c, s, a, nullptr, &l);
        if (st) return st;
    }
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_nv12_frames_dev(mi_ctx* c, const mi_nv12_frame_dev* frames, int n_frames, int width, int height,
                                           size_t y_in_pitch, size_t uv_in_pitch, size_t y_out_pitch, size_t uv_out_pitch,
                                           mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const FramesShape sh{width, height, y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch, uv_mode};
    bool work = false;
    mi_status st = check_frames(c, frames, n_frames, sh, &work);
    if (st || !work) return st;
    return nv12_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_nv12_frames_dev(mi_ctx* c, const mi_nv12_frame_dev* frames, int n_frames, int width, int height,
                                   size_t y_in_pitch, size_t uv_in_pitch, size_t y_out_pitch, size_t uv_out_pitch,
                                   mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    if (tiles_x <= 0 || tiles_y <= 0) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    const FramesShape sh{width, height, y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch, uv_mode};
    bool work = false;
    mi_status st = check_frames(c, frames, n_frames, sh, &work);
    if (st || !work) return st;
    return nv12_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
