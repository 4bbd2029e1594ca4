// packed422_frames.inc.hpp -- packed 4:2:2 frames given as a list of addresses (mi_*_packed422_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip (one translation unit; not a stand-alone header).
//
// A capture card's buffer pool is not one allocation at a fixed frame stride: every buffer is its own allocation, padded to
// bytesperline, at whatever alignment the driver gave it.  The call is cut into chunks of kPacked422FramesPerLaunch frames; each
// chunk's {in, out} pairs travel by value in the kernel arguments (Packed422List), and the chunk runs the stage sequences of
// packed422.inc.hpp, whose launches pick the *_frames_kernel entries.  Same grids, same tile splits, same bytes as the batch forms.

namespace {

struct P422FramesShape {
    int width, height;
    size_t in_pitch, out_pitch;
    int format;
    mi_uv_mode uv_mode;
};

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
mi_status check_packed422_frames(mi_ctx* c, const mi_packed422_frame_dev* frames, int n_frames, const P422FramesShape& s, bool is_clahe,
                                 int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_packed422's own answers (format, uv_mode, sizes, tiles, odd width, pitches, the planar forms' size limits), on
    // stand-in addresses that pass its pointer checks
    const P422Args shape{(const uint8_t*)16, s.in_pitch, 0, (uint8_t*)16, s.out_pitch, 0, s.width, s.height, n_frames, s.format, s.uv_mode};
    bool any = false;
    const mi_status st = check_packed422(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t row = 2 * (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_packed422_frame_dev& f = frames[k];
        if (!f.in || !f.out) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
        if (((uintptr_t)f.in | (uintptr_t)f.out) & 3) return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 frame addresses are multiples of 4");
        if (f.out == f.in && s.in_pitch != s.out_pitch) return fail(c, MI_ERR_BAD_ARG, "an in-place frame needs equal pitches");
        // the output against the input of the same frame: disjoint, or the very same rows (in place)
        if (f.out != f.in && Span(f.out, s.out_pitch, row, rows).meets(Span(f.in, s.in_pitch, row, rows)))
            return fail(c, MI_ERR_BAD_ARG, "an output frame partly overlaps its own input frame");
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE
mi_status packed422_frames_dev(mi_ctx* c, hipStream_t s, const mi_packed422_frame_dev* frames, int n_frames, const P422FramesShape& sh,
                               int op, double clip_limit, int tiles_x, int tiles_y)
{
    for (int f0 = 0; f0 < n_frames; f0 += kPacked422FramesPerLaunch) {
        const int nf = std::min(kPacked422FramesPerLaunch, n_frames - f0);
        Packed422List l{};                                           // this chunk's frames of the list, from index 0
        for (int k = 0; k < nf; ++k) l.f[k] = Packed422Frame{(const uint8_t*)frames[f0 + k].in, (uint8_t*)frames[f0 + k].out};
        const P422Args a{l.f[0].in, sh.in_pitch, 0, l.f[0].out, sh.out_pitch, 0, sh.width, sh.height, nf, sh.format, sh.uv_mode};
        const mi_status st = packed422_dev<PackedOut>(c, s, a, op, clip_limit, tiles_x, tiles_y, &l, &l);
        if (st) return st;
    }
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_frames_dev(mi_ctx* c, const mi_packed422_frame_dev* frames, int n_frames,
                                                int width, int height, size_t in_pitch, size_t out_pitch,
                                                int format, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const P422FramesShape sh{width, height, in_pitch, out_pitch, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422_frames(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : packed422_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_frames_dev(mi_ctx* c, const mi_packed422_frame_dev* frames, int n_frames,
                                        int width, int height, size_t in_pitch, size_t out_pitch,
                                        int format, mi_uv_mode uv_mode,
                                        double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422FramesShape sh{width, height, in_pitch, out_pitch, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422_frames(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
