// yuv420_frames.inc.hpp -- 8-bit 4:2:0 frames, planar or interleaved chroma on either side, given as a list of plane addresses
// (mi_*_yuv420_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip after yuv420.inc.hpp (one translation unit; not a stand-alone header).
//
// A software decoder's frame pool hands out every frame as three separately allocated, pitched planes (data[0..2], linesize[0..2]); a
// hardware encoder's surface pool hands out every NV12 surface as its own allocation.  The call is cut into chunks of kFramesPerLaunch
// frames.  A chunk's Y planes travel to the planar launchers as a FrameList with no chroma job (equalize_dev / clahe_dev, as
// bgr_nv12_frames.inc.hpp and nv12_bgr_frames.inc.hpp use them), its chroma addresses to yuv420_chroma_frames_kernel as a Yuv420List,
// both by value in the kernel arguments.  Same grids, same bytes as the batch form on one frame; each frame takes the 16-byte or the
// byte path of a layout change, and skips the planes it has in place, by its own addresses.

namespace {

struct Yuv420FramesShape {
    int width, height;
    size_t y_in_pitch, c_in_pitch; int in_chroma;
    size_t y_out_pitch, c_out_pitch; int out_chroma;
    mi_uv_mode uv_mode;
};

// entry k as the two descriptors check_yuv420_planes takes (there is no frame stride)
inline void yuv420_frame_planes(const mi_yuv420_frame_dev& f, const Yuv420FramesShape& s, mi_yuv420_planes* in, mi_yuv420_planes* out)
{
    *in = mi_yuv420_planes{const_cast<void*>(f.y_in), s.y_in_pitch, const_cast<void*>(f.c0_in), const_cast<void*>(f.c1_in), s.c_in_pitch, 0,
                           s.in_chroma};
    *out = mi_yuv420_planes{f.y_out, s.y_out_pitch, f.c0_out, f.c1_out, s.c_out_pitch, 0, s.out_chroma};
}

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
// The batch form's checks (check_yuv420's three parts), the middle one applied to every frame.
mi_status check_yuv420_frames(mi_ctx* c, const mi_yuv420_frame_dev* frames, int n_frames, const Yuv420FramesShape& s, bool is_clahe,
                              int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    bool any = false;
    mi_status st = check_yuv420_call(c, s.in_chroma, s.out_chroma, s.width, s.height, n_frames, s.uv_mode, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    for (int k = 0; k < n_frames; ++k) {
        mi_yuv420_planes in, out;
        yuv420_frame_planes(frames[k], s, &in, &out);
        if ((st = check_yuv420_planes(c, &in, &out, s.width, s.uv_mode, true))) return st;
    }
    if ((st = check_yuv420_limits(c, s.width, s.height, is_clahe, tiles_x, tiles_y))) return st;
    *work = true;
    return MI_OK;
}

// The chroma of one chunk: one launch (MI_K_LUT_APPLY); none when every frame of the chunk copies all of its chroma in place.
mi_status yuv420_chroma_frames_dev(mi_ctx* c, hipStream_t s, const mi_yuv420_frame_dev* frames, int nf, const Yuv420FramesShape& sh)
{
    const bool copy = sh.uv_mode == MI_UV_COPY, in_planar = sh.in_chroma == MI_CHROMA_PLANAR, out_planar = sh.out_chroma == MI_CHROMA_PLANAR;
    const bool relayout = copy && in_planar != out_planar;
    Yuv420Job j{};                                                    // the shape; a table launch ignores its addresses and frame strides
    j.out.step = (long long)sh.c_out_pitch; j.out.planar = out_planar ? 1 : 0;
    if (copy) { j.in.step = (long long)sh.c_in_pitch; j.in.planar = in_planar ? 1 : 0; }
    j.width = sh.width; j.rows = sh.height / 2; j.mode = copy ? 1 : 0;
    const size_t row = out_planar ? (size_t)sh.width / 2 : (size_t)sh.width;
    if (relayout) j.vec = sh.width % 32 == 0 && ((sh.c_in_pitch | sh.c_out_pitch) & 15) == 0;      // what the shape allows
    else j.flat = j.rows == 1 || (sh.c_out_pitch == row && (!copy || sh.c_in_pitch == row));
    Yuv420List l{};
    bool any = false;                                                 // a plane to write in this chunk
    unsigned long long n_vec = 0;
    for (int k = 0; k < nf; ++k) {
        const mi_yuv420_frame_dev& f = frames[k];
        // with MI_UV_FILL128 the input's chroma pointers are ignored, and so is the c1 of an interleaved side
        Yuv420Frame& e = l.f[k];
        e.c0_in = copy ? (uint8_t*)f.c0_in : nullptr;
        e.c1_in = copy && in_planar ? (uint8_t*)f.c1_in : nullptr;
        e.c0_out = (uint8_t*)f.c0_out;
        e.c1_out = out_planar ? (uint8_t*)f.c1_out : nullptr;
        // check_yuv420_planes: an equal address is exactly the same plane
        any = any || e.c0_in != e.c0_out || e.c1_in != e.c1_out;
        if (relayout && yuv420_frame_vec(j.vec, e.c0_in, e.c1_in, e.c0_out, e.c1_out)) ++n_vec;
    }
    if (!any) return MI_OK;
    const long long bytes = (long long)sh.width * j.rows * (copy ? 2 : 1);       // read + written per frame
    const int B = blocks_per_frame(c, bytes, j.rows, nf, 2048);
    LAUNCH(c, s, MI_K_LUT_APPLY, yuv420_chroma_frames_kernel, dim3(B, nf), dim3(kThreads), 0, j, l);
    if (relayout) { c->yuv420_list_frames_vec += n_vec; c->yuv420_list_frames_bytes += (unsigned long long)nf - n_vec; }
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE.  Per chunk: the luma as mi_*_nv12_frames_dev enqueues it for the same Y planes without a chroma job
// (never the fused kernel), then the chroma.
mi_status yuv420_frames_dev(mi_ctx* c, hipStream_t s, const mi_yuv420_frame_dev* frames, int n_frames, const Yuv420FramesShape& sh, int op,
                            double clip_limit, int tiles_x, int tiles_y)
{
    mi_status st;
    for (int f0 = 0; f0 < n_frames; f0 += kFramesPerLaunch) {
        const int nf = std::min(kFramesPerLaunch, n_frames - f0);
        FrameList ys{};                                              // this chunk's Y planes (uv.rows = 0: no UV work)
        for (int k = 0; k < nf; ++k)
            ys.f[k] = FramePlanes{(const uint8_t*)frames[f0 + k].y_in, nullptr, (uint8_t*)frames[f0 + k].y_out, nullptr};
        // the Y shape as the planar launchers take it with a list: the chunk's first frame, frame strides 0
        const PlaneArgs ya{ys.f[0].y_in, sh.y_in_pitch, 0, ys.f[0].y_out, sh.y_out_pitch, 0, sh.width, sh.height, nf};
        if ((st = op ? clahe_dev(c, s, ya, clip_limit, tiles_x, tiles_y, nullptr, &ys) : equalize_dev(c, s, ya, nullptr, &ys))) return st;
        if ((st = yuv420_chroma_frames_dev(c, s, frames + f0, nf, sh))) return st;
    }
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_yuv420_frames_dev(mi_ctx* c, const mi_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                             size_t y_in_pitch, size_t c_in_pitch, int in_chroma, size_t y_out_pitch, size_t c_out_pitch,
                                             int out_chroma, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const Yuv420FramesShape sh{width, height, y_in_pitch, c_in_pitch, in_chroma, y_out_pitch, c_out_pitch, out_chroma, uv_mode};
    bool work = false;
    const mi_status st = check_yuv420_frames(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : yuv420_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_yuv420_frames_dev(mi_ctx* c, const mi_yuv420_frame_dev* frames, int n_frames, int width, int height,
                                     size_t y_in_pitch, size_t c_in_pitch, int in_chroma, size_t y_out_pitch, size_t c_out_pitch,
                                     int out_chroma, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const Yuv420FramesShape sh{width, height, y_in_pitch, c_in_pitch, in_chroma, y_out_pitch, c_out_pitch, out_chroma, uv_mode};
    bool work = false;
    const mi_status st = check_yuv420_frames(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : yuv420_frames_dev(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
