// packed422_nv12.inc.hpp -- packed 4:2:2 frames in (YUY2 / UYVY), NV12 frames out: checks, launch sequences, extern "C" entry points
// Included by ../mi_lumaeq.hip after packed422.inc.hpp (one translation unit; not a stand-alone header).
//
// capture -> equalize -> encoder without a format conversion of its own.  The histogram half is packed422.inc.hpp's, launch for launch
// (hist422_partial_kernel -> equalize_lut_kernel; launch_tile_luts422): same scratch, same chunks, same grids and splits.  Only the
// last stage differs: the pixel-writing kernels of kernels/packed422_nv12.hip.h put the new luma into a Y plane and the chroma of each
// row pair, halved vertically, into an interleaved UV plane -- in the launch that writes the luma, there is no chroma launch.  Never
// the fused kernel and never hist_lut_kernel, as the packed forms.

namespace {

struct P422Nv12Args {
    P422Args in;                      // the input side (in.out* mirror the input: only check_packed422 and the read-only stages look at them)
    uint8_t* y; size_t y_pitch;
    uint8_t* uv; size_t uv_pitch;
    size_t out_frame;
};

P422Nv12Args p422_nv12_args(const void* d_in, size_t in_pitch, size_t in_frame, void* d_y, size_t y_pitch, void* d_uv, size_t uv_pitch,
                            size_t out_frame, int width, int height, int n_frames, int format, mi_uv_mode uv_mode)
{
    P422Nv12Args a;
    a.in = P422Args{(const uint8_t*)d_in, in_pitch, in_frame, (uint8_t*)const_cast<void*>(d_in), in_pitch, in_frame,
                    width, height, n_frames, format, uv_mode};
    a.y = (uint8_t*)d_y; a.y_pitch = y_pitch; a.uv = (uint8_t*)d_uv; a.uv_pitch = uv_pitch; a.out_frame = out_frame;
    return a;
}

// Everything is checked before anything is enqueued.  The input side, the shape and the modes are check_packed422's own checks (run on
// the input alone); the NV12 side adds the even height and the two planes.  *work = false: MI_OK with nothing to do.
mi_status check_packed422_nv12(mi_ctx* c, const P422Nv12Args& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.in.height > 0 && (a.in.height & 1)) return fail(c, MI_ERR_BAD_ARG, "NV12 frames have an even height");
    bool in_work = false;
    const mi_status st = check_packed422(c, a.in, is_clahe, tiles_x, tiles_y, &in_work);
    if (st || !in_work) return st;
    if (!a.y || !a.uv) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
    if (a.y_pitch < (size_t)a.in.width || a.uv_pitch < (size_t)a.in.width) return fail(c, MI_ERR_BAD_ARG, "NV12 pitch < width");
    if (((uintptr_t)a.y | (uintptr_t)a.uv | a.y_pitch | a.uv_pitch | a.out_frame) & 3)
        return fail(c, MI_ERR_BAD_ARG, "NV12 plane pointers, pitches and the frame stride are multiples of 4 here (pad the pitch when W % 4 == 2)");
    if (a.y == a.in.in || a.uv == a.in.in) return fail(c, MI_ERR_BAD_ARG, "packed in, NV12 out has no in-place form");
    *work = true;
    return MI_OK;
}

Packed422Nv12 packed422_nv12_batch(const P422Nv12Args& a, int f0)
{
    Packed422Nv12 p;
    p.src = a.in.in + (size_t)f0 * a.in.in_frame;
    p.y = a.y + (size_t)f0 * a.out_frame; p.uv = a.uv + (size_t)f0 * a.out_frame;
    p.src_step = (long long)a.in.in_pitch; p.y_step = (long long)a.y_pitch; p.uv_step = (long long)a.uv_pitch;
    p.src_frame = (long long)a.in.in_frame; p.out_frame = (long long)a.out_frame;
    p.dwords = a.in.width / 2; p.rows = a.in.height;
    p.copy_uv = a.in.uv_mode == MI_UV_COPY ? 1 : 0;
    return p;
}

// One chunk of a frame list (mi_*_packed422_to_nv12_frames_dev, packed422_nv12_frames.inc.hpp): the inputs as the histogram stages'
// Packed422List (they only read: out mirrors in, as in p422_nv12_args) and the three addresses of every frame for the writers.
struct P422Nv12Lists {
    Packed422List in;
    Packed422Nv12List io;
};

// The stage sequences below take an optional chunk of a frame list (a.in.n_frames of its entries, indices from 0): with one, every
// launch goes to the *_frames_kernel entry of the same body -- same grids, same splits, same scratch -- and the base addresses and
// frame strides of `a` are not used.

// equalize422_dev with the NV12 writer as its last stage: one MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch per chunk
template <int OFF>
mi_status equalize422_nv12_dev(mi_ctx* c, hipStream_t s, const P422Nv12Args& a, const P422Nv12Lists* fl = nullptr)
{
    const int width = a.in.width, height = a.in.height;
    const long long frame_bytes = 2LL * width * height;
    for (int f0 = 0; f0 < a.in.n_frames; f0 += kMaxGridY) {
        const int nf = std::min(kMaxGridY, a.in.n_frames - f0);
        const Packed422 pin = packed422_batch(a.in, f0);
        const Packed422Nv12 p = packed422_nv12_batch(a, f0);
        const int B = blocks_per_frame(c, frame_bytes, height, nf, 256);
        mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t));
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        if (fl) LAUNCH(c, s, MI_K_HIST, hist422_partial_frames_kernel<OFF>, dim3(B, nf), dim3(kHistThreads), 0, fl->in, pin, c->d_partial);
        else    LAUNCH(c, s, MI_K_HIST, hist422_partial_kernel<OFF>, dim3(B, nf), dim3(kHistThreads), 0, pin, c->d_partial);
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, B, (int)((long long)width * height), c->d_luts, (int32_t*)nullptr);
        const int BA = blocks_per_frame(c, frame_bytes, height / 2, nf, 2048);       // bands of row pairs
        if (fl) LAUNCH(c, s, MI_K_LUT_APPLY, lut_apply422_nv12_frames_kernel<OFF>, dim3(BA, nf), dim3(kThreads), 0, fl->io, p, (const uint8_t*)c->d_luts);
        else    LAUNCH(c, s, MI_K_LUT_APPLY, lut_apply422_nv12_kernel<OFF>, dim3(BA, nf), dim3(kThreads), 0, p, (const uint8_t*)c->d_luts);
    }
    return MI_OK;
}

// launch_interp422 on the NV12 writers: the same plan (plan_interp422: tables, column segments, bands, sub-bands), other kernels
template <int OFF>
mi_status launch_interp422_nv12(mi_ctx* c, hipStream_t s, const Packed422Nv12& p, const ClaheGeom& g, int nf, const uint8_t* d_luts,
                                const Packed422Nv12List* fl = nullptr)
{
    Interp422Plan pl;
    if (mi_status st = plan_interp422(c, g, p.dwords, nf, &pl)) return st;
    const dim3 grid = pl.grid;
    const size_t lds = pl.lds;
    const int subs = pl.subs, groups = pl.groups, cap = pl.cap;
    if (pl.global) {
        if (fl) LAUNCH(c, s, MI_K_CLAHE_INTERP, clahe_interp422_nv12_global_frames_kernel<OFF>, grid, dim3(kThreads), 0, *fl, p, g, d_luts);
        else    LAUNCH(c, s, MI_K_CLAHE_INTERP, clahe_interp422_nv12_global_kernel<OFF>, grid, dim3(kThreads), 0, p, g, d_luts);
    } else if (pl.float_tables) {
        if (fl) {
            if (g.contract) LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_frames_kernel<true, true, OFF>), grid, dim3(kThreads), lds, *fl, p, g, d_luts, subs, groups, cap);
            else            LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_frames_kernel<true, false, OFF>), grid, dim3(kThreads), lds, *fl, p, g, d_luts, subs, groups, cap);
        } else if (g.contract) LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_kernel<true, true, OFF>), grid, dim3(kThreads), lds, p, g, d_luts, subs, groups, cap);
        else                   LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_kernel<true, false, OFF>), grid, dim3(kThreads), lds, p, g, d_luts, subs, groups, cap);
    } else {
        if (fl) {
            if (g.contract) LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_frames_kernel<false, true, OFF>), grid, dim3(kThreads), lds, *fl, p, g, d_luts, subs, groups, cap);
            else            LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_frames_kernel<false, false, OFF>), grid, dim3(kThreads), lds, *fl, p, g, d_luts, subs, groups, cap);
        } else if (g.contract) LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_kernel<false, true, OFF>), grid, dim3(kThreads), lds, p, g, d_luts, subs, groups, cap);
        else                   LAUNCH(c, s, MI_K_CLAHE_INTERP, (clahe_interp422_nv12_kernel<false, false, OFF>), grid, dim3(kThreads), lds, p, g, d_luts, subs, groups, cap);
    }
    return MI_OK;
}

template <int OFF>
mi_status clahe422_nv12_dev(mi_ctx* c, hipStream_t s, const P422Nv12Args& a, double clip_limit, int tiles_x, int tiles_y,
                            const P422Nv12Lists* fl = nullptr)
{
    ClaheGeom g;
    mi_status st = clahe_geometry(c, a.in.width, a.in.height, clip_limit, tiles_x, tiles_y, &g);
    if (st) return st;
    const int tiles = tiles_x * tiles_y;
    for (int f0 = 0; f0 < a.in.n_frames; f0 += kMaxGridY) {
        const int nf = std::min(kMaxGridY, a.in.n_frames - f0);
        const Packed422 pin = packed422_batch(a.in, f0);
        const Packed422Nv12 p = packed422_nv12_batch(a, f0);
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
        if ((st = launch_tile_luts422<OFF>(c, s, pin, g, nf, c->d_luts, fl ? &fl->in : nullptr))) return st;
        if ((st = launch_interp422_nv12<OFF>(c, s, p, g, nf, c->d_luts, fl ? &fl->io : nullptr))) return st;
    }
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE.  `a` has passed check_packed422_nv12 (with a list: check_packed422_nv12_frames).
mi_status packed422_nv12_dev(mi_ctx* c, hipStream_t s, const P422Nv12Args& a, int op, double clip_limit, int tiles_x, int tiles_y,
                             const P422Nv12Lists* fl = nullptr)
{
    if (a.in.format == MI_FMT_UYVY) return op ? clahe422_nv12_dev<1>(c, s, a, clip_limit, tiles_x, tiles_y, fl) : equalize422_nv12_dev<1>(c, s, a, fl);
    return op ? clahe422_nv12_dev<0>(c, s, a, clip_limit, tiles_x, tiles_y, fl) : equalize422_nv12_dev<0>(c, s, a, fl);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_nv12_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                                       void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
                                                       int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Nv12Args a = p422_nv12_args(d_in, in_pitch, in_frame_stride, d_y_out, y_pitch, d_uv_out, uv_pitch, out_frame_stride,
                                          width, height, n_frames, format, uv_mode);
    bool work = false;
    const mi_status st = check_packed422_nv12(c, a, false, 0, 0, &work);
    if (st || !work) return st;
    hipStream_t s = pick_stream(c, stream);
    return format == MI_FMT_UYVY ? equalize422_nv12_dev<1>(c, s, a) : equalize422_nv12_dev<0>(c, s, a);
}

mi_status mi_clahe_packed422_to_nv12_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
                                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Nv12Args a = p422_nv12_args(d_in, in_pitch, in_frame_stride, d_y_out, y_pitch, d_uv_out, uv_pitch, out_frame_stride,
                                          width, height, n_frames, format, uv_mode);
    bool work = false;
    const mi_status st = check_packed422_nv12(c, a, true, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    hipStream_t s = pick_stream(c, stream);
    return format == MI_FMT_UYVY ? clahe422_nv12_dev<1>(c, s, a, clip_limit, tiles_x, tiles_y)
                                 : clahe422_nv12_dev<0>(c, s, a, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
