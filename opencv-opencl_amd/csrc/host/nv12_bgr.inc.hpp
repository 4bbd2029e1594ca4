// nv12_bgr.inc.hpp -- NV12 frames in, interleaved 8-bit BGR / RGB out in the pass that maps the luma: checks, launch sequences, extern "C"
// Included by ../mi_lumaeq.hip (one translation unit; not a stand-alone header).
//
// decoder -> equalize -> display / image writer / model without an NV12 intermediate.  Y is a plane: the histogram stages are the planar
// forms' own launchers (launch_hist_partials -> equalize_lut_kernel; launch_tile_luts), unchanged, with the same scratch.  Only the stage
// that writes pixels differs (kernels/nv12_bgr.hip.h): it maps the luma and decodes 4:2:0 to 3 bytes per pixel in one kernel.  Never the
// fused kernel and never hist_lut_kernel: option two_kernel_max_frames does not apply (the bytes are the same on every path).
// CLAHE shapes the one-pass interpolation kernel does not take (REFLECT_101 padding, tile_w % 16 != 0, unaligned rows, tiles_x > 14,
// clahe_fp_contract) run the planar CLAHE into a scratch Y plane and then the decode alone: the same bytes in one more pass.

namespace {

// frames per launch sequence: bounds the scratch Y planes of the two-pass fallback (256 x 4K = 2 GiB) as well as the grids
constexpr int kNv12BgrFramesPerLaunch = 256;

struct Nv12BgrArgs {
    const uint8_t* y; size_t y_pitch;
    const uint8_t* uv; size_t uv_pitch;
    size_t in_frame;
    uint8_t* out; size_t out_pitch, out_frame;
    int width, height, n_frames, order;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.
mi_status check_nv12_bgr(mi_ctx* c, const Nv12BgrArgs& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.order != MI_ORDER_BGR && a.order != MI_ORDER_RGB) return fail(c, MI_ERR_BAD_ARG, "order must be MI_ORDER_BGR or MI_ORDER_RGB");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if ((a.width & 1) || (a.height & 1)) return fail(c, MI_ERR_BAD_ARG, "NV12 frames have an even width and an even height");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.y || !a.uv || !a.out) return fail(c, MI_ERR_BAD_ARG, "null plane pointer");
    if (a.y_pitch < (size_t)a.width || a.uv_pitch < (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "NV12 pitch < width");
    if (a.out_pitch < 3 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "out_pitch < 3 * width");
    if (a.out == a.y || a.out == a.uv) return fail(c, MI_ERR_BAD_ARG, "NV12 in, BGR out has no in-place form");
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

// The Y plane as the planar stage launchers see it (they only read: dst mirrors nothing)
PlaneArgs nv12_bgr_y_plane(const Nv12BgrArgs& a)
{
    return PlaneArgs{a.y, a.y_pitch, a.in_frame, nullptr, 0, 0, a.width, a.height, a.n_frames};
}

bool nv12_bgr_aligned16(const Nv12BgrArgs& a)
{
    return (((uintptr_t)a.y | (uintptr_t)a.uv | (uintptr_t)a.out | a.y_pitch | a.uv_pitch | a.out_pitch | a.in_frame | a.out_frame) & 15) == 0;
}

// the job of frames f0.. of the call; y / y_pitch / y_frame say where the luma comes from (the caller's planes, or scratch)
Nv12BgrJob nv12_bgr_job(const Nv12BgrArgs& a, int f0, const uint8_t* y, size_t y_pitch, size_t y_frame)
{
    Nv12BgrJob j{};
    j.y = y; j.uv = a.uv + (size_t)f0 * a.in_frame; j.out = a.out + (size_t)f0 * a.out_frame;
    j.y_step = (long long)y_pitch; j.uv_step = (long long)a.uv_pitch; j.out_step = (long long)a.out_pitch;
    j.y_frame = (long long)y_frame; j.uv_frame = (long long)a.in_frame; j.out_frame = (long long)a.out_frame;
    j.width = a.width; j.height = a.height;
    j.vec = a.width % 16 == 0 && nv12_bgr_aligned16(a) && (((uintptr_t)y | y_pitch | y_frame) & 15) == 0;
    return j;
}

// LUT apply + decode (luts != nullptr, MI_K_LUT_APPLY) or the decode alone (MI_K_COLOR).  `fl`: a chunk of a frame list (at most
// kFramesPerLaunch frames, nv12_bgr_frames.inc.hpp): the same grid on the *_frames_kernel entry; `j` then carries the shape, and
// j.vec what the shape allows.
mi_status launch_nv12_to_bgr(mi_ctx* c, hipStream_t s, const Nv12BgrJob& j, int nf, int order, const uint8_t* luts,
                             const Nv12BgrList* fl = nullptr)
{
    const long long px = (long long)j.width * j.height;
    // bytes per workgroup as the other apply kernels count them (half of what is read and written: 1.5 + 3 B/px); in 16 x 2 groups a
    // workgroup pass covers 8192 pixels, in 2 x 2 blocks 1024
    int B = blocks_per_frame(c, px * 9 / 4, j.height / 2, nf, 2048);
    const long long items = j.vec ? px / 32 : px / 4;
    B = (int)std::max<long long>(1, std::min<long long>(B, (items + kThreads - 1) / kThreads));
    const dim3 grid(B, nf), block(kThreads);
    if (fl && luts) {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_LUT_APPLY, (nv12_to_bgr_frames_kernel<1, true>), grid, block, 0, *fl, j, luts);
        else                       LAUNCH(c, s, MI_K_LUT_APPLY, (nv12_to_bgr_frames_kernel<0, true>), grid, block, 0, *fl, j, luts);
    } else if (fl) {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_COLOR, (nv12_to_bgr_frames_kernel<1, false>), grid, block, 0, *fl, j, luts);
        else                       LAUNCH(c, s, MI_K_COLOR, (nv12_to_bgr_frames_kernel<0, false>), grid, block, 0, *fl, j, luts);
    } else if (luts) {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_LUT_APPLY, (nv12_to_bgr_kernel<1, true>), grid, block, 0, j, luts);
        else                       LAUNCH(c, s, MI_K_LUT_APPLY, (nv12_to_bgr_kernel<0, true>), grid, block, 0, j, luts);
    } else {
        if (order == MI_ORDER_RGB) LAUNCH(c, s, MI_K_COLOR, (nv12_to_bgr_kernel<1, false>), grid, block, 0, j, luts);
        else                       LAUNCH(c, s, MI_K_COLOR, (nv12_to_bgr_kernel<0, false>), grid, block, 0, j, luts);
    }
    return MI_OK;
}

mi_status equalize_nv12_bgr_dev(mi_ctx* c, hipStream_t s, const Nv12BgrArgs& a)
{
    const PlaneArgs ya = nv12_bgr_y_plane(a);
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        int nparts = 0;
        mi_status st = launch_hist_partials(c, s, ya, f0, nf, &nparts);
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, nparts, (int)((long long)a.width * a.height), c->d_luts, (int32_t*)nullptr);
        const Nv12BgrJob j = nv12_bgr_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
        if ((st = launch_nv12_to_bgr(c, s, j, nf, a.order, c->d_luts))) return st;
    }
    ++c->nv12_bgr_onepass;
    return MI_OK;
}

// The shapes nv12_bgr_clahe_interp_kernel is taken for: no REFLECT_101 padding, 16-pixel groups that never straddle a tile, f32 pair
// tables that hold the whole grid, separately rounded arithmetic.  The caller adds the alignment: 16-byte aligned rows.
bool nv12_bgr_onepass_shape(const ClaheGeom& g, int width, int height, int tiles_x, int tiles_y)
{
    return !g.contract && width % tiles_x == 0 && height % tiles_y == 0 && g.tile_w % 16 == 0 && tiles_x + 1 <= kMaxPairsLdsF32 &&
           tiles_x * tiles_y <= kMaxGridY && width / kInterpPx <= kThreads * kMaxGridY;
}

// CLAHE blend + decode of nf frames whose tile LUTs are in `luts`: launch_interp's bands, sub-bands and column segments.  `fl`: as
// for launch_nv12_to_bgr.
mi_status launch_nv12_bgr_interp(mi_ctx* c, hipStream_t s, const Nv12BgrJob& j, const ClaheGeom& g, int nf, int order, const uint8_t* luts,
                                 const Nv12BgrList* fl = nullptr)
{
    const int ngroups = j.width / kInterpPx;
    const int groups = std::min(ngroups, kThreads);
    const int segs = (ngroups + groups - 1) / groups;
    const int bands = g.tiles_y + 1;
    const long long want = ((long long)c->cu_count * 8 + (long long)bands * nf * segs - 1) / ((long long)bands * nf * segs);
    const int subs = (int)std::max<long long>(1, std::min<long long>({want, (long long)std::max(1, (g.tile_h + 2 * kBandMargin) / 8), 64LL}));
    const dim3 grid(bands * subs, nf, segs);
    const size_t lds = (size_t)(g.tiles_x + 1) * 256 * 4 * sizeof(float);
    if (fl) {
        if (order == MI_ORDER_RGB)
            LAUNCH(c, s, MI_K_CLAHE_INTERP, nv12_bgr_clahe_interp_frames_kernel<1>, grid, dim3(kThreads), lds, *fl, j, g, luts, subs, groups);
        else
            LAUNCH(c, s, MI_K_CLAHE_INTERP, nv12_bgr_clahe_interp_frames_kernel<0>, grid, dim3(kThreads), lds, *fl, j, g, luts, subs, groups);
        return MI_OK;
    }
    if (order == MI_ORDER_RGB)
        LAUNCH(c, s, MI_K_CLAHE_INTERP, nv12_bgr_clahe_interp_kernel<1>, grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    else
        LAUNCH(c, s, MI_K_CLAHE_INTERP, nv12_bgr_clahe_interp_kernel<0>, grid, dim3(kThreads), lds, j, g, luts, subs, groups);
    return MI_OK;
}

mi_status clahe_nv12_bgr_dev(mi_ctx* c, hipStream_t s, const Nv12BgrArgs& a, double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g;
    mi_status st = clahe_geometry(c, a.width, a.height, clip_limit, tiles_x, tiles_y, &g);
    if (st) return st;
    const int tiles = tiles_x * tiles_y;
    const bool onepass = nv12_bgr_onepass_shape(g, a.width, a.height, tiles_x, tiles_y) && nv12_bgr_aligned16(a);
    const PlaneArgs ya = nv12_bgr_y_plane(a);
    if (onepass) {
        for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
            const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
            if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
            if ((st = launch_tile_luts(c, s, ya, g, f0, nf, c->d_luts))) return st;
            const Nv12BgrJob j = nv12_bgr_job(a, f0, a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame);
            if ((st = launch_nv12_bgr_interp(c, s, j, g, nf, a.order, c->d_luts))) return st;
        }
        ++c->nv12_bgr_onepass;
        return MI_OK;
    }
    // fallback: the planar CLAHE into tight scratch Y planes (each 16-byte aligned), then the decode alone
    const size_t plane = ((size_t)a.width * a.height + 15) & ~(size_t)15;
    const int chunk = std::min(kNv12BgrFramesPerLaunch, a.n_frames);
    if ((st = grow_dev(c, &c->d_planes, &c->planes_bytes, plane * (size_t)chunk))) return st;
    for (int f0 = 0; f0 < a.n_frames; f0 += kNv12BgrFramesPerLaunch) {
        const int nf = std::min(kNv12BgrFramesPerLaunch, a.n_frames - f0);
        const PlaneArgs pa{a.y + (size_t)f0 * a.in_frame, a.y_pitch, a.in_frame, c->d_planes, (size_t)a.width, plane, a.width, a.height, nf};
        if ((st = clahe_dev(c, s, pa, clip_limit, tiles_x, tiles_y, nullptr))) return st;
        const Nv12BgrJob j = nv12_bgr_job(a, f0, c->d_planes, (size_t)a.width, plane);
        if ((st = launch_nv12_to_bgr(c, s, j, nf, a.order, nullptr))) return st;
    }
    ++c->nv12_bgr_twopass;
    return MI_OK;
}

// One tight host NV12 frame up (1.5 B/px), one CV_8UC3 image back (3 B/px), as mi_nv12_bgr_equalize / mi_cvt_color_420_u8 stage
// theirs: pinned tight images are DMA'd as they are, everything else goes through the context's pinned staging; every error exit
// after the first copy on caller memory drains the stream first.
mi_status nv12_bgr_host(mi_ctx* c, const uint8_t* nv12_in, uint8_t* out, size_t out_step, int width, int height, int order,
                        bool is_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    // (the UV plane lies behind the Y plane: for the checks the frame pointer stands for both)
    const Nv12BgrArgs a{nv12_in, (size_t)std::max(width, 0), nv12_in, (size_t)std::max(width, 0), 0, out, out_step, 0, width, height, 1, order};
    bool work = false;
    mi_status st = check_nv12_bgr(c, a, is_clahe, tiles_x, tiles_y, &work);
    if (st || !work) return st;
    const size_t ysz = (size_t)width * height, in_bytes = ysz * 3 / 2, row = 3 * (size_t)width, out_bytes = row * height;
    if ((long long)width * height > 0x7fffffffLL / 3) return fail(c, MI_ERR_UNSUPPORTED, "image too large");
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    if ((st = stage_in(c, s, nv12_in, in_bytes, in_bytes, 1, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, out_bytes))) return st;
    const Nv12BgrArgs d{c->d_stage_in, (size_t)width, c->d_stage_in + ysz, (size_t)width, in_bytes, c->d_stage_out, row, out_bytes,
                        width, height, 1, order};
    st = is_clahe ? clahe_nv12_bgr_dev(c, s, d, clip_limit, tiles_x, tiles_y) : equalize_nv12_bgr_dev(c, s, d);
    if (st) return st;
    return stage_out(c, s, out, out_step, row, (size_t)height, drain);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_nv12_to_bgr_batch_dev(mi_ctx* c, const void* d_y, size_t y_pitch, const void* d_uv, size_t uv_pitch,
                                                 size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride,
                                                 int width, int height, int n_frames, int order, void* stream)
{
    ENTER_COMPUTE(c);
    const Nv12BgrArgs a{(const uint8_t*)d_y, y_pitch, (const uint8_t*)d_uv, uv_pitch, in_frame_stride, (uint8_t*)d_out, out_pitch,
                        out_frame_stride, width, height, n_frames, order};
    bool work = false;
    const mi_status st = check_nv12_bgr(c, a, false, 0, 0, &work);
    return (st || !work) ? st : equalize_nv12_bgr_dev(c, pick_stream(c, stream), a);
}

mi_status mi_clahe_nv12_to_bgr_batch_dev(mi_ctx* c, const void* d_y, size_t y_pitch, const void* d_uv, size_t uv_pitch,
                                         size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride,
                                         int width, int height, int n_frames, int order,
                                         double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const Nv12BgrArgs a{(const uint8_t*)d_y, y_pitch, (const uint8_t*)d_uv, uv_pitch, in_frame_stride, (uint8_t*)d_out, out_pitch,
                        out_frame_stride, width, height, n_frames, order};
    bool work = false;
    const mi_status st = check_nv12_bgr(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : clahe_nv12_bgr_dev(c, pick_stream(c, stream), a, clip_limit, tiles_x, tiles_y);
}

mi_status mi_equalize_hist_nv12_to_bgr(mi_ctx* c, const uint8_t* nv12_in, uint8_t* out, size_t out_step, int width, int height, int order)
{
    ENTER_COMPUTE(c);
    return nv12_bgr_host(c, nv12_in, out, out_step, width, height, order, false, 0.0, 0, 0);
}

mi_status mi_clahe_nv12_to_bgr(mi_ctx* c, const uint8_t* nv12_in, uint8_t* out, size_t out_step, int width, int height, int order,
                               double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    return nv12_bgr_host(c, nv12_in, out, out_step, width, height, order, true, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
