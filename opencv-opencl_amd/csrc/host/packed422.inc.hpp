// packed422.inc.hpp -- equalizeHist and CLAHE on packed 4:2:2 frames (YUY2 / UYVY): checks, launch sequences, extern "C" entry points
// Included by ../mi_lumaeq.hip (one translation unit; not a stand-alone header).
//
// A capture device's frame has no Y plane: luma sample (x, y) is byte y * pitch + 2 * x + off.  The stage sequences are those of the
// planar forms -- histogram partials -> equalize_lut_kernel -> apply; tile histograms (-> tile_lut_kernel) -> interpolation -- with the
// four pixel-touching kernels of kernels/packed422.hip.h, the same scratch, grids and splits, and the chroma written by the kernel that
// writes the luma (one dword per macropixel).  Never the fused kernel and never hist_lut_kernel: option two_kernel_max_frames does not
// apply (the bytes are the same on every path).

namespace {

struct P422Args {
    const uint8_t* in; size_t in_pitch, in_frame;
    uint8_t* out; size_t out_pitch, out_frame;
    int width, height, n_frames, format;
    mi_uv_mode uv_mode;
};

// Everything is checked before anything is enqueued.  *work = false: MI_OK with nothing to do.
mi_status check_packed422(mi_ctx* c, const P422Args& a, bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (a.format != MI_FMT_YUY2 && a.format != MI_FMT_UYVY) return fail(c, MI_ERR_BAD_ARG, "format must be MI_FMT_YUY2 or MI_FMT_UYVY");
    if (a.uv_mode != MI_UV_FILL128 && a.uv_mode != MI_UV_COPY) return fail(c, MI_ERR_BAD_ARG, "bad uv_mode");
    if (a.width < 0 || a.height < 0 || a.n_frames < 0) return fail(c, MI_ERR_BAD_ARG, "negative size");
    if (is_clahe && (tiles_x <= 0 || tiles_y <= 0)) return fail(c, MI_ERR_BAD_ARG, "tile grid must be >= 1x1");
    if (a.width & 1) return fail(c, MI_ERR_BAD_ARG, "4:2:2 frames have an even width");
    if (a.width == 0 || a.height == 0 || a.n_frames == 0) return MI_OK;
    if (!a.in || !a.out) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
    if (a.in_pitch < 2 * (size_t)a.width || a.out_pitch < 2 * (size_t)a.width) return fail(c, MI_ERR_BAD_ARG, "pitch < 2 * width");
    if (((uintptr_t)a.in | (uintptr_t)a.out | a.in_pitch | a.out_pitch | a.in_frame | a.out_frame) & 3)
        return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 pointers, pitches and frame strides are multiples of 4");
    if ((long long)a.width * a.height > 0x7fffffffLL) return fail(c, MI_ERR_UNSUPPORTED, "width*height must be < 2^31 (OpenCV: int total)");
    if (a.width > (1 << 24) || a.height > (1 << 24)) return fail(c, MI_ERR_UNSUPPORTED, "width/height must be <= 2^24");
    *work = true;
    return MI_OK;
}

Packed422 packed422_batch(const P422Args& a, int f0)
{
    Packed422 p;
    p.src = a.in + (size_t)f0 * a.in_frame; p.dst = a.out + (size_t)f0 * a.out_frame;
    p.src_step = (long long)a.in_pitch; p.dst_step = (long long)a.out_pitch;
    p.src_frame = (long long)a.in_frame; p.dst_frame = (long long)a.out_frame;
    p.dwords = a.width / 2; p.rows = a.height;
    const uint32_t chroma = a.format == MI_FMT_UYVY ? 0x00ff00ffu : 0xff00ff00u;
    p.keep = a.uv_mode == MI_UV_COPY ? chroma : 0u;
    p.fill = a.uv_mode == MI_UV_COPY ? 0u : (0x80808080u & chroma);
    return p;
}

// The two entries of one kernel body: `frames` takes a chunk of a frame list in front of the arguments of `batch`.
template <class KF, class KB> struct KernelPair { KF frames; KB batch; };
template <class KF, class KB> KernelPair(KF, KB) -> KernelPair<KF, KB>;

// One launch of a pair: the list entry when the call came with a frame list, else the batch entry.
template <class KF, class KB, class L, class... A>
mi_status launch_pair(mi_ctx* c, hipStream_t s, int kid, const KernelPair<KF, KB>& k, const L* fl, dim3 grid, dim3 block, size_t lds,
                      const A&... args)
{
    if (fl) LAUNCH(c, s, kid, k.frames, grid, block, lds, *fl, args...);
    else    LAUNCH(c, s, kid, k.batch, grid, block, lds, args...);
    return MI_OK;
}

// The stage sequences below are written once for every writer of packed input: W says what the last stage writes.
//   Args          the host-side arguments of a call; input(a) is their packed side, all that the histogram stages see
//   Block         the argument block of the writer's kernels, cut(a, f0) for the chunk of frames from f0
//   List          the frame list its *_frames_kernel entries take
//   apply_rows(h) the row units the LUT-apply grid is sized by
//   K<OFF>        its kernels for luma byte offset OFF
// PackedOut writes a packed frame; Nv12Out (packed422_nv12.inc.hpp) a Y plane and a UV plane.
struct PackedOut {
    using Args = P422Args;
    using Block = Packed422;
    using List = Packed422List;
    static const P422Args& input(const Args& a) { return a; }
    static Block cut(const Args& a, int f0) { return packed422_batch(a, f0); }
    static int apply_rows(int height) { return height; }
    template <int OFF> struct K {
        static constexpr KernelPair apply{lut_apply422_frames_kernel<OFF>, lut_apply422_kernel<OFF>};
        static constexpr KernelPair interp_global{clahe_interp422_global_frames_kernel<OFF>, clahe_interp422_global_kernel<OFF>};
        template <bool FT, bool FMA>
        static constexpr KernelPair interp{clahe_interp422_frames_kernel<FT, FMA, OFF>, clahe_interp422_kernel<FT, FMA, OFF>};
    };
};

// The sequences take an optional chunk of a frame list (at most kPacked422FramesPerLaunch frames, input(a).n_frames of them, indices
// from 0) as the histogram stages' Packed422List (they only read: a writer that has a list type of its own hands them one whose out
// mirrors in) and as the writer's own list, both or neither: with one, every launch goes to the *_frames_kernel entry of the same
// body -- same grids, same splits, same scratch -- and the base addresses and frame strides of `a` are not used.
template <class W, int OFF>
mi_status equalize422_dev(mi_ctx* c, hipStream_t s, const typename W::Args& a, const Packed422List* fl_in, const typename W::List* fl_out)
{
    const P422Args& in = W::input(a);
    const long long frame_bytes = 2LL * in.width * in.height;
    for (int f0 = 0; f0 < in.n_frames; f0 += kMaxGridY) {
        const int nf = std::min(kMaxGridY, in.n_frames - f0);
        const int B = blocks_per_frame(c, frame_bytes, in.height, nf, 256);
        mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * B * 256 * sizeof(uint32_t));
        if (st) return st;
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * 256))) return st;
        if ((st = launch_pair(c, s, MI_K_HIST, KernelPair{hist422_partial_frames_kernel<OFF>, hist422_partial_kernel<OFF>}, fl_in,
                              dim3(B, nf), dim3(kHistThreads), 0, packed422_batch(in, f0), c->d_partial))) return st;
        LAUNCH(c, s, MI_K_EQ_LUT, equalize_lut_kernel, dim3(nf), dim3(kThreads), 0,
               (const uint32_t*)c->d_partial, B, (int)((long long)in.width * in.height), c->d_luts, (int32_t*)nullptr);
        const int BA = blocks_per_frame(c, frame_bytes, W::apply_rows(in.height), nf, 2048);
        if ((st = launch_pair(c, s, MI_K_LUT_APPLY, W::template K<OFF>::apply, fl_out, dim3(BA, nf), dim3(kThreads), 0,
                              W::cut(a, f0), (const uint8_t*)c->d_luts))) return st;
    }
    return MI_OK;
}

// launch_tile_luts' splits and tile order (one tile per workgroup: the multi-tile variant has no packed sibling)
template <int OFF>
mi_status launch_tile_luts422(mi_ctx* c, hipStream_t s, const Packed422& p, const ClaheGeom& g, int nf, uint8_t* d_luts_out,
                              const Packed422List* fl)
{
    const int tiles = g.tiles_x * g.tiles_y;
    const long long tile_px = (long long)g.tile_w * g.tile_h;
    const long long want = tile_px >= 65536 ? (long long)c->cu_count / ((long long)tiles * nf) : 1;
    const int S = (int)std::max<long long>(1, std::min<long long>({want, (long long)std::max(1, g.tile_h / 8), 64LL}));
    mi_status st = grow_dev(c, &c->d_partial, &c->partial_bytes, (size_t)nf * tiles * S * 256 * sizeof(uint32_t));
    if (st) return st;
    if (tiles > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "more than 65535 tiles per frame");
    uint8_t* direct = S == 1 ? d_luts_out : nullptr;
    const int xcd_map = (c->clahe_xcd_map && S == 1 && tiles % 8 == 0) ? 1 : 0;
    if (fl) LAUNCH(c, s, MI_K_TILE_HIST, (tile_hist422_frames_kernel<OFF, 512>), dim3(S, tiles, nf), dim3(512), 0,
                   *fl, p.src_step, g, c->d_partial, direct, xcd_map);
    else    LAUNCH(c, s, MI_K_TILE_HIST, (tile_hist422_kernel<OFF, 512>), dim3(S, tiles, nf), dim3(512), 0,
                   p.src, p.src_step, p.src_frame, g, c->d_partial, direct, xcd_map);
    if (!direct)
        LAUNCH(c, s, MI_K_TILE_LUT, tile_lut_kernel, dim3(tiles, nf), dim3(kThreads), 0, (const uint32_t*)c->d_partial, S, g, d_luts_out);
    return MI_OK;
}

// launch_interp's choice of tables, column segments, bands and sub-bands, the same for every writer of packed input.  global: the
// grid is too wide for the LDS pair table.
struct Interp422Plan {
    bool global, float_tables;
    dim3 grid;
    size_t lds;
    int subs, groups, cap;
};
mi_status plan_interp422(mi_ctx* c, const ClaheGeom& g, int dwords, int nf, Interp422Plan* pl)
{
    const int npairs = g.tiles_x + 1;
    pl->global = npairs > kMaxPairsLds;
    pl->float_tables = false; pl->lds = 0; pl->subs = pl->groups = pl->cap = 0;
    if (pl->global) {
        if (g.height > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "height > 65535 with tiles_x > 62");
        pl->grid = dim3((dwords + kThreads - 1) / kThreads, g.height, nf);
        return MI_OK;
    }
    const int ngroups = (g.width + kInterpPx - 1) / kInterpPx;
    int groups = std::min(ngroups, kThreads);
    bool seg_tables = false;
    const int seg_cap = std::max(4, std::min(c->clahe_seg_pairs, kMaxPairsLdsF32));
    if (npairs > kMaxPairsLdsF32 && c->clahe_float_tables) {
        const int gmax = (int)(((long long)(seg_cap - 3) * g.tile_w) / kInterpPx);
        if (gmax >= 40) {
            const int nseg = (ngroups + std::min(groups, gmax) - 1) / std::min(groups, gmax);
            groups = (ngroups + nseg - 1) / nseg;
            seg_tables = true;
        }
    }
    const int segs = (ngroups + groups - 1) / groups;
    const int bands = g.tiles_y + 1;
    const long long want = ((long long)c->cu_count * 8 + (long long)bands * nf * segs - 1) / ((long long)bands * nf * segs);
    const int rows_per_band = g.tile_h + 2 * kBandMargin;
    const int subs = (int)std::max<long long>(1, std::min<long long>({want, (long long)std::max(1, rows_per_band / 8), 64LL}));
    if ((long long)bands * subs > 0x7fffffffLL || segs > kMaxGridY) return fail(c, MI_ERR_UNSUPPORTED, "image too wide");
    pl->grid = dim3(bands * subs, nf, segs);
    pl->subs = subs; pl->groups = groups;
    if ((npairs <= kMaxPairsLdsF32 || seg_tables) && c->clahe_float_tables) {
        pl->float_tables = true;
        pl->cap = seg_tables ? seg_cap : kMaxPairsLdsF32;
        pl->lds = (size_t)std::min(npairs, pl->cap) * 256 * 4 * sizeof(float);
    } else {
        pl->cap = kMaxPairsLds + 1;
        pl->lds = (size_t)npairs * 256 * sizeof(uint32_t);
    }
    return MI_OK;
}

// The one place that picks an interpolation kernel: the writer's family for the plan's tables, the arithmetic mode and OFF
template <class W, int OFF>
mi_status launch_interp422(mi_ctx* c, hipStream_t s, const typename W::Block& p, const ClaheGeom& g, int nf, const uint8_t* d_luts,
                           const typename W::List* fl)
{
    using K = typename W::template K<OFF>;
    Interp422Plan pl;
    if (mi_status st = plan_interp422(c, g, p.dwords, nf, &pl)) return st;
    if (pl.global) return launch_pair(c, s, MI_K_CLAHE_INTERP, K::interp_global, fl, pl.grid, dim3(kThreads), 0, p, g, d_luts);
    const auto lds_tables = [&](const auto& k) {
        return launch_pair(c, s, MI_K_CLAHE_INTERP, k, fl, pl.grid, dim3(kThreads), pl.lds, p, g, d_luts, pl.subs, pl.groups, pl.cap);
    };
    if (pl.float_tables) return g.contract ? lds_tables(K::template interp<true, true>) : lds_tables(K::template interp<true, false>);
    return g.contract ? lds_tables(K::template interp<false, true>) : lds_tables(K::template interp<false, false>);
}

template <class W, int OFF>
mi_status clahe422_dev(mi_ctx* c, hipStream_t s, const typename W::Args& a, double clip_limit, int tiles_x, int tiles_y,
                       const Packed422List* fl_in, const typename W::List* fl_out)
{
    const P422Args& in = W::input(a);
    ClaheGeom g;
    mi_status st = clahe_geometry(c, in.width, in.height, clip_limit, tiles_x, tiles_y, &g);
    if (st) return st;
    const int tiles = tiles_x * tiles_y;
    for (int f0 = 0; f0 < in.n_frames; f0 += kMaxGridY) {
        const int nf = std::min(kMaxGridY, in.n_frames - f0);
        if ((st = grow_dev(c, &c->d_luts, &c->luts_bytes, (size_t)nf * tiles * 256))) return st;
        if ((st = launch_tile_luts422<OFF>(c, s, packed422_batch(in, f0), g, nf, c->d_luts, fl_in))) return st;
        if ((st = launch_interp422<W, OFF>(c, s, W::cut(a, f0), g, nf, c->d_luts, fl_out))) return st;
    }
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE.  `a` has passed the checks of its form (check_packed422*).
template <class W>
mi_status packed422_dev(mi_ctx* c, hipStream_t s, const typename W::Args& a, int op, double clip_limit, int tiles_x, int tiles_y,
                        const Packed422List* fl_in = nullptr, const typename W::List* fl_out = nullptr)
{
    if (W::input(a).format == MI_FMT_UYVY)
        return op ? clahe422_dev<W, 1>(c, s, a, clip_limit, tiles_x, tiles_y, fl_in, fl_out) : equalize422_dev<W, 1>(c, s, a, fl_in, fl_out);
    return op ? clahe422_dev<W, 0>(c, s, a, clip_limit, tiles_x, tiles_y, fl_in, fl_out) : equalize422_dev<W, 0>(c, s, a, fl_in, fl_out);
}

// Host frame: the whole frame goes up and comes back (there is no luma plane to send on its own), tight on the device; pinned tight
// frames are DMA'd as they are, anything else through the context's pinned staging (stage_in / stage_out, which drain the stream on
// every error exit).  Only the 2 * W bytes of each row are read and written.
mi_status packed422_host(mi_ctx* c, const P422Args& h, int op, double clip_limit, int tiles_x, int tiles_y)
{
    const size_t row = 2 * (size_t)h.width, bytes = row * h.height;
    hipStream_t s = c->stream;
    StreamDrain drain(HipStreamSync{}, drain_counter(c));
    mi_status st;
    if ((st = stage_in(c, s, h.in, h.in_pitch, row, (size_t)h.height, drain))) return st;
    if ((st = grow_dev(c, &c->d_stage_out, &c->stage_out_bytes, bytes))) return st;
    P422Args d = h;
    d.in = c->d_stage_in; d.in_pitch = row; d.in_frame = bytes;
    d.out = c->d_stage_out; d.out_pitch = row; d.out_frame = bytes;
    if ((st = packed422_dev<PackedOut>(c, s, d, op, clip_limit, tiles_x, tiles_y))) return st;
    return stage_out(c, s, h.out, h.out_pitch, row, (size_t)h.height, drain);
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                               void* d_out, size_t out_pitch, size_t out_frame_stride,
                                               int width, int height, int n_frames, int format, mi_uv_mode uv_mode, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Args a{(const uint8_t*)d_in, in_pitch, in_frame_stride, (uint8_t*)d_out, out_pitch, out_frame_stride, width, height, n_frames, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422(c, a, false, 0, 0, &work);
    return (st || !work) ? st : packed422_dev<PackedOut>(c, pick_stream(c, stream), a, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_batch_dev(mi_ctx* c, const void* d_in, size_t in_pitch, size_t in_frame_stride,
                                       void* d_out, size_t out_pitch, size_t out_frame_stride,
                                       int width, int height, int n_frames, int format, mi_uv_mode uv_mode,
                                       double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422Args a{(const uint8_t*)d_in, in_pitch, in_frame_stride, (uint8_t*)d_out, out_pitch, out_frame_stride, width, height, n_frames, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_dev<PackedOut>(c, pick_stream(c, stream), a, 1, clip_limit, tiles_x, tiles_y);
}

mi_status mi_equalize_hist_packed422(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_pitch,
                                     int width, int height, int format, mi_uv_mode uv_mode)
{
    ENTER_COMPUTE(c);
    const P422Args a{in, in_pitch, 0, out, out_pitch, 0, width, height, 1, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422(c, a, false, 0, 0, &work);
    return (st || !work) ? st : packed422_host(c, a, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422(mi_ctx* c, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_pitch,
                             int width, int height, int format, mi_uv_mode uv_mode, double clip_limit, int tiles_x, int tiles_y)
{
    ENTER_COMPUTE(c);
    const P422Args a{in, in_pitch, 0, out, out_pitch, 0, width, height, 1, format, uv_mode};
    bool work = false;
    const mi_status st = check_packed422(c, a, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_host(c, a, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
