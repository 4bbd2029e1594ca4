// packed422_bgr_frames.inc.hpp -- packed 4:2:2 in (YUY2 / UYVY), interleaved BGR / RGB out on a LIST of device frames
// (mi_*_packed422_to_bgr_frames_dev): checks, chunking, extern "C"
// Included by ../mi_lumaeq.hip after packed422_bgr.inc.hpp (one translation unit; not a stand-alone header).
//
// Neither end of a capture -> display / image writer / model pipeline is one allocation at a fixed frame stride: the capture card hands
// out a buffer pool (packed422_frames.inc.hpp), the images go to a pool of tensors or cv::Mats.  The list form joins the two: the call
// is cut into chunks of at most kPacked422FramesPerLaunch frames; a chunk's inputs travel to the histogram stages as a Packed422List
// whose out mirrors in (they only read), its {in, out} pairs to the writers as a second Packed422List, both by value in the kernel
// arguments, through the stage sequences of packed422.inc.hpp with the BgrOut writer -- same grids, same tile splits, same bytes as the
// batch form, every shape in one pass.  Each frame takes the vector or the byte store path by its own address (Table422Bgr::wide_of).
// The check and the chunk loop are templates on the pixel form F of packed422_bgr.inc.hpp, written once for every form.

namespace {

struct P422BgrFramesShape {
    int width, height;
    size_t in_pitch, out_pitch;
    int format, order;
};

// Everything is checked before anything is enqueued: a refused call writes nothing.  *work = false: MI_OK with nothing to do.
template <class F>
mi_status check_packed422_bgr_frames(mi_ctx* c, const mi_packed422_bgr_frame_dev* frames, int n_frames, const P422BgrFramesShape& s,
                                     bool is_clahe, int tiles_x, int tiles_y, bool* work)
{
    *work = false;
    if (n_frames > 0 && !frames) return fail(c, MI_ERR_BAD_ARG, "null frame list");
    // the shape: check_packed422_bgr's own answers (order, format, even width, sizes, tiles, the pitches, the tile grids and heights the
    // stage sequences would refuse), on stand-in addresses that pass its pointer checks
    const P422BgrArgs shape = p422_bgr_args((const void*)16, s.in_pitch, 0, (void*)32, s.out_pitch, 0, s.width, s.height, n_frames,
                                            s.format, s.order);
    bool any = false;
    const mi_status st = check_packed422_bgr<F>(c, shape, is_clahe, tiles_x, tiles_y, &any);
    if (st || !any) return st;
    const size_t w = (size_t)s.width, rows = (size_t)s.height;
    for (int k = 0; k < n_frames; ++k) {
        const mi_packed422_bgr_frame_dev& f = frames[k];
        if (!f.in || !f.out) return fail(c, MI_ERR_BAD_ARG, "null frame pointer");
        if ((uintptr_t)f.in & 3) return fail(c, MI_ERR_BAD_ARG, "packed 4:2:2 frame addresses are multiples of 4");
        // there is no in-place form (2 bytes per pixel in, kPx out): the image's rows may not meet the rows of its own input
        if (Span(f.out, s.out_pitch, F::kPx * w, rows).meets(Span(f.in, s.in_pitch, 2 * w, rows)))
            return fail(c, MI_ERR_BAD_ARG, F::kListOverlap);
    }
    *work = true;
    return MI_OK;
}

// op: 0 equalizeHist, 1 CLAHE
template <class F>
mi_status packed422_bgr_frames_dev(mi_ctx* c, hipStream_t s, const mi_packed422_bgr_frame_dev* frames, int n_frames,
                                   const P422BgrFramesShape& sh, int op, double clip_limit, int tiles_x, int tiles_y)
{
    unsigned long long n_wide = 0;
    for (int f0 = 0; f0 < n_frames; f0 += kPacked422FramesPerLaunch) {
        const int nf = std::min(kPacked422FramesPerLaunch, n_frames - f0);
        Packed422List in{};                                          // this chunk's frames of the list, from index 0: the inputs for the
        Packed422List io{};                                          // histogram stages (out mirrors in), the {in, out} pairs for the writers
        for (int k = 0; k < nf; ++k) {
            const mi_packed422_bgr_frame_dev& f = frames[f0 + k];
            in.f[k] = Packed422Frame{(const uint8_t*)f.in, (uint8_t*)const_cast<void*>(f.in)};
            io.f[k] = Packed422Frame{(const uint8_t*)f.in, (uint8_t*)f.out};
            n_wide += packed422_image_wide(f.out, (long long)sh.out_pitch, 0);     // a frame's store path: its own address and the pitch
        }
        // a table launch ignores the block's base addresses and frame strides: a null image base and stride 0 leave its `wide` to
        // out_pitch % 4 == 0 alone (packed422_bgr_batch), and every frame adds its own address in the kernel
        const P422BgrArgs a = p422_bgr_args(io.f[0].in, sh.in_pitch, 0, nullptr, sh.out_pitch, 0, sh.width, sh.height, nf, sh.format, sh.order);
        const mi_status st = packed422_bgr_dev<F>(c, s, a, op, clip_limit, tiles_x, tiles_y, &in, &io);
        if (st) return st;
    }
    // the FRAMES by the store path their pixel-writing kernel took, once the whole call is enqueued
    F::count_list(c, n_frames, n_wide);
    return MI_OK;
}

}  // namespace

extern "C" {

mi_status mi_equalize_hist_packed422_to_bgr_frames_dev(mi_ctx* c, const mi_packed422_bgr_frame_dev* frames, int n_frames,
                                                       int width, int height, size_t in_pitch, size_t out_pitch, int format, int order,
                                                       void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrFramesShape sh{width, height, in_pitch, out_pitch, format, order};
    bool work = false;
    const mi_status st = check_packed422_bgr_frames<Bgr422Image>(c, frames, n_frames, sh, false, 0, 0, &work);
    return (st || !work) ? st : packed422_bgr_frames_dev<Bgr422Image>(c, pick_stream(c, stream), frames, n_frames, sh, 0, 0.0, 0, 0);
}

mi_status mi_clahe_packed422_to_bgr_frames_dev(mi_ctx* c, const mi_packed422_bgr_frame_dev* frames, int n_frames,
                                               int width, int height, size_t in_pitch, size_t out_pitch, int format, int order,
                                               double clip_limit, int tiles_x, int tiles_y, void* stream)
{
    ENTER_COMPUTE(c);
    const P422BgrFramesShape sh{width, height, in_pitch, out_pitch, format, order};
    bool work = false;
    const mi_status st = check_packed422_bgr_frames<Bgr422Image>(c, frames, n_frames, sh, true, tiles_x, tiles_y, &work);
    return (st || !work) ? st : packed422_bgr_frames_dev<Bgr422Image>(c, pick_stream(c, stream), frames, n_frames, sh, 1, clip_limit, tiles_x, tiles_y);
}

}  // extern "C"
