"""The strided device batch forms on pitched, guarded layouts (run with -m gpu on an MI355X).

Every *_batch_dev entry takes a row pitch and a frame stride per side and the library branches on them: flattened or row-wise
addressing, 16-byte or byte accesses, one pass or through scratch planes.  Tight layouts reach one side of each branch only.  Here
every side of a call is a tests/strided_layouts.py Side -- frames inside one sentinel-filled allocation with guard bytes -- and whole
allocations are compared with the oracle's bytes, inputs included: a wrong pitch or stride term, or a vector store that runs into the
padding, fails like a wrong pixel does.  Exact bytes throughout, three frames of different content unless a group says otherwise."""
import functools

import numpy as np
import pytest

import mi_lumaeq
import oracle
import strided_layouts as L
from mi_lumaeq import xfer

pytestmark = pytest.mark.gpu

N = 3
ALL = list(L.PAIRINGS)


def sync():
    import torch
    torch.cuda.synchronize()


def dev_filled(shape, dtype, value):
    """A plain device tensor (numpy dtype) for the outputs that have no pitch: histograms, LUTs, statistics."""
    return xfer.to_device(np.full(shape, value, dtype))


def strides(src, dst):
    return dict(src_step=src.pitch, src_frame=src.frame_stride, dst_step=dst.pitch, dst_frame=dst.frame_stride)


def check(src, dst, frames, want, call, why):
    """Upload `frames` into src (dst, when it is another Side, stays sentinel), run call(src, dst), compare both allocations whole."""
    src.upload(frames)
    if dst is not src:
        dst.upload(None)
    for s in (src, dst):
        assert s.buf.data_ptr() % 16 == 0, "the layout classes count on a 16-byte aligned allocation"
    call(src, dst)
    sync()
    if dst is src:
        L.assert_sides(src, src.image(want), why)
    else:
        L.assert_sides([src, dst], [src.image(frames), dst.image(want)], why)


def aligned_rows(side):
    """How many rows of the side start 16-byte aligned (the allocation is), and how many rows there are."""
    rows = [(side.off + k * side.frame_stride + r * side.pitch) % 16 == 0 for k in range(side.n) for r in range(side.rows)]
    return sum(rows), len(rows)


def u_row1(rows, row_bytes, n):
    """Class U (pitch row_bytes + 1, stride rows * pitch + 7) with `off` chosen so that row 1 of frame 0 is 16-byte aligned: on a few
    rows class U itself may meet no aligned row at all, and then no image mixes vector and byte rows."""
    pitch = row_bytes + 1
    return L.Side(rows, row_bytes, pitch, (16 - pitch) % 16 or 16, n, rows * pitch + 7, "Urow1")


@functools.lru_cache(maxsize=None)
def bgr_frames(w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    return tuple(rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(N))


# ---- a. cvt_color_batch_dev ------------------------------------------------------------------------------------------------------
# Host: color_job() flattens to one row of W*H pixels only when BOTH pitches are 3*W (T, Tgap), else rows are addressed as
# row * src_step / row * dst_step.  Kernel: color_kernel<0/1> takes the 48-byte vector body for a row only when s3 and d3 are both
# 16-byte aligned (a3s && a3d), else one pixel per lane; 48x5 is whole groups, 50x5 groups and a ragged tail, 7x3 no group at all.
@functools.lru_cache(maxsize=None)
def cvt_want(w, h, code):
    f = bgr_frames(w, h)
    return tuple((oracle.bgr2yuv if code == mi_lumaeq.COLOR_BGR2YUV else oracle.yuv2bgr)(x) for x in f)


@pytest.mark.parametrize("pairing", ALL)
@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV, mi_lumaeq.COLOR_YUV2BGR], ids=["BGR2YUV", "YUV2BGR"])
def test_cvt_color(ctx, code, pairing):
    for (w, h) in [(48, 5), (50, 5), (7, 3)]:
        src, dst = L.make_pair(pairing, h, 3 * w, N)
        check(src, dst, bgr_frames(w, h), cvt_want(w, h, code),
              lambda s, d: ctx.cvt_color_batch_dev(s.ptr, d.ptr, w, h, N, code, **strides(s, d)), (pairing, code, w, h))


@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV, mi_lumaeq.COLOR_YUV2BGR], ids=["BGR2YUV", "YUV2BGR"])
def test_cvt_color_vector_and_byte_rows_in_one_image(ctx, code):
    """One side with rows of every alignment, one aligned row among them for certain, against an all-aligned other side."""
    for (w, h) in [(48, 5), (50, 5)]:
        for u_is_src in (True, False):
            u, a = u_row1(h, 3 * w, N), L.make_side("A16", h, 3 * w, N)
            hit, total = aligned_rows(u)
            assert 0 < hit < total
            src, dst = (u, a) if u_is_src else (a, u)
            check(src, dst, bgr_frames(w, h), cvt_want(w, h, code),
                  lambda s, d: ctx.cvt_color_batch_dev(s.ptr, d.ptr, w, h, N, code, **strides(s, d)), (code, w, h, u_is_src))


# ---- b. bgr_luma_op_batch_dev ----------------------------------------------------------------------------------------------------
# bgr_fused 1, OP_EQUALIZE: bgr_luma_hist_kernel (vector groups per row iff s3 is aligned) and bgr_luma_apply_kernel (iff s3 and d3
# are), on color_job() addressing as above.  bgr_fused 1, OP_CLAHE: bgr_luma_dev's shape_ok wants both pointers, both steps and both
# frame strides multiples of 16 -- (A16,A16) and in-place A16 run bgr_tile_hist_kernel + bgr_clahe_interp_kernel, every other pairing
# (and 50x10 with a 3x2 grid always: REFLECT_101 padding) goes through planes.  Through planes (also everything with bgr_fused 0) the
# <2> job is built from the source alone and the <3> job from the destination alone: with (T,A16) the split is flattened, poff = 0,
# and the merge row-wise, poff = row * W; color_kernel's `ap` then sends the rows whose poff is not a multiple of 16 down the byte body.
@functools.lru_cache(maxsize=None)
def luma_want(w, h, op, clip, tx, ty):
    return tuple(oracle.bgr_luma_op(x, op, clip, tx, ty) for x in bgr_frames(w, h, 5))


def luma_case(ctx, pairing, w, h, op, clip=3.0, tx=4, ty=4):
    src, dst = L.make_pair(pairing, h, 3 * w, N)
    check(src, dst, bgr_frames(w, h, 5), luma_want(w, h, op, clip, tx, ty),
          lambda s, d: ctx.bgr_luma_op_batch_dev(s.ptr, d.ptr, w, h, N, op, clip, tx, ty, **strides(s, d)), (pairing, w, h, op, clip, tx, ty))


@pytest.mark.parametrize("fused", [1, 0], ids=["bgr_fused", "planes"])
@pytest.mark.parametrize("pairing", ALL)
def test_bgr_luma_equalize(ctx, pairing, fused):
    try:
        ctx.set_option("bgr_fused", fused)
        for (w, h) in [(48, 6), (50, 5)]:
            luma_case(ctx, pairing, w, h, mi_lumaeq.OP_EQUALIZE)
    finally:
        ctx.set_option("bgr_fused", 1)


@pytest.mark.parametrize("fused", [1, 0], ids=["bgr_fused", "planes"])
def test_bgr_luma_equalize_vector_and_byte_rows_in_one_image(ctx, fused):
    try:
        ctx.set_option("bgr_fused", fused)
        for (w, h) in [(48, 6), (50, 5)]:
            for u_is_src in (True, False):
                u, a = u_row1(h, 3 * w, N), L.make_side("A16", h, 3 * w, N)
                src, dst = (u, a) if u_is_src else (a, u)
                check(src, dst, bgr_frames(w, h, 5), luma_want(w, h, mi_lumaeq.OP_EQUALIZE, 3.0, 4, 4),
                      lambda s, d: ctx.bgr_luma_op_batch_dev(s.ptr, d.ptr, w, h, N, mi_lumaeq.OP_EQUALIZE, **strides(s, d)),
                      (fused, w, h, u_is_src))
    finally:
        ctx.set_option("bgr_fused", 1)


@pytest.mark.parametrize("fused", [1, 0], ids=["bgr_fused", "planes"])
@pytest.mark.parametrize("pairing", ["A16-A16", "inplace-A16", "U-A16", "A16-U", "T-A16"])
def test_bgr_luma_clahe_one_pass_or_planes(ctx, pairing, fused):
    """64x8, grid 2x2 (tile_w 32, no padding): the one-pass kernels where shape_ok holds, the planes elsewhere -- the same bytes."""
    try:
        ctx.set_option("bgr_fused", fused)
        luma_case(ctx, pairing, 64, 8, mi_lumaeq.OP_CLAHE, 2.0, 2, 2)
    finally:
        ctx.set_option("bgr_fused", 1)


@pytest.mark.parametrize("fused", [1, 0], ids=["bgr_fused", "planes"])
@pytest.mark.parametrize("pairing", ["A16-A16", "U-U", "T-A16", "A16-T"])
def test_bgr_luma_clahe_never_one_pass(ctx, pairing, fused):
    try:
        ctx.set_option("bgr_fused", fused)
        luma_case(ctx, pairing, 50, 10, mi_lumaeq.OP_CLAHE, 3.0, 3, 2)
    finally:
        ctx.set_option("bgr_fused", 1)


# ---- c. cvt_color_420_batch_dev --------------------------------------------------------------------------------------------------
# Host: cvt420_dev's `vec` needs W % 16 == 0 and both addresses, c3_step, c3_frame and planar_frame multiples of 16: 32x4 with T or A16
# against a planar stride of tight or tight + 16 is the 16 x 2 group body of cvt420_kernel, everything else (18x6; Tgap, U; tight + 5)
# the 2 x 2 block body.  The planar side must be tight (step == W): anything else is MI_ERR_UNSUPPORTED before a launch.
def planar_side(w, h, stride_extra, pitch_extra=0):
    rows = h * 3 // 2
    return L.Side(rows, w, w + pitch_extra, 0, N, rows * (w + pitch_extra) + stride_extra, f"planar+{stride_extra}")


@functools.lru_cache(maxsize=None)
def nv12_frames(w, h, seed=0):
    rng = np.random.default_rng(77 * w + h + seed)
    return tuple(rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for _ in range(N))


@functools.lru_cache(maxsize=None)
def c420_case(w, h, enc):
    if enc:
        f = bgr_frames(w, h, 9)
        return f, tuple(oracle.bgr_to_i420(x) for x in f)
    f = nv12_frames(w, h)
    return f, tuple(oracle.nv12_to_bgr(x, w, h) for x in f)


@pytest.mark.parametrize("c3", ["T", "Tgap", "A16", "U"])
@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV_I420, mi_lumaeq.COLOR_YUV2BGR_NV12], ids=["BGR2YUV_I420", "YUV2BGR_NV12"])
def test_cvt_color_420(ctx, code, c3):
    enc = code == mi_lumaeq.COLOR_BGR2YUV_I420
    for (w, h) in [(32, 4), (18, 6)]:
        frames, want = c420_case(w, h, enc)
        for extra in (0, 16, 5):
            c3_side, pl = L.make_side(c3, h, 3 * w, N), planar_side(w, h, extra)
            src, dst = (c3_side, pl) if enc else (pl, c3_side)
            check(src, dst, frames, want, lambda s, d: ctx.cvt_color_420_batch_dev(s.ptr, d.ptr, w, h, N, code, **strides(s, d)),
                  (code, c3, w, h, extra))


@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV_I420, mi_lumaeq.COLOR_YUV2BGR_NV12], ids=["BGR2YUV_I420", "YUV2BGR_NV12"])
def test_cvt_color_420_pitched_planar_side_is_refused(ctx, code):
    enc = code == mi_lumaeq.COLOR_BGR2YUV_I420
    w, h = 32, 4
    frames, _ = c420_case(w, h, enc)
    c3_side, pl = L.make_side("A16", h, 3 * w, N), planar_side(w, h, 16, pitch_extra=16)
    src, dst = (c3_side, pl) if enc else (pl, c3_side)
    src.upload(frames); dst.upload(None)
    with pytest.raises(mi_lumaeq.MiError) as e:
        ctx.cvt_color_420_batch_dev(src.ptr, dst.ptr, w, h, N, code, **strides(src, dst))
    assert e.value.status == 2                                      # MI_ERR_UNSUPPORTED
    sync()
    L.assert_sides([src, dst], [src.image(frames), dst.image(None)], "refused call")


# ---- d. nv12_bgr_equalize_batch_dev ----------------------------------------------------------------------------------------------
# Host: nv12_bgr_equalize_dev's `vec` needs W % 16 == 0 and in, out, in_frame and out_frame multiples of 16, and the API lets the two
# strides differ: 32x4 with (tight, tight + 16) and (tight + 16, tight + 48) is the vector body of nv12_bgr_hist_kernel /
# nv12_bgr_apply_kernel on two different strides, (tight + 16, tight + 5) and (tight + 3, tight + 3) in place the 2 x 2 body; 18x6 always is.
@functools.lru_cache(maxsize=None)
def nv12_eq_want(w, h):
    return tuple(oracle.nv12_bgr_equalize(x, w, h).reshape(h * 3 // 2, w) for x in nv12_frames(w, h, 3))


@pytest.mark.parametrize("extras", [(0, 16), (16, 48), (16, 5), (3, None)], ids=["t_t16", "t16_t48", "t16_t5", "t3_inplace"])
def test_nv12_bgr_equalize(ctx, extras):
    for (w, h) in [(32, 4), (18, 6)]:
        src = planar_side(w, h, extras[0])
        dst = src if extras[1] is None else planar_side(w, h, extras[1])
        check(src, dst, nv12_frames(w, h, 3), nv12_eq_want(w, h),
              lambda s, d: ctx.nv12_bgr_equalize_batch_dev(s.ptr, d.ptr, w, h, N, in_frame=s.frame_stride, out_frame=d.frame_stride),
              (w, h, extras))


def test_nv12_bgr_equalize_frame_stride_still_means_both_sides(ctx):
    w, h = 32, 4
    src, dst = planar_side(w, h, 16), planar_side(w, h, 16)
    check(src, dst, nv12_frames(w, h, 3), nv12_eq_want(w, h),
          lambda s, d: ctx.nv12_bgr_equalize_batch_dev(s.ptr, d.ptr, w, h, N, frame_stride=s.frame_stride), "frame_stride")


# ---- e. clahe16_batch_dev --------------------------------------------------------------------------------------------------------
# Host: clahe16_dev's `vec` (tile_hist12_kernel's bet, the vector loads of tile_hist16_kernel) needs the tile geometry of 64x16 / 4x2
# AND (src | src_step | src_frame) & 15 == 0: T and A16 sources have it, U sources and all of 62x15 / 3x2 do not.  Kernels:
# interp16_item decides `aligned` (16-byte loads and stores) per frame from src | dst | src_step | dst_step and `al16` from the source
# alone.  10-bit content is one window of the small table; full-range content is several (the `multi` walk, in place the wide kernel,
# with clahe16_wide = 2 the mid kernel launched as well).
@functools.lru_cache(maxsize=None)
def u16_case(w, h, tx, ty, content):
    rng = np.random.default_rng(w + 7 * h + (0 if content == "10bit" else 1))
    hi = 1024 if content == "10bit" else 65536
    f = tuple(rng.integers(0, hi, (h, w), dtype=np.uint16) for _ in range(N))
    return f, tuple(oracle.clahe16(x, 2.0, tx, ty) for x in f)


@pytest.mark.parametrize("wide", [None, 2], ids=["default", "clahe16_wide2"])
@pytest.mark.parametrize("content", ["10bit", "full"])
@pytest.mark.parametrize("pairing", ["T-A16", "A16-A16", "U-A16", "A16-U", "U-U", "inplace-A16", "inplace-U"])
def test_clahe16(ctx, pairing, content, wide):
    try:
        if wide is not None:
            ctx.set_option("clahe16_wide", wide)
        for (w, h, tx, ty) in [(64, 16, 4, 2), (62, 15, 3, 2)]:
            frames, want = u16_case(w, h, tx, ty, content)
            src, dst = L.make_pair(pairing, h, 2 * w, N, elem=2)
            check(src, dst, frames, want, lambda s, d: ctx.clahe16_batch_dev(s.ptr, d.ptr, w, h, N, 2.0, tx, ty, **strides(s, d)),
                  (pairing, content, wide, w, h))
    finally:
        ctx.set_option("clahe16_wide", 1)                           # the context's default


# ---- f. clahe_batch_dev (8-bit) --------------------------------------------------------------------------------------------------
# The strided batch entries of the planar stages: tile_hist_kernel and the interpolation kernels on base + f * frame_stride with
# row * step -- 64x32 4x4 clahe_interp_kernel with float tables, 16x4 with uchar quads (17 pairs > 15), 128x8 64x2
# clahe_interp_global_kernel (65 pairs > 63), 62x31 3x5 REFLECT_101 on both axes.  (The frame-list tests run the same bodies on a table
# of addresses, not on this stride arithmetic.)
@functools.lru_cache(maxsize=None)
def y_case(w, h, tx, ty, n=N, clip=2.0):
    rng = np.random.default_rng(3 * w + h + tx)
    f = tuple(rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n))
    return f, tuple(oracle.clahe(x, clip, tx, ty) for x in f)


@pytest.mark.parametrize("pairing", ["A16-A16", "U-A16", "A16-U", "Tgap-Tgap", "inplace-U"])
@pytest.mark.parametrize("case", [(64, 32, 4, 4), (64, 32, 16, 4), (128, 8, 64, 2), (62, 31, 3, 5)], ids=str)
def test_clahe_u8(ctx, case, pairing):
    w, h, tx, ty = case
    frames, want = y_case(w, h, tx, ty)
    src, dst = L.make_pair(pairing, h, w, N)
    check(src, dst, frames, want, lambda s, d: ctx.clahe_batch_dev(s.ptr, d.ptr, w, h, N, 2.0, tx, ty, **strides(s, d)), (case, pairing))


@pytest.mark.parametrize("pairing", ["U-A16", "A16-U"])
def test_clahe_u8_several_tiles_per_workgroup(ctx, pairing):
    """tile_hist_multi_kernel on a strided batch: 64 frames of 64x32, grid 8x8, option clahe_tiles_per_wg = 2.  launch_tile_luts on a
    256-CU part: tiles of 32 pixels are never split (S = 1, LUTs written directly), 512 threads are the default, the XCD map is on
    (64 tiles), so a workgroup may take run = 64 / 8 = 8 tiles in a row; K starts at 2, 8 % 2 == 0, and the fill rule lets it stand:
    64 / 2 * 64 = 2048 workgroups is not below 256 * 8 = 2048.  K = 2."""
    w, h, tx, ty, n = 64, 32, 8, 8, 64
    frames, want = y_case(w, h, tx, ty, n)
    s_cls, d_cls = L.PAIRINGS[pairing]
    src, dst = L.make_side(s_cls, h, w, n), L.make_side(d_cls, h, w, n)
    try:
        ctx.set_option("clahe_tiles_per_wg", 2)
        check(src, dst, frames, want, lambda s, d: ctx.clahe_batch_dev(s.ptr, d.ptr, w, h, n, 2.0, tx, ty, **strides(s, d)), pairing)
    finally:
        ctx.set_option("clahe_tiles_per_wg", 0)


# ---- g. stage forms --------------------------------------------------------------------------------------------------------------
# hist_batch_dev, lut_apply_batch_dev and clahe_tile_luts_batch_dev on a pitched source: A16 keeps the 16-byte loads of
# hist_partial_kernel / lut_apply_kernel / tile_hist_kernel on row-wise addressing, U takes them off; lut_apply writes the other class.
@pytest.mark.parametrize("classes", [("A16", "U"), ("U", "A16")], ids=str)
def test_stage_forms(ctx, classes):
    w, h = 50, 9
    clip, tx, ty = 2.0, 3, 2
    frames, _ = y_case(w, h, tx, ty)
    src, dst = L.make_side(classes[0], h, w, N), L.make_side(classes[1], h, w, N)
    src.upload(frames); dst.upload(None)
    d_hist, d_lut, d_tile = dev_filled((N, 256), np.int32, 0), dev_filled((N, 256), np.uint8, 0), dev_filled((N, tx * ty, 256), np.uint8, 0)
    ctx.hist_batch_dev(src.ptr, w, h, N, d_hist, src_step=src.pitch, src_frame=src.frame_stride)
    ctx.equalize_lut_batch_dev(d_hist, w * h, N, d_lut)
    ctx.lut_apply_batch_dev(src.ptr, dst.ptr, w, h, N, d_lut, **strides(src, dst))
    ctx.clahe_tile_luts_batch_dev(src.ptr, w, h, N, clip, tx, ty, d_tile, src_step=src.pitch, src_frame=src.frame_stride)
    sync()
    hist, lut, tile = xfer.to_host(d_hist), xfer.to_host(d_lut), xfer.to_host(d_tile)
    for k in range(N):
        oh = oracle.hist(frames[k])
        assert np.array_equal(hist[k], oh), k
        ol, first = oracle.equalize_lut(oh, w * h)
        assert np.array_equal(lut[k][first:], ol[first:]), k
        assert np.array_equal(tile[k], oracle.clahe_tile_luts(frames[k], clip, tx, ty)), k
    L.assert_sides([src, dst], [src.image(frames), dst.image([oracle.equalize_hist(f) for f in frames])], classes)


# ---- h. analyze_diff_batch_dev ---------------------------------------------------------------------------------------------------
# Host: the diff job's `contiguous` test flattens only when a, b (if given) and diff (if given) are all tight; with three different
# classes it never does, and analyze_diff_kernel addresses each plane by its own step and frame stride; diff_flat cuts every row into
# head, 16-byte vectors and tail by the alignment of `a` alone, b and diff following unaligned.  a, b and diff never share a class.
DIFF_CLASSES = [("A16", "U", "T"), ("U", "Tgap", "A16"), ("T", "A16", "U"), ("Tgap", "T", "A16")]


def stats_of(t):
    return (xfer.to_host(t).astype(np.int64) & 0xFFFFFFFF).tolist()


@pytest.mark.parametrize("classes", DIFF_CLASSES, ids=str)
@pytest.mark.parametrize("wh", [(50, 7), (48, 7)], ids=str)
def test_analyze_diff(ctx, wh, classes):
    w, h = wh
    rng = np.random.default_rng(w)
    fa = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(N)]
    fb = [np.clip(x.astype(np.int16) + rng.integers(-3, 4, x.shape), 0, 255).astype(np.uint8) for x in fa]
    a, b, diff = (L.make_side(c, h, w, N) for c in classes)
    want = [oracle.np_analyze_diff(x, y, 1) for x, y in zip(fa, fb)]
    ws = [[r["above"], r["max_diff"], r["min_diff"], r["total"]] for r in want]
    kw = dict(a_step=a.pitch, a_frame=a.frame_stride, b_step=b.pitch, b_frame=b.frame_stride)
    a.upload(fa); b.upload(fb); diff.upload(None)
    # statistics alone: nothing is written anywhere
    stats = dev_filled((N, 4), np.int32, -1)
    ctx.analyze_diff_batch_dev(a.ptr, b.ptr, w, h, N, stats, threshold=1, **kw)
    sync()
    assert stats_of(stats) == ws
    L.assert_sides([a, b, diff], [a.image(fa), b.image(fb), diff.image(None)], (classes, "no diff"))
    # with the difference image
    stats.fill_(-1)
    ctx.analyze_diff_batch_dev(a.ptr, b.ptr, w, h, N, stats, threshold=1, diff=diff.ptr, diff_step=diff.pitch, diff_frame=diff.frame_stride, **kw)
    sync()
    assert stats_of(stats) == ws
    L.assert_sides([a, b, diff], [a.image(fa), b.image(fb), diff.image([r["diff"] for r in want])], (classes, "diff"))
    # b absent: the statistics of the difference image alone, read where the call above wrote it
    alone = [oracle.np_analyze_diff(r["diff"], None, 1) for r in want]
    stats.fill_(-1)
    ctx.analyze_diff_batch_dev(diff.ptr, None, w, h, N, stats, threshold=1, a_step=diff.pitch, a_frame=diff.frame_stride)
    sync()
    assert stats_of(stats) == [[r["above"], r["max_diff"], r["min_diff"], r["total"]] for r in alone] == ws
    L.assert_sides(diff, diff.image([r["diff"] for r in want]), (classes, "b absent"))
