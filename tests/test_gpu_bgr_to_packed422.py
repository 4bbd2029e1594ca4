"""Interleaved BGR / RGB images in, pitched packed 4:2:2 frames (YUY2 / UYVY) out on the GPU: mi_equalize_hist_bgr_to_packed422_batch_dev,
mi_clahe_bgr_to_packed422_batch_dev and their host forms.  Expected bytes (bgr_packed422_ref.expected): oracle.bgr_to_nv12 on the
row-doubled image gives every row's luma and the chroma of the left pixel of each of its macropixels, the luma is mapped by
oracle.equalize_hist / oracle.clahe, the bytes are interleaved by format and the image's last axis is reversed first for MI_ORDER_RGB;
tests/test_bgr_to_packed422_abi.py shows on the CPU that this is bt601_y / bt601_uv on the left pixel.  Pixels are full-range random
bytes unless a test says otherwise (equalization then changes about 99 % of the luma bytes and 99 % of the odd-row chroma bytes differ
from the row above: neither an identity map nor a 4:2:0 chroma can pass).  The input and the output live in sentinel-filled allocations
with 64 guard bytes and the WHOLE allocation is compared, input and output: every comparison in this file is exact.  After every call
the test asserts which of "bgr_packed422_vec" / "bgr_packed422_bytes" moved, by the header's rule restated in
bgr_packed422_ref.misaligned.

How many workgroups bgr_to_packed422_hist_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_bgr_to_packed422 computes
B = min(blocks_per_frame(W*H*5/2 bytes, H rows, n, 2048), ceil(items / 256)), and blocks_per_frame never returns more than
max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which only lowers it.  So
B <= max(1, floor(W*H*5/2 / 16384)),  B <= H, and the 256 lanes of a workgroup step through the frame by stride = 256 * B items:
16 x 1 pixel groups on the vector path (gx_n = W/16 per row, the carried walk y += dy, gx += dgx with dy = stride / gx_n,
dgx = stride % gx_n and a wrap when gx >= gx_n), macropixels on the byte path.  A shape with more items than 256 * min(both bounds)
makes at least one lane take a second step; 8192 x 2 (1024 groups, B <= 2) makes every lane take one, 4112 x 4 (gx_n = 257, 1028
groups, B <= 2: dy = 1, dgx = 255 at B = 2) ends on a partial step whose lanes wrap into the next row, and the 1155 macropixels of
66 x 35 (B = 1) take five steps."""
import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY, COLOR_BGR2YUV_I420
from bgr_packed422_ref import SENT, COUNTERS, BgrIn, P422Out, convert, mapped_luma, pack, misaligned, rand_images

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
ORDERS = [ORDER_BGR, ORDER_RGB]
FMTS = [FMT_YUY2, FMT_UYVY]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)
_ref = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in COUNTERS)


def expected(img, op, order, fmt, uv_mode, contract=False):
    """bgr_packed422_ref.expected with the conversion and the mapped luma of an image computed once and shared: they do not depend on
    the format or the UV mode."""
    key = (img.shape, img.tobytes(), order)
    if key not in _ref:
        _ref[key] = convert(img, order)
    y, uv = _ref[key]
    mkey = key + (op, contract)
    if mkey not in _ref:
        _ref[mkey] = mapped_luma(y, op, contract)
    return pack(_ref[mkey], uv if uv_mode == UV_COPY else np.full_like(uv, 128), fmt)


def run(c, op, src, dst, order, fmt, uv_mode, n=None, st=None):
    kind, cfg = op
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_bgr_to_packed422_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, order, fmt, uv_mode, **kw)
    else:
        c.clahe_bgr_to_packed422_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, order, fmt, uv_mode, *cfg, **kw)


def check(c, images, op, order, fmt, uv_mode, src, dst, contract=False):
    """One call on uploaded `images`: the whole output allocation is the oracle's image of it, the whole input allocation is what was
    uploaded, and the counter that names the walk moved by exactly one."""
    src.upload(images)
    dst.clear()
    before = counters(c)
    run(c, op, src, dst, order, fmt, uv_mode)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same([expected(img, op, order, fmt, uv_mode, contract) for img in images])
    assert ok, (src.w, src.h, op, order, fmt, uv_mode, nbad, where)
    assert np.array_equal(src.host(), src.image(images)), "the input allocation was written"
    vec = not misaligned(src.w, src, dst)
    after = counters(c)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if vec else (0, 1)), (before, after, vec)


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small batches leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    _ref.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
ODD_66 = (dict(pitch=201, frame_gap=7, off=1), dict(pitch=136, frame_gap=12, off=4))
# in: 208 * 32 + 64 = 6720 = 420 * 16; out: 144 * 32 + 32 = 4640 = 290 * 16
PITCHED_64 = (dict(pitch=208, frame_gap=64, off=32), dict(pitch=144, frame_gap=32, off=16))
PARITY = [
    # id, W, H, n, BgrIn layout, P422Out layout, vector path, the ops
    ("16x1", 16, 1, 1, {}, {}, True, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),                  # one vector group
    ("2x1", 2, 1, 1, {}, {}, False, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),                   # one macropixel
    ("48x5", 48, 5, 2, {}, {}, True, [EQ, ("clahe", (2.0, 3, 5)), ("clahe", (2.0, 5, 4))]),                  # gx_n = 3, odd height; 5 x 4 does not divide
    ("66x35-odd", 66, 35, 2, *ODD_66, False, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (3.0, 4, 3))]),          # nothing aligned; neither grid divides
    ("64x32-pitched", 64, 32, 2, *PITCHED_64, True, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 5, 3))]),   # padding, gaps, aligned
]


@pytest.mark.parametrize("name,w,h,n,si,do,vec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, si, do, vec, ops):
    src, dst = BgrIn(w, h, n, **si), P422Out(w, h, n, **do)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    images = rand_images(w, h, n, 31)
    for op in ops:
        for order in ORDERS:
            for fmt in FMTS:
                for uv_mode in UV_MODES:
                    check(c, images, op, order, fmt, uv_mode, src, dst)


# ---- 2. one alignment term at a time ---------------------------------------------------------------------------------------------
# 32 x 3 x 2 frames; tight: in pitch 96, in frame 288 = 18 * 16, out pitch 64, out frame 192 = 12 * 16
ONE_TERM = [
    # the broken term (None: the positive case), W, BgrIn layout, P422Out layout
    (None, 32, {}, {}),
    ("in", 32, dict(off=8), {}),
    ("in_pitch", 32, dict(pitch=104, frame_gap=8), {}),                         # 104 * 3 + 8 = 320
    ("in_frame", 32, dict(frame_gap=8), {}),                                    # 296
    ("out", 32, {}, dict(off=4)),
    ("out_pitch", 32, {}, dict(pitch=72, frame_gap=8)),                         # 72 = 8 (mod 16); 72 * 3 + 8 = 224
    ("out_frame", 32, {}, dict(frame_gap=4)),                                   # 196 = 4 (mod 16)
    ("width", 24, dict(pitch=80), {}),                                          # in 80, 240; out 48, 144: every term a multiple of 16
]


@pytest.mark.parametrize("term,w,si,do", ONE_TERM, ids=[str(t[0]) for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, term, w, si, do):
    """Exactly one of the six terms misses 16 (the output terms at 4 or 8 mod 16, as the packed forms' rule of multiples of 4 allows), or
    the width does: the byte walk, the same bytes, the same untouched guards, the counter that names the walk.  None does: the vector walk."""
    h, n = 3, 2
    src, dst = BgrIn(w, h, n, **si), P422Out(w, h, n, **do)
    assert misaligned(w, src, dst) == ([term] if term else [])
    images = rand_images(w, h, n, 32)
    for op, order, fmt, uv_mode in ((EQ, ORDER_BGR, FMT_YUY2, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, FMT_UYVY, UV_FILL128)):
        check(c, images, op, order, fmt, uv_mode, src, dst)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
LOOP_SHAPES = [
    # id, W, H, n, BgrIn layout, P422Out layout, vector path (see the module docstring for the bound on B)
    ("8192x2", 8192, 2, 1, {}, {}, True),
    ("4112x4", 4112, 4, 1, {}, {}, True),
    ("66x35-odd", 66, 35, 2, *ODD_66, False),
]


@pytest.mark.parametrize("name,w,h,n,si,do,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, si, do, vec):
    """bgr_to_packed422_hist_kernel where a lane owns more than one group / macropixel: with the histogram (equalizeHist, U and V
    computed) and without it (CLAHE 2 x 2, chroma filled)."""
    src, dst = BgrIn(w, h, n, **si), P422Out(w, h, n, **do)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    bound = max(1, w * h * 5 // 2 // 16384)
    assert (w * h // 16 if vec else w * h // 2) > 256 * min(bound, h), "the shape would not loop"
    images = rand_images(w, h, n, 33)
    for order, fmt in ((ORDER_BGR, FMT_YUY2), (ORDER_RGB, FMT_UYVY)):
        check(c, images, EQ, order, fmt, UV_COPY, src, dst)
        check(c, images, ("clahe", (2.0, 2, 2)), order, fmt, UV_FILL128, src, dst)


# ---- 4. histogram isolation ------------------------------------------------------------------------------------------------------
def test_histograms_do_not_leak_across_frames(c):
    """Three frames whose luma ranges are disjoint (dark, middle, bright pixels: Y = 16 + 0.86 * grey stays inside 16..85, 93..162 and
    170..236): each frame equals its own oracle result, so no count of one frame reached another frame's LUT."""
    w, h = 48, 5
    rng = np.random.default_rng(34)
    images = [rng.integers(lo, hi, (h, w, 3), dtype=np.uint8) for lo, hi in ((0, 80), (90, 170), (180, 256))]
    lumas = [convert(img)[0] for img in images]
    assert lumas[0].max() < lumas[1].min() and lumas[1].max() < lumas[2].min()
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        for order, fmt in ((ORDER_BGR, FMT_YUY2), (ORDER_RGB, FMT_UYVY)):
            check(c, images, op, order, fmt, UV_COPY, BgrIn(w, h, 3), P422Out(w, h, 3))


# ---- 5. composition with the library's own pieces --------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=["yuy2", "uyvy"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_composition_with_the_librarys_own_pieces(c, op, fmt):
    """The output equals mi_*_packed422_batch_dev with MI_UV_COPY run on the library's own unequalized stage-1 result.  That result is
    obtained without the new kernel: mi_cvt_color_420_u8_batch_dev(BGR2YUV_I420) on the row-doubled images gives row r's luma in Y row
    2r and its left-pixel U and V in row r of the U and V planes; torch interleaves them into packed frames."""
    w, h, n = 64, 32, 3
    images = rand_images(w, h, n, 35)
    d_bgr = xfer.to_device(np.stack(images))
    d_dbl = d_bgr.repeat_interleave(2, dim=1).contiguous()
    ysz = 2 * h * w
    d_i420 = torch.empty((n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0")
    c.cvt_color_420_batch_dev(d_dbl, d_i420, w, 2 * h, n, COLOR_BGR2YUV_I420, stream=stream())
    y = d_i420[:, :ysz].reshape(n, 2 * h, w)[:, 0::2]
    u = d_i420[:, ysz: ysz + ysz // 4].reshape(n, h, w // 2)
    v = d_i420[:, ysz + ysz // 4:].reshape(n, h, w // 2)
    raw = torch.empty((n, h, w // 2, 4), dtype=torch.uint8, device="cuda:0")
    yi, ui, vi = ((0, 2), 1, 3) if fmt == FMT_YUY2 else ((1, 3), 0, 2)
    raw[..., yi[0]], raw[..., yi[1]], raw[..., ui], raw[..., vi] = y[:, :, 0::2], y[:, :, 1::2], u, v
    raw = raw.reshape(n, h, 2 * w).contiguous()
    assert np.array_equal(xfer.to_host(raw)[0], pack(*convert(images[0]), fmt)), "the stand-in is not the reference's unequalized frame"
    two = torch.full((n, h, 2 * w), SENT, dtype=torch.uint8, device="cuda:0")
    one = torch.full((n, h, 2 * w), SENT, dtype=torch.uint8, device="cuda:0")
    if op is EQ:
        c.equalize_hist_packed422_batch_dev(raw, two, w, h, n, fmt, UV_COPY, stream=stream())
        c.equalize_hist_bgr_to_packed422_batch_dev(d_bgr, one, w, h, n, ORDER_BGR, fmt, UV_COPY, stream=stream())
    else:
        c.clahe_packed422_batch_dev(raw, two, w, h, n, fmt, UV_COPY, *op[1], stream=stream())
        c.clahe_bgr_to_packed422_batch_dev(d_bgr, one, w, h, n, ORDER_BGR, fmt, UV_COPY, *op[1], stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(one, two), (op, fmt)
    assert not torch.equal(one, raw), "the luma was not mapped"


# ---- 6. stage 2 through every interpolation family, in place ---------------------------------------------------------------------
# kMaxPairsLdsF32 = 15, kMaxPairsLds = 63, pairs = tiles_x + 1 (tests/test_gpu_packed422_interp_paths.py derives the four branches)
INTERP = [
    # id, W, H, tiles_x, tiles_y, clahe_fp_contract
    ("float-tables", 64, 48, 8, 8, 0),
    ("segment-float-tables", 1792, 8, 16, 2, 0),
    ("quad-tables", 64, 8, 16, 2, 0),
    ("global-luts", 128, 4, 64, 2, 0),
    ("quad-tables-contract", 96, 10, 16, 2, 1),
    ("float-tables-contract", 66, 35, 3, 2, 1),
]


@pytest.mark.parametrize("name,w,h,tx,ty,contract", INTERP, ids=[s[0] for s in INTERP])
def test_stage_two_through_every_interpolation_family_in_place(name, w, h, tx, ty, contract):
    """The packed form's interpolation kernels with src == dst on the frame stage 1 has just written: LDS float tables, float tables on
    column segments, uchar quads, the global-LUT kernel, and the FMA bodies under clahe_fp_contract (the option is restored)."""
    n = 2
    images = rand_images(w, h, n, 36)
    src, dst = BgrIn(w, h, n), P422Out(w, h, n)
    with mi_lumaeq.Context(0) as c:
        c.set_option("clahe_fp_contract", contract)
        try:
            for order, fmt, uv_mode in ((ORDER_BGR, FMT_YUY2, UV_COPY), (ORDER_RGB, FMT_UYVY, UV_FILL128)):
                check(c, images, ("clahe", (2.0, tx, ty)), order, fmt, uv_mode, src, dst, contract=bool(contract))
        finally:
            c.set_option("clahe_fp_contract", 0)
        check(c, images, ("clahe", (2.0, tx, ty)), ORDER_BGR, FMT_YUY2, UV_COPY, src, dst)


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 1, 1))], ids=["eq", "clahe-1x1"])
def test_chunking(c, op):
    """One frame past the chunk of 256: two launch sequences, the second of one frame; every frame distinct, every frame checked."""
    w, h, n = 16, 2, 257
    check(c, rand_images(w, h, n, 37), op, ORDER_RGB, FMT_UYVY, UV_COPY, BgrIn(w, h, n), P422Out(w, h, n))


# ---- 8. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass",
               "bgr_yuv420_vec", "bgr_yuv420_bytes")


def test_launch_contract():
    """equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch per call of n <= 256 frames.  CLAHE, for
    a dividing and a non-dividing grid: one MI_K_COLOR launch plus what mi_clahe_packed422_batch_dev launches for the same frames in
    place."""
    w, h, n = 64, 32, 2
    images = rand_images(w, h, n, 38)
    src, dst = BgrIn(w, h, n, **PITCHED_64[0]), P422Out(w, h, n, **PITCHED_64[1])
    with mi_lumaeq.Context(0) as c:
        before = {k: c.get_stat(k) for k in OTHER_STATS}
        c.set_profiling(1)
        c.profile_read(reset=True)
        check(c, images, EQ, ORDER_BGR, FMT_YUY2, UV_COPY, src, dst)
        got = launches(c)
        want = {"color_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}
        assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, got
        for cfg in ((2.0, 4, 2), (2.0, 3, 5)):
            c.profile_read(reset=True)
            c.clahe_packed422_batch_dev(dst.ptr, dst.ptr, w, h, n, FMT_UYVY, UV_COPY, *cfg, in_pitch=dst.pitch, in_frame=dst.fstride,
                                        out_pitch=dst.pitch, out_frame=dst.fstride, stream=stream())
            torch.cuda.synchronize()
            packed = launches(c)
            assert packed["color_kernel"] == 0 and sum(packed.values()) >= 2, packed
            c.profile_read(reset=True)
            check(c, images, ("clahe", cfg), ORDER_RGB, FMT_UYVY, UV_FILL128, src, dst)
            got = launches(c)
            assert got == dict(packed, color_kernel=1), (cfg, got, packed)
        c.set_profiling(0)
        assert {k: c.get_stat(k) for k in OTHER_STATS} == before


# ---- 9. errors, zero sizes, busy, hipGraph ---------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 15, 2
    images = rand_images(w, h, n, 39)
    src = BgrIn(w, h, n, pitch=112, frame_gap=16).upload(images)
    dst = P422Out(w, h, n, pitch=80, frame_gap=16)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        before = counters(c)
        base = dict(ctx=hd, i=src.ptr, ip=src.pitch, fi=src.fstride, o=dst.ptr, op=dst.pitch, fo=dst.fstride, w=w, h=h, n=n,
                    order=ORDER_BGR, fmt=FMT_YUY2, uvm=UV_COPY)

        def args(kw):
            a = dict(base)
            a.update(kw)
            return (a["ctx"], a["i"], a["ip"], a["fi"], a["o"], a["op"], a["fo"], a["w"], a["h"], a["n"], a["order"], a["fmt"], a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgr_to_packed422_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgr_to_packed422_batch_dev(*args(kw), 2.0, tx, ty, stream())
        bad = [dict(ctx=None), dict(i=None), dict(o=None),                                    # null pointers
               dict(order=2), dict(order=-1), dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),
               dict(w=-2), dict(h=-1), dict(n=-1),                                            # negative sizes
               dict(w=31), dict(w=31, h=0), dict(w=31, n=0),                                  # an odd width, also when another size is 0
               dict(ip=3 * w - 1), dict(op=2 * w - 4),                                        # a pitch below its row
               dict(o=dst.ptr + 2), dict(op=dst.pitch + 2), dict(fo=dst.fstride + 2),          # an output term that is no multiple of 4
               dict(o=src.ptr)]                                                               # no in-place form
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, i=None, o=None)):                # zero sizes: MI_OK, nothing written
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the packed and planar forms refuse: their status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, op=1 << 26, fi=1 << 28, fo=1 << 27)
        packed = L.mi_clahe_packed422_batch_dev(hd, dst.ptr, 1 << 26, 1 << 27, dst.ptr, 1 << 26, 1 << 27, big["w"], 2, 1, FMT_YUY2, UV_COPY,
                                                2.0, 2, 2, stream())
        assert packed == UNSUPPORTED and eq(**big) == packed and cl(**big) == packed
        planar = L.mi_clahe_u8_batch_dev(hd, dst.ptr, dst.pitch, dst.fstride, dst.ptr, dst.pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(images)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert counters(c) == before
        c.set_profiling(0)
        # and the context still works
        check(c, images, EQ, ORDER_RGB, FMT_UYVY, UV_FILL128, src, dst)


def test_host_form_errors():
    w, h = 32, 15
    img = rand_images(w, h, 1, 40)[0]
    out = np.full(h * 2 * w, SENT, np.uint8)
    ip, op = img.ctypes.data, out.ctypes.data
    good = dict(ctx=None, i=ip, step=3 * w, o=op, op=2 * w, w=w, h=h, order=0, fmt=FMT_UYVY, uvm=1)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        good["ctx"] = hd
        before = counters(c)

        def args(kw):
            a = dict(good)
            a.update(kw)
            return (a["ctx"], a["i"], a["step"], a["o"], a["op"], a["w"], a["h"], a["order"], a["fmt"], a["uvm"])
        for kw in (dict(ctx=None), dict(i=None), dict(o=None), dict(step=3 * w - 1), dict(op=2 * w - 1), dict(w=w - 1), dict(w=-2), dict(h=-1),
                   dict(order=2), dict(fmt=1), dict(fmt=4), dict(uvm=2), dict(o=ip), dict(w=w - 1, h=0)):
            assert L.mi_equalize_hist_bgr_to_packed422(*args(kw)) == BAD_ARG, kw
            assert L.mi_clahe_bgr_to_packed422(*args(kw), 2.0, 2, 2) == BAD_ARG, kw
        assert L.mi_clahe_bgr_to_packed422(*args({}), 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_bgr_to_packed422(*args({}), 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_bgr_to_packed422(*args(dict(w=0))) == 0
        assert L.mi_equalize_hist_bgr_to_packed422(*args(dict(h=0))) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0
        assert counters(c) == before


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    images = rand_images(w, h, 1, 41)
    src = BgrIn(w, h, 1).upload(images)
    dst = P422Out(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        before = counters(c)
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, ORDER_BGR, FMT_YUY2, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"
        assert counters(c) == before
        check(c, images, EQ, ORDER_BGR, FMT_YUY2, UV_COPY, src, dst)                     # and the context still works


def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist and one CLAHE call captured on a single stream (one linear chain, no parallel
    branches) and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    cl = ("clahe", (2.0, 4, 2))
    src = BgrIn(w, h, n, **PITCHED_64[0])
    dst_eq, dst_cl = P422Out(w, h, n, **PITCHED_64[1]), P422Out(w, h, n, **PITCHED_64[1])
    calls = ((EQ, dst_eq, FMT_YUY2, UV_COPY), (cl, dst_cl, FMT_UYVY, UV_FILL128))
    with mi_lumaeq.Context(0) as c:
        images = rand_images(w, h, n, 42)
        src.upload(images)
        for op, dst, fmt, uv_mode in calls:                                              # the eager calls size the scratch
            dst.clear()
            run(c, op, src, dst, ORDER_BGR, fmt, uv_mode)
            torch.cuda.synchronize()
            assert dst.same([expected(img, op, ORDER_BGR, fmt, uv_mode) for img in images])[0], ("eager", op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            for op, dst, fmt, uv_mode in calls:
                run(c, op, src, dst, ORDER_BGR, fmt, uv_mode, st=st)
        for rep in range(2):
            fresh = rand_images(w, h, n, 43 + rep)
            src.upload(fresh)
            dst_eq.clear()
            dst_cl.clear()
            g.replay()
            torch.cuda.synchronize()
            for op, dst, fmt, uv_mode in calls:
                assert dst.same([expected(img, op, ORDER_BGR, fmt, uv_mode) for img in fresh])[0], ("graph replay", op, rep)
            assert np.array_equal(src.host(), src.image(fresh))


# ---- 10. host forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(2, 1), (48, 5), (66, 35)])
def test_host_forms(w, h):
    """A view with padded rows at an odd address in; a new tight H x 2W frame out, and a caller's padded view at an odd address out whose
    padding and guards stay untouched: both ops, both orders, both formats, both UV modes; the source is unchanged; the counter names
    the walk of the tight, aligned device copy (W % 16 == 0: the groups)."""
    img = rand_images(w, h, 1, 45)[0]
    pitch = 3 * w + 23
    raw = np.full(h * pitch + 1, SENT, np.uint8)
    view = raw[1:].reshape(h, pitch)[:, : 3 * w].reshape(h, w, 3)
    assert np.shares_memory(view, raw) and view.ctypes.data % 2 == 1
    view[:] = img
    raw0 = raw.copy()
    opitch = 2 * w + 5
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 3, 2)) if h > 1 else ("clahe", (2.0, 1, 1))):
            for order in ORDERS:
                for fmt in FMTS:
                    for uv_mode in UV_MODES:
                        want = expected(img, op, order, fmt, uv_mode)
                        before = counters(c)
                        if op is EQ:
                            got = c.equalize_hist_bgr_to_packed422(view, order, fmt, uv_mode)
                        else:
                            got = c.clahe_bgr_to_packed422(view, order, fmt, uv_mode, *op[1])
                        assert got.shape == (h, 2 * w) and np.array_equal(got, want), (op, order, fmt, uv_mode)
                        after = counters(c)
                        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if w % 16 == 0 else (0, 1))
                        buf = np.full(h * opitch + 1 + 64, SENT, np.uint8)
                        oview = buf[1: 1 + h * opitch].reshape(h, opitch)[:, : 2 * w]
                        assert oview.ctypes.data % 2 == 1
                        if op is EQ:
                            ret = c.equalize_hist_bgr_to_packed422(view, order, fmt, uv_mode, out=oview)
                        else:
                            ret = c.clahe_bgr_to_packed422(view, order, fmt, uv_mode, *op[1], out=oview)
                        assert ret is oview
                        ref = np.full(buf.size, SENT, np.uint8)
                        ref[1: 1 + h * opitch].reshape(h, opitch)[:, : 2 * w] = want
                        assert np.array_equal(buf, ref), (op, order, fmt, uv_mode, "padded host view")
                        assert np.array_equal(raw, raw0), "the source was written"
        assert c.get_stat("error_drains") == 0
