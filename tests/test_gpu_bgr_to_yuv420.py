"""Interleaved BGR / RGB images in, pitched planar 4:2:0 frames (I420 / YV12) out on the GPU: mi_equalize_hist_bgr_to_yuv420_batch_dev,
mi_clahe_bgr_to_yuv420_batch_dev and their host forms.  Expected bytes (bgr_yuv420_layouts.expected): Y is
oracle.nv12_frame(oracle.bgr_to_nv12(img), W, H, uv_mode, op, ...)[:W*H], U and V that frame's chroma de-interleaved, the image's last
axis reversed first for MI_ORDER_RGB; tests/test_bgr_to_yuv420_abi.py shows on the CPU that this is cv::cvtColor(COLOR_BGR2YUV_I420)
plane by plane.  Pixels are full-range random bytes unless a test says otherwise (equalization then changes about 99 % of the luma bytes:
an identity map cannot pass).  The input and the three output planes live in sentinel-filled allocations with 64 guard bytes and the
WHOLE allocation is compared, input and output: every comparison in this file is exact.  After every call the test asserts which of
"bgr_yuv420_vec" / "bgr_yuv420_bytes" moved, by the header's rule restated in bgr_yuv420_layouts.misaligned.

How many workgroups bgr_to_yuv420_hist_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_bgr_to_yuv420 takes the rule of launch_bgr_to_nv12:
B = min(blocks_per_frame(W*H*9/4 bytes, H/2 rows, n, 2048), ceil(items / 256)), and blocks_per_frame never returns more than
max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which only lowers it.  So
B <= max(1, floor(W*H*9/4 / 16384)),  B <= H/2, and the 256 lanes of a workgroup step through the frame by stride = 256 * B items:
16 x 2 pixel groups on the vector path (gx_n = W/16 per row pair, the carried walk by += dby, gx += dgx with dby = stride / gx_n,
dgx = stride % gx_n and a wrap when gx >= gx_n), 2 x 2 pixel blocks on the byte path.  A shape with more items than 256 * min(both
bounds) makes at least one lane take a second step."""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, COLOR_BGR2YUV_I420, Yuv420Planes
from bgr_yuv420_layouts import SENT, COUNTERS, BgrIn, Yuv420Out, as_fmt, expected, misaligned, rand_images

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
ORDERS = [ORDER_BGR, ORDER_RGB]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in COUNTERS)


def run(c, op, src, dst, order, uv_mode, n=None, st=None, planes=None):
    kind, cfg = op
    kw = dict(src.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    planes = dst.planes() if planes is None else planes
    if kind == "eq":
        c.equalize_hist_bgr_to_yuv420_batch_dev(src.ptr, planes, src.w, src.h, n, order, uv_mode, **kw)
    else:
        c.clahe_bgr_to_yuv420_batch_dev(src.ptr, planes, src.w, src.h, n, order, uv_mode, *cfg, **kw)


def check(c, images, op, order, uv_mode, src, dst):
    """One call on uploaded `images`: the whole output allocation is the oracle's image of it, the whole input allocation is what was
    uploaded, and the counter that names the walk moved by exactly one."""
    src.upload(images)
    dst.clear()
    before = counters(c)
    run(c, op, src, dst, order, uv_mode)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same([expected(img, op, order, uv_mode) for img in images])
    assert ok, (src.w, src.h, op, order, uv_mode, nbad, where)
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
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
ODD_66 = (dict(pitch=201, frame_gap=7, off=1), dict(y_pitch=67, c_pitch=35, u_gap=3, v_gap=5, frame_gap=7, off=1))
# 80 * 32 + 32 = 2592 (U), + 40 * 16 + 8 = 3240 (V, a multiple of 8 and not of 16), + 640 + 40 = 3920 = 245 * 16 (frame stride)
PITCHED_64 = (dict(pitch=208, frame_gap=64, off=32), dict(y_pitch=80, c_pitch=40, u_gap=32, v_gap=8, frame_gap=40, off=16))
PARITY = [
    # id, W, H, n, BgrIn layout, Yuv420Out layout, vector path, the ops
    ("16x2", 16, 2, 1, {}, {}, True, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),                  # one vector group
    ("48x6", 48, 6, 2, {}, {}, True, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 5, 4))]),                  # gx_n = 3: the row walk wraps
    ("2x2", 2, 2, 1, {}, {}, False, [EQ]),                                                                   # one byte-path block
    ("66x34-odd", 66, 34, 2, *ODD_66, False, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (3.0, 4, 3))]),          # nothing aligned: the byte path
    ("64x32-pitched", 64, 32, 2, *PITCHED_64, True, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 8, 8))]),   # padding, gaps, aligned
    ("64x32-yv12", 64, 32, 1, {}, dict(v_first=True), True, [EQ, ("clahe", (2.0, 4, 2))]),                   # V plane before U
    ("64x32-side-by-side", 64, 32, 1, {}, dict(side_by_side=True), True, [EQ, ("clahe", (2.0, 4, 2))]),      # c1 = c0 + W/2, c_pitch = W
]


@pytest.mark.parametrize("name,w,h,n,si,do,vec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, si, do, vec, ops):
    src, dst = BgrIn(w, h, n, **si), Yuv420Out(w, h, n, **do)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    if do.get("v_first"):
        assert dst.v_ptr < dst.u_ptr
    if do.get("side_by_side"):
        assert dst.v_ptr == dst.u_ptr + w // 2 and dst.c_pitch == w
    images = rand_images(w, h, n, 31)
    for op in ops:
        for order in ORDERS:
            for uv_mode in UV_MODES:
                check(c, images, op, order, uv_mode, src, dst)


# ---- 2. one alignment term at a time ---------------------------------------------------------------------------------------------
# 32 x 4 x 2 frames.  The positive case has every chroma term at 8 (mod 16): Y rows 128 + 8 = 136 (U), + 24 * 2 = 184 (V), + 48 + 8 = 240
POSITIVE = dict(c_pitch=24, u_gap=8, frame_gap=8)
ONE_TERM = [
    # the broken term (None: the positive case), BgrIn layout, Yuv420Out layout
    (None, {}, POSITIVE),
    ("in", dict(off=8), POSITIVE),
    ("in_pitch", dict(pitch=104), POSITIVE),
    ("in_frame", dict(frame_gap=8), POSITIVE),
    ("y", {}, dict(POSITIVE, off=8)),                                           # c0 and c1 move by 8 with it: still multiples of 8
    ("y_pitch", {}, dict(POSITIVE, y_pitch=40)),                                # 160 + 8 = 168, 216, 264 + 8 = 272
    ("frame_stride", {}, dict(POSITIVE, frame_gap=16)),                         # 248
    ("c0", {}, dict(c_pitch=24, u_gap=12, v_gap=4, frame_gap=0)),               # 140, 192, 240
    ("c1", {}, dict(c_pitch=24, u_gap=8, v_gap=4, frame_gap=4)),                # 136, 188, 240
    ("c_pitch", {}, dict(c_pitch=28, u_gap=8, frame_gap=8)),                    # 136, 192, 256
]


@pytest.mark.parametrize("term,si,do", ONE_TERM, ids=[str(t[0]) for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, term, si, do):
    """Exactly one of the nine terms misses its modulus (16 for the image and Y terms, 8 for the chroma terms): the byte path, the same
    bytes, the same untouched guards, the counter that names the path.  With c0, c1 and c_pitch all at 8 (mod 16): the vector path."""
    w, h, n = 32, 4, 2
    src, dst = BgrIn(w, h, n, **si), Yuv420Out(w, h, n, **do)
    assert misaligned(w, src, dst) == ([term] if term else [])
    if term is None:
        assert [dst.terms()[k] % 16 for k in ("c0", "c1", "c_pitch")] == [8, 8, 8]
    images = rand_images(w, h, n, 32)
    for op, order, uv_mode in ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, UV_FILL128)):
        check(c, images, op, order, uv_mode, src, dst)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
# 128 * 160 + 32 = 20512 (U), + 72 * 80 + 8 = 26280 (V), + 5760 + 40 = 32080 = 2005 * 16
PITCHED_112 = (dict(pitch=352, frame_gap=64, off=32), dict(y_pitch=128, c_pitch=72, u_gap=32, v_gap=8, frame_gap=40, off=16))
LOOP_SHAPES = [
    # id, W, H, n, BgrIn layout, Yuv420Out layout, vector path (see the module docstring for the bound on B)
    # bytes/16384 = 1.9: B = 1, stride 256; gx_n 6, groups 432, dby 42, dgx 4: the wrap fires whenever gx >= 2, the second step is partial
    ("96x144", 96, 144, 1, {}, {}, True),
    # bytes/16384 = 2.46: B <= 2, stride <= 512; gx_n 7, groups 560, dby 73, dgx 1; pitches, gaps and bases at their moduli
    ("112x160-pitched", 112, 160, 2, *PITCHED_112, True),
    # bytes/16384 = 4.5, H/2 = 4: B <= 4, stride <= 1024; gx_n 257, groups 1028, dby 3, dgx 253: four lanes take a second step, and wrap
    ("4112x8", 4112, 8, 1, {}, {}, True),
    # bytes/16384 = 4.5 but H/2 = 2 rows: B <= 2, stride <= 512; gx_n 512, groups 1024, dby 1, dgx 0: every lane steps straight down a row pair
    ("8192x4", 8192, 4, 1, {}, {}, True),
    # byte path, bytes/16384 = 0.3: B = 1; 33 x 17 = 561 blocks of 2 x 2 for 256 lanes: three steps, the last of 49 lanes
    ("66x34-odd", 66, 34, 2, *ODD_66, False),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,w,h,n,si,do,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, si, do, vec, order):
    """bgr_to_yuv420_hist_kernel where a lane owns more than one group / block: with the histogram (equalizeHist, U and V computed) and
    without it (CLAHE 2 x 2, chroma filled)."""
    src, dst = BgrIn(w, h, n, **si), Yuv420Out(w, h, n, **do)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    bound = max(1, w * h * 9 // 4 // 16384)
    assert (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2), "the shape would not loop"
    images = rand_images(w, h, n, 33)
    check(c, images, EQ, order, UV_COPY, src, dst)
    check(c, images, ("clahe", (2.0, 2, 2)), order, UV_FILL128, src, dst)


# ---- 4. histogram isolation ------------------------------------------------------------------------------------------------------
def test_histograms_do_not_leak_across_frames(c):
    """A constant colour (equalizeHist's single-bin shortcut: every pixel keeps its luma), noise and a horizontal ramp in one batch: each
    frame equals its own oracle result.  Then a two-colour checkerboard in one vector group."""
    w, h = 48, 6
    const = np.empty((h, w, 3), np.uint8)
    const[:] = (200, 31, 7)
    ramp = np.empty((h, w, 3), np.uint8)
    ramp[:] = (np.arange(w) * 255 // (w - 1)).astype(np.uint8)[None, :, None]
    ramp[:, :, 1] //= 2
    images = [const, rand_images(w, h, 1, 34)[0], ramp]
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        for order in ORDERS:
            check(c, images, op, order, UV_COPY, BgrIn(w, h, 3), Yuv420Out(w, h, 3))
    w, h = 16, 2
    board = np.empty((h, w, 3), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    board[:] = np.where(((xx + yy) % 2 == 0)[:, :, None], np.array([250, 10, 90], np.uint8), np.array([5, 180, 220], np.uint8))
    for order in ORDERS:
        for uv_mode in UV_MODES:
            check(c, [board], EQ, order, uv_mode, BgrIn(w, h, 1), Yuv420Out(w, h, 1))


# ---- 5. composition with the library's own pieces --------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_composition_with_the_librarys_own_pieces(c, op):
    """Tight I420: Y equals the planar op applied to the Y rows of mi_cvt_color_420_u8_batch_dev(BGR2YUV_I420), U and V equal that
    call's U and V rows.  The same call with an INTERLEAVED `out` is byte for byte mi_*_bgr_to_nv12_batch_dev on the same layout and
    moves neither counter."""
    w, h, n = 64, 32, 3
    ysz = w * h
    d_bgr = xfer.to_device(np.stack(rand_images(w, h, n, 35)))
    d_i420 = torch.full((n, ysz * 3 // 2), SENT, dtype=torch.uint8, device="cuda:0")
    d_y = torch.full((n, ysz), SENT, dtype=torch.uint8, device="cuda:0")
    d_one = torch.full((n, ysz * 3 // 2), SENT, dtype=torch.uint8, device="cuda:0")
    d_il = torch.full((n, ysz * 3 // 2), SENT, dtype=torch.uint8, device="cuda:0")
    d_nv12 = torch.full((n, ysz * 3 // 2), SENT, dtype=torch.uint8, device="cuda:0")
    c.cvt_color_420_batch_dev(d_bgr, d_i420, w, h, n, COLOR_BGR2YUV_I420, stream=stream())
    before = counters(c)
    if op is EQ:
        c.equalize_hist_batch_dev(d_i420, d_y, w, h, n, src_frame=ysz * 3 // 2, stream=stream())
        c.equalize_hist_bgr_to_yuv420_batch_dev(d_bgr, Yuv420Planes.i420(d_one, w, h), w, h, n, ORDER_BGR, UV_COPY, stream=stream())
        mid = counters(c)
        c.equalize_hist_bgr_to_yuv420_batch_dev(d_bgr, Yuv420Planes.nv12(d_il, w, h), w, h, n, ORDER_BGR, UV_COPY, stream=stream())
        c.equalize_hist_bgr_to_nv12_batch_dev(d_bgr, d_nv12, None, w, h, n, ORDER_BGR, UV_COPY, stream=stream())
    else:
        c.clahe_batch_dev(d_i420, d_y, w, h, n, *op[1], src_frame=ysz * 3 // 2, stream=stream())
        c.clahe_bgr_to_yuv420_batch_dev(d_bgr, Yuv420Planes.i420(d_one, w, h), w, h, n, ORDER_BGR, UV_COPY, *op[1], stream=stream())
        mid = counters(c)
        c.clahe_bgr_to_yuv420_batch_dev(d_bgr, Yuv420Planes.nv12(d_il, w, h), w, h, n, ORDER_BGR, UV_COPY, *op[1], stream=stream())
        c.clahe_bgr_to_nv12_batch_dev(d_bgr, d_nv12, None, w, h, n, ORDER_BGR, UV_COPY, *op[1], stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(d_one[:, :ysz], d_y), op
    assert not torch.equal(d_one[:, :ysz], d_i420[:, :ysz]), "the luma was not mapped"
    assert torch.equal(d_one[:, ysz:], d_i420[:, ysz:]), op
    assert torch.equal(d_il, d_nv12), op
    assert mid == (before[0] + 1, before[1]) and counters(c) == mid, (before, mid, counters(c))


# ---- 6. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass")


def test_launch_contract():
    """equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch per call of n <= 256 frames -- at a
    batch size (n = 2) where the planar form would take hist_lut_kernel.  CLAHE, for a dividing and a non-dividing grid: one MI_K_COLOR
    launch plus what mi_clahe_u8_batch_dev launches for the same plane in place."""
    w, h, n = 64, 32, 2
    images = rand_images(w, h, n, 36)
    src, dst = BgrIn(w, h, n, **PITCHED_64[0]), Yuv420Out(w, h, n, **PITCHED_64[1])
    with mi_lumaeq.Context(0) as c:
        before = {k: c.get_stat(k) for k in OTHER_STATS}
        c.set_profiling(1)
        c.profile_read(reset=True)
        check(c, images, EQ, ORDER_BGR, UV_COPY, src, dst)
        got = launches(c)
        want = {"color_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}
        assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, got
        for cfg in ((2.0, 4, 2), (2.0, 3, 5)):
            c.profile_read(reset=True)
            c.clahe_batch_dev(dst.y_ptr, dst.y_ptr, w, h, n, *cfg, src_step=dst.y_pitch, src_frame=dst.fstride, dst_step=dst.y_pitch,
                              dst_frame=dst.fstride, stream=stream())
            torch.cuda.synchronize()
            planar = launches(c)
            assert planar["color_kernel"] == 0 and sum(planar.values()) >= 2, planar
            c.profile_read(reset=True)
            check(c, images, ("clahe", cfg), ORDER_RGB, UV_FILL128, src, dst)
            got = launches(c)
            assert got == dict(planar, color_kernel=1), (cfg, got, planar)
        c.set_profiling(0)
        assert {k: c.get_stat(k) for k in OTHER_STATS} == before


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 1, 1))], ids=["eq", "clahe-1x1"])
def test_chunking(c, op):
    """One frame past the chunk of 256: two launch sequences, the second of one frame; every frame distinct, every frame checked."""
    w, h, n = 16, 2, 257
    check(c, rand_images(w, h, n, 37), op, ORDER_RGB, UV_COPY, BgrIn(w, h, n), Yuv420Out(w, h, n))


# ---- 8. errors, zero sizes, busy -------------------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    images = rand_images(w, h, n, 38)
    src = BgrIn(w, h, n, pitch=112, frame_gap=16).upload(images)
    dst = Yuv420Out(w, h, n, y_pitch=48, c_pitch=24, u_gap=16, v_gap=8, frame_gap=8)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        before = counters(c)
        base = dict(ctx=hd, i=src.ptr, ip=src.pitch, fi=src.fstride, y=dst.y_ptr, yp=dst.y_pitch, c0=dst.u_ptr, c1=dst.v_ptr,
                    cp=dst.c_pitch, fo=dst.fstride, chroma=mi_lumaeq.CHROMA_PLANAR, w=w, h=h, n=n, order=ORDER_BGR, uvm=UV_COPY, out=True)

        def args(kw):
            a = dict(base)
            a.update(kw)
            planes = Yuv420Planes(a["y"], a["yp"], a["c0"], a["c1"], a["cp"], a["fo"], a["chroma"])
            return (a["ctx"], a["i"], a["ip"], a["fi"], ctypes.byref(planes) if a["out"] else None, a["w"], a["h"], a["n"], a["order"],
                    a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgr_to_yuv420_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgr_to_yuv420_batch_dev(*args(kw), 2.0, tx, ty, stream())
        il = dict(chroma=mi_lumaeq.CHROMA_INTERLEAVED, cp=w)
        bad = [dict(ctx=None), dict(i=None), dict(out=False),                                 # a null ctx, d_in or out
               dict(y=None), dict(c0=None), dict(c1=None), dict(il, y=None), dict(il, c0=None),    # a null plane pointer
               dict(chroma=2), dict(chroma=-1),                                               # a chroma other than the two values
               dict(order=2), dict(order=-1),                                                 # an order other than the two
               dict(uvm=2), dict(uvm=-1),                                                     # a bad uv_mode
               dict(w=-2), dict(h=-2), dict(n=-1),                                            # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),      # odd sizes, also when another size is 0
               dict(il, w=31, h=0), dict(il, h=15, n=0),
               dict(ip=3 * w - 1), dict(yp=w - 1), dict(cp=w // 2 - 1), dict(il, cp=w - 1),    # a pitch below its row
               dict(c0=dst.y_ptr), dict(c1=dst.y_ptr), dict(c1=dst.u_ptr), dict(il, c0=dst.y_ptr),   # two output planes at one address
               dict(y=src.ptr), dict(c0=src.ptr), dict(c1=src.ptr), dict(il, c0=src.ptr)]     # an output plane at d_in
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, **il) == BAD_ARG, (tx, ty)
        # a c1 of an INTERLEAVED output is ignored; zero sizes: MI_OK, nothing written
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(il, n=0, c1=None)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: their status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, yp=1 << 25, cp=1 << 24)
        planar = L.mi_clahe_u8_batch_dev(hd, dst.y_ptr, 1 << 25, 1 << 26, dst.y_ptr, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, dst.y_ptr, dst.y_pitch, dst.fstride, dst.y_ptr, dst.y_pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024,
                                         stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(images)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert counters(c) == before
        c.set_profiling(0)
        # and the context still works
        check(c, images, EQ, ORDER_RGB, UV_FILL128, src, dst)


def test_host_form_errors():
    w, h = 32, 16
    img = rand_images(w, h, 1, 39)[0]
    out = np.full(w * h * 3 // 2, SENT, np.uint8)
    ip, op = img.ctypes.data, out.ctypes.data
    ysz, csz = w * h, w * h // 4
    good = dict(ctx=None, i=ip, step=3 * w, y=op, yp=w, c0=op + ysz, c1=op + ysz + csz, cp=w // 2, chroma=mi_lumaeq.CHROMA_PLANAR, w=w, h=h,
                order=0, uvm=1, out=True)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        good["ctx"] = hd
        before = counters(c)

        def args(kw):
            a = dict(good)
            a.update(kw)
            planes = Yuv420Planes(a["y"], a["yp"], a["c0"], a["c1"], a["cp"], 12345, a["chroma"])      # frame_stride is ignored
            return (a["ctx"], a["i"], a["step"], ctypes.byref(planes) if a["out"] else None, a["w"], a["h"], a["order"], a["uvm"])
        il = dict(chroma=mi_lumaeq.CHROMA_INTERLEAVED, cp=w)
        for kw in (dict(ctx=None), dict(i=None), dict(out=False), dict(y=None), dict(c0=None), dict(c1=None), dict(il, c0=None),
                   dict(chroma=7), dict(step=3 * w - 1), dict(yp=w - 1), dict(cp=w // 2 - 1), dict(il, cp=w - 1), dict(w=w - 1), dict(h=h - 1),
                   dict(w=-2), dict(order=2), dict(uvm=2), dict(y=ip), dict(c1=ip), dict(c1=op + ysz), dict(c0=op), dict(w=w - 1, h=0)):
            assert L.mi_equalize_hist_bgr_to_yuv420(*args(kw)) == BAD_ARG, kw
            assert L.mi_clahe_bgr_to_yuv420(*args(kw), 2.0, 2, 2) == BAD_ARG, kw
        assert L.mi_clahe_bgr_to_yuv420(*args({}), 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_bgr_to_yuv420(*args({}), 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_bgr_to_yuv420(*args(dict(w=0))) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0
        assert counters(c) == before


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    images = rand_images(w, h, 1, 40)
    src = BgrIn(w, h, 1).upload(images)
    dst = Yuv420Out(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        before = counters(c)
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, ORDER_BGR, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"
        assert counters(c) == before
        check(c, images, EQ, ORDER_BGR, UV_COPY, src, dst)                     # and the context still works


# ---- 9. hipGraph -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist and one CLAHE call captured on a single stream (one linear chain, no parallel
    branches) and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    cl = ("clahe", (2.0, 4, 2))
    src = BgrIn(w, h, n, **PITCHED_64[0])
    dst_eq, dst_cl = Yuv420Out(w, h, n, **PITCHED_64[1]), Yuv420Out(w, h, n, **PITCHED_64[1])
    with mi_lumaeq.Context(0) as c:
        images = rand_images(w, h, n, 41)
        src.upload(images)
        for op, dst, uv_mode in ((EQ, dst_eq, UV_COPY), (cl, dst_cl, UV_FILL128)):        # the eager calls size the scratch
            dst.clear()
            run(c, op, src, dst, ORDER_BGR, uv_mode)
            torch.cuda.synchronize()
            assert dst.same([expected(img, op, ORDER_BGR, uv_mode) for img in images])[0], ("eager", op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            run(c, EQ, src, dst_eq, ORDER_BGR, UV_COPY, st=st)
            run(c, cl, src, dst_cl, ORDER_BGR, UV_FILL128, st=st)
        for rep in range(2):
            fresh = rand_images(w, h, n, 42 + rep)
            src.upload(fresh)
            dst_eq.clear()
            dst_cl.clear()
            g.replay()
            torch.cuda.synchronize()
            assert dst_eq.same([expected(img, EQ, ORDER_BGR, UV_COPY) for img in fresh])[0], ("graph replay", "eq", rep)
            assert dst_cl.same([expected(img, cl, ORDER_BGR, UV_FILL128) for img in fresh])[0], ("graph replay", "clahe", rep)
            assert np.array_equal(src.host(), src.image(fresh))


# ---- 10. host forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 6), (66, 34)])
def test_host_forms(w, h):
    """A view with padded rows at an odd address in; a tight I420, YV12 or NV12 frame out through the binding, and pitched host planes
    with guard bytes through raw ctypes: both ops, both orders, both UV modes; the source is unchanged."""
    img = rand_images(w, h, 1, 43)[0]
    pitch = 3 * w + 23
    raw = np.full(h * pitch + 1, SENT, np.uint8)
    padded = raw[1:].reshape(h, pitch)
    view = padded[:, : 3 * w].reshape(h, w, 3)
    assert np.shares_memory(view, raw) and view.ctypes.data % 2 == 1
    view[:] = img
    raw0 = raw.copy()
    ysz, csz, cw, rows = w * h, w * h // 4, w // 2, h // 2
    yp, cp = w + 5, cw + 3                                  # pitched host planes: Y at 1, U behind it, V behind U, 7 bytes between planes
    y_off, u_off = 1, 1 + yp * h + 7
    v_off = u_off + cp * rows + 7
    total = v_off + cp * rows + 64
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 3, 2))):
            for order in ORDERS:
                for uv_mode in UV_MODES:
                    want = expected(img, op, order, uv_mode)
                    for fmt in ("i420", "yv12", "nv12"):
                        if op is EQ:
                            got = c.equalize_hist_bgr_to_yuv420(view, fmt, order, uv_mode)
                        else:
                            got = c.clahe_bgr_to_yuv420(view, fmt, order, uv_mode, *op[1])
                        assert got.shape == (w * h * 3 // 2,) and np.array_equal(got, as_fmt(want, w, h, fmt)), (op, order, uv_mode, fmt)
                    assert np.array_equal(raw, raw0), "the source was written"
                    buf = np.full(total, SENT, np.uint8)
                    b = buf.ctypes.data
                    planes = Yuv420Planes(b + y_off, yp, b + u_off, b + v_off, cp, 0, mi_lumaeq.CHROMA_PLANAR)
                    a = (c._h, view.ctypes.data, pitch, ctypes.byref(planes), w, h, order, uv_mode)
                    st = c._L.mi_equalize_hist_bgr_to_yuv420(*a) if op is EQ else c._L.mi_clahe_bgr_to_yuv420(*a, *op[1])
                    assert st == 0
                    ref = np.full(total, SENT, np.uint8)
                    ref[y_off: y_off + yp * h].reshape(h, yp)[:, :w] = want[:ysz].reshape(h, w)
                    ref[u_off: u_off + cp * rows].reshape(rows, cp)[:, :cw] = want[ysz: ysz + csz].reshape(rows, cw)
                    ref[v_off: v_off + cp * rows].reshape(rows, cp)[:, :cw] = want[ysz + csz:].reshape(rows, cw)
                    assert np.array_equal(buf, ref), (op, order, uv_mode, "pitched host planes")
                    assert np.array_equal(raw, raw0), "the source was written"
        # a caller's own output buffer is filled and returned
        out = np.full(w * h * 3 // 2, SENT, np.uint8)
        assert c.equalize_hist_bgr_to_yuv420(view, out=out) is out
        assert np.array_equal(out, expected(img, EQ, ORDER_BGR, UV_COPY))
        assert c.get_stat("error_drains") == 0
