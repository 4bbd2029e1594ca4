"""Four-channel BGRA / RGBA (CV_8UC4) images in, pitched 4:2:0 frames (I420 / YV12 planes, or NV12) out on the GPU:
mi_equalize_hist_bgra_to_yuv420_batch_dev, mi_clahe_bgra_to_yuv420_batch_dev and their host forms.  Expected bytes
(bgra_yuv420_layouts.expected4): the three-channel builder of tests/bgr_yuv420_layouts.py on the image with its fourth byte removed;
tests/test_bgra_to_yuv420_abi.py shows on the CPU that this is cv::cvtColor(COLOR_BGR2YUV_I420) plane by plane on the first three
channels and that a wrong channel offset or pixel stride gives other bytes.  Pixels are full-range random bytes, the fourth byte
included (equalization then changes about 99 % of the luma bytes: an identity map cannot pass).  The input and the output planes live
in sentinel-filled allocations with 64 guard bytes and the WHOLE allocation is compared, input and output: every comparison in this
file is exact.  After every call the test asserts which of "bgra_yuv420_vec" / "bgra_yuv420_bytes" moved, by the header's rule restated
in bgra_yuv420_layouts.misaligned, and that no list counter moved.  Both chroma layouts are this form's own kernels, so every property
is checked on a planar and on an interleaved output.

How many workgroups bgra_to_yuv420_hist_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_bgra_to_yuv420 takes the siblings' rule on its own byte basis, half of the
4 + 1.5 bytes per pixel stage 1 moves: B = min(blocks_per_frame(W*H*11/4 bytes, H/2 rows, n, 2048), ceil(items / 256)), and
blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which
only lowers it.  So B <= max(1, floor(W*H*11/4 / 16384)), B <= H/2, and the 256 lanes of a workgroup step through the frame by
stride = 256 * B items: 16 x 2 pixel groups on the vector walk (gx_n = W/16 per row pair, the carried walk by += dby, gx += dgx with
dby = stride / gx_n, dgx = stride % gx_n and a wrap when gx >= gx_n), 2 x 2 pixel blocks on the byte walk.  A shape with more items
than 256 * min(both bounds) makes at least one lane take a second step:
  112 x 80: 8960 pixels, 24640 bytes, floor(24640 / 16384) = 1: ONE workgroup whatever the device; gx_n 7, 280 groups for 256 lanes,
            dby 36, dgx 4: 24 lanes take a second step, and those with gx >= 3 wrap.
  16000 x 6: H/2 = 3, so B is 1, 2 or 3 and the stride 256, 512 or 768 < gx_n = 1000: dby 0, every step is a pure gx step, a lane
            takes 4 to 12 steps for the 3000 groups and its gx wraps past the row end on MORE THAN ONE of them (walk_wraps below
            counts them for every B the rule allows).
  66 x 34:  the byte walk; 6171 bytes: B = 1; 33 x 17 = 561 blocks for 256 lanes: three steps, the last of 49 lanes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, Yuv420Planes
import bgra_yuv420_layouts as layouts
from bgra_yuv420_layouts import SENT, COUNTERS, LIST_COUNTERS, BgraIn, Nv12Out, Yuv420Out, as_fmt, complement_x, is_planar, misaligned, \
    rand_images4

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
ORDERS = [ORDER_BGR, ORDER_RGB]
UV_MODES = [UV_COPY, UV_FILL128]
FMTS = ["i420", "yv12", "nv12", "side"]          # side: U and V rows side by side in one pitched plane (c1 = c0 + W/2)
EQ = ("eq", None)
ALL_COUNTERS = COUNTERS + LIST_COUNTERS


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in ALL_COUNTERS)


def moved(c, before):
    return tuple(a - b for a, b in zip(counters(c), before))


@functools.lru_cache(maxsize=None)
def _expected(img_bytes, w, h, op, order, uv_mode):
    out = layouts.expected4(np.frombuffer(img_bytes, np.uint8).reshape(h, w, 4), op, order, uv_mode)
    out.setflags(write=False)
    return out


def expected4(img, op, order, uv_mode):
    """The tight I420 frame the call must produce for `img` (H x W x 4): computed once per (image, op, order, uv_mode), read-only."""
    h, w = img.shape[:2]
    return _expected(img.tobytes(), w, h, op, order, uv_mode)


def make_out(fmt, w, h, n, lay):
    """The output allocation of layout `fmt` with the keyword arguments lay[fmt] (Yuv420Out's, or Nv12Out's for "nv12")."""
    kw = dict(lay.get(fmt, {}))
    if fmt == "nv12":
        return Nv12Out(w, h, n, **kw)
    return Yuv420Out(w, h, n, v_first=fmt == "yv12", side_by_side=fmt == "side", **kw)


def run(c, op, src, dst, order, uv_mode, n=None, st=None, planes=None):
    kind, cfg = op
    kw = dict(src.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    planes = dst.planes() if planes is None else planes
    if kind == "eq":
        c.equalize_hist_bgra_to_yuv420_batch_dev(src.ptr, planes, src.w, src.h, n, order, uv_mode, **kw)
    else:
        c.clahe_bgra_to_yuv420_batch_dev(src.ptr, planes, src.w, src.h, n, order, uv_mode, *cfg, **kw)


def check(c, images, op, order, uv_mode, src, dst):
    """One call on uploaded `images`: the whole output allocation is the oracle's image of it, the whole input allocation is what was
    uploaded, and the counter that names the walk moved by exactly one, no other."""
    src.upload(images)
    dst.clear()
    before = counters(c)
    run(c, op, src, dst, order, uv_mode)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same([expected4(img, op, order, uv_mode) for img in images])
    assert ok, (src.w, src.h, op, order, uv_mode, nbad, where)
    assert np.array_equal(src.host(), src.image(images)), "the input allocation was written"
    vec = not misaligned(src.w, src, dst)
    assert moved(c, before) == ((1, 0, 0, 0) if vec else (0, 1, 0, 0)), (moved(c, before), vec)


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
TIGHT = {"in": {}}
# nothing aligned: pitch 4 * 66 + 1, offset 1, odd plane pitches and gaps, odd frame strides
ODD_66 = {"in": dict(pitch=265, frame_gap=7, off=1),
          "i420": dict(y_pitch=67, c_pitch=35, u_gap=3, v_gap=5, frame_gap=7, off=1),
          "yv12": dict(y_pitch=67, c_pitch=35, u_gap=3, v_gap=5, frame_gap=7, off=1),
          "side": dict(y_pitch=67, c_pitch=67, u_gap=3, frame_gap=7, off=1),
          "nv12": dict(y_pitch=67, c_pitch=67, uv_gap=3, frame_gap=7, off=1)}
# pitched and aligned, the planar chroma terms at 8 (mod 16).  i420: 16 + 80 * 32 + 24 = 2600 (U), 2584 + 40 * 16 + 16 = 3240, + 16 = 3256
# (V), 3240 + 640 + 8 = 3888 = 243 * 16 (frame stride); yv12 the same with the two gaps exchanged; side: c_pitch 72, 2600 (U), 2632 (V),
# 2584 + 72 * 16 + 8 = 3744 = 234 * 16; nv12: everything a multiple of 16: 16 + 2560 + 32 = 2608 (UV), 2592 + 96 * 16 + 48 = 4176 = 261 * 16
PITCHED_64 = {"in": dict(pitch=272, frame_gap=64, off=32),
              "i420": dict(y_pitch=80, c_pitch=40, u_gap=24, v_gap=16, frame_gap=8, off=16),
              "yv12": dict(y_pitch=80, c_pitch=40, u_gap=16, v_gap=24, frame_gap=8, off=16),
              "side": dict(y_pitch=80, c_pitch=72, u_gap=24, frame_gap=8, off=16),
              "nv12": dict(y_pitch=80, c_pitch=96, uv_gap=32, frame_gap=48, off=16)}
PARITY = [
    # id, W, H, n, layouts, vector walk, the ops
    ("16x2", 16, 2, 1, TIGHT, True, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),                  # one vector group
    ("48x6", 48, 6, 2, TIGHT, True, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 5, 4))]),                  # gx_n = 3: the row walk wraps; 5 x 4: REFLECT_101
    ("2x2", 2, 2, 1, TIGHT, False, [EQ]),                                                                   # one byte block
    ("66x34-odd", 66, 34, 2, ODD_66, False, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 4, 3))]),          # nothing aligned: the byte walk
    ("64x32-pitched", 64, 32, 2, PITCHED_64, True, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 8, 8))]),   # padding, gaps, aligned
]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,w,h,n,lay,vec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, lay, vec, ops, fmt):
    src, dst = BgraIn(w, h, n, **lay["in"]), make_out(fmt, w, h, n, lay)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    assert is_planar(dst) == (fmt != "nv12")
    if fmt == "yv12":
        assert dst.v_ptr < dst.u_ptr
    if fmt == "side":
        assert dst.v_ptr == dst.u_ptr + w // 2 and dst.c_pitch >= w
    if name == "66x34-odd":
        assert src.pitch == 4 * w + 1 and set(misaligned(w, src, dst)) == set(src.terms()) | set(dst.terms()) | {"width"}, "nothing is aligned"
    if name == "64x32-pitched" and fmt != "nv12":
        assert [dst.terms()[k] % 16 for k in ("c0", "c1", "c_pitch")] == [8, 8, 8]
    images = rand_images4(w, h, n, 31)
    for op in ops:
        for order in ORDERS:
            for uv_mode in UV_MODES:
                check(c, images, op, order, uv_mode, src, dst)


# ---- 2. one alignment term at a time ---------------------------------------------------------------------------------------------
# 32 x 4 x 2 frames.  Planar: the positive case has every chroma term at 8 (mod 16): Y rows 128 + 8 = 136 (U), + 24 * 2 = 184 (V),
# + 48 + 8 = 240
POSITIVE = dict(c_pitch=24, u_gap=8, frame_gap=8)
ONE_TERM_PLANAR = [
    # the broken term (None: the positive case), BgraIn layout, Yuv420Out layout
    (None, {}, POSITIVE),
    ("in", dict(off=8), POSITIVE),
    ("in_pitch", dict(pitch=136), POSITIVE),
    ("in_frame", dict(frame_gap=8), POSITIVE),
    ("y", {}, dict(POSITIVE, off=8)),                                           # c0 and c1 move by 8 with it: still multiples of 8
    ("y_pitch", {}, dict(POSITIVE, y_pitch=40)),                                # 160 + 8 = 168, 216, 264 + 8 = 272
    ("frame_stride", {}, dict(POSITIVE, frame_gap=16)),                         # 248
    ("c0", {}, dict(c_pitch=24, u_gap=12, v_gap=4, frame_gap=0)),               # 140, 192, 240
    ("c1", {}, dict(c_pitch=24, u_gap=8, v_gap=4, frame_gap=4)),                # 136, 188, 240
    ("c_pitch", {}, dict(c_pitch=28, u_gap=8, frame_gap=8)),                    # 136, 192, 256
]
# Interleaved: every term a multiple of 16 (Y rows 128, UV at 128, c_pitch 32, frame stride 192); 8 (mod 16) is not enough for c0 and c_pitch
ONE_TERM_INTERLEAVED = [
    (None, {}, {}),
    ("in", dict(off=8), {}),
    ("in_pitch", dict(pitch=136), {}),
    ("in_frame", dict(frame_gap=8), {}),
    ("y", {}, dict(off=8, uv_gap=8, frame_gap=8)),                              # y 8; c0 8 + 128 + 8 = 144; 136 + 64 + 8 = 208
    ("y_pitch", {}, dict(y_pitch=40)),                                          # UV at 160, frame stride 224
    ("frame_stride", {}, dict(frame_gap=8)),                                    # 200
    ("c0", {}, dict(uv_gap=8, frame_gap=8)),                                    # 136; 136 + 64 + 8 = 208
    ("c_pitch", {}, dict(c_pitch=40)),                                          # 128 + 80 = 208
]
ONE_TERM = [("planar",) + t for t in ONE_TERM_PLANAR] + [("interleaved",) + t for t in ONE_TERM_INTERLEAVED]


@pytest.mark.parametrize("chroma,term,si,do", ONE_TERM, ids=[f"{t[0]}-{t[1]}" for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, chroma, term, si, do):
    """Exactly one term misses its modulus (16 for the image and Y terms; 8 for the planar chroma terms, 16 for the interleaved ones):
    the byte walk, the same bytes, the same untouched guards, the other counter.  With every term on its modulus -- the planar c0, c1
    and c_pitch all at 8 (mod 16) -- the vector walk."""
    w, h, n = 32, 4, 2
    src = BgraIn(w, h, n, **si)
    dst = Yuv420Out(w, h, n, **do) if chroma == "planar" else Nv12Out(w, h, n, **do)
    assert misaligned(w, src, dst) == ([term] if term else [])
    if term is None and chroma == "planar":
        assert [dst.terms()[k] % 16 for k in ("c0", "c1", "c_pitch")] == [8, 8, 8]
    if chroma == "interleaved" and term in ("c0", "c_pitch"):
        assert dst.terms()[term] % 16 == 8, "a multiple of 8 is not enough for the 16-byte UV store"
    images = rand_images4(w, h, n, 32)
    for op, order, uv_mode in ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, UV_FILL128)):
        check(c, images, op, order, uv_mode, src, dst)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
# 112 x 80: i420 16 + 128 * 80 + 24 = 10280 (U), 10264 + 72 * 40 + 16 + 16 = 13176 (V), 13160 + 2880 + 8 = 16048 = 1003 * 16;
# nv12 16 + 10240 + 32 = 10288 (UV), 10272 + 128 * 40 + 48 = 15440 = 965 * 16
PITCHED_112 = {"in": dict(pitch=464, frame_gap=64, off=32),
               "i420": dict(y_pitch=128, c_pitch=72, u_gap=24, v_gap=16, frame_gap=8, off=16),
               "nv12": dict(y_pitch=128, c_pitch=128, uv_gap=32, frame_gap=48, off=16)}
# 16000 x 6: i420 16 + 16016 * 6 + 24 = 96136 (U), 96120 + 8008 * 3 + 8 + 16 = 120168 (V), 120152 + 24024 = 144176 = 9011 * 16;
# nv12 16 + 96096 + 32 = 96144 (UV), 96128 + 16016 * 3 + 16 = 144192 = 9012 * 16
PITCHED_16000 = {"in": dict(pitch=64016, frame_gap=64, off=32),
                 "i420": dict(y_pitch=16016, c_pitch=8008, u_gap=24, v_gap=8, frame_gap=0, off=16),
                 "nv12": dict(y_pitch=16016, c_pitch=16016, uv_gap=32, frame_gap=16, off=16)}
LOOP_SHAPES = [
    # id, W, H, n, layouts, vector walk (see the module docstring for the bound on B and the arithmetic of each shape)
    ("112x80-pitched", 112, 80, 2, PITCHED_112, True),
    ("16000x6-pitched", 16000, 6, 2, PITCHED_16000, True),
    ("66x34-odd", 66, 34, 2, ODD_66, False),
]


def walk_wraps(w, h, b):
    """The carried (by, gx) walk of the vector path with b workgroups a frame, restated: for each lane the number of its steps INSIDE
    the frame on which gx wrapped past the row end.  Returns the largest count and checks that the walk visits every group once."""
    gx_n, groups, stride = w // 16, (w // 16) * (h // 2), 256 * b
    dby, dgx = divmod(stride, gx_n)
    seen, most = set(), 0
    for lane in range(min(stride, groups)):
        gi, (by, gx), wraps = lane, divmod(lane, gx_n), 0
        while gi < groups:
            if gx >= gx_n:
                gx, by, wraps = gx - gx_n, by + 1, wraps + 1
            assert (by, gx) == divmod(gi, gx_n)
            seen.add(gi)
            gi, by, gx = gi + stride, by + dby, gx + dgx
        most = max(most, wraps)
    assert len(seen) == groups
    return most


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("name,w,h,n,lay,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, lay, vec, fmt, order):
    """bgra_to_yuv420_hist_kernel where a lane owns more than one group / block: with the histogram (equalizeHist, U and V computed) and
    without it (CLAHE 2 x 2, chroma filled), pitched, two frames, planar and interleaved chroma."""
    src, dst = BgraIn(w, h, n, **lay["in"]), make_out(fmt, w, h, n, lay)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    bound = min(max(1, w * h * 11 // 4 // 16384), h // 2)
    assert (w * h // 32 if vec else w * h // 4) > 256 * bound, "the shape would not loop"
    if name == "112x80-pitched":
        assert bound == 1 and w * h // 32 == 280
    if name == "16000x6-pitched":
        assert bound == 3 and all(walk_wraps(w, h, b) >= 2 for b in (1, 2, 3)), "gx wraps on more than one step of a lane"
    images = rand_images4(w, h, n, 33)
    check(c, images, EQ, order, UV_COPY, src, dst)
    check(c, images, ("clahe", (2.0, 2, 2)), order, UV_FILL128, src, dst)


# ---- 4. X is ignored -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("name,w,h,n,lay,vec", [("48x6", 48, 6, 2, TIGHT, True), ("66x34-odd", 66, 34, 2, ODD_66, False)],
                         ids=["vector", "bytes"])
def test_the_fourth_byte_is_ignored(c, name, w, h, n, lay, vec, fmt):
    """Two uploads that differ in EVERY fourth byte and in nothing else (random against its complement): the two output allocations
    are byte-identical and both are expected4's."""
    src, dst = BgraIn(w, h, n, **lay["in"]), make_out(fmt, w, h, n, lay)
    assert (not misaligned(w, src, dst)) == vec
    images = rand_images4(w, h, n, 34)
    flipped = complement_x(images)
    for a, b in zip(images, flipped):
        assert np.array_equal(a[:, :, :3], b[:, :, :3]) and (a[:, :, 3] != b[:, :, 3]).all()
    for op, order, uv_mode in ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 3, 2)), ORDER_RGB, UV_COPY)):
        check(c, images, op, order, uv_mode, src, dst)
        one = xfer.to_host(dst.buf)
        check(c, flipped, op, order, uv_mode, src, dst)
        two = xfer.to_host(dst.buf)
        assert np.array_equal(one, two), (op, np.flatnonzero(one != two)[:8])


# ---- 5. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "bgr_yuv420_vec", "bgr_yuv420_bytes")


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_launch_contract(fmt):
    """equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch per call of n <= 256 frames -- at a
    batch size (n = 2) where the planar form would take hist_lut_kernel.  CLAHE, for a dividing and a non-dividing grid: one MI_K_COLOR
    launch plus what mi_clahe_u8_batch_dev launches for the same plane in place.  An interleaved output launches the same."""
    w, h, n = 64, 32, 2
    images = rand_images4(w, h, n, 36)
    src, dst = BgraIn(w, h, n, **PITCHED_64["in"]), make_out(fmt, w, h, n, PITCHED_64)
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


# ---- 6. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 1, 1))], ids=["eq", "clahe-1x1"])
def test_chunking(c, op, fmt):
    """One frame past the chunk of 256: two launch sequences, the second of one frame; every frame distinct, every frame checked, ONE
    count for the call."""
    w, h, n = 16, 2, 257
    check(c, rand_images4(w, h, n, 37), op, ORDER_RGB, UV_COPY, BgraIn(w, h, n), make_out(fmt, w, h, n, TIGHT))


# ---- 7. errors, zero sizes, busy -------------------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    images = rand_images4(w, h, n, 38)
    src = BgraIn(w, h, n, pitch=144, frame_gap=16).upload(images)
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
            return L.mi_equalize_hist_bgra_to_yuv420_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgra_to_yuv420_batch_dev(*args(kw), 2.0, tx, ty, stream())
        il = dict(chroma=mi_lumaeq.CHROMA_INTERLEAVED, cp=w)
        bad = [dict(ctx=None), dict(i=None), dict(out=False),                                 # a null ctx, d_in or out
               dict(y=None), dict(c0=None), dict(c1=None), dict(il, y=None), dict(il, c0=None),    # a null plane pointer
               dict(chroma=2), dict(chroma=-1),                                               # a chroma other than the two values
               dict(order=2), dict(order=-1),                                                 # an order other than the two
               dict(uvm=2), dict(uvm=-1),                                                     # a bad uv_mode
               dict(w=-2), dict(h=-2), dict(n=-1),                                            # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),      # odd sizes, also when another size is 0
               dict(il, w=31, h=0), dict(il, h=15, n=0),
               dict(ip=4 * w - 1), dict(ip=3 * w), dict(il, ip=4 * w - 1),                     # in_pitch < 4*W (a three-channel pitch is too small)
               dict(yp=w - 1), dict(cp=w // 2 - 1), dict(il, cp=w - 1),                        # a pitch below its row
               dict(c0=dst.y_ptr), dict(c1=dst.y_ptr), dict(c1=dst.u_ptr), dict(il, c0=dst.y_ptr),   # two output planes at one address
               dict(y=src.ptr), dict(c0=src.ptr), dict(c1=src.ptr), dict(il, c0=src.ptr), dict(il, y=src.ptr)]   # an output plane at d_in
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, **il) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written, no pointer is looked at
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(il, n=0, c1=None), dict(w=0, i=None, y=None, c0=None, c1=None),
                   dict(n=0, i=None, y=None, c0=None, c1=None, ip=0, yp=0, cp=0)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: their status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, yp=1 << 25, cp=1 << 24)
        planar = L.mi_clahe_u8_batch_dev(hd, dst.y_ptr, 1 << 25, 1 << 26, dst.y_ptr, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        assert eq(**dict(il, **dict(big, cp=1 << 25))) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, dst.y_ptr, dst.y_pitch, dst.fstride, dst.y_ptr, dst.y_pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024,
                                         stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(images)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert counters(c) == before
        c.set_profiling(0)
        # and the context still works; on an interleaved output c1 is ignored, whatever it is
        check(c, images, EQ, ORDER_RGB, UV_FILL128, src, dst)
        nv = Nv12Out(w, h, n)
        src.upload(images)
        planes = Yuv420Planes(nv.y_ptr, nv.y_pitch, nv.uv_ptr, nv.y_ptr, nv.c_pitch, nv.fstride, mi_lumaeq.CHROMA_INTERLEAVED)
        run(c, EQ, src, nv, ORDER_BGR, UV_COPY, planes=planes)
        torch.cuda.synchronize()
        assert nv.same([expected4(img, EQ, ORDER_BGR, UV_COPY) for img in images])[0]


def test_host_form_errors():
    w, h = 32, 16
    img = rand_images4(w, h, 1, 39)[0]
    out = np.full(w * h * 3 // 2, SENT, np.uint8)
    ip, op = img.ctypes.data, out.ctypes.data
    ysz, csz = w * h, w * h // 4
    good = dict(ctx=None, i=ip, step=4 * w, y=op, yp=w, c0=op + ysz, c1=op + ysz + csz, cp=w // 2, chroma=mi_lumaeq.CHROMA_PLANAR, w=w, h=h,
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
                   dict(chroma=7), dict(step=4 * w - 1), dict(yp=w - 1), dict(cp=w // 2 - 1), dict(il, cp=w - 1), dict(w=w - 1), dict(h=h - 1),
                   dict(w=-2), dict(order=2), dict(uvm=2), dict(y=ip), dict(c1=ip), dict(c1=op + ysz), dict(c0=op), dict(w=w - 1, h=0)):
            assert L.mi_equalize_hist_bgra_to_yuv420(*args(kw)) == BAD_ARG, kw
            assert L.mi_clahe_bgra_to_yuv420(*args(kw), 2.0, 2, 2) == BAD_ARG, kw
        assert L.mi_clahe_bgra_to_yuv420(*args({}), 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_bgra_to_yuv420(*args({}), 2.0, 2048, 1024) == UNSUPPORTED
        # W*H > 0x7fffffff / 4 (and within the planar forms' limits): refused before any byte is copied
        bw, bh = 1 << 15, (1 << 14) + 2
        assert 0x7fffffff // 4 < bw * bh <= 0x7fffffff
        huge = dict(w=bw, h=bh, step=4 * bw, yp=bw, cp=bw // 2)
        assert L.mi_equalize_hist_bgra_to_yuv420(*args(huge)) == UNSUPPORTED
        assert L.mi_clahe_bgra_to_yuv420(*args(dict(il, **dict(huge, cp=bw))), 2.0, 2, 2) == UNSUPPORTED
        assert L.mi_equalize_hist_bgra_to_yuv420(*args(dict(w=0))) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0
        assert counters(c) == before


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    images = rand_images4(w, h, 1, 40)
    src = BgraIn(w, h, 1).upload(images)
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


# ---- 8. host forms ---------------------------------------------------------------------------------------------------------------
def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


@pytest.mark.parametrize("w,h", [(16, 2), (66, 34), (64, 32)])
def test_host_forms(w, h):
    """Pageable memory: a view with padded rows at an odd address in; a tight I420, YV12 or NV12 frame out through the binding, and
    pitched host planes with guard bytes (I420 and NV12) through raw ctypes: both ops, both orders, both UV modes.  Registered memory:
    a tight image in, a tight frame out.  The source is unchanged, one call counter moves per call (the staged frame is tight with
    every plane at a 16-byte aligned offset: W % 16 decides)."""
    img = rand_images4(w, h, 1, 43)[0]
    pitch = 4 * w + 23
    raw = np.full(h * pitch + 1, SENT, np.uint8)
    padded = raw[1:].reshape(h, pitch)
    view = padded[:, : 4 * w].reshape(h, w, 4)
    assert np.shares_memory(view, raw) and view.ctypes.data % 2 == 1
    view[:] = img
    raw0 = raw.copy()
    ysz, csz, cw, rows = w * h, w * h // 4, w // 2, h // 2
    yp, cp, uvp = w + 5, cw + 3, w + 7                      # pitched host planes: Y at 1, the chroma behind it, 7 bytes between planes
    y_off, u_off = 1, 1 + yp * h + 7
    v_off = u_off + cp * rows + 7
    total = max(v_off + cp * rows, u_off + uvp * rows) + 64
    one = (1, 0, 0, 0) if w % 16 == 0 else (0, 1, 0, 0)
    ops = (EQ, ("clahe", (2.0, 1, 1))) if h == 2 else (EQ, ("clahe", (2.0, 3, 2)))
    with mi_lumaeq.Context(0) as c:
        for op in ops:
            for order in ORDERS:
                for uv_mode in UV_MODES:
                    want = expected4(img, op, order, uv_mode)
                    for fmt in ("i420", "yv12", "nv12"):
                        before = counters(c)
                        if op is EQ:
                            got = c.equalize_hist_bgra_to_yuv420(view, fmt, order, uv_mode)
                        else:
                            got = c.clahe_bgra_to_yuv420(view, fmt, order, uv_mode, *op[1])
                        assert got.shape == (w * h * 3 // 2,) and np.array_equal(got, as_fmt(want, w, h, fmt)), (op, order, uv_mode, fmt)
                        assert moved(c, before) == one, (fmt, moved(c, before))
                    assert np.array_equal(raw, raw0), "the source was written"
                    for planar in (True, False):
                        buf = np.full(total, SENT, np.uint8)
                        b = buf.ctypes.data
                        planes = (Yuv420Planes(b + y_off, yp, b + u_off, b + v_off, cp, 0, mi_lumaeq.CHROMA_PLANAR) if planar else
                                  Yuv420Planes(b + y_off, yp, b + u_off, None, uvp, 0, mi_lumaeq.CHROMA_INTERLEAVED))
                        a = (c._h, view.ctypes.data, pitch, ctypes.byref(planes), w, h, order, uv_mode)
                        st = c._L.mi_equalize_hist_bgra_to_yuv420(*a) if op is EQ else c._L.mi_clahe_bgra_to_yuv420(*a, *op[1])
                        assert st == 0
                        ref = np.full(total, SENT, np.uint8)
                        ref[y_off: y_off + yp * h].reshape(h, yp)[:, :w] = want[:ysz].reshape(h, w)
                        if planar:
                            ref[u_off: u_off + cp * rows].reshape(rows, cp)[:, :cw] = want[ysz: ysz + csz].reshape(rows, cw)
                            ref[v_off: v_off + cp * rows].reshape(rows, cp)[:, :cw] = want[ysz + csz:].reshape(rows, cw)
                        else:
                            ref[u_off: u_off + uvp * rows].reshape(rows, uvp)[:, :w] = as_fmt(want, w, h, "nv12")[ysz:].reshape(rows, w)
                        assert np.array_equal(buf, ref), (op, order, uv_mode, planar, "pitched host planes")
                        assert np.array_equal(raw, raw0), "the source was written"
        # registered (pinned) tight memory
        raw_i, pin_in = aligned_bytes(w * h * 4)
        raw_o, pin_out = aligned_bytes(w * h * 3 // 2)
        pin_img = pin_in.reshape(h, w, 4)
        pin_img[:] = img
        mi_lumaeq.host_register(pin_in)
        mi_lumaeq.host_register(pin_out)
        try:
            for op in ops:
                for fmt in ("i420", "nv12"):
                    pin_out[:] = SENT
                    if op is EQ:
                        got = c.equalize_hist_bgra_to_yuv420(pin_img, fmt, ORDER_BGR, UV_COPY, out=pin_out)
                    else:
                        got = c.clahe_bgra_to_yuv420(pin_img, fmt, ORDER_BGR, UV_COPY, *op[1], out=pin_out)
                    assert got is pin_out and np.array_equal(pin_out, as_fmt(expected4(img, op, ORDER_BGR, UV_COPY), w, h, fmt)), (op, fmt)
                    assert np.array_equal(pin_img, img), "the source was written"
        finally:
            mi_lumaeq.host_unregister(pin_out)
            mi_lumaeq.host_unregister(pin_in)
        assert (raw_i[: (-raw_i.ctypes.data) % 4096] == SENT).all() and (raw_o[: (-raw_o.ctypes.data) % 4096] == SENT).all()
        assert c.get_stat("error_drains") == 0


# ---- 9. streams and hipGraph -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_stream_and_graph_capture(fmt):
    """A call on a non-default stream.  Then one eager call of each shape, one equalizeHist and one CLAHE call captured on a single
    stream (one linear chain, no parallel branches) and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    cl = ("clahe", (2.0, 4, 2))
    src = BgraIn(w, h, n, **PITCHED_64["in"])
    dst_eq, dst_cl = make_out(fmt, w, h, n, PITCHED_64), make_out(fmt, w, h, n, PITCHED_64)
    with mi_lumaeq.Context(0) as c:
        images = rand_images4(w, h, n, 41)
        src.upload(images)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(c, cl, src, dst_cl, ORDER_RGB, UV_COPY, st=side.cuda_stream)
        side.synchronize()
        assert dst_cl.same([expected4(img, cl, ORDER_RGB, UV_COPY) for img in images])[0], "side stream"
        for op, dst, uv_mode in ((EQ, dst_eq, UV_COPY), (cl, dst_cl, UV_FILL128)):        # the eager calls size the scratch
            dst.clear()
            run(c, op, src, dst, ORDER_BGR, uv_mode)
            torch.cuda.synchronize()
            assert dst.same([expected4(img, op, ORDER_BGR, uv_mode) for img in images])[0], ("eager", op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            run(c, EQ, src, dst_eq, ORDER_BGR, UV_COPY, st=st)
            run(c, cl, src, dst_cl, ORDER_BGR, UV_FILL128, st=st)
        for rep in range(2):
            fresh = rand_images4(w, h, n, 42 + rep)
            src.upload(fresh)
            dst_eq.clear()
            dst_cl.clear()
            g.replay()
            torch.cuda.synchronize()
            assert dst_eq.same([expected4(img, EQ, ORDER_BGR, UV_COPY) for img in fresh])[0], ("graph replay", "eq", rep)
            assert dst_cl.same([expected4(img, cl, ORDER_BGR, UV_FILL128) for img in fresh])[0], ("graph replay", "clahe", rep)
            assert np.array_equal(src.host(), src.image(fresh))
