"""Four-channel BGRA / RGBA (CV_8UC4) images in, pitched packed 4:2:2 frames (YUY2 / UYVY) out on the GPU:
mi_equalize_hist_bgra_to_packed422_batch_dev, mi_clahe_bgra_to_packed422_batch_dev and their host forms.  Expected bytes
(bgra_packed422_ref.expected): the three-channel reference of tests/bgr_packed422_ref.py on the image with its fourth byte removed;
tests/test_bgra_to_packed422_abi.py backs it on the CPU.  Pixels are full-range random bytes, the fourth byte included.  The input and
the output live in sentinel-filled allocations with 64 guard bytes and the WHOLE allocation is compared, input and output: every
comparison in this file is exact.  After every call the test asserts which of "bgra_packed422_vec" / "bgra_packed422_bytes" moved, by
the header's rule restated in bgra_packed422_ref.misaligned, and that no bgr_packed422* counter did.

How many workgroups bgra_to_packed422_hist_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_bgra_to_packed422 computes
B = min(blocks_per_frame(W*H*3 bytes, H rows, n, 2048), ceil(items / 256)) -- the three-channel form's rule on this form's byte basis,
half of 4 + 2 bytes per pixel -- and blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than
rows, whatever the CU count, which only lowers it.  So B <= max(1, floor(W*H*3 / 16384)), B <= H, and the 256 lanes of a workgroup step
through the frame by stride = 256 * B items: 16 x 1 pixel groups on the vector walk (gx_n = W/16 per row, the carried walk y += dy,
gx += dgx with dy = stride / gx_n, dgx = stride % gx_n and a wrap when gx >= gx_n), macropixels on the byte walk.
  8192 x 2: 1024 groups, bytes 49152 -> 3, rows 2: B <= 2.  B = 2: stride 512, every lane takes exactly two steps.  B = 1: stride 256,
    every lane takes four.
  4112 x 4: gx_n = 257, 1028 groups, bytes 49344 -> 3, rows 4: B <= 3 (the three-channel basis gave 2).  B = 3: stride 768, dy = 2,
    dgx = 254; lanes gi < 260 take a second, partial step, and those with gx >= 3 wrap into the next row.  B = 2: stride 512, dy = 1,
    dgx = 255; every lane takes a second step and wraps unless gx < 2, lanes gi < 4 a third.  B = 1: stride 256, dy = 0, dgx = 256;
    every lane takes four steps, wrapping when gx >= 1, lanes gi < 4 a fifth.
  66 x 35, byte walk: 1155 macropixels, bytes 6930 -> B = 1: lanes t < 131 take five steps, the others four."""
import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY
from bgra_packed422_ref import (SENT, COUNTERS, SIBLING_COUNTERS, BgraIn, P422Out, convert, mapped_luma, pack, misaligned, rand_images4,
                                first3, with_x)

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


def siblings(c):
    return tuple(c.get_stat(k) for k in SIBLING_COUNTERS)


def expected(img, op, order, fmt, uv_mode, contract=False):
    """bgra_packed422_ref.expected with the conversion and the mapped luma of an image computed once and shared: they do not depend on
    the format or the UV mode (nor on the fourth byte, which is dropped before the key is made)."""
    img = first3(img)
    key = (img.shape, img.tobytes(), order)
    if key not in _ref:
        _ref[key] = convert(img, order)
    y, uv = _ref[key]
    if op is None:
        return pack(y, uv if uv_mode == UV_COPY else np.full_like(uv, 128), fmt)
    mkey = key + (op, contract)
    if mkey not in _ref:
        _ref[mkey] = mapped_luma(y, op, contract)
    return pack(_ref[mkey], uv if uv_mode == UV_COPY else np.full_like(uv, 128), fmt)


def run(c, op, src, dst, order, fmt, uv_mode, n=None, st=None):
    kind, cfg = op
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_bgra_to_packed422_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, order, fmt, uv_mode, **kw)
    else:
        c.clahe_bgra_to_packed422_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, order, fmt, uv_mode, *cfg, **kw)


def check(c, images, op, order, fmt, uv_mode, src, dst, contract=False):
    """One call on uploaded `images`: the whole output allocation is the reference's image of it, the whole input allocation is what
    was uploaded, the counter that names the walk moved by exactly one and no three-channel counter moved."""
    src.upload(images)
    dst.clear()
    before, sib = counters(c), siblings(c)
    run(c, op, src, dst, order, fmt, uv_mode)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same([expected(img, op, order, fmt, uv_mode, contract) for img in images])
    assert ok, (src.w, src.h, op, order, fmt, uv_mode, nbad, where)
    assert np.array_equal(src.host(), src.image(images)), "the input allocation was written"
    vec = not misaligned(src.w, src, dst)
    after = counters(c)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if vec else (0, 1)), (before, after, vec)
    assert siblings(c) == sib, "a three-channel counter moved"


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
# in pitch 4 * 66 + 1 = 265, offsets 1 / 4, odd gaps
ODD_66 = (dict(pitch=265, frame_gap=7, off=1), dict(pitch=136, frame_gap=12, off=4))
# in: 272 * 32 + 64 = 8768 = 548 * 16; out: 144 * 32 + 32 = 4640 = 290 * 16
PITCHED_64 = (dict(pitch=272, frame_gap=64, off=32), dict(pitch=144, frame_gap=32, off=16))
PARITY = [
    # id, W, H, n, BgraIn layout, P422Out layout, vector walk, the ops
    ("16x1", 16, 1, 1, {}, {}, True, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 3, 1))]),                  # one vector group; 3 does not divide 16
    ("2x1", 2, 1, 1, {}, {}, False, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),                   # one macropixel; 2 x 1 leaves odd tiles
    ("48x5", 48, 5, 2, {}, {}, True, [EQ, ("clahe", (2.0, 3, 5)), ("clahe", (2.0, 5, 4))]),                  # gx_n = 3, odd height; 5 x 4 does not divide
    ("66x35-odd", 66, 35, 2, *ODD_66, False, [EQ, ("clahe", (2.0, 3, 5)), ("clahe", (3.0, 4, 3))]),          # nothing aligned; 4 x 3 does not divide
    ("64x32-pitched", 64, 32, 2, *PITCHED_64, True, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 5, 3))]),   # padding, gaps, aligned
]


@pytest.mark.parametrize("name,w,h,n,si,do,vec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, si, do, vec, ops):
    src, dst = BgraIn(w, h, n, **si), P422Out(w, h, n, **do)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    images = rand_images4(w, h, n, 31)
    for op in ops:
        for order in ORDERS:
            for fmt in FMTS:
                for uv_mode in UV_MODES:
                    check(c, images, op, order, fmt, uv_mode, src, dst)


# ---- 2. one alignment term at a time ---------------------------------------------------------------------------------------------
# 32 x 3 x 2 frames; tight: in pitch 128, in frame 384, out pitch 64, out frame 192 = 12 * 16
ONE_TERM = [
    # the broken term (None: the positive case), W, BgraIn layout, P422Out layout
    (None, 32, {}, {}),
    ("in", 32, dict(off=8), {}),
    ("in_pitch", 32, dict(pitch=136, frame_gap=8), {}),                         # 136 = 8 (mod 16); 136 * 3 + 8 = 416 = 26 * 16
    ("in_frame", 32, dict(frame_gap=8), {}),                                    # 392
    ("out", 32, {}, dict(off=4)),
    ("out_pitch", 32, {}, dict(pitch=72, frame_gap=8)),                         # 72 = 8 (mod 16); 72 * 3 + 8 = 224
    ("out_frame", 32, {}, dict(frame_gap=4)),                                   # 196 = 4 (mod 16)
    ("width", 24, {}, {}),                                                      # in 96, 288; out 48, 144: every term a multiple of 16
]


@pytest.mark.parametrize("term,w,si,do", ONE_TERM, ids=[str(t[0]) for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, term, w, si, do):
    """Exactly one of the six terms misses 16 (the output terms at 4 or 8 mod 16, as the packed forms' rule of multiples of 4 allows), or
    the width does: the byte walk, the same bytes, the same untouched guards, the counter that names the walk.  None does: the vector walk."""
    h, n = 3, 2
    src, dst = BgraIn(w, h, n, **si), P422Out(w, h, n, **do)
    assert misaligned(w, src, dst) == ([term] if term else [])
    images = rand_images4(w, h, n, 32)
    for op, order, fmt, uv_mode in ((EQ, ORDER_BGR, FMT_YUY2, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, FMT_UYVY, UV_FILL128)):
        check(c, images, op, order, fmt, uv_mode, src, dst)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
LOOP_SHAPES = [
    # id, W, H, n, BgraIn layout, P422Out layout, vector walk, the bound on B (see the module docstring)
    ("8192x2", 8192, 2, 1, {}, {}, True, 2),
    ("4112x4", 4112, 4, 1, {}, {}, True, 3),
    ("66x35-odd", 66, 35, 2, *ODD_66, False, 1),
]


@pytest.mark.parametrize("name,w,h,n,si,do,vec,bmax", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, si, do, vec, bmax):
    """bgra_to_packed422_hist_kernel where a lane owns more than one group / macropixel: with the histogram (equalizeHist, U and V
    computed) and without it (CLAHE 2 x 2, chroma filled).  The bound is re-derived here from the launch rule on this form's byte basis
    (W*H*3): it differs from the three-channel form's at 4112 x 4 (3, not 2), where the shape still loops for every B it allows."""
    src, dst = BgraIn(w, h, n, **si), P422Out(w, h, n, **do)
    assert (not misaligned(w, src, dst)) == vec, misaligned(w, src, dst)
    bound = min(max(1, w * h * 3 // 16384), h)
    assert bound == bmax
    assert (w * h // 16 if vec else w * h // 2) > 256 * bound, "the shape would not loop"
    images = rand_images4(w, h, n, 33)
    for order, fmt in ((ORDER_BGR, FMT_YUY2), (ORDER_RGB, FMT_UYVY)):
        check(c, images, EQ, order, fmt, UV_COPY, src, dst)
        check(c, images, ("clahe", (2.0, 2, 2)), order, fmt, UV_FILL128, src, dst)


# ---- 4. the fourth byte is ignored -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,si,do", [("vec", 64, 32, *PITCHED_64), ("bytes", 66, 35, *ODD_66)], ids=["vec", "bytes"])
def test_fourth_byte_is_ignored(c, name, w, h, si, do):
    """Uploads that differ only in byte 3 of every pixel (0x00, 0xFF, random) give identical output allocations, and the reference's."""
    n = 2
    images = rand_images4(w, h, n, 34)
    src, dst = BgraIn(w, h, n, **si), P422Out(w, h, n, **do)
    variants = [with_x(images, 0x00), with_x(images, 0xFF), with_x(images, "random")]
    assert all(np.array_equal(v[0][:, :, :3], images[0][:, :, :3]) for v in variants)
    assert not np.array_equal(variants[0][0], variants[1][0]) and not np.array_equal(variants[1][0], variants[2][0])
    for op, order, fmt, uv_mode in ((EQ, ORDER_BGR, FMT_YUY2, UV_COPY), (("clahe", (2.0, 4, 2)), ORDER_RGB, FMT_UYVY, UV_COPY)):
        outs = []
        for v in variants:
            check(c, v, op, order, fmt, uv_mode, src, dst)
            outs.append(dst.host().copy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2]), (op, "the fourth byte reached the output")


# ---- 5. equal to the three-channel form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=["yuy2", "uyvy"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_equal_to_the_three_channel_form(c, op, fmt):
    """On one pitched layout the output allocation equals what mi_*_bgr_to_packed422_batch_dev writes into the same layout for the
    images sliced to three channels (the route this form replaces)."""
    w, h, n = 64, 32, 3
    images = rand_images4(w, h, n, 35)
    src = BgraIn(w, h, n, **PITCHED_64[0]).upload(images)
    one, two = (P422Out(w, h, n, **PITCHED_64[1]) for _ in range(2))
    d3 = xfer.to_device(np.stack([first3(img) for img in images]))
    for order in ORDERS:
        one.clear()
        two.clear()
        run(c, op, src, one, order, fmt, UV_COPY)
        if op is EQ:
            c.equalize_hist_bgr_to_packed422_batch_dev(d3, two.ptr, w, h, n, order, fmt, UV_COPY, **two.kw(), stream=stream())
        else:
            c.clahe_bgr_to_packed422_batch_dev(d3, two.ptr, w, h, n, order, fmt, UV_COPY, *op[1], **two.kw(), stream=stream())
        torch.cuda.synchronize()
        assert np.array_equal(one.host(), two.host()), (op, fmt, order)
        assert one.same([expected(img, op, order, fmt, UV_COPY) for img in images])[0], (op, fmt, order)
        assert not np.array_equal(one.host(), one.image([expected(img, None, order, fmt, UV_COPY) for img in images])), "the luma was not mapped"


# ---- 6. clahe_fp_contract --------------------------------------------------------------------------------------------------------
def test_clahe_fp_contract():
    """Both settings on one shape: the bytes are the reference's in that arithmetic mode (the option is restored)."""
    w, h, n = 66, 35, 2
    images = rand_images4(w, h, n, 36)
    src, dst = BgraIn(w, h, n, **ODD_66[0]), P422Out(w, h, n, **ODD_66[1])
    cl = ("clahe", (2.0, 3, 2))
    with mi_lumaeq.Context(0) as c:
        c.set_option("clahe_fp_contract", 1)
        try:
            check(c, images, cl, ORDER_RGB, FMT_UYVY, UV_COPY, src, dst, contract=True)
        finally:
            c.set_option("clahe_fp_contract", 0)
        check(c, images, cl, ORDER_RGB, FMT_UYVY, UV_COPY, src, dst)


# ---- 7. chunk seam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 1, 1))], ids=["eq", "clahe-1x1"])
def test_chunk_seam(c, op):
    """One frame past the chunk of 256: two launch sequences, the second of one frame.  Every frame has its own random content and
    every frame -- the seam frames 255 and 256, the last, among them -- is compared with the reference, exactly."""
    w, h, n = 16, 2, 257
    check(c, rand_images4(w, h, n, 37), op, ORDER_RGB, FMT_UYVY, UV_COPY, BgraIn(w, h, n), P422Out(w, h, n))


# ---- 8. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


def test_launch_contract():
    """equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch per call of n <= 256 frames.  CLAHE, for
    a dividing and a non-dividing grid: one MI_K_COLOR launch plus what mi_clahe_packed422_batch_dev launches for the same frames in
    place."""
    w, h, n = 64, 32, 2
    images = rand_images4(w, h, n, 38)
    src, dst = BgraIn(w, h, n, **PITCHED_64[0]), P422Out(w, h, n, **PITCHED_64[1])
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        c.profile_read(reset=True)
        check(c, images, EQ, ORDER_BGR, FMT_YUY2, UV_COPY, src, dst)
        got = launches(c)
        want = {"color_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}
        assert got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, got
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
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 9. errors, zero sizes, busy, hipGraph ---------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 15, 2
    images = rand_images4(w, h, n, 39)
    src = BgraIn(w, h, n, pitch=144, frame_gap=16).upload(images)
    dst = P422Out(w, h, n, pitch=80, frame_gap=16)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        before, sib = counters(c), siblings(c)
        base = dict(ctx=hd, i=src.ptr, ip=src.pitch, fi=src.fstride, o=dst.ptr, op=dst.pitch, fo=dst.fstride, w=w, h=h, n=n,
                    order=ORDER_BGR, fmt=FMT_YUY2, uvm=UV_COPY)

        def args(kw):
            a = dict(base)
            a.update(kw)
            return (a["ctx"], a["i"], a["ip"], a["fi"], a["o"], a["op"], a["fo"], a["w"], a["h"], a["n"], a["order"], a["fmt"], a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgra_to_packed422_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgra_to_packed422_batch_dev(*args(kw), 2.0, tx, ty, stream())
        bad = [dict(ctx=None), dict(i=None), dict(o=None),                                    # null pointers
               dict(order=2), dict(order=-1), dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),
               dict(w=-2), dict(h=-1), dict(n=-1),                                            # negative sizes
               dict(w=31), dict(w=31, h=0), dict(w=31, n=0),                                  # an odd width, also when another size is 0
               dict(ip=4 * w - 1), dict(ip=3 * w), dict(op=2 * w - 4),                        # a pitch below its row (3*W is not enough)
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
        # sizes and tile grids the sibling refuses: its status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, op=1 << 26, fi=1 << 28, fo=1 << 27)
        sib_big = L.mi_clahe_bgr_to_packed422_batch_dev(*args(big), 2.0, 2, 2, stream())
        assert sib_big == UNSUPPORTED and eq(**big) == sib_big and cl(**big) == sib_big
        sib_tiles = L.mi_clahe_bgr_to_packed422_batch_dev(*args({}), 2.0, 2048, 1024, stream())
        assert sib_tiles == UNSUPPORTED and cl(2048, 1024) == sib_tiles
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(images)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert counters(c) == before and siblings(c) == sib
        c.set_profiling(0)
        # and the context still works
        check(c, images, EQ, ORDER_RGB, FMT_UYVY, UV_FILL128, src, dst)


def test_host_form_errors():
    w, h = 32, 15
    img = rand_images4(w, h, 1, 40)[0]
    out = np.full(h * 2 * w, SENT, np.uint8)
    ip, op = img.ctypes.data, out.ctypes.data
    good = dict(ctx=None, i=ip, step=4 * w, o=op, op=2 * w, w=w, h=h, order=0, fmt=FMT_UYVY, uvm=1)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        good["ctx"] = hd
        before = counters(c)

        def args(kw):
            a = dict(good)
            a.update(kw)
            return (a["ctx"], a["i"], a["step"], a["o"], a["op"], a["w"], a["h"], a["order"], a["fmt"], a["uvm"])
        for kw in (dict(ctx=None), dict(i=None), dict(o=None), dict(step=4 * w - 1), dict(op=2 * w - 1), dict(w=w - 1), dict(w=-2), dict(h=-1),
                   dict(order=2), dict(fmt=1), dict(fmt=4), dict(uvm=2), dict(o=ip), dict(w=w - 1, h=0)):
            assert L.mi_equalize_hist_bgra_to_packed422(*args(kw)) == BAD_ARG, kw
            assert L.mi_clahe_bgra_to_packed422(*args(kw), 2.0, 2, 2) == BAD_ARG, kw
        assert L.mi_clahe_bgra_to_packed422(*args({}), 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_bgra_to_packed422(*args({}), 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_bgra_to_packed422(*args(dict(w=0))) == 0
        assert L.mi_equalize_hist_bgra_to_packed422(*args(dict(h=0))) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0
        assert counters(c) == before


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    images = rand_images4(w, h, 1, 41)
    src = BgraIn(w, h, 1).upload(images)
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


def test_stream_and_graph_capture():
    """A call on a side stream and one on MI_STREAM_CTX.  Then one eager call of each shape, one equalizeHist and one CLAHE call captured
    on a single stream (one linear chain, no parallel branches) and one replay onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 2
    cl = ("clahe", (2.0, 4, 2))
    src = BgraIn(w, h, n, **PITCHED_64[0])
    dst_eq, dst_cl = P422Out(w, h, n, **PITCHED_64[1]), P422Out(w, h, n, **PITCHED_64[1])
    calls = ((EQ, dst_eq, FMT_YUY2, UV_COPY), (cl, dst_cl, FMT_UYVY, UV_FILL128))
    with mi_lumaeq.Context(0) as c:
        images = rand_images4(w, h, n, 42)
        src.upload(images)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        run(c, cl, src, dst_cl, ORDER_RGB, FMT_YUY2, UV_COPY, st=side.cuda_stream)
        side.synchronize()
        assert dst_cl.same([expected(img, cl, ORDER_RGB, FMT_YUY2, UV_COPY) for img in images])[0], "side stream"
        dst_eq.clear()
        torch.cuda.synchronize()
        run(c, EQ, src, dst_eq, ORDER_RGB, FMT_UYVY, UV_COPY, st=mi_lumaeq.STREAM_CTX)
        c.synchronize(mi_lumaeq.STREAM_CTX)
        assert dst_eq.same([expected(img, EQ, ORDER_RGB, FMT_UYVY, UV_COPY) for img in images])[0], "context stream"
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
        fresh = rand_images4(w, h, n, 43)
        src.upload(fresh)
        dst_eq.clear()
        dst_cl.clear()
        g.replay()
        torch.cuda.synchronize()
        for op, dst, fmt, uv_mode in calls:
            assert dst.same([expected(img, op, ORDER_BGR, fmt, uv_mode) for img in fresh])[0], ("graph replay", op)
        assert np.array_equal(src.host(), src.image(fresh))


# ---- 10. host forms --------------------------------------------------------------------------------------------------------------
def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


@pytest.mark.parametrize("w,h", [(16, 1), (66, 35), (64, 32)])
def test_host_forms(w, h):
    """Pageable memory: a tight image and a view with padded rows at an odd address in; a new tight H x 2W frame out, and a caller's
    padded view at an odd address out whose padding and guards stay untouched: both ops, both orders, both formats, both UV modes; the
    source is unchanged; the counter names the walk of the tight, aligned device copy (W % 16 == 0: the groups).  Then registered
    (pinned) tight memory on both sides."""
    img = rand_images4(w, h, 1, 45)[0]
    pitch = 4 * w + 23
    raw = np.full(h * pitch + 1, SENT, np.uint8)
    view = raw[1:].reshape(h, pitch)[:, : 4 * w].reshape(h, w, 4)
    assert np.shares_memory(view, raw) and view.ctypes.data % 2 == 1
    view[:] = img
    raw0 = raw.copy()
    opitch = 2 * w + 5
    ops = (EQ, ("clahe", (2.0, 3, 2)) if h > 1 else ("clahe", (2.0, 1, 1)))
    with mi_lumaeq.Context(0) as c:
        sib = siblings(c)
        for op in ops:
            for order in ORDERS:
                for fmt in FMTS:
                    for uv_mode in UV_MODES:
                        want = expected(img, op, order, fmt, uv_mode)
                        before = counters(c)
                        if op is EQ:
                            got = c.equalize_hist_bgra_to_packed422(img, order, fmt, uv_mode)              # tight in, tight out
                        else:
                            got = c.clahe_bgra_to_packed422(img, order, fmt, uv_mode, *op[1])
                        assert got.shape == (h, 2 * w) and np.array_equal(got, want), (op, order, fmt, uv_mode)
                        after = counters(c)
                        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if w % 16 == 0 else (0, 1))
                        buf = np.full(h * opitch + 1 + 64, SENT, np.uint8)
                        oview = buf[1: 1 + h * opitch].reshape(h, opitch)[:, : 2 * w]
                        assert oview.ctypes.data % 2 == 1
                        if op is EQ:
                            ret = c.equalize_hist_bgra_to_packed422(view, order, fmt, uv_mode, out=oview)  # pitched, odd addresses
                        else:
                            ret = c.clahe_bgra_to_packed422(view, order, fmt, uv_mode, *op[1], out=oview)
                        assert ret is oview
                        ref = np.full(buf.size, SENT, np.uint8)
                        ref[1: 1 + h * opitch].reshape(h, opitch)[:, : 2 * w] = want
                        assert np.array_equal(buf, ref), (op, order, fmt, uv_mode, "padded host view")
                        assert np.array_equal(raw, raw0), "the source was written"
        # registered (pinned) tight memory
        raw_i, pin_in = aligned_bytes(w * h * 4)
        raw_o, pin_out = aligned_bytes(w * h * 2)
        pin_img = pin_in.reshape(h, w, 4)
        pin_img[:] = img
        pin_frame = pin_out.reshape(h, 2 * w)
        mi_lumaeq.host_register(pin_in)
        mi_lumaeq.host_register(pin_out)
        try:
            for op in ops:
                for fmt in FMTS:
                    pin_out[:] = SENT
                    if op is EQ:
                        got = c.equalize_hist_bgra_to_packed422(pin_img, ORDER_BGR, fmt, UV_COPY, out=pin_frame)
                    else:
                        got = c.clahe_bgra_to_packed422(pin_img, ORDER_BGR, fmt, UV_COPY, *op[1], out=pin_frame)
                    assert got is pin_frame and np.array_equal(pin_frame, expected(img, op, ORDER_BGR, fmt, UV_COPY)), (op, fmt)
                    assert np.array_equal(pin_img, img), "the source was written"
        finally:
            mi_lumaeq.host_unregister(pin_out)
            mi_lumaeq.host_unregister(pin_in)
        assert (raw_i[: (-raw_i.ctypes.data) % 4096] == SENT).all() and (raw_o[: (-raw_o.ctypes.data) % 4096] == SENT).all()
        assert (raw_i[(-raw_i.ctypes.data) % 4096 + w * h * 4:] == SENT).all() and (raw_o[(-raw_o.ctypes.data) % 4096 + w * h * 2:] == SENT).all()
        assert c.get_stat("error_drains") == 0
        assert siblings(c) == sib, "a three-channel counter moved"
