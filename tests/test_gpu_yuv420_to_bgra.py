"""4:2:0 frames (I420 / YV12 planes, NV12, or U and V rows side by side in one plane) in, four-channel BGRA / RGBA (CV_8UC4, A = 255)
images out on the GPU: mi_equalize_hist_yuv420_to_bgra_batch_dev, mi_clahe_yuv420_to_bgra_batch_dev and their host forms.  Expected
bytes are tests/yuv420_bgra_layouts.py's: oracle.nv12_to_bgr(oracle.nv12_frame(...)), channels 0 and 2 exchanged for MI_ORDER_RGB, a
fourth byte of 255.  Y, U and V are independent full-range random bytes, so an identity map, a swapped U / V order or a mixed-up row
cannot pass.  Every side of a call lives in a sentinel-filled allocation with 64 guard bytes and the WHOLE allocation is compared, input
and output: every comparison in this file is exact.  After every GPU call the exact delta of the six yuv420_bgra_* counters is asserted,
and that no nv12_bgr_* / yuv420_bgr_* counter moved.

How many workgroups the pixel-writing kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_yuv420_to_bgra takes
    B = min(blocks_per_frame(W*H*11/4 bytes, H/2 rows, n, 2048), ceil(items / 256)),
and blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count,
which only lowers it.  So  B <= max(1, floor(W*H*11/4 / 16384)),  B <= H/2,  and the 256 lanes of a workgroup step through a frame by
stride = 256 * B items: 16 x 2 pixel groups on the vector walk (gx_n = W/16 a row pair, the carried walk by += dby, gx += dgx with
dby = stride / gx_n, dgx = stride % gx_n and a wrap when gx >= gx_n), 2 x 2 blocks on the byte walk.
  112 x 80 : 24640 bytes, B = 1, stride 256; gx_n 7, 280 groups for 256 lanes: dby 36, dgx 4, the wrap fires for gx >= 3
  16000 x 6: 264000 bytes allow 16, H/2 = 3 rows allow 3: stride <= 768 < gx_n 1000, so dby 0 and every step is a pure gx step;
             3000 groups: a lane takes four or more steps and its gx wraps more than once
  66 x 34  : byte walk, 6171 bytes, B = 1; 33 x 17 = 561 blocks for 256 lanes: three steps, the last of 49 lanes"""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
import yuv420_bgra_layouts as lay
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, CHROMA_PLANAR, Yuv420Planes
from yuv420_bgra_layouts import SENT, EQ, Side, SideBySide, BgraOut, content, tight_frame, expected_bgra
from test_gpu_nv12_to_bgr_geometry import ONEPASS_SHAPES, K

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
ORDERS = [ORDER_BGR, ORDER_RGB]
FMTS = ["i420", "yv12", "nv12", "side"]
ONE, TWO, VEC, BYTES = (1, 0), (0, 1), (1, 0), (0, 1)


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_src(fmt, w, h, n, **kw):
    return SideBySide(w, h, n, **kw) if fmt == "side" else Side(w, h, n, fmt, **kw)


def run(c, op, src, dst, order, n=None, st=None, planes=None):
    kind, cfg = op
    a = planes or src.planes()
    kw = dict(dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_yuv420_to_bgra_batch_dev(a, dst.ptr, src.w, src.h, n, order, **kw)
    else:
        c.clahe_yuv420_to_bgra_batch_dev(a, dst.ptr, src.w, src.h, n, order, *cfg, **kw)


def stats(c):
    return tuple(c.get_stat(s) for s in lay.COUNTERS)


def foreign(c):
    return tuple(c.get_stat(s) for s in lay.FOREIGN)


def delta(before, after):
    return tuple(a - b for a, b in zip(after, before))


def check(c, w, h, n, seed, op, order, src, dst, want, contract=False):
    """One call on the uploaded content: exact output, untouched guards and input, the six counters moved by `want` =
    ((onepass, twopass), (vec, bytes)) + (0, 0) for the list pair, and no counter of the forms next door moved."""
    frames = content(w, h, n, seed)
    src.upload(frames)
    dst.clear()
    before, fbefore = stats(c), foreign(c)
    run(c, op, src, dst, order)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same(expected_bgra(w, h, n, seed, op, order, contract))
    assert ok, (w, h, src.fmt, op, order, nbad, where)
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"
    assert delta(before, stats(c)) == want[0] + want[1] + (0, 0), (op, before, stats(c), want)
    assert foreign(c) == fbefore, "a counter of another form moved"


def want_of(w, h, op, src, dst):
    """The counter deltas the documented rule gives for a batch call on these two allocations."""
    vec = lay.side_vec(w, src, dst)
    if op is EQ:
        return ONE, (VEC if vec else BYTES)
    one = vec and lay.onepass_shape(w, h, op[1][1], op[1][2], K)
    return (ONE if one else TWO), (VEC if vec else BYTES)


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
def odd_66(fmt):
    kw = dict(y_pitch=67, gap0=3, frame_gap=7, off=1)
    return dict(kw, c_pitch=35, gap1=5) if fmt in ("i420", "yv12") else dict(kw, c_pitch=69)


def pitched_64(fmt):
    """every Y and image term a multiple of 16; the planar chroma terms 8 past one, the interleaved ones multiples of 16"""
    if fmt in ("i420", "yv12"):
        return dict(y_pitch=80, c_pitch=40, gap0=16, gap1=8, frame_gap=24, off=16)
    if fmt == "side":
        return dict(y_pitch=80, c_pitch=72, gap0=16, frame_gap=16, off=16)
    return dict(y_pitch=80, c_pitch=96, gap0=32, frame_gap=48, off=16)


PARITY = [
    # id, W, H, n, source layout, image layout, ops with their hand-written counter deltas
    ("16x2-tight", 16, 2, 2, lambda f: {}, {}, [(EQ, (ONE, VEC)), (("clahe", (2.0, 1, 1)), (ONE, VEC))]),
    # gx_n = 3: the row walk wraps; 3 x 2 tiles of 16 x 3 in one pass, 5 x 4 pads by REFLECT_101
    ("48x6-tight", 48, 6, 2, lambda f: {}, {}, [(EQ, (ONE, VEC)), (("clahe", (2.0, 3, 2)), (ONE, VEC)), (("clahe", (2.0, 5, 4)), (TWO, VEC))]),
    ("2x2", 2, 2, 2, lambda f: {}, {}, [(EQ, (ONE, BYTES)), (("clahe", (2.0, 1, 1)), (TWO, BYTES))]),
    ("66x34-odd", 66, 34, 2, odd_66, dict(pitch=269, frame_gap=7, off=1), [(EQ, (ONE, BYTES)), (("clahe", (2.0, 3, 2)), (TWO, BYTES))]),
    # 4 x 2: tiles of 16 x 16, one pass; 8 x 8: tile width 8, the fallback
    ("64x32-pitched", 64, 32, 2, pitched_64, dict(pitch=272, frame_gap=64, off=32),
     [(EQ, (ONE, VEC)), (("clahe", (2.0, 4, 2)), (ONE, VEC)), (("clahe", (2.0, 8, 8)), (TWO, VEC))]),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,w,h,n,si,di,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, si, di, ops, fmt, order):
    src, dst = make_src(fmt, w, h, n, **si(fmt)), BgraOut(w, h, n, **di)
    if name == "64x32-pitched":
        p = src.planes()
        assert src.fstride % 16 == 0 and dst.fstride % 16 == 0
        assert (p.c0 % 16, p.c_pitch % 16) == (0, 0) if fmt == "nv12" else (p.c_pitch % 16 == 8 and p.c1 % 8 == 0)
    for op, want in ops:
        assert want == want_of(w, h, op, src, dst), ("the restated rule disagrees with the table", name, fmt, op)
        check(c, w, h, n, 31, op, order, src, dst, want)


# ---- 2. the alignment rule, one term at a time -----------------------------------------------------------------------------------
def rule_layout(fmt, term, by):
    """32 x 4, two frames, every term a multiple of 16 (the planar chroma pitch 32, so that + 8 is still a multiple of 8), then ONE
    term moved by `by` (4 or 8) without moving another modulo 16: Side and BgraOut keyword arguments.  A Side lays a frame out as Y,
    gap0, first chroma plane, gap1, second chroma plane, frame_gap; "yv12" has V first, so its c0 is the second plane."""
    planar = fmt != "nv12"
    si = dict(y_pitch=48, c_pitch=32 if planar else 48, gap0=16, frame_gap=16, off=16)
    if planar:
        si["gap1"] = 16
    di = dict(pitch=144, frame_gap=16, off=16)
    first, second = ("c1", "c0") if fmt == "yv12" else ("c0", "c1")
    if term == "y":                              # the frame starts later, its chroma planes and its stride stay
        si["off"] += by
        si["gap0"] -= by
        si["frame_gap"] += by
    elif term == "y_pitch":                      # 4 rows: everything behind moves by 4 * by, a multiple of 16
        si["y_pitch"] += by
    elif term == "frame_stride":
        si["frame_gap"] += by
    elif term == first:
        si["gap0"] += by
        si["gap1" if planar else "frame_gap"] -= by
    elif term == second:
        si["gap1"] += by
        si["frame_gap"] -= by
    elif term == "c_pitch":                      # 2 chroma rows a plane: the second plane and the stride are put back on their residues
        si["c_pitch"] += by
        if planar:
            si["gap1"] += (-2 * by) % 16
            si["frame_gap"] += (-(4 * by + (-2 * by) % 16)) % 16
        else:
            si["frame_gap"] += (-2 * by) % 16
    elif term == "d_out":
        di["off"] += by
    elif term == "out_pitch":                    # 4 rows
        di["pitch"] += by
    elif term == "out_frame_stride":
        di["frame_gap"] += by
    return si, di


def rule_terms(src, dst):
    y, c0, c1 = src.offsets()
    return dict(y=y, y_pitch=src.y_pitch, frame_stride=src.fstride, d_out=dst.off, out_pitch=dst.pitch, out_frame_stride=dst.fstride,
                c0=c0, c1=c1 if c1 is not None else 0, c_pitch=src.c_pitch)


SIX = ("y", "y_pitch", "frame_stride", "d_out", "out_pitch", "out_frame_stride")
ONE_TERM = [("i420", t, 8, False) for t in SIX] + [("nv12", t, 8, False) for t in SIX] + \
           [("i420", t, 8, True) for t in ("c0", "c1", "c_pitch")] + [("yv12", t, 4, False) for t in ("c0", "c1", "c_pitch")] + \
           [("nv12", t, 8, False) for t in ("c0", "c_pitch")]


@pytest.mark.parametrize("fmt,term,by,vec", ONE_TERM, ids=[f"{f}-{t}+{b}" for f, t, b, _ in ONE_TERM])
def test_one_alignment_term_at_a_time(c, fmt, term, by, vec):
    """Each of the six 16-terms broken by 8, each planar chroma term by 8 (stays on the 16 x 2 groups) and by 4 (byte walk), each
    interleaved chroma term by 8 (byte walk): exactly one term differs from the all-aligned layout, and the counter names the walk.
    CLAHE 2 x 1 (tiles of 16 x 4) is one-pass exactly when the call is on the groups."""
    w, h, n = 32, 4, 2
    base = make_src(fmt, w, h, n, **rule_layout(fmt, None, 0)[0]), BgraOut(w, h, n, **rule_layout(fmt, None, 0)[1])
    si, di = rule_layout(fmt, term, by)
    src, dst = make_src(fmt, w, h, n, **si), BgraOut(w, h, n, **di)
    t0, t1 = rule_terms(*base), rule_terms(src, dst)
    assert all(v % 16 == 0 for v in t0.values()) and lay.side_vec(w, *base)
    moved = {k for k in t0 if t0[k] % 16 != t1[k] % 16}
    assert moved == {term} and t1[term] % 16 == by, (moved, t1)
    assert lay.side_vec(w, src, dst) == vec
    check(c, w, h, n, 32, EQ, ORDER_BGR, src, dst, (ONE, VEC if vec else BYTES))
    check(c, w, h, n, 32, ("clahe", (2.0, 2, 1)), ORDER_RGB, src, dst, (ONE, VEC) if vec else (TWO, BYTES))


def test_all_terms_aligned_is_the_control(c):
    w, h, n = 32, 4, 2
    for fmt in ("i420", "nv12"):
        si, di = rule_layout(fmt, None, 0)
        src, dst = make_src(fmt, w, h, n, **si), BgraOut(w, h, n, **di)
        check(c, w, h, n, 32, EQ, ORDER_BGR, src, dst, (ONE, VEC))
        check(c, w, h, n, 32, ("clahe", (2.0, 2, 1)), ORDER_RGB, src, dst, (ONE, VEC))


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
LOOPS = [("112x80", 112, 80, 2, "i420", {}, {}, True), ("112x80-nv12", 112, 80, 1, "nv12", {}, {}, True),
         ("16000x6", 16000, 6, 1, "yv12", {}, {}, True), ("16000x6-nv12", 16000, 6, 1, "nv12", {}, {}, True),
         ("66x34-odd", 66, 34, 2, "i420", odd_66("i420"), dict(pitch=269, frame_gap=7, off=1), False),
         ("66x34-odd-nv12", 66, 34, 2, "nv12", odd_66("nv12"), dict(pitch=269, frame_gap=7, off=1), False)]


@pytest.mark.parametrize("name,w,h,n,fmt,si,di,vec", LOOPS, ids=[s[0] for s in LOOPS])
def test_loops_past_their_first_step(c, name, w, h, n, fmt, si, di, vec):
    """LUT apply + decode where a lane owns more than one item (see the module docstring); at 112 x 80 also the decode alone, behind
    a 5 x 3 grid that pads by REFLECT_101."""
    bound = max(1, w * h * 11 // 4 // 16384)
    assert (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2), "the shape would not loop"
    src, dst = make_src(fmt, w, h, n, **si), BgraOut(w, h, n, **di)
    assert lay.side_vec(w, src, dst) == vec
    check(c, w, h, n, 33, EQ, ORDER_BGR if fmt == "nv12" else ORDER_RGB, src, dst, (ONE, VEC if vec else BYTES))
    if w == 112:
        check(c, w, h, n, 33, ("clahe", (2.0, 5, 3)), ORDER_BGR, src, dst, (TWO, VEC))


# ---- 4. CLAHE one-pass geometry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("w,h,tx,ty,clip,want", ONEPASS_SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}x{s[3]}-clip{s[4]:g}" for s in ONEPASS_SHAPES])
def test_onepass_geometry(c, w, h, tx, ty, clip, want, fmt):
    """The shapes of tests/test_gpu_nv12_to_bgr_geometry.py on both chroma layouts: straddling row pairs, tile width 48, two column
    segments at 4112 x 8, the largest pair table (60 KiB of LDS), one tile wider (the fallback), clip 0 and clip 40."""
    n = 2 if w < 1000 else 1
    src, dst = make_src(fmt, w, h, n), BgraOut(w, h, n)
    assert lay.side_vec(w, src, dst)
    check(c, w, h, n, 34, ("clahe", (clip, tx, ty)), ORDER_BGR if tx % 2 else ORDER_RGB, src, dst, (want, VEC))


# ---- 5. clahe_fp_contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_fp_contract_takes_the_fallback(c, fmt):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    c.set_option("clahe_fp_contract", 1)
    prev = oracle.set_fp_contract(True)
    try:
        check(c, w, h, n, 35, ("clahe", (2.0, 4, 2)), ORDER_BGR, make_src(fmt, w, h, n), BgraOut(w, h, n), (TWO, VEC), contract=True)
    finally:
        oracle.set_fp_contract(prev)
        c.set_option("clahe_fp_contract", 0)
    check(c, w, h, n, 35, ("clahe", (2.0, 4, 2)), ORDER_BGR, make_src(fmt, w, h, n), BgraOut(w, h, n), (ONE, VEC))


# ---- 6. identity with the three-channel form: device against device --------------------------------------------------------------
IDENTITY_OPS = [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("op", IDENTITY_OPS, ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_identity_with_the_three_channel_form(c, op, order):
    """128 x 64, three frames, pitched: for each layout the first three bytes of every pixel are what mi_*_yuv420_to_bgr_batch_dev
    writes for the same call and the fourth is 255; and an interleaved input gives the image of the planar input of the same pixels.
    No oracle takes part."""
    w, h, n = 128, 64, 3
    frames = content(w, h, n, 36)
    got = {}
    for fmt in ("i420", "nv12"):
        kw = dict(y_pitch=144, c_pitch=72, gap0=16, gap1=8, frame_gap=40, off=16) if fmt == "i420" else \
            dict(y_pitch=144, c_pitch=160, gap0=16, frame_gap=32, off=16)
        src = make_src(fmt, w, h, n, **kw).upload(frames)
        assert src.fstride % 16 == 0
        d4 = torch.full((n, h, w + 4, 4), SENT, dtype=torch.uint8, device="cuda:0")
        d3 = torch.full((n, h, w + 16, 3), SENT, dtype=torch.uint8, device="cuda:0")
        kw4 = dict(out_pitch=4 * (w + 4), out_frame=4 * (w + 4) * h, stream=stream())
        kw3 = dict(out_pitch=3 * (w + 16), out_frame=3 * (w + 16) * h, stream=stream())
        before = stats(c)
        if op is EQ:
            c.equalize_hist_yuv420_to_bgra_batch_dev(src.planes(), d4, w, h, n, order, **kw4)
            c.equalize_hist_yuv420_to_bgr_batch_dev(src.planes(), d3, w, h, n, order, **kw3)
        else:
            c.clahe_yuv420_to_bgra_batch_dev(src.planes(), d4, w, h, n, order, *op[1], **kw4)
            c.clahe_yuv420_to_bgr_batch_dev(src.planes(), d3, w, h, n, order, *op[1], **kw3)
        torch.cuda.synchronize()
        assert delta(before, stats(c)) == ((TWO if op[1] == (2.0, 3, 2) else ONE) + VEC + (0, 0)), (fmt, op)
        assert torch.equal(d4[:, :, :w, :3], d3[:, :, :w, :]), (fmt, "not the bytes of the three-channel form")
        assert bool((d4[:, :, :w, 3] == 255).all()), (fmt, "alpha")
        assert bool((d4[:, :, w:, :] == SENT).all()), (fmt, "the pitch padding was written")
        assert np.array_equal(src.host(), src.image(frames))
        got[fmt] = d4
    assert torch.equal(got["i420"], got["nv12"]), "an interleaved input is not the planar input of the same pixels"


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,op,want", [("yv12", EQ, ONE), ("nv12", ("clahe", (2.0, 1, 1)), ONE), ("i420", ("clahe", (2.0, 3, 1)), TWO)],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, fmt, op, want):
    """257 frames of 16 x 2: one full launch sequence of 256 and one of a single frame; every frame distinct, every frame checked, the
    first and the last among them (the fallback reuses its scratch planes from chunk to chunk)."""
    w, h, n = 16, 2, 257
    check(c, w, h, n, 37, op, ORDER_RGB, make_src(fmt, w, h, n), BgraOut(w, h, n), (want, VEC))


# ---- 8. host form ----------------------------------------------------------------------------------------------------------------
def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


def host_want(w, h, op):
    """The counter deltas of a host call: the staged frame is tight with every plane at a 16-byte aligned offset."""
    vec = w % 16 == 0
    if op is EQ:
        return ONE + (VEC if vec else BYTES) + (0, 0)
    return (ONE if vec and lay.onepass_shape(w, h, op[1][1], op[1][2], K) else TWO) + (VEC if vec else BYTES) + (0, 0)


def padded_plane(p, extra):
    """a plane in an array of its own, rows `extra` bytes longer than they need be, at an odd address"""
    raw = np.full(p.shape[0] * (p.shape[1] + extra) + 1, SENT, np.uint8)
    view = raw[1:].reshape(p.shape[0], p.shape[1] + extra)
    view[:, : p.shape[1]] = p
    return raw, view


@pytest.mark.parametrize("w,h", [(16, 2), (66, 34)])
def test_host_form(w, h):
    """Tight frames through the binding, pageable and registered; planes in separate arrays at odd addresses and odd pitches through
    the C entry points; out rows an odd number of bytes apart: only the 4*W bytes of each row are written, the input is not."""
    y, u, v = content(w, h, 1, 38)[0]
    ops = (EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 3, 2)))
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        for fmt in ("i420", "yv12", "nv12"):
            frame = tight_frame(fmt, y, u, v)
            raw_i, pin_in = aligned_bytes(frame.size)
            pin_in[:] = frame
            raw_o, pin_flat = aligned_bytes(w * h * 4)
            pin_out = pin_flat.reshape(h, w, 4)
            for op in ops:
                for order in ORDERS:
                    want = expected_bgra(w, h, 1, 38, op, order)[0]
                    padded = np.full((h, 4 * w + 25), SENT, np.uint8)          # pageable memory, out rows padded to an odd step
                    assert padded.strides[0] % 2 == 1
                    out = padded[:, : 4 * w].reshape(h, w, 4)
                    src = frame.copy()
                    before, fbefore = stats(c), foreign(c)
                    if op is EQ:
                        got = c.equalize_hist_yuv420_to_bgra(src, w, h, fmt, order, out=out)
                    else:
                        got = c.clahe_yuv420_to_bgra(src, w, h, fmt, order, *op[1], out=out)
                    bad = np.flatnonzero(out != want)
                    assert got is out and bad.size == 0, (fmt, op, order, bad.size, bad[:8])
                    assert (padded[:, 4 * w:] == SENT).all() and np.array_equal(src, frame)
                    assert delta(before, stats(c)) == host_want(w, h, op), (fmt, op)
                    assert foreign(c) == fbefore
            mi_lumaeq.host_register(pin_in)                                    # registered (pinned) tight memory
            mi_lumaeq.host_register(pin_flat)
            try:
                for op in ops:
                    pin_out[:] = SENT
                    if op is EQ:
                        c.equalize_hist_yuv420_to_bgra(pin_in, w, h, fmt, ORDER_BGR, out=pin_out)
                    else:
                        c.clahe_yuv420_to_bgra(pin_in, w, h, fmt, ORDER_BGR, *op[1], out=pin_out)
                    assert np.array_equal(pin_out, expected_bgra(w, h, 1, 38, op, ORDER_BGR)[0]), (fmt, op)
                    assert np.array_equal(pin_in, frame)
            finally:
                mi_lumaeq.host_unregister(pin_flat)
                mi_lumaeq.host_unregister(pin_in)
        # separate arrays, odd addresses, odd pitches; frame_stride is ignored; planar, then interleaved with c1 NULL
        ry, py = padded_plane(y, 5)
        ru, pu = padded_plane(u, 3)
        rv, pv = padded_plane(v, 3)
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = u, v
        ruv, puv = padded_plane(uv, 7)
        keep = [r.copy() for r in (ry, ru, rv, ruv)]
        assert py.ctypes.data % 2 == 1 and py.strides[0] % 2 == 1 and pu.strides[0] == w // 2 + 3 and puv.strides[0] % 2 == 1
        planar = Yuv420Planes(py.ctypes.data, py.strides[0], pu.ctypes.data, pv.ctypes.data, pu.strides[0], 12345, CHROMA_PLANAR)
        inter = Yuv420Planes(py.ctypes.data, py.strides[0], puv.ctypes.data, None, puv.strides[0], 12345, mi_lumaeq.CHROMA_INTERLEAVED)
        for a in (planar, inter):
            for op in ops:
                padded = np.full((h, 4 * w + 25), SENT, np.uint8)
                if op is EQ:
                    st = L.mi_equalize_hist_yuv420_to_bgra(hd, ctypes.byref(a), padded.ctypes.data, padded.strides[0], w, h, ORDER_RGB)
                else:
                    st = L.mi_clahe_yuv420_to_bgra(hd, ctypes.byref(a), padded.ctypes.data, padded.strides[0], w, h, ORDER_RGB, *op[1])
                assert st == 0, (op, st)
                assert np.array_equal(padded[:, : 4 * w].reshape(h, w, 4), expected_bgra(w, h, 1, 38, op, ORDER_RGB)[0]), op
                assert (padded[:, 4 * w:] == SENT).all()
                assert all(np.array_equal(r, k) for r, k in zip((ry, ru, rv, ruv), keep)), "the input was written"
        assert c.get_stat("error_drains") == 0


# ---- 9. hipGraph -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_graph_capture_and_replay(fmt):
    """One eager call of the shape, then one call captured and two replays onto changed input bytes: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    src, dst = make_src(fmt, w, h, n, **pitched_64(fmt)), BgraOut(w, h, n, pitch=272, frame_gap=64, off=32)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            src.upload(content(w, h, n, 39))
            dst.clear()
            run(c, op, src, dst, ORDER_BGR)                         # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert dst.same(expected_bgra(w, h, n, 39, op, ORDER_BGR))[0], ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, src, dst, ORDER_BGR, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                src.upload(content(w, h, n, 40 + rep))
                dst.clear()
                g.replay()
                torch.cuda.synchronize()
                assert dst.same(expected_bgra(w, h, n, 40 + rep, op, ORDER_BGR))[0], ("graph replay", op, rep)
                assert np.array_equal(src.host(), src.image(content(w, h, n, 40 + rep)))


# ---- 10. errors, zero sizes, launch accounting -----------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    frames = content(w, h, n, 42)
    src = Side(w, h, n, "i420", y_pitch=48, c_pitch=24, gap0=16, gap1=8, frame_gap=8).upload(frames)
    isrc = Side(w, h, n, "nv12", y_pitch=48, c_pitch=48).upload(frames)
    dst = BgraOut(w, h, n, pitch=144)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)

        def call(a, ctx=hd, o=dst.ptr, op=dst.pitch, fo=dst.fstride, w=w, h=h, n=n, order=ORDER_BGR, tiles=None):
            pa = None if a is None else ctypes.byref(a)
            if tiles is None:
                return L.mi_equalize_hist_yuv420_to_bgra_batch_dev(ctx, pa, o, op, fo, w, h, n, order, stream())
            return L.mi_clahe_yuv420_to_bgra_batch_dev(ctx, pa, o, op, fo, w, h, n, order, 2.0, tiles[0], tiles[1], stream())

        def both(a, **kw):
            return call(a, **kw), call(a, tiles=(2, 2), **kw)
        A, I = src.planes, isrc.planes
        s = A()
        bad = [
            (A(), dict(ctx=None)), (None, {}),                                                   # a null ctx or in
            (A(chroma=2), {}), (A(chroma=-1), {}), (A(chroma=2), dict(w=0)),                     # a chroma other than the two values
            (A(), dict(order=2)), (A(), dict(order=-1)), (I(), dict(order=2)),                   # an order other than the two
            (A(), dict(w=-2)), (A(), dict(h=-2)), (A(), dict(n=-1)),                             # negative sizes
            (A(), dict(w=31)), (A(), dict(h=15)), (A(), dict(w=31, h=0)), (A(), dict(h=15, w=0)), (A(), dict(h=15, n=0)),
            (I(), dict(w=31, n=0)),                                                              # odd sizes, also next to a 0
            (A(y=None), {}), (A(c0=None), {}), (A(), dict(o=None)), (I(y=None), {}), (I(c0=None), {}),   # null y, c0, d_out
            (A(c1=None), {}),                                                                    # a null c1 on a planar input
            (A(y_pitch=w - 1), {}), (I(y_pitch=w - 1), {}),                                      # y_pitch < W
            (A(c_pitch=w // 2 - 1), {}), (I(c_pitch=w - 1), {}),                                 # c_pitch below its row
            (A(), dict(op=4 * w - 1)), (I(), dict(op=4 * w - 1)), (A(), dict(op=3 * w)),         # out_pitch < 4*W
            (A(), dict(o=s.y)), (A(), dict(o=s.c0)), (A(), dict(o=s.c1)), (I(), dict(o=I().y)), (I(), dict(o=I().c0)),   # no in-place form
        ]
        for a, kw in bad:
            assert both(a, **kw) == (BAD_ARG, BAD_ARG), (kw, None if a is None else bytes(a))
        for tiles in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert call(A(), tiles=tiles) == BAD_ARG, tiles
            assert call(A(), tiles=tiles, n=0) == BAD_ARG, tiles
        for kw in (dict(w=0), dict(h=0), dict(n=0)):                                             # zero sizes: MI_OK, nothing written
            assert both(A(), **kw) == (0, 0), kw
            assert both(I(), **kw) == (0, 0), kw
        # sizes and tile grids the planar forms refuse: their status
        bw = (1 << 24) + 2
        planar = L.mi_clahe_u8_batch_dev(hd, s.y, 1 << 25, 1 << 26, dst.ptr, 1 << 25, 1 << 26, bw, 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and both(A(y_pitch=1 << 25, c_pitch=1 << 25), w=bw, h=2, op=1 << 27) == (planar, planar)
        planar = L.mi_clahe_u8_batch_dev(hd, s.y, s.y_pitch, s.frame_stride, dst.ptr, dst.pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and call(A(), tiles=(2048, 1024)) == planar
        # an interleaved input ignores c1: junk there is no error
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0,) * 6 and foreign(c) == (0,) * 8
        # launch accounting of the three sequences, by role; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (ONE, VEC)),
                             (("clahe", (2.0, 2, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (ONE, VEC)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (TWO, VEC))):
            for side in (src, isrc):
                c.profile_read(reset=True)
                check(c, w, h, n, 42, op, ORDER_RGB, side, dst, st)
                got = launches(c)
                assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        p = isrc.planes(c1=0xDEAD0)
        dst.clear()
        run(c, EQ, isrc, dst, ORDER_BGR, planes=p)
        torch.cuda.synchronize()
        assert dst.same(expected_bgra(w, h, n, 42, EQ, ORDER_BGR))[0], "c1 is ignored on an interleaved input"
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_host_form_errors():
    w, h = 32, 16
    src = Side(w, h, 1, "i420", dev=False).upload(content(w, h, 1, 43))
    isrc = Side(w, h, 1, "nv12", dev=False).upload(content(w, h, 1, 43))
    out = np.full((h, w, 4), SENT, np.uint8)
    o = out.ctypes.data
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        A, I = src.planes, isrc.planes
        for ctx, a, po, step, ww, hh, order in (
                (None, A(), o, 4 * w, w, h, 0), (hd, None, o, 4 * w, w, h, 0), (hd, A(chroma=3), o, 4 * w, w, h, 0),
                (hd, A(), o, 4 * w, w, h, 2), (hd, A(), o, 4 * w, -2, h, 0), (hd, A(), o, 4 * w, w - 1, h, 0),
                (hd, A(), o, 4 * w, w, h - 1, 0), (hd, A(), o, 4 * w, w - 1, 0, 0), (hd, A(y=None), o, 4 * w, w, h, 0),
                (hd, A(c0=None), o, 4 * w, w, h, 0), (hd, A(c1=None), o, 4 * w, w, h, 0), (hd, A(), None, 4 * w, w, h, 0),
                (hd, A(y_pitch=w - 1), o, 4 * w, w, h, 0), (hd, A(c_pitch=w // 2 - 1), o, 4 * w, w, h, 0),
                (hd, I(c_pitch=w - 1), o, 4 * w, w, h, 0), (hd, A(), o, 4 * w - 1, w, h, 0), (hd, I(), o, 3 * w, w, h, 0),
                (hd, A(), A().y, 4 * w, w, h, 0), (hd, A(), A().c0, 4 * w, w, h, 0), (hd, A(), A().c1, 4 * w, w, h, 0)):
            pa = None if a is None else ctypes.byref(a)
            assert L.mi_equalize_hist_yuv420_to_bgra(ctx, pa, po, step, ww, hh, order) == BAD_ARG
            assert L.mi_clahe_yuv420_to_bgra(ctx, pa, po, step, ww, hh, order, 2.0, 2, 2) == BAD_ARG
        a = A()
        assert L.mi_clahe_yuv420_to_bgra(hd, ctypes.byref(a), o, 4 * w, w, h, 0, 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_yuv420_to_bgra(hd, ctypes.byref(a), o, 4 * w, w, h, 0, 2.0, 2048, 1024) == UNSUPPORTED
        # W*H > 0x7fffffff / 4: refused before anything is staged (the pitches make the rows legal, nothing is read)
        bw, bh = 1 << 15, (1 << 14) + 2
        assert bw * bh > 0x7fffffff // 4 and bw * bh <= 0x7fffffff
        big = A(y_pitch=bw, c_pitch=bw // 2)
        assert L.mi_equalize_hist_yuv420_to_bgra(hd, ctypes.byref(big), o, 4 * bw, bw, bh, 0) == UNSUPPORTED
        assert L.mi_clahe_yuv420_to_bgra(hd, ctypes.byref(big), o, 4 * bw, bw, bh, 0, 2.0, 2, 2) == UNSUPPORTED
        assert L.mi_equalize_hist_yuv420_to_bgra(hd, ctypes.byref(a), o, 4 * w, 0, h, 0) == 0
        assert L.mi_clahe_yuv420_to_bgra(hd, ctypes.byref(a), o, 4 * w, w, 0, 0, 2.0, 2, 2) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0 and stats(c) == (0,) * 6
        assert src.same(content(w, h, 1, 43))[0]


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Side(w, h, 1, "i420").upload(content(w, h, 1, 44))
    dst = BgraOut(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            with pytest.raises(mi_lumaeq.MiError) as e:
                c.equalize_hist_yuv420_to_bgra(tight_frame("i420", *content(w, h, 1, 44)[0]), w, h, "i420")
            assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"
        assert stats(c) == (0,) * 6
