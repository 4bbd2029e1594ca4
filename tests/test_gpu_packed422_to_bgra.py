"""Packed 4:2:2 frames in (YUY2 / UYVY), four-channel BGRA / RGBA images (CV_8UC4, A = 255) out on the GPU: the batch forms
mi_equalize_hist_packed422_to_bgra_batch_dev / mi_clahe_packed422_to_bgra_batch_dev and the host forms mi_equalize_hist_packed422_to_bgra
/ mi_clahe_packed422_to_bgra.  The expected image is tests/packed422_bgra_ref.py: the three-channel reference (the oracle's luma in the
call's arithmetic mode, every row decoded with its OWN chroma) with a fourth channel of 255.  Inputs and outputs live in sentinel-filled
allocations with guard bytes and the WHOLE allocation is compared: every comparison in this file is exact bytes.  After every call the
four counters of the form must have moved by exactly the store path of the call, and the neighbouring forms' counters not at all."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import packed422_bgra_ref as ref
from packed422_bgra_ref import (Batch, BgraOut, SENT, EQ, CL22, CL54, CL642, COUNTERS, FOREIGN, FMT_YUY2, FMT_UYVY, ORDER_BGR,
                                ORDER_RGB)

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
FMTS = [FMT_YUY2, FMT_UYVY]
ORDERS = [ORDER_BGR, ORDER_RGB]
# input: (pitch - 2W, gap between frames, base offset from a 16-byte boundary)
LAYOUTS = [(4, 20, 4), (36, 0, 8), (0, 12, 12)]
WIDE, BYTES = (1, 0, 0, 0), (0, 1, 0, 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


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


def counters(c):
    return [c.get_stat(s) for s in COUNTERS + FOREIGN]


def moved(c, before):
    now = counters(c)
    return tuple(a - b for a, b in zip(now, before))


def run(c, op, src, dst, fmt, order, n=None, st=None):
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if op[0] == "eq":
        c.equalize_hist_packed422_to_bgra_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, fmt, order, **kw)
    else:
        c.clahe_packed422_to_bgra_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, fmt, order, *op[1], **kw)


def run_bgr(c, op, src, d_out, fmt, order):
    """The existing three-channel form on the same input, into a tight tensor."""
    kw = dict(src.kw(), stream=stream())
    if op[0] == "eq":
        c.equalize_hist_packed422_to_bgr_batch_dev(src.ptr, d_out, src.w, src.h, src.n, fmt, order, **kw)
    else:
        c.clahe_packed422_to_bgr_batch_dev(src.ptr, d_out, src.w, src.h, src.n, fmt, order, *op[1], **kw)


_planar_cache = {}


def planar_status(c, w, h, n, op):
    """What the planar form answers for this size / grid pair (0 = accepted)."""
    k = (w, h, n, op)
    if k not in _planar_cache:
        a = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        status = 0
        try:
            if op[0] == "eq":
                c.equalize_hist_batch_dev(a, b, w, h, n, stream=stream())
            else:
                c.clahe_batch_dev(a, b, w, h, n, *op[1], stream=stream())
        except mi_lumaeq.MiError as e:
            status = e.status
        finally:
            torch.cuda.synchronize()
        _planar_cache[k] = status
    return _planar_cache[k]


_frames, _luma = {}, {}


def frames_of(w, h, fmt, seed=100, n=2):
    """Frame 0: independent random Y, U, V; frame 1: strong chroma on even rows, 128 on odd rows (a shared chroma row cannot pass);
    further frames random."""
    k = (w, h, fmt, seed, n)
    if k not in _frames:
        fs = [ref.random_frame(w, h, fmt, seed + i) for i in range(n)]
        if n > 1:
            fs[1] = ref.alternating_chroma_frame(w, h, fmt, seed + 1)
        _frames[k] = fs
    return _frames[k]


def expected(key, frames, w, fmt, order, op, contract=False):
    """The reference images; the oracle's luma is computed once per (content, op, arithmetic mode) and shared, unchanged."""
    out = []
    for k, f in enumerate(frames):
        lk = (key, w, f.shape[0], fmt, k, op, bool(contract))
        if lk not in _luma:
            _luma[lk] = ref.mapped_luma(ref.luma(f, w, fmt), op[0], op[1], contract)
        out.append(ref.expected(f, w, fmt, order, op[0], op[1], contract, _luma[lk]))
    return out


def check_case(c, frames, w, h, fmt, order, op, li, dst, key, contract=False):
    n = len(frames)
    src = Batch(w, h, n, LAYOUTS[li % 3]).upload(frames)
    why = (w, h, fmt, order, op, li, dst.pitch, dst.fstride, dst.off, contract)
    before = counters(c)
    status = planar_status(c, w, h, n, op)
    if status != 0:                                   # a size / grid pair the planar form refuses: the same status, nothing written
        with pytest.raises(mi_lumaeq.MiError) as e:
            run(c, op, src, dst, fmt, order)
        torch.cuda.synchronize()
        assert e.value.status == status, (why, e.value.status, status)
        assert dst.same(), "a refused call wrote"
        assert not any(moved(c, before)), "a refused call was counted"
        return
    run(c, op, src, dst, fmt, order)
    torch.cuda.synchronize()
    d = moved(c, before)
    assert d[:4] == (WIDE if dst.wide else BYTES), (why, d)
    assert not any(d[4:]), (why, "a neighbouring form's counter moved", d)
    want = dst.image(expected(key, frames, w, fmt, order, op, contract))
    got = dst.host()
    assert np.array_equal(got, want), (why, int((got != want).sum()), np.flatnonzero(got != want)[:8])
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"


# ---- 1. parity matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ref.PARITY_OPS, ids=["eq", "clahe2x2", "clahe5x4-pads", "clahe64x2-global"])
@pytest.mark.parametrize("w,h", ref.PARITY_SHAPES, ids=["%dx%d" % s for s in ref.PARITY_SHAPES])
def test_parity_matrix(c, w, h, op):
    """Both formats x both orders x the four image layouts (16-byte stores at 16- and at 4-byte alignment, byte stores at an odd base
    with pitch 4W + 1, a tight image), two frames a call; the LDS rungs with clahe_float_tables and clahe_fp_contract both ways.  A
    size / grid pair the planar form refuses is refused with its status and writes nothing."""
    options = ref.OPTIONS if op in ref.LDS_OPS else ref.OPTIONS[:1]
    try:
        i = 0
        for fmt in FMTS:
            frames = frames_of(w, h, fmt)
            for float_tables, contract in options:
                c.set_option("clahe_float_tables", float_tables)
                c.set_option("clahe_fp_contract", contract)
                for order in ORDERS:
                    for lo in ref.OUT_LAYOUTS:
                        dst = BgraOut(w, h, 2, lo)
                        assert dst.wide == (lo != "odd")
                        check_case(c, frames, w, h, fmt, order, op, i, dst, "parity", contract)
                        i += 1
    finally:
        c.set_option("clahe_float_tables", 1)
        c.set_option("clahe_fp_contract", 0)


# ---- 2. the store-path rule, one term at a time --------------------------------------------------------------------------------------
RULE_TERMS = [(t, by) for t in ("address", "out_pitch", "out_frame_stride") for by in (4, 1)]


def test_all_terms_aligned_is_the_control(c):
    w, h = 32, 4
    dst = BgraOut(w, h, 2, pitch=4 * w + 16, fstride=(4 * w + 16) * h + 16, off=0)
    assert dst.ptr % 16 == 0 and dst.pitch % 16 == 0 and dst.fstride % 16 == 0 and dst.wide
    for op in (EQ, CL22, CL642):
        check_case(c, frames_of(w, h, FMT_YUY2, 200), w, h, FMT_YUY2, ORDER_BGR, op, 0, dst, "rule")
        dst.clear()


@pytest.mark.parametrize("term,by", RULE_TERMS, ids=["%s+%d" % t for t in RULE_TERMS])
def test_one_rule_term_at_a_time(c, term, by):
    """32 x 4, two frames, image address, out_pitch and out_frame_stride all multiples of 16; exactly one of them moves, by 4 (still
    wide) or by 1 (bytes).  The counter names the path; the bytes are exact both ways, for the LUT-apply kernel, the LDS interpolation
    and the global-memory interpolation."""
    w, h = 32, 4
    pitch, off = 4 * w + 16, 0
    fstride = pitch * h + 16
    if term == "address":
        off += by
    elif term == "out_pitch":
        pitch += by
    else:
        fstride += by
    for fi, fmt in enumerate(FMTS):
        frames = frames_of(w, h, fmt, 200)
        for oi, op in enumerate((EQ, CL22, CL642)):
            dst = BgraOut(w, h, 2, pitch=pitch, fstride=fstride, off=off)
            assert dst.wide == (by == 4)
            check_case(c, frames, w, h, fmt, ORDERS[(fi + oi) % 2], op, fi + oi, dst, "rule")


# ---- 3. walks past their first step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,n,op", ref.LOOP_SHAPES, ids=[s[0] for s in ref.LOOP_SHAPES])
def test_walks_past_their_first_step(c, name, w, h, n, op):
    """The shapes of packed422_bgra_ref.LOOP_SHAPES (tests/test_packed422_to_bgra_shapes.py shows on the CPU that they loop): tight on
    both sides, then with the source pitch at 2W + 4 and the image pitch at 4W + 4, then on the byte path."""
    for fi, fmt in enumerate(FMTS):
        frames = frames_of(w, h, fmt, 300, n)
        order = ORDERS[fi]
        for dst in (BgraOut(w, h, n, "tight"), BgraOut(w, h, n, pitch=4 * w + 4, fstride=(4 * w + 4) * h, off=0),
                    BgraOut(w, h, n, "odd")):
            src_layout = (0, 0, 0) if dst.pitch == 4 * w else (4, 0, 0)
            src = Batch(w, h, n, src_layout).upload(frames)
            before = counters(c)
            run(c, op, src, dst, fmt, order)
            torch.cuda.synchronize()
            d = moved(c, before)
            assert d[:4] == (WIDE if dst.wide else BYTES) and not any(d[4:]), (name, fmt, d)
            want, got = dst.image(expected(("loop", name), frames, w, fmt, order, op)), dst.host()
            assert np.array_equal(got, want), (name, fmt, dst.pitch, int((got != want).sum()), np.flatnonzero(got != want)[:8])
            assert np.array_equal(src.host(), src.image(frames))


# ---- 4. the first three bytes are the three-channel form's -----------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, CL22, CL54, CL642], ids=["eq", "clahe2x2", "clahe5x4-pads", "clahe64x2-global"])
def test_identity_with_the_three_channel_form(c, op):
    """66 x 34, two frames, pitched input: out[..., :3] is what mi_*_packed422_to_bgr_batch_dev writes for the same call on the GPU, and
    out[..., 3] == 255.  No oracle takes part."""
    w, h, n = 66, 34, 2
    for fmt in FMTS:
        frames = frames_of(w, h, fmt)
        src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
        for order in ORDERS:
            three = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0")
            four = torch.full((n, h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
            run_bgr(c, op, src, three, fmt, order)
            kw = dict(src.kw(), stream=stream())
            if op[0] == "eq":
                c.equalize_hist_packed422_to_bgra_batch_dev(src.ptr, four, w, h, n, fmt, order, **kw)
            else:
                c.clahe_packed422_to_bgra_batch_dev(src.ptr, four, w, h, n, fmt, order, *op[1], **kw)
            torch.cuda.synchronize()
            a, b = four.cpu().numpy(), three.cpu().numpy()
            assert np.array_equal(a[..., :3], b), (op, fmt, order)
            assert (a[..., 3] == 255).all(), (op, fmt, order)
            assert not (b == SENT).all()


# ---- 5. the host form ----------------------------------------------------------------------------------------------------------------
def rows_in(buf, off, rows, pitch):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, pitch), strides=(pitch, 1), writeable=True)


def image_in(buf, off, rows, w, step):
    """An H x W x 4 view with rows `step` bytes apart."""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, w, 4), strides=(step, 4, 1), writeable=True)


def call_host(c, op, frame, w, fmt, order, out=None):
    if op[0] == "eq":
        return c.equalize_hist_packed422_to_bgra(frame, w, fmt, order, out=out)
    return c.clahe_packed422_to_bgra(frame, w, fmt, order, *op[1], out=out)


@pytest.mark.parametrize("w,h", [(18, 3), (66, 34)])
def test_host_form_pageable(c, w, h):
    """Pageable memory: a tight frame to a new tight image, then a pitched input and an image at an ODD address with out_step = 4W + 3
    inside sentinel borders that must survive.  The device image is tight and aligned: the call counts as wide."""
    for fmt in FMTS:
        frame = frames_of(w, h, fmt, 400)[1]
        f0 = frame.copy()
        ipitch, ostep = 2 * w + 12, 4 * w + 3
        inbuf = np.full(16 + ipitch * h + 32, SENT, np.uint8)
        ioff = 4 - inbuf.ctypes.data % 4 + 4
        pitched = rows_in(inbuf, ioff, h, ipitch)
        pitched[:, :2 * w] = frame
        in0 = inbuf.copy()
        for op in (EQ, CL22, CL54, CL642):
            for order in ORDERS:
                want = expected(("host", 1), [frame], w, fmt, order, op)[0]
                before = counters(c)
                got = call_host(c, op, frame, w, fmt, order)
                assert moved(c, before) == WIDE + (0,) * 8
                assert got.shape == (h, w, 4) and got.flags.c_contiguous
                assert np.array_equal(got, want), ("tight", w, h, fmt, order, op)
                assert np.array_equal(frame, f0)
                obuf = np.full(16 + ostep * h + 32, SENT, np.uint8)
                ooff = 9 if obuf.ctypes.data % 2 == 0 else 8        # an odd address
                ov = image_in(obuf, ooff, h, w, ostep)
                assert ov.ctypes.data % 2 == 1
                call_host(c, op, pitched, w, fmt, order, out=ov)
                wo = np.full_like(obuf, SENT)
                image_in(wo, ooff, h, w, ostep)[:] = want
                assert np.array_equal(obuf, wo), ("pitched", w, h, fmt, order, op)
                assert np.array_equal(inbuf, in0), "the input was written"


def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


def test_host_form_pinned_tight_pair(c):
    """A tight frame and a tight image, both registered with mi_host_register (DMA'd as they are)."""
    w, h, fmt, order = 66, 34, FMT_UYVY, ORDER_RGB
    frame = frames_of(w, h, fmt, 400)[0]
    raw_i, ib = aligned_bytes(2 * w * h)
    raw_o, ob = aligned_bytes(4 * w * h + 64)
    for a in (ib, ob):
        mi_lumaeq.host_register(a)
    try:
        fin = ib.reshape(h, 2 * w)
        fin[:] = frame
        for op in (EQ, CL22):
            ob[:] = SENT
            tight = ob[: 4 * w * h].reshape(h, w, 4)
            call_host(c, op, fin, w, fmt, order, out=tight)
            assert np.array_equal(tight, expected(("host", 0), [frame], w, fmt, order, op)[0]), op
            assert (ob[4 * w * h:] == SENT).all()
            assert np.array_equal(fin, frame)
    finally:
        for a in (ib, ob):
            mi_lumaeq.host_unregister(a)


def test_host_form_errors_write_nothing(c):
    w, h = 64, 47
    frame = frames_of(w, h, FMT_YUY2, 500)[0]
    f0 = frame.copy()
    big = np.full(16 + 4 * w * h * 2, SENT, np.uint8)
    big = big[(-big.ctypes.data) % 4:]
    big[: 2 * w * h] = frame.ravel()
    b0 = big.copy()
    out = np.full((h, w, 4), SENT, np.uint8)
    L, hd = c._L, c._h
    base = dict(i=frame.ctypes.data, ipitch=2 * w, o=out.ctypes.data, ostep=4 * w, w=w, h=h, fmt=FMT_YUY2, order=ORDER_BGR)

    def args(kw):
        a = dict(base)
        a.update(kw)
        return (hd, a["i"], a["ipitch"], a["o"], a["ostep"], a["w"], a["h"], a["fmt"], a["order"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_bgra(*args(kw))

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_bgra(*args(kw), 2.0, tx, ty)
    bp = big.ctypes.data
    before = counters(c)
    bad = [dict(i=None), dict(o=None),
           dict(w=63), dict(w=63, h=0), dict(w=-2), dict(h=-2), dict(h=-1),
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(order=2), dict(order=-1),
           dict(ipitch=2 * w - 4), dict(ostep=4 * w - 1), dict(ostep=3 * w),
           dict(i=bp + 2), dict(i=bp, ipitch=2 * w + 2),                                 # the input side: multiples of 4
           dict(i=bp, o=bp), dict(i=bp, o=bp + 1), dict(i=bp, o=bp + 2 * w * h - 1)]     # the rows of the image meet the input's
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8)):
        assert cl(tx, ty) == BAD_ARG
    # W * H beyond 0x7fffffff / 4 (and within what the packed input allows)
    assert eq(w=32768, h=16384, ipitch=2 * 32768, ostep=4 * 32768) == UNSUPPORTED
    assert cl(w=32768, h=16384, ipitch=2 * 32768, ostep=4 * 32768) == UNSUPPORTED
    assert cl(512, 256) == UNSUPPORTED                                                  # 131072 tiles
    for kw in (dict(w=0), dict(h=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    assert (out == SENT).all() and np.array_equal(frame, f0) and np.array_equal(big, b0)
    assert not any(moved(c, before)), "a refused or empty call was counted"
    # an image directly behind the input does not meet it; the context still works, and a refused call left no copy in flight
    behind = image_in(big, 2 * w * h, h, w, 4 * w)
    got = c.equalize_hist_packed422_to_bgra(rows_in(big, 0, h, 2 * w), w, FMT_YUY2, ORDER_BGR, out=behind)
    assert np.array_equal(got, expected(("host", "err"), [frame], w, FMT_YUY2, ORDER_BGR, EQ)[0])
    assert np.array_equal(big[: 2 * w * h], b0[: 2 * w * h]) and (big[2 * w * h + 4 * w * h:] == SENT).all()


# ---- 6. streams, hipGraph, the pipe ------------------------------------------------------------------------------------------------
def test_streams(c):
    w, h, n = 40, 6, 2
    frames = frames_of(w, h, FMT_UYVY, 600)
    src = Batch(w, h, n, LAYOUTS[1]).upload(frames)
    dst = BgraOut(w, h, n, "aligned4")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for st in (side.cuda_stream, mi_lumaeq.STREAM_CTX):
        for op in (EQ, CL22):
            dst.clear()
            torch.cuda.synchronize()
            run(c, op, src, dst, FMT_UYVY, ORDER_RGB, st=st)
            if st == side.cuda_stream:
                side.synchronize()
            else:
                c.synchronize(mi_lumaeq.STREAM_CTX)
            assert dst.same(expected("streams", frames, w, FMT_UYVY, ORDER_RGB, op)), (st, op)


def test_graph_capture_and_replay():
    """One eager call of the shape, then one call captured and two replays onto changed input bytes: the bytes of an eager call."""
    w, h, n = 66, 34, 2
    src, dst = Batch(w, h, n, LAYOUTS[0]), BgraOut(w, h, n, "aligned4")
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, CL22, CL642):
            frames = frames_of(w, h, FMT_YUY2, 700)
            src.upload(frames)
            dst.clear()
            run(c, op, src, dst, FMT_YUY2, ORDER_BGR)                   # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert dst.same(expected(("graph", 700), frames, w, FMT_YUY2, ORDER_BGR, op)), ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, src, dst, FMT_YUY2, ORDER_BGR, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                frames = frames_of(w, h, FMT_YUY2, 710 + 10 * rep)
                src.upload(frames)
                dst.clear()
                g.replay()
                torch.cuda.synchronize()
                assert dst.same(expected(("graph", 710 + 10 * rep), frames, w, FMT_YUY2, ORDER_BGR, op)), ("graph replay", op, rep)
                assert np.array_equal(src.host(), src.image(frames))


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Batch(w, h, 1).upload(frames_of(w, h, FMT_YUY2, 800)[:1])
    dst = BgraOut(w, h, 1, "tight")
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 8, 8))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, FMT_YUY2, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same(), "a refused call wrote"
        assert not any(counters(c))


# ---- 7. errors, zero sizes, launch accounting ----------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    w, h, n = 64, 47, 2
    frames = frames_of(w, h, FMT_YUY2, 900)
    src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
    dst = BgraOut(w, h, n, "aligned4")
    L, hd = c._L, c._h
    ip, op_ = src.ptr, dst.ptr
    base = dict(i=ip, ipitch=src.pitch, ifs=src.fstride, o=op_, opitch=dst.pitch, ofs=dst.fstride, w=w, h=h, n=n, fmt=FMT_YUY2,
                order=ORDER_BGR)

    def args(kw):
        a = dict(base)
        a.update(kw)
        return (hd, a["i"], a["ipitch"], a["ifs"], a["o"], a["opitch"], a["ofs"], a["w"], a["h"], a["n"], a["fmt"], a["order"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_bgra_batch_dev(*args(kw), stream())

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_bgra_batch_dev(*args(kw), 2.0, tx, ty, stream())
    before = counters(c)
    bad = [dict(i=None), dict(o=None),                                                            # null frame pointers
           dict(w=63), dict(w=63, h=0), dict(w=63, n=0), dict(w=1),                               # odd width, also next to a zero size
           dict(w=-2), dict(h=-2), dict(h=-1), dict(n=-1),                                        # negative sizes
           dict(ipitch=2 * w - 4), dict(opitch=4 * w - 1), dict(opitch=4 * w - 4), dict(opitch=3 * w),   # pitches too small
           dict(i=ip + 2), dict(i=ip + 1), dict(ipitch=2 * w + 2), dict(ifs=src.fstride + 2), dict(ifs=src.fstride + 1),   # input not multiples of 4
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(order=2), dict(order=-1),     # format, order
           dict(o=ip)]                                                                            # no in-place form
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert cl(tx, ty) == BAD_ARG
    # the grids and heights the batch form refuses: more than 65535 tiles; a height above 65535 with tiles_x > 62 (checked before any
    # pointer is followed: the shape alone decides)
    assert cl(512, 256) == UNSUPPORTED
    assert cl(64, 1, w=64, h=65536, n=1, ipitch=128, ifs=128 * 65536, opitch=256, ofs=256 * 65536) == UNSUPPORTED
    # zero sizes: MI_OK, nothing written
    for kw in (dict(w=0), dict(h=0), dict(n=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    torch.cuda.synchronize()
    assert dst.same(), "a refused or empty call wrote"
    assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
    assert not any(moved(c, before)), "a refused or empty call was counted"
    # and the context still works
    run(c, ("clahe", (2.0, 8, 8)), src, dst, FMT_YUY2, ORDER_RGB)
    torch.cuda.synchronize()
    assert dst.same(expected("errors", frames, w, FMT_YUY2, ORDER_RGB, ("clahe", (2.0, 8, 8))))


def test_launch_accounting():
    """The slots of the three-channel form, by role: never the fused kernel, never hist_lut_kernel, no MI_K_COLOR launch."""
    w, h, n = 64, 48, 2
    frames = frames_of(w, h, FMT_YUY2, 1000)
    src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
    dst = BgraOut(w, h, n, "aligned4")
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        c.profile_read(reset=True)
        run(c, EQ, src, dst, FMT_YUY2, ORDER_BGR)
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
        assert len(prof) == 10
        for k in mi_lumaeq.KERNEL_NAMES:
            want = 1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0
            assert prof[k]["launches"] == want, (k, prof[k])
        assert dst.same(expected("prof", frames, w, FMT_YUY2, ORDER_BGR, EQ))
        for op in (("clahe", (2.0, 8, 8)), CL642):
            c.profile_read(reset=True)
            run(c, op, src, dst, FMT_YUY2, ORDER_BGR)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            for k in ("equalize_fused_kernel", "fused_finish_kernel", "color_kernel", "analyze_diff_kernel", "hist_partial_kernel",
                      "equalize_lut_kernel", "lut_apply_kernel"):
                assert prof[k]["launches"] == 0, (op, k, prof[k])
            assert prof["tile_hist_kernel"]["launches"] == 1 and prof["clahe_interp_kernel"]["launches"] == 1, (op, prof)
            assert prof["tile_lut_kernel"]["launches"] in (0, 1)
            assert dst.same(expected("prof", frames, w, FMT_YUY2, ORDER_BGR, op))
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
