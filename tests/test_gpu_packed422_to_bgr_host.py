"""Packed 4:2:2 host frames in (YUY2 / UYVY), BGR / RGB host images out: mi_equalize_hist_packed422_to_bgr and
mi_clahe_packed422_to_bgr against tests/packed422_bgr_ref.py (every row decoded with its own chroma), exact bytes.  Pageable memory and
memory registered with mi_host_register, a pitched input and an output at an odd address with out_step = 3W + 5 inside sentinel borders
that must survive, odd heights and W % 4 == 2; refused and empty calls write nothing."""
import numpy as np
import pytest

import mi_lumaeq
import packed422_bgr_ref as ref
from mi_lumaeq import synth, FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
SIZES = [(64, 48), (62, 47), (18, 1), (320, 91)]
OPS = [("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (3.0, 4, 3)), ("clahe", (2.0, 64, 2))]        # the last: the wide-grid kernel
FMTS = [FMT_YUY2, FMT_UYVY]
ORDERS = [ORDER_BGR, ORDER_RGB]

_luma = {}


def expected(frame, w, fmt, order, op, cfg, key):
    k = (key, fmt, op, cfg)
    if k not in _luma:
        _luma[k] = ref.mapped_luma(ref.luma(frame, w, fmt), op, cfg)
    return ref.expected(frame, w, fmt, order, op, cfg, y_mapped=_luma[k])


def rows_in(buf, off, rows, pitch):
    """A rows x pitch view of the byte buffer `buf` from byte `off`, row-strided over exactly the bytes it needs."""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, pitch), strides=(pitch, 1), writeable=True)


def image_in(buf, off, rows, w, step):
    """An H x W x 3 view with rows `step` bytes apart."""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, w, 3), strides=(step, 3, 1), writeable=True)


def call(c, op, cfg, frame, w, fmt, order, out=None):
    if op == "eq":
        return c.equalize_hist_packed422_to_bgr(frame, w, fmt, order, out=out)
    return c.clahe_packed422_to_bgr(frame, w, fmt, order, *cfg, out=out)


def planar_ok(c, w, h, op, cfg):
    if op == "eq":
        return True
    try:
        c.clahe(np.zeros((h, w), np.uint8), *cfg)
        return True
    except mi_lumaeq.MiError:
        return False


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.mark.parametrize("w,h", SIZES)
def test_pageable_tight_and_pitched(c, w, h):
    """Pageable memory.  A tight frame to a new tight image (62 x 47: W % 4 == 2 and an odd height; 18 x 1: one row), then a pitched
    input and an image at an ODD address with out_step = 3W + 5, both inside sentinel borders."""
    for fmt in FMTS:
        frame = synth.packed422_frame(w, h, fmt, "D2", 40 + fmt)
        f0 = frame.copy()
        ipitch, ostep = 2 * w + 12, 3 * w + 5
        inbuf = np.full(16 + ipitch * h + 32, SENT, np.uint8)
        ioff = 4 - inbuf.ctypes.data % 4 + 4                        # the input side keeps the packed forms' rule: a multiple of 4
        pitched = rows_in(inbuf, ioff, h, ipitch)
        pitched[:, :2 * w] = frame
        in0 = inbuf.copy()
        for oi, (op, cfg) in enumerate(OPS):
            if not planar_ok(c, w, h, op, cfg):
                continue
            for order in ORDERS:
                want = expected(frame, w, fmt, order, op, cfg, ("host", w, h))
                got = call(c, op, cfg, frame, w, fmt, order)
                assert got.shape == (h, w, 3) and got.flags.c_contiguous
                assert np.array_equal(got, want), ("tight", w, h, fmt, order, op, cfg)
                assert np.array_equal(frame, f0)
                obuf = np.full(16 + ostep * h + 32, SENT, np.uint8)
                ooff = 9 if obuf.ctypes.data % 2 == 0 else 8        # an odd address
                ov = image_in(obuf, ooff, h, w, ostep)
                assert ov.ctypes.data % 2 == 1
                call(c, op, cfg, pitched, w, fmt, order, out=ov)
                wo = np.full_like(obuf, SENT)
                image_in(wo, ooff, h, w, ostep)[:] = want
                assert np.array_equal(obuf, wo), ("pitched", w, h, fmt, order, op, cfg)
                assert np.array_equal(inbuf, in0), "the input was written"


def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


@pytest.mark.parametrize("w,h", [(64, 48), (62, 47)])
def test_registered_memory(c, w, h):
    """Tight buffers registered with mi_host_register (DMA'd as they are), then a pitched registered image (staged): the same bytes
    either way, nothing written behind the image or into its row padding."""
    fmt, order = FMT_UYVY, ORDER_RGB
    frame = synth.packed422_frame(w, h, fmt, "D3", 77)
    raw_i, ib = aligned_bytes(2 * w * h)
    raw_o, ob = aligned_bytes((3 * w + 8) * h)
    for a in (ib, ob):                                               # page-aligned, each one registration
        mi_lumaeq.host_register(a)
    try:
        fin = ib.reshape(h, 2 * w)
        fin[:] = frame
        for op, cfg in OPS[:2]:
            want = expected(frame, w, fmt, order, op, cfg, ("reg", w, h))
            ob[:] = SENT
            tight = ob[: 3 * w * h].reshape(h, w, 3)
            call(c, op, cfg, fin, w, fmt, order, out=tight)
            assert np.array_equal(tight, want), ("tight registered", w, h, op, cfg)
            assert (ob[3 * w * h:] == SENT).all()
            ob[:] = SENT
            pitched = ob.reshape(h, 3 * w + 8)
            call(c, op, cfg, fin, w, fmt, order, out=image_in(ob, 0, h, w, 3 * w + 8))
            assert np.array_equal(pitched[:, :3 * w].reshape(h, w, 3), want), ("pitched registered", w, h, op, cfg)
            assert (pitched[:, 3 * w:] == SENT).all()
            assert np.array_equal(fin, frame)
    finally:
        for a in (ib, ob):
            mi_lumaeq.host_unregister(a)


def test_errors_write_nothing(c):
    w, h = 64, 47
    frame = synth.packed422_frame(w, h, FMT_YUY2, "D1", 5)
    f0 = frame.copy()
    big = np.full(16 + 3 * w * h * 2, SENT, np.uint8)
    big = big[(-big.ctypes.data) % 4:]
    big[: 2 * w * h] = frame.ravel()
    b0 = big.copy()
    out = np.full((h, w, 3), SENT, np.uint8)
    L, hd = c._L, c._h
    ip, op_ = frame.ctypes.data, out.ctypes.data
    base = dict(i=ip, ipitch=2 * w, o=op_, ostep=3 * w, w=w, h=h, fmt=FMT_YUY2, order=ORDER_BGR)

    def args(kw):
        a = dict(base)
        a.update(kw)
        return (hd, a["i"], a["ipitch"], a["o"], a["ostep"], a["w"], a["h"], a["fmt"], a["order"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_bgr(*args(kw))

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_bgr(*args(kw), 2.0, tx, ty)
    bp = big.ctypes.data
    bad = [dict(i=None), dict(o=None),
           dict(w=63), dict(w=63, h=0), dict(w=-2), dict(h=-2), dict(h=-1),
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(order=2), dict(order=-1),
           dict(ipitch=2 * w - 4), dict(ostep=3 * w - 1),
           dict(i=bp + 2), dict(i=bp, ipitch=2 * w + 2),                                 # the input side: multiples of 4
           dict(i=bp, o=bp), dict(i=bp, o=bp + 1), dict(i=bp, o=bp + 2 * w * h - 1)]     # the image meets the input
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8)):
        assert cl(tx, ty) == BAD_ARG
    assert eq(w=65536, h=32768, ipitch=2 * 65536, ostep=3 * 65536) == UNSUPPORTED
    for kw in (dict(w=0), dict(h=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    assert (out == SENT).all() and np.array_equal(frame, f0) and np.array_equal(big, b0)
    # an image directly behind the input does not meet it; the context still works, and a refused call left no copy in flight
    behind = image_in(big, 2 * w * h, h, w, 3 * w)
    got = c.equalize_hist_packed422_to_bgr(rows_in(big, 0, h, 2 * w), w, FMT_YUY2, ORDER_BGR, out=behind)
    want = expected(frame, w, FMT_YUY2, ORDER_BGR, "eq", None, "err")
    assert np.array_equal(got, want) and np.array_equal(big[: 2 * w * h], b0[: 2 * w * h])
    assert (big[2 * w * h + 3 * w * h:] == SENT).all()
