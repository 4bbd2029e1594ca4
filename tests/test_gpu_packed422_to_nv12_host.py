"""Packed 4:2:2 host frames in (YUY2 / UYVY), NV12 host planes out: mi_equalize_hist_packed422_to_nv12 and mi_clahe_packed422_to_nv12
against the oracle (Y: oracle.equalize_hist / oracle.clahe on the gathered luma; UV: 128 or the row-pair rounding mean), exact bytes.
Pageable memory and memory registered with mi_host_register, pitched input and outputs inside sentinel borders that must survive, a
tight output with W % 4 == 2, an output at an odd address; the statistics host_planes_staged / host_planes_direct move as the
pinned-ness says; refused and empty calls write nothing."""
import numpy as np
import pytest

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
SIZES = [(64, 48), (62, 46), (640, 360)]
OPS = [("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (3.0, 4, 4)), ("clahe", (2.0, 64, 2))]        # the last: the wide-grid kernel
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]


def luma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, fmt - 2:2 * w:2])


def chroma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, 3 - fmt:2 * w:2])


_ref_cache = {}


def expected_planes(frame, w, fmt, op, cfg, uv_mode, key):
    h = frame.shape[0]
    k = (key, fmt, op, cfg)
    if k not in _ref_cache:
        y = luma(frame, w, fmt)
        _ref_cache[k] = oracle.equalize_hist(y) if op == "eq" else oracle.clahe(y, *cfg)
    if uv_mode == UV_COPY:
        c = chroma(frame, w, fmt)
        uv = ((c[0::2].astype(np.uint16) + c[1::2] + 1) >> 1).astype(np.uint8)
    else:
        uv = np.full((h // 2, w), 128, np.uint8)
    return _ref_cache[k], uv


def plane_in(buf, off, rows, pitch):
    """A rows x pitch view of the byte buffer `buf` from byte `off` (the last row may be shorter than the pitch in memory: the view
    is built row-strided over exactly the bytes it needs)."""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, pitch), strides=(pitch, 1), writeable=True)


def call(c, op, cfg, frame, w, fmt, uv_mode, y_out=None, uv_out=None):
    if op == "eq":
        return c.equalize_hist_packed422_to_nv12(frame, w, fmt, uv_mode, y_out=y_out, uv_out=uv_out)
    return c.clahe_packed422_to_nv12(frame, w, fmt, uv_mode, *cfg, y_out=y_out, uv_out=uv_out)


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
    """Pageable memory.  Tight planes (62 x 46: a tight output with W % 4 == 2, which the device form refuses), then a pitched input
    and pitched outputs inside sentinel borders, the Y plane at an ODD address, the UV plane 2 bytes past a multiple of 4."""
    for fmt in FMTS:
        frame = synth.packed422_frame(w, h, fmt, "D2", 40 + fmt)
        f0 = frame.copy()
        ipitch, ypitch, uvpitch = 2 * w + 12, w + 7, w + 2
        inbuf = np.full(16 + ipitch * h + 32, SENT, np.uint8)
        ioff = 4 - inbuf.ctypes.data % 4 + 4                        # the input side keeps the packed forms' rule: a multiple of 4
        pitched = plane_in(inbuf, ioff, h, ipitch)
        pitched[:, :2 * w] = frame
        in0 = inbuf.copy()
        for uv_mode in UVS:
            for op, cfg in OPS:
                if not planar_ok(c, w, h, op, cfg):
                    continue
                want_y, want_uv = expected_planes(frame, w, fmt, op, cfg, uv_mode, ("host", w, h))
                s0, d0 = c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")
                y, uv = call(c, op, cfg, frame, w, fmt, uv_mode)
                assert y.shape == (h, w) and uv.shape == (h // 2, w) and y.strides[0] == w
                assert np.array_equal(y, want_y) and np.array_equal(uv, want_uv), ("tight", w, h, fmt, uv_mode, op, cfg)
                assert np.array_equal(frame, f0)
                assert (c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")) == (s0 + 3, d0), "pageable planes are staged"
                ybuf = np.full(16 + ypitch * h + 32, SENT, np.uint8)
                ubuf = np.full(16 + uvpitch * (h // 2) + 32, SENT, np.uint8)
                yoff = 9 if ybuf.ctypes.data % 2 == 0 else 8        # an odd address
                uoff = 4 - ubuf.ctypes.data % 4 + 2
                yv, uvv = plane_in(ybuf, yoff, h, ypitch), plane_in(ubuf, uoff, h // 2, uvpitch)
                assert yv.ctypes.data % 2 == 1 and uvv.ctypes.data % 4 == 2
                call(c, op, cfg, pitched, w, fmt, uv_mode, y_out=yv, uv_out=uvv)
                wy, wu = np.full_like(ybuf, SENT), np.full_like(ubuf, SENT)
                plane_in(wy, yoff, h, ypitch)[:, :w] = want_y
                plane_in(wu, uoff, h // 2, uvpitch)[:, :w] = want_uv
                assert np.array_equal(ybuf, wy) and np.array_equal(ubuf, wu), ("pitched", w, h, fmt, uv_mode, op, cfg)
                assert np.array_equal(inbuf, in0), "the input was written"


def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


@pytest.mark.parametrize("w,h", SIZES)
def test_registered_memory(c, w, h):
    """Planes registered with mi_host_register: tight planes with W % 4 == 0 are DMA'd as they are (three direct planes); with
    W % 4 == 2 the device rows are pitched, so the outputs stage while the input still goes directly; pitched registered outputs
    stage.  The same bytes either way."""
    fmt, uv_mode = FMT_UYVY, UV_COPY
    frame = synth.packed422_frame(w, h, fmt, "D3", 77)
    raw_i, ib = aligned_bytes(2 * w * h)
    raw_y, yb = aligned_bytes((w + 8) * h)
    raw_u, ub = aligned_bytes((w + 8) * (h // 2))
    for a in (ib, yb, ub):                                           # page-aligned, each one registration
        mi_lumaeq.host_register(a)
    try:
        fin = ib.reshape(h, 2 * w)
        fin[:] = frame
        for op, cfg in OPS[:2]:
            want_y, want_uv = expected_planes(frame, w, fmt, op, cfg, uv_mode, ("reg", w, h))
            yb[:] = SENT
            ub[:] = SENT
            y, uv = yb[: w * h].reshape(h, w), ub[: w * (h // 2)].reshape(h // 2, w)
            s0, d0 = c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")
            call(c, op, cfg, fin, w, fmt, uv_mode, y_out=y, uv_out=uv)
            ds, dd = c.get_stat("host_planes_staged") - s0, c.get_stat("host_planes_direct") - d0
            assert (ds, dd) == ((0, 3) if w % 4 == 0 else (2, 1)), (w, ds, dd)
            assert np.array_equal(y, want_y) and np.array_equal(uv, want_uv), ("tight registered", w, h, op, cfg)
            assert (yb[w * h:] == SENT).all() and (ub[w * (h // 2):] == SENT).all()
            # pitched registered outputs: staged, the padding untouched
            yb[:] = SENT
            ub[:] = SENT
            yp, up = yb.reshape(h, w + 8), ub.reshape(h // 2, w + 8)
            s0, d0 = c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")
            call(c, op, cfg, fin, w, fmt, uv_mode, y_out=yp, uv_out=up)
            assert (c.get_stat("host_planes_staged") - s0, c.get_stat("host_planes_direct") - d0) == (2, 1)
            assert np.array_equal(yp[:, :w], want_y) and np.array_equal(up[:, :w], want_uv), ("pitched registered", w, h, op, cfg)
            assert (yp[:, w:] == SENT).all() and (up[:, w:] == SENT).all()
            assert np.array_equal(fin, frame)
    finally:
        for a in (ib, yb, ub):
            mi_lumaeq.host_unregister(a)


def test_errors_write_nothing(c):
    w, h = 64, 48
    frame = synth.packed422_frame(w, h, FMT_YUY2, "D1", 5)
    f0 = frame.copy()
    big = np.full(16 + 2 * w * h * 2, SENT, np.uint8)
    big = big[(-big.ctypes.data) % 4:]
    big[: 2 * w * h] = frame.ravel()
    b0 = big.copy()
    y = np.full((h, w), SENT, np.uint8)
    uv = np.full((h // 2, w), SENT, np.uint8)
    L, hd = c._L, c._h
    ip, yp, up = frame.ctypes.data, y.ctypes.data, uv.ctypes.data
    base = dict(i=ip, ipitch=2 * w, y=yp, ypitch=w, uv=up, uvpitch=w, w=w, h=h, fmt=FMT_YUY2, uvm=UV_COPY)

    def args(kw):
        a = dict(base)
        a.update(kw)
        return (hd, a["i"], a["ipitch"], a["y"], a["ypitch"], a["uv"], a["uvpitch"], a["w"], a["h"], a["fmt"], a["uvm"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_nv12(*args(kw))

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_nv12(*args(kw), 2.0, tx, ty)
    bp = big.ctypes.data
    bad = [dict(i=None), dict(y=None), dict(uv=None),
           dict(w=63), dict(h=47), dict(w=63, h=47), dict(w=0, h=47), dict(w=63, h=0),
           dict(w=-2), dict(h=-2), dict(h=-1),
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),
           dict(ipitch=2 * w - 4), dict(ypitch=w - 1), dict(uvpitch=w - 2),
           dict(i=bp + 2), dict(i=bp, ipitch=2 * w + 2),                                 # the input side: multiples of 4
           dict(i=bp, y=bp), dict(i=bp, uv=bp), dict(i=bp, y=bp + 2 * w * 3 + 1), dict(i=bp, uv=bp + 2 * w * (h - 1)),   # an output meets the input
           dict(y=bp, uv=bp), dict(y=bp, uv=bp + w * (h - 1) + 3), dict(y=bp + w * (h // 2 - 1), uv=bp)]              # the planes meet
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8)):
        assert cl(tx, ty) == BAD_ARG
    assert eq(w=65536, h=32768, ipitch=2 * 65536, ypitch=65536, uvpitch=65536) == UNSUPPORTED
    for kw in (dict(w=0), dict(h=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    assert (y == SENT).all() and (uv == SENT).all() and np.array_equal(frame, f0) and np.array_equal(big, b0)
    # the context still works, and a refused call left no copy in flight
    gy, guv = c.equalize_hist_packed422_to_nv12(frame, w, FMT_YUY2, UV_COPY, y_out=y, uv_out=uv)
    wy, wuv = expected_planes(frame, w, FMT_YUY2, "eq", None, UV_COPY, "err")
    assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
