"""Packed 4:2:2 host frames in (YUY2 / UYVY), planar 4:2:0 host planes out: mi_equalize_hist_packed422_to_yuv420 and
mi_clahe_packed422_to_yuv420.  The result equals the device batch form's bytes (which tests/test_gpu_packed422_to_yuv420.py pins to the
oracle) and, independently, the oracle's Y and the row-pair rounding mean de-interleaved.  Host planes at odd addresses and odd pitches
inside sentinel borders that must survive, a tight 36 x 4 frame (chroma pitch 18, which the device forms refuse), a pitched input,
registered tight planes on the direct path with the statistics host_planes_staged / host_planes_direct moving by four a call, an output
that overlaps the input refused.  Exact bytes."""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
import test_gpu_packed422_to_nv12 as nv                 # helpers only
import test_gpu_packed422_to_nv12_host as nvh           # helpers only: plane_in, aligned_bytes
import test_gpu_packed422_to_yuv420 as pl               # helpers only: PlanarOut, run, expected_planes
from mi_lumaeq import synth, UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY
from mi_lumaeq.capi import Yuv420Planes, CHROMA_PLANAR

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = nv.SENT
OPS = [("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", pl.WIDE)]
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]


def call(c, op, cfg, frame, w, fmt, uv_mode, **kw):
    if op == "eq":
        return c.equalize_hist_packed422_to_yuv420(frame, w, "i420", fmt, uv_mode, **kw)
    return c.clahe_packed422_to_yuv420(frame, w, "i420", fmt, uv_mode, *cfg, **kw)


def batch_planes(c, frame, w, h, fmt, op, cfg, uv_mode):
    """(Y, U, V) from the device batch form with n_frames = 1."""
    src = nv.Batch(w, h, 1, nv.LAYOUTS[0]).upload([frame])
    dst = pl.PlanarOut(w, h, 1, "one")
    pl.run(c, op, cfg, src, dst.planes(), fmt, uv_mode)
    torch.cuda.synchronize()
    return tuple(dst.plane(name, 0) for name in ("y", "u", "v"))


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.mark.parametrize("w,h", [(36, 4), (62, 46), (64, 48)])
def test_pageable_tight_and_odd(c, w, h):
    """Pageable memory.  A tight I420 frame (36 x 4 and 62 x 46: tight chroma pitches 18 and 31, which the device forms refuse), then a
    pitched input and the three planes at odd pitches inside sentinel borders, Y and V at ODD addresses."""
    for fmt in FMTS:
        frame = synth.packed422_frame(w, h, fmt, "D2", 40 + fmt)
        f0 = frame.copy()
        ipitch, ypitch, cpitch = 2 * w + 12, w + 7, w // 2 + 3
        inbuf = np.full(16 + ipitch * h + 32, SENT, np.uint8)
        ioff = 4 - inbuf.ctypes.data % 4 + 4                        # the input side keeps the packed forms' rule: a multiple of 4
        pitched = nvh.plane_in(inbuf, ioff, h, ipitch)
        pitched[:, :2 * w] = frame
        in0 = inbuf.copy()
        for uv_mode in UVS:
            for op, cfg in OPS:
                assert nv.planar_status(c, w, h, 1, op, cfg) == 0
                want = pl.expected_planes(frame, w, fmt, op, cfg, uv_mode, ("host", w, h, fmt))
                dev = batch_planes(c, frame, w, h, fmt, op, cfg, uv_mode)
                for a, b in zip(want, dev):
                    assert np.array_equal(a, b), ("batch form vs oracle", w, h, fmt, uv_mode, op, cfg)
                s0, d0 = c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")
                out = call(c, op, cfg, frame, w, fmt, uv_mode)
                assert out.shape == (w * h * 3 // 2,)
                tight = np.concatenate([p.ravel() for p in want])
                assert np.array_equal(out, tight), ("tight", w, h, fmt, uv_mode, op, cfg)
                assert np.array_equal(frame, f0)
                assert (c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")) == (s0 + 4, d0), "pageable planes are staged"
                bufs = [np.full(16 + p * r + 32, SENT, np.uint8) for p, r in ((ypitch, h), (cpitch, h // 2), (cpitch, h // 2))]
                offs = [9 if bufs[0].ctypes.data % 2 == 0 else 8, 4 - bufs[1].ctypes.data % 4 + 2, 9 if bufs[2].ctypes.data % 2 == 0 else 8]
                views = [nvh.plane_in(b, o, r, p) for b, o, (p, r) in zip(bufs, offs, ((ypitch, h), (cpitch, h // 2), (cpitch, h // 2)))]
                assert views[0].ctypes.data % 2 == 1 and views[1].ctypes.data % 4 == 2 and views[2].ctypes.data % 2 == 1
                planes = Yuv420Planes(views[0].ctypes.data, ypitch, views[1].ctypes.data, views[2].ctypes.data, cpitch, 12345, CHROMA_PLANAR)
                call(c, op, cfg, pitched, w, fmt, uv_mode, planes=planes)
                for b, o, (p, r), cols, wnt in zip(bufs, offs, ((ypitch, h), (cpitch, h // 2), (cpitch, h // 2)), (w, w // 2, w // 2), want):
                    exp = np.full_like(b, SENT)
                    nvh.plane_in(exp, o, r, p)[:, :cols] = wnt
                    assert np.array_equal(b, exp), ("pitched", w, h, fmt, uv_mode, op, cfg)
                assert np.array_equal(inbuf, in0), "the input was written"


@pytest.mark.parametrize("w,h", [(64, 48), (36, 4)])
def test_registered_memory(c, w, h):
    """Planes registered with mi_host_register.  64 x 48: tight planes whose device rows are tight too (W % 8 == 0) are DMA'd as they
    are, four direct planes.  36 x 4: W % 4 == 0 but W % 8 != 0, so the Y plane and the input go directly and the two chroma planes
    stage.  Pitched registered outputs stage.  The counters move by four in total either way, and the bytes are the same."""
    fmt, uv_mode = FMT_UYVY, UV_COPY
    frame = synth.packed422_frame(w, h, fmt, "D3", 77)
    csz = (w // 2) * (h // 2)
    raw_i, ib = nvh.aligned_bytes(2 * w * h)
    raw_y, yb = nvh.aligned_bytes((w + 8) * h)
    raw_u, ub = nvh.aligned_bytes((w // 2 + 8) * (h // 2))
    raw_v, vb = nvh.aligned_bytes((w // 2 + 8) * (h // 2))
    regs = (ib, yb, ub, vb)
    for a in regs:
        mi_lumaeq.host_register(a)
    try:
        fin = ib.reshape(h, 2 * w)
        fin[:] = frame
        for op, cfg in OPS[:2]:
            want = pl.expected_planes(frame, w, fmt, op, cfg, uv_mode, ("reg", w, h))
            for b in (yb, ub, vb):
                b[:] = SENT
            planes = Yuv420Planes(yb.ctypes.data, w, ub.ctypes.data, vb.ctypes.data, w // 2, 0, CHROMA_PLANAR)
            s0, d0 = c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")
            call(c, op, cfg, fin, w, fmt, uv_mode, planes=planes)
            ds, dd = c.get_stat("host_planes_staged") - s0, c.get_stat("host_planes_direct") - d0
            assert (ds, dd) == ((0, 4) if w % 8 == 0 else (2, 2)), (w, ds, dd)
            assert np.array_equal(yb[: w * h].reshape(h, w), want[0]), ("tight registered Y", w, h, op, cfg)
            assert np.array_equal(ub[:csz].reshape(h // 2, w // 2), want[1]) and np.array_equal(vb[:csz].reshape(h // 2, w // 2), want[2])
            assert (yb[w * h:] == SENT).all() and (ub[csz:] == SENT).all() and (vb[csz:] == SENT).all()
            # pitched registered outputs: staged, the padding untouched
            for b in (yb, ub, vb):
                b[:] = SENT
            yp, up, vp = yb.reshape(h, w + 8), ub.reshape(h // 2, w // 2 + 8), vb.reshape(h // 2, w // 2 + 8)
            planes = Yuv420Planes(yb.ctypes.data, w + 8, ub.ctypes.data, vb.ctypes.data, w // 2 + 8, 0, CHROMA_PLANAR)
            s0, d0 = c.get_stat("host_planes_staged"), c.get_stat("host_planes_direct")
            call(c, op, cfg, fin, w, fmt, uv_mode, planes=planes)
            assert (c.get_stat("host_planes_staged") - s0, c.get_stat("host_planes_direct") - d0) == (3, 1)
            assert np.array_equal(yp[:, :w], want[0]) and np.array_equal(up[:, : w // 2], want[1]) and np.array_equal(vp[:, : w // 2], want[2])
            assert (yp[:, w:] == SENT).all() and (up[:, w // 2:] == SENT).all() and (vp[:, w // 2:] == SENT).all()
            assert np.array_equal(fin, frame)
    finally:
        for a in regs:
            mi_lumaeq.host_unregister(a)


def test_interleaved_host_output_is_the_nv12_host_form(c):
    w, h, fmt = 36, 4, FMT_YUY2
    frame = synth.packed422_frame(w, h, fmt, "D1", 9)
    for op, cfg in OPS[:2]:
        if op == "eq":
            y, uv = c.equalize_hist_packed422_to_nv12(frame, w, fmt, UV_COPY)
            out = c.equalize_hist_packed422_to_yuv420(frame, w, "nv12", fmt, UV_COPY)
        else:
            y, uv = c.clahe_packed422_to_nv12(frame, w, fmt, UV_COPY, *cfg)
            out = c.clahe_packed422_to_yuv420(frame, w, "nv12", fmt, UV_COPY, *cfg)
        assert np.array_equal(out, np.concatenate([y.ravel(), uv.ravel()])), (op, cfg)


def test_errors_write_nothing(c):
    w, h = 64, 48
    frame = synth.packed422_frame(w, h, FMT_YUY2, "D1", 5)
    f0 = frame.copy()
    big = np.full(16 + 2 * w * h * 2, SENT, np.uint8)
    big = big[(-big.ctypes.data) % 4:]
    big[: 2 * w * h] = frame.ravel()
    b0 = big.copy()
    y = np.full((h, w), SENT, np.uint8)
    u = np.full((h // 2, w // 2), SENT, np.uint8)
    v = np.full((h // 2, w // 2), SENT, np.uint8)
    L, hd = c._L, c._h
    base = dict(i=frame.ctypes.data, ipitch=2 * w, y=y.ctypes.data, ypitch=w, c0=u.ctypes.data, c1=v.ctypes.data, cpitch=w // 2,
                chroma=CHROMA_PLANAR, w=w, h=h, fmt=FMT_YUY2, uvm=UV_COPY)

    def args(kw):
        a = dict(base)
        a.update(kw)
        planes = Yuv420Planes(a["y"], a["ypitch"], a["c0"], a["c1"], a["cpitch"], 2, a["chroma"])       # frame_stride is ignored
        return planes, (hd, a["i"], a["ipitch"], ctypes.byref(planes), a["w"], a["h"], a["fmt"], a["uvm"])

    def eq(**kw):
        keep, a = args(kw)
        return L.mi_equalize_hist_packed422_to_yuv420(*a)

    def cl(tx=8, ty=8, **kw):
        keep, a = args(kw)
        return L.mi_clahe_packed422_to_yuv420(*a, 2.0, tx, ty)
    bp = big.ctypes.data
    bad = [dict(i=None), dict(y=None), dict(c0=None), dict(c1=None),
           dict(w=63), dict(h=47), dict(w=63, h=47), dict(w=0, h=47), dict(w=63, h=0),
           dict(w=-2), dict(h=-2), dict(h=-1),
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1), dict(chroma=2), dict(chroma=-1),
           dict(ipitch=2 * w - 4), dict(ypitch=w - 1), dict(cpitch=w // 2 - 1),
           dict(i=bp + 2), dict(i=bp, ipitch=2 * w + 2),                                 # the input side: multiples of 4
           dict(i=bp, y=bp), dict(i=bp, c0=bp), dict(i=bp, c1=bp + 2 * w * 3 + 1), dict(i=bp, c0=bp + 2 * w * (h - 1)),   # an output meets the input
           dict(c1=u.ctypes.data), dict(c0=y.ctypes.data), dict(c1=y.ctypes.data + w * (h - 1) + 3)]                      # the planes meet
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    assert L.mi_equalize_hist_packed422_to_yuv420(hd, frame.ctypes.data, 2 * w, None, w, h, FMT_YUY2, UV_COPY) == BAD_ARG
    for tx, ty in ((0, 8), (8, 0), (-1, 8)):
        assert cl(tx, ty) == BAD_ARG
    assert eq(w=65536, h=32768, ipitch=2 * 65536, ypitch=65536, cpitch=32768) == UNSUPPORTED
    for kw in (dict(w=0), dict(h=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    assert (y == SENT).all() and (u == SENT).all() and (v == SENT).all() and np.array_equal(frame, f0) and np.array_equal(big, b0)
    # the context still works, and a refused call left no copy in flight
    out = c.equalize_hist_packed422_to_yuv420(frame, w, "i420", FMT_YUY2, UV_COPY)
    want = pl.expected_planes(frame, w, FMT_YUY2, "eq", None, UV_COPY, "err")
    assert np.array_equal(out, np.concatenate([p.ravel() for p in want]))
