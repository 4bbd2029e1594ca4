"""Planar 4:2:0 frames (I420 / YV12) in, interleaved BGR / RGB images out on the GPU: mi_equalize_hist_yuv420_to_bgr_batch_dev,
mi_clahe_yuv420_to_bgr_batch_dev and their host forms.  Expected bytes are oracle.nv12_to_bgr(oracle.nv12_frame(<Y, then U and V
interleaved>, W, H, uv_mode=1, op...), W, H), the last axis reversed for MI_ORDER_RGB.  Y, U and V are independent full-range random
bytes, so a swapped U / V order or a mixed-up row cannot pass.  Every side of a call lives in a sentinel-filled allocation with 64 guard
bytes and the WHOLE allocation is compared, input and output: every comparison in this file is exact.  Every call also asserts its
counter deltas: (yuv420_bgr_onepass, yuv420_bgr_twopass) and (yuv420_bgr_vec, yuv420_bgr_bytes).
tests/test_gpu_yuv420_to_bgr_geometry.py has the alignment rule term by term, the shapes where the loops repeat and the random sweep."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, COLOR_YUV2BGR_NV12, CHROMA_PLANAR, Yuv420Planes
from test_gpu_yuv420 import ROOT, SENT, EQ, Side, content, tight_frame
from test_gpu_nv12_to_bgr import BgrOut

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
ORDERS = [ORDER_BGR, ORDER_RGB]
ONE, TWO, VEC, BYTES = (1, 0), (0, 1), (1, 0), (0, 1)


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def expected_bgr(w, h, n, seed, op, contract=False):
    """The BGR images the call must produce for content(w, h, n, seed); computed once, never modified.  `contract` only keys the cache:
    the caller has switched the oracle."""
    kind, cfg = op
    out = []
    for y, u, v in content(w, h, n, seed):
        frame = tight_frame("nv12", y, u, v)
        nv12 = oracle.nv12_frame(frame, w, h, 1, 0) if kind == "eq" else oracle.nv12_frame(frame, w, h, 1, 1, *cfg)
        bgr = oracle.nv12_to_bgr(nv12, w, h)
        bgr.setflags(write=False)
        out.append(bgr)
    return tuple(out)


def expected(w, h, n, seed, op, order, contract=False):
    imgs = expected_bgr(w, h, n, seed, op, contract)
    return list(imgs) if order == ORDER_BGR else [np.ascontiguousarray(i[:, :, ::-1]) for i in imgs]


class SideBySide(Side):
    """A planar side whose U and V rows lie side by side in ONE pitched plane: c1 = c0 + W/2, both at c_pitch >= W.  The allocation is
    that of an "nv12" Side (one chroma plane of W-byte rows)."""

    def __init__(self, w, h, n, c_pitch=None, **kw):
        super().__init__(w, h, n, "nv12", c_pitch=c_pitch, **kw)

    def planes(self, **over):
        d = dict(c1=self.base + self.offsets()[1] + self.w // 2, chroma=CHROMA_PLANAR)
        d.update(over)
        return super().planes(**d)

    def image(self, frames=None, chroma=True, luma=True):
        a = np.full(self.total, SENT, np.uint8)
        w, h = self.w, self.h
        for k, (y, u, v) in enumerate(frames or []):
            yo, c0 = self.off + k * self.fstride, self.off + self.a_off + k * self.fstride
            for r in range(h):
                a[yo + r * self.y_pitch: yo + r * self.y_pitch + w] = y[r]
            for r in range(h // 2):
                a[c0 + r * self.c_pitch: c0 + r * self.c_pitch + w // 2] = u[r]
                a[c0 + r * self.c_pitch + w // 2: c0 + r * self.c_pitch + w] = v[r]
        return a


def run(c, op, src, dst, order, n=None, st=None, planes=None):
    kind, cfg = op
    a = planes or src.planes()
    kw = dict(dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_yuv420_to_bgr_batch_dev(a, dst.ptr, src.w, src.h, n, order, **kw)
    else:
        c.clahe_yuv420_to_bgr_batch_dev(a, dst.ptr, src.w, src.h, n, order, *cfg, **kw)


STATS = ("yuv420_bgr_onepass", "yuv420_bgr_twopass", "yuv420_bgr_vec", "yuv420_bgr_bytes")


def stats(c):
    return tuple(c.get_stat(s) for s in STATS)


def nv12_stats(c):
    return c.get_stat("nv12_bgr_onepass"), c.get_stat("nv12_bgr_twopass")


def delta(before, after):
    d = tuple(a - b for a, b in zip(after, before))
    return d[:2], d[2:]


def check(c, w, h, n, seed, op, order, src, dst, want, contract=False):
    """One call on the uploaded content: exact output, untouched guards and input, and the counters moved by `want` =
    ((onepass, twopass), (vec, bytes))."""
    frames = content(w, h, n, seed)
    src.upload(frames)
    dst.clear()
    before = stats(c)
    run(c, op, src, dst, order)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same(expected(w, h, n, seed, op, order, contract))
    assert ok, (w, h, src.fmt, op, order, nbad, where)
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"
    assert delta(before, stats(c)) == want, (op, before, stats(c), want)


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


# ---- 1. layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", ["i420", "yv12"])
def test_smallest_frames_tight(c, fmt, order):
    """2 x 2: one block with byte accesses, one sample per chroma plane (no grid gives 16-column tiles: CLAHE goes two-pass).  16 x 2:
    one 16 x 2 group; the chroma planes are 8 bytes each, so the second lies 8 past a 16-byte boundary; CLAHE 1 x 1 is one-pass."""
    n = 3
    for op, want in ((EQ, (ONE, BYTES)), (("clahe", (2.0, 1, 1)), (TWO, BYTES))):
        check(c, 2, 2, n, 11, op, order, Side(2, 2, n, fmt), BgrOut(2, 2, n), want)
    src = Side(16, 2, n, fmt)
    assert sorted(o % 16 for o in src.offsets()[1:]) == [0, 8]
    for op in (EQ, ("clahe", (2.0, 1, 1))):
        check(c, 16, 2, n, 12, op, order, src, BgrOut(16, 2, n), (ONE, VEC))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", ["i420", "yv12"])
def test_pitched_planes_with_gaps(c, fmt, order):
    """64 x 32, CLAHE 4 x 2, a nonzero base, every pitch larger than its row, gaps between the planes and between the frames; the Y and
    output terms multiples of 16, the chroma pitch and the second chroma plane multiples of 8 only: the vector path, and the pitch
    padding, the gaps and the guards keep their pattern, in the output and in the input."""
    w, h, n = 64, 32, 3
    src = Side(w, h, n, fmt, y_pitch=80, c_pitch=40, gap0=16, gap1=8, frame_gap=24, off=16)
    assert src.fstride % 16 == 0 and src.c_pitch % 16 == 8 and sorted(o % 16 for o in src.offsets()[1:]) == [0, 8]
    dst = BgrOut(w, h, n, pitch=208, frame_gap=64, off=32)
    check(c, w, h, n, 13, ("clahe", (2.0, 4, 2)), order, src, dst, (ONE, VEC))
    check(c, w, h, n, 13, EQ, order, src, dst, (ONE, VEC))
    check(c, w, h, n, 13, ("clahe", (2.0, 3, 2)), order, src, dst, (TWO, VEC))       # REFLECT_101 padding: the fallback, decode on groups


@pytest.mark.parametrize("order", ORDERS)
def test_unaligned_planes_take_the_byte_path(c, order):
    """34 x 18 at odd pitches, odd gaps and an odd base: 2 x 2 blocks with byte accesses; CLAHE 3 x 2 pads by REFLECT_101."""
    w, h, n = 34, 18, 2
    for fmt in ("i420", "yv12"):
        src = Side(w, h, n, fmt, y_pitch=35, c_pitch=19, gap0=3, gap1=5, frame_gap=7, off=1)
        dst = BgrOut(w, h, n, pitch=103, frame_gap=7, off=1)
        check(c, w, h, n, 14, EQ, order, src, dst, (ONE, BYTES))
        check(c, w, h, n, 14, ("clahe", (2.0, 3, 2)), order, src, dst, (TWO, BYTES))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("w,tx", [(16, 1), (32, 2)])
def test_u_and_v_rows_side_by_side_in_one_plane(c, w, tx, order):
    """c1 = c0 + W/2, c_pitch = W: legal (the overlap checks are pointer equality) and, c1 being a multiple of 8, on the vector path."""
    h, n = 4, 2
    src = SideBySide(w, h, n)
    p = src.planes()
    assert p.c1 == p.c0 + w // 2 and p.c_pitch == w and p.chroma == CHROMA_PLANAR and p.c1 % 8 == 0
    for op in (EQ, ("clahe", (2.0, tx, 1))):
        check(c, w, h, n, 15, op, order, src, BgrOut(w, h, n), (ONE, VEC))
    pitched = SideBySide(w, h, n, c_pitch=w + 8, y_pitch=w + 16, gap0=16, frame_gap=16 - (8 * (h // 2)) % 16, off=16)
    assert pitched.fstride % 16 == 0
    check(c, w, h, n, 15, ("clahe", (2.0, tx, 1)), order, pitched, BgrOut(w, h, n), (ONE, VEC))


# ---- 5. clahe_fp_contract --------------------------------------------------------------------------------------------------------
def test_fp_contract_takes_the_fallback(c):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    c.set_option("clahe_fp_contract", 1)
    prev = oracle.set_fp_contract(True)
    try:
        check(c, w, h, n, 16, ("clahe", (2.0, 4, 2)), ORDER_BGR, Side(w, h, n, "i420"), BgrOut(w, h, n), (TWO, VEC), contract=True)
    finally:
        oracle.set_fp_contract(prev)
        c.set_option("clahe_fp_contract", 0)
    check(c, w, h, n, 16, ("clahe", (2.0, 4, 2)), ORDER_BGR, Side(w, h, n, "i420"), BgrOut(w, h, n), (ONE, VEC))


# ---- 6. identity -----------------------------------------------------------------------------------------------------------------
IDENTITY_OPS = [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))]


@pytest.mark.parametrize("op", IDENTITY_OPS, ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_identity_with_the_nv12_form_and_the_two_call_composition(c, op):
    """The header's contract sentences as written: the bytes of mi_*_nv12_to_bgr_batch_dev on the same pixels with U and V interleaved,
    and of mi_*_yuv420_batch_dev(I420 -> NV12, MI_UV_COPY) followed by mi_cvt_color_420_u8_batch_dev(YUV2BGR_NV12)."""
    w, h, n = 64, 32, 3
    frames = content(w, h, n, 17)
    src = Side(w, h, n, "i420").upload(frames)
    inter = xfer.to_device(np.stack([tight_frame("nv12", *f) for f in frames]))
    mid = Side(w, h, n, "nv12")                                                          # the tight NV12 batch in between
    d_new, d_nv12, d_two = (torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0") for _ in range(3))
    before = stats(c)
    if op is EQ:
        c.equalize_hist_yuv420_to_bgr_batch_dev(src.planes(), d_new, w, h, n, ORDER_BGR, stream=stream())
        c.equalize_hist_nv12_to_bgr_batch_dev(inter, None, d_nv12, w, h, n, ORDER_BGR, stream=stream())
        c.equalize_hist_yuv420_batch_dev(src.planes(), mid.planes(), w, h, n, UV_COPY, stream=stream())
    else:
        c.clahe_yuv420_to_bgr_batch_dev(src.planes(), d_new, w, h, n, ORDER_BGR, *op[1], stream=stream())
        c.clahe_nv12_to_bgr_batch_dev(inter, None, d_nv12, w, h, n, ORDER_BGR, *op[1], stream=stream())
        c.clahe_yuv420_batch_dev(src.planes(), mid.planes(), w, h, n, UV_COPY, *op[1], stream=stream())
    c.cvt_color_420_batch_dev(mid.buf, d_two, w, h, n, COLOR_YUV2BGR_NV12, stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(d_new, d_nv12), "not the bytes of the NV12 form"
    assert torch.equal(d_new, d_two), "not the bytes of the two-call composition"
    assert np.array_equal(xfer.to_host(d_new), np.stack(expected(w, h, n, 17, op, ORDER_BGR)))
    assert delta(before, stats(c)) == ((TWO if op[1] == (2.0, 3, 2) else ONE), VEC)


@pytest.mark.parametrize("op", IDENTITY_OPS, ids=["eq", "clahe-onepass", "clahe-twopass"])
@pytest.mark.parametrize("order", ORDERS)
def test_an_interleaved_input_is_the_nv12_form(c, op, order):
    """in->chroma == MI_CHROMA_INTERLEAVED: the bytes and the counters of mi_*_nv12_to_bgr_batch_dev; in->c1 is ignored."""
    w, h, n = 64, 32, 2
    frames = content(w, h, n, 18)
    src = Side(w, h, n, "nv12", y_pitch=80, c_pitch=96, gap0=32, frame_gap=48, off=16).upload(frames)
    dst, ref = BgrOut(w, h, n, pitch=208, frame_gap=64, off=32), BgrOut(w, h, n, pitch=208, frame_gap=64, off=32)
    p = src.planes(c1=0xDEAD0)
    before, nbefore = stats(c), nv12_stats(c)
    run(c, op, src, dst, order, planes=p)
    nafter = nv12_stats(c)
    kw = dict(y_pitch=src.y_pitch, uv_pitch=src.c_pitch, in_frame=src.fstride, **ref.kw(), stream=stream())
    if op is EQ:
        c.equalize_hist_nv12_to_bgr_batch_dev(p.y, p.c0, ref.ptr, w, h, n, order, **kw)
    else:
        c.clahe_nv12_to_bgr_batch_dev(p.y, p.c0, ref.ptr, w, h, n, order, *op[1], **kw)
    torch.cuda.synchronize()
    assert torch.equal(dst.buf, ref.buf)
    assert dst.same(expected(w, h, n, 18, op, order))[0]
    assert np.array_equal(src.host(), src.image(frames))
    assert stats(c) == before, "a yuv420_bgr_* counter moved on an interleaved input"
    want = TWO if op[1] == (2.0, 3, 2) else ONE
    assert (nafter[0] - nbefore[0], nafter[1] - nbefore[1]) == want


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------
def test_chunk_size_is_that_of_the_nv12_form():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "nv12_bgr.inc.hpp").read_text()
    assert int(re.search(r"constexpr\s+int\s+kNv12BgrFramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1)) == 256
    new = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "yuv420_bgr.inc.hpp").read_text()
    assert new.count("f0 += kNv12BgrFramesPerLaunch") == 3


@pytest.mark.parametrize("op,want", [(EQ, ONE), (("clahe", (2.0, 1, 1)), ONE), (("clahe", (2.0, 3, 1)), TWO)],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, op, want):
    """257 frames of 16 x 4: one full launch sequence and one of a single frame; every frame distinct, every frame checked (the
    fallback reuses its scratch planes from chunk to chunk)."""
    w, h, n = 16, 4, 257
    check(c, w, h, n, 19, op, ORDER_RGB, Side(w, h, n, "yv12"), BgrOut(w, h, n), (want, VEC))


# ---- 8. host form ----------------------------------------------------------------------------------------------------------------
def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


def host_want(w, h, fmt, op):
    """The counter deltas of a host call: the staged frame is tight with every plane at a 16-byte aligned offset."""
    if fmt == "nv12":
        return (0, 0), (0, 0)
    vec = w % 16 == 0
    if op is EQ:
        return ONE, (VEC if vec else BYTES)
    onepass = vec and w % op[1][1] == 0 and h % op[1][2] == 0 and (w // op[1][1]) % 16 == 0
    return (ONE if onepass else TWO), (VEC if vec else BYTES)


def padded_plane(p, extra):
    """a plane in an array of its own, rows `extra` bytes longer than they need be, at an odd address"""
    raw = np.full(p.shape[0] * (p.shape[1] + extra) + 1, SENT, np.uint8)
    view = raw[1:].reshape(p.shape[0], p.shape[1] + extra)
    view[:, : p.shape[1]] = p
    return raw, view


@pytest.mark.parametrize("w,h", [(2, 2), (34, 18), (96, 144)])
def test_host_form(w, h):
    """Tight frames through the binding, pageable and registered; planes in three separate arrays at odd addresses and odd pitches
    through the C entry points; out rows an odd number of bytes apart: only the 3*W bytes of each row are written, the input is not."""
    y, u, v = content(w, h, 1, 20)[0]
    ops = (EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 2) if w == 2 else (2.0, 3, 2)))
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        for fmt in ("i420", "yv12", "nv12"):
            frame = tight_frame(fmt, y, u, v)
            raw_i, pin_in = aligned_bytes(frame.size)
            pin_in[:] = frame
            raw_o, pin_flat = aligned_bytes(w * h * 3)
            pin_out = pin_flat.reshape(h, w, 3)
            for op in ops:
                for order in ORDERS:
                    want = expected(w, h, 1, 20, op, order)[0]
                    # pageable memory, out rows padded to an odd step
                    padded = np.full((h, 3 * w + 25), SENT, np.uint8)
                    assert padded.strides[0] % 2 == 1
                    out = padded[:, : 3 * w].reshape(h, w, 3)
                    src = frame.copy()
                    before, nbefore = stats(c), nv12_stats(c)
                    if op is EQ:
                        got = c.equalize_hist_yuv420_to_bgr(src, w, h, fmt, order, out=out)
                    else:
                        got = c.clahe_yuv420_to_bgr(src, w, h, fmt, order, *op[1], out=out)
                    bad = np.flatnonzero(out != want)
                    assert got is out and bad.size == 0, (fmt, op, order, bad.size, bad[:8])
                    assert (padded[:, 3 * w:] == SENT).all() and np.array_equal(src, frame)
                    assert delta(before, stats(c)) == host_want(w, h, fmt, op), (fmt, op)
                    assert sum(nv12_stats(c)) - sum(nbefore) == (1 if fmt == "nv12" else 0)
            # registered (pinned) tight memory, each image one registration
            mi_lumaeq.host_register(pin_in)
            mi_lumaeq.host_register(pin_flat)
            try:
                for op in ops:
                    pin_out[:] = SENT
                    if op is EQ:
                        c.equalize_hist_yuv420_to_bgr(pin_in, w, h, fmt, ORDER_BGR, out=pin_out)
                    else:
                        c.clahe_yuv420_to_bgr(pin_in, w, h, fmt, ORDER_BGR, *op[1], out=pin_out)
                    assert np.array_equal(pin_out, expected(w, h, 1, 20, op, ORDER_BGR)[0]), (fmt, op)
                    assert np.array_equal(pin_in, frame)
            finally:
                mi_lumaeq.host_unregister(pin_flat)
                mi_lumaeq.host_unregister(pin_in)
        # three separate arrays, odd addresses, odd pitches; frame_stride is ignored
        ry, py = padded_plane(y, 5)
        ru, pu = padded_plane(u, 3)
        rv, pv = padded_plane(v, 3)
        keep = [r.copy() for r in (ry, ru, rv)]
        assert py.ctypes.data % 2 == 1 and py.strides[0] % 2 == 1 and pu.strides[0] == w // 2 + 3
        a = Yuv420Planes(py.ctypes.data, py.strides[0], pu.ctypes.data, pv.ctypes.data, pu.strides[0], 12345, CHROMA_PLANAR)
        for op in ops:
            padded = np.full((h, 3 * w + 25), SENT, np.uint8)
            if op is EQ:
                st = L.mi_equalize_hist_yuv420_to_bgr(hd, ctypes.byref(a), padded.ctypes.data, padded.strides[0], w, h, ORDER_RGB)
            else:
                st = L.mi_clahe_yuv420_to_bgr(hd, ctypes.byref(a), padded.ctypes.data, padded.strides[0], w, h, ORDER_RGB, *op[1])
            assert st == 0, (op, st)
            assert np.array_equal(padded[:, : 3 * w].reshape(h, w, 3), expected(w, h, 1, 20, op, ORDER_RGB)[0]), op
            assert (padded[:, 3 * w:] == SENT).all()
            assert all(np.array_equal(r, k) for r, k in zip((ry, ru, rv), keep)), "the input was written"
        assert c.get_stat("error_drains") == 0


# ---- 9. hipGraph -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then one call captured on a side stream and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    src = Side(w, h, n, "i420", y_pitch=80, c_pitch=40, gap0=16, gap1=8, frame_gap=24, off=16)
    dst = BgrOut(w, h, n, pitch=208, frame_gap=64, off=32)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            src.upload(content(w, h, n, 21))
            dst.clear()
            run(c, op, src, dst, ORDER_BGR)                         # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert dst.same(expected(w, h, n, 21, op, ORDER_BGR))[0], ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, src, dst, ORDER_BGR, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                src.upload(content(w, h, n, 22 + rep))
                dst.clear()
                g.replay()
                torch.cuda.synchronize()
                assert dst.same(expected(w, h, n, 22 + rep, op, ORDER_BGR))[0], ("graph replay", op, rep)
                assert np.array_equal(src.host(), src.image(content(w, h, n, 22 + rep)))


# ---- 10. errors, zero sizes, launch accounting -----------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    frames = content(w, h, n, 24)
    src = Side(w, h, n, "i420", y_pitch=48, c_pitch=24, gap0=16, gap1=8, frame_gap=8).upload(frames)
    isrc = Side(w, h, n, "nv12", y_pitch=48, c_pitch=48).upload(frames)
    dst = BgrOut(w, h, n, pitch=112)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)

        def call(a, ctx=hd, o=dst.ptr, op=dst.pitch, fo=dst.fstride, w=w, h=h, n=n, order=ORDER_BGR, tiles=None):
            pa = None if a is None else ctypes.byref(a)
            if tiles is None:
                return L.mi_equalize_hist_yuv420_to_bgr_batch_dev(ctx, pa, o, op, fo, w, h, n, order, stream())
            return L.mi_clahe_yuv420_to_bgr_batch_dev(ctx, pa, o, op, fo, w, h, n, order, 2.0, tiles[0], tiles[1], stream())

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
            (A(), dict(op=3 * w - 1)), (I(), dict(op=3 * w - 1)),                                # out_pitch < 3*W
            (A(), dict(o=s.y)), (A(), dict(o=s.c0)), (A(), dict(o=s.c1)), (I(), dict(o=I().y)), (I(), dict(o=I().c0)),   # no in-place form
        ]
        for a, kw in bad:
            assert both(a, **kw) == (BAD_ARG, BAD_ARG), (kw, None if a is None else bytes(a))
        for tiles in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert call(A(), tiles=tiles) == BAD_ARG, tiles
            assert call(A(), tiles=tiles, n=0) == BAD_ARG, tiles
        # zero sizes: MI_OK, nothing written
        for kw in (dict(w=0), dict(h=0), dict(n=0)):
            assert both(A(), **kw) == (0, 0), kw
        # sizes and tile grids the planar forms refuse: their status
        bw = (1 << 24) + 2
        planar = L.mi_clahe_u8_batch_dev(hd, s.y, 1 << 25, 1 << 26, dst.ptr, 1 << 25, 1 << 26, bw, 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and both(A(y_pitch=1 << 25, c_pitch=1 << 25), w=bw, h=2, op=1 << 27) == (planar, planar)
        planar = L.mi_clahe_u8_batch_dev(hd, s.y, s.y_pitch, s.frame_stride, dst.ptr, dst.pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and call(A(), tiles=(2048, 1024)) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0, 0, 0, 0) and nv12_stats(c) == (0, 0)
        # launch accounting of the three sequences, by role; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (ONE, VEC)),
                             (("clahe", (2.0, 2, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (ONE, VEC)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (TWO, VEC))):
            c.profile_read(reset=True)
            check(c, w, h, n, 24, op, ORDER_RGB, src, dst, st)
            got = launches(c)
            assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_host_form_errors():
    w, h = 32, 16
    src = Side(w, h, 1, "i420", dev=False).upload(content(w, h, 1, 25))
    isrc = Side(w, h, 1, "nv12", dev=False).upload(content(w, h, 1, 25))
    out = np.full((h, w, 3), SENT, np.uint8)
    o = out.ctypes.data
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        A, I = src.planes, isrc.planes
        for ctx, a, po, step, ww, hh, order in (
                (None, A(), o, 3 * w, w, h, 0), (hd, None, o, 3 * w, w, h, 0), (hd, A(chroma=3), o, 3 * w, w, h, 0),
                (hd, A(), o, 3 * w, w, h, 2), (hd, A(), o, 3 * w, -2, h, 0), (hd, A(), o, 3 * w, w - 1, h, 0),
                (hd, A(), o, 3 * w, w, h - 1, 0), (hd, A(), o, 3 * w, w - 1, 0, 0), (hd, A(y=None), o, 3 * w, w, h, 0),
                (hd, A(c0=None), o, 3 * w, w, h, 0), (hd, A(c1=None), o, 3 * w, w, h, 0), (hd, A(), None, 3 * w, w, h, 0),
                (hd, A(y_pitch=w - 1), o, 3 * w, w, h, 0), (hd, A(c_pitch=w // 2 - 1), o, 3 * w, w, h, 0),
                (hd, I(c_pitch=w - 1), o, 3 * w, w, h, 0), (hd, A(), o, 3 * w - 1, w, h, 0),
                (hd, A(), A().y, 3 * w, w, h, 0), (hd, A(), A().c0, 3 * w, w, h, 0), (hd, A(), A().c1, 3 * w, w, h, 0)):
            pa = None if a is None else ctypes.byref(a)
            assert L.mi_equalize_hist_yuv420_to_bgr(ctx, pa, po, step, ww, hh, order) == BAD_ARG
            assert L.mi_clahe_yuv420_to_bgr(ctx, pa, po, step, ww, hh, order, 2.0, 2, 2) == BAD_ARG
        a = A()
        assert L.mi_clahe_yuv420_to_bgr(hd, ctypes.byref(a), o, 3 * w, w, h, 0, 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_yuv420_to_bgr(hd, ctypes.byref(a), o, 3 * w, w, h, 0, 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_yuv420_to_bgr(hd, ctypes.byref(a), o, 3 * w, 0, h, 0) == 0
        assert L.mi_clahe_yuv420_to_bgr(hd, ctypes.byref(a), o, 3 * w, w, 0, 0, 2.0, 2, 2) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0 and stats(c) == (0, 0, 0, 0)
        assert src.same(content(w, h, 1, 25))[0]


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Side(w, h, 1, "i420").upload(content(w, h, 1, 26))
    dst = BgrOut(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            with pytest.raises(mi_lumaeq.MiError) as e:
                c.equalize_hist_yuv420_to_bgr(tight_frame("i420", *content(w, h, 1, 26)[0]), w, h, "i420")
            assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"
        assert stats(c) == (0, 0, 0, 0)
