"""NV12 frames in, interleaved BGR / RGB images out on the GPU: mi_equalize_hist_nv12_to_bgr_batch_dev, mi_clahe_nv12_to_bgr_batch_dev and
their host forms.  Expected bytes are oracle.nv12_to_bgr(oracle.nv12_frame(frame, W, H, uv_mode=1, op=...), W, H), the last axis reversed
for MI_ORDER_RGB.  Y, U and V are full-range random bytes (Y < 16 and extreme chroma saturate both ends of the decode).  Every batch
lives in sentinel-filled allocations and the WHOLE allocation is compared, input and output: every comparison in this file is exact."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, COLOR_YUV2BGR_NV12

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
ORDERS = [ORDER_BGR, ORDER_RGB]
EQ = ("eq", None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def rand_frames(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8) for _ in range(n)]


def expected(frame, w, h, op, order):
    kind, cfg = op
    nv12 = oracle.nv12_frame(frame, w, h, 1, 0) if kind == "eq" else oracle.nv12_frame(frame, w, h, 1, 1, *cfg)
    bgr = oracle.nv12_to_bgr(nv12, w, h)
    return bgr if order == ORDER_BGR else np.ascontiguousarray(bgr[:, :, ::-1])


class Nv12In:
    """n NV12 frames in one sentinel-filled allocation: the Y plane of frame f at off + f * fstride (H rows at y_pitch), its UV plane
    plane_gap bytes behind the Y rows (H/2 rows at uv_pitch), frame_gap bytes before the next frame."""

    def __init__(self, w, h, n, y_pitch=None, uv_pitch=None, plane_gap=0, frame_gap=0, off=0):
        self.w, self.h, self.n, self.off = w, h, n, off
        self.y_pitch, self.uv_pitch = y_pitch or w, uv_pitch or w
        self.uv_off = self.y_pitch * h + plane_gap
        self.fstride = self.uv_off + self.uv_pitch * (h // 2) + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def y_ptr(self):
        return self.buf.data_ptr() + self.off

    @property
    def uv_ptr(self):
        return self.y_ptr + self.uv_off

    def image(self, frames):
        a = np.full(self.total, SENT, np.uint8)
        w, h = self.w, self.h
        for k, f in enumerate(frames):
            o = self.off + k * self.fstride
            a[o: o + self.y_pitch * h].reshape(h, self.y_pitch)[:, :w] = f[: w * h].reshape(h, w)
            o += self.uv_off
            a[o: o + self.uv_pitch * (h // 2)].reshape(h // 2, self.uv_pitch)[:, :w] = f[w * h:].reshape(h // 2, w)
        return a

    def upload(self, frames):
        self.buf.copy_(xfer.to_device(self.image(frames)))
        return self

    def host(self):
        return xfer.to_host(self.buf)

    def kw(self):
        return {"y_pitch": self.y_pitch, "uv_pitch": self.uv_pitch, "in_frame": self.fstride}


class BgrOut:
    """n interleaved images in one sentinel-filled allocation: H rows of 3W bytes at `pitch`, frames `fstride` apart."""

    def __init__(self, w, h, n, pitch=None, frame_gap=0, off=0):
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = pitch or 3 * w
        self.fstride = self.pitch * h + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, images=None):
        a = np.full(self.total, SENT, np.uint8)
        for k, img in enumerate(images or []):
            o = self.off + k * self.fstride
            a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 3 * self.w] = img.reshape(self.h, 3 * self.w)
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def same(self, images=None):
        got, want = xfer.to_host(self.buf), self.image(images)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]

    def kw(self):
        return {"out_pitch": self.pitch, "out_frame": self.fstride}


def run(c, op, src, dst, order, n=None, st=None):
    kind, cfg = op
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_nv12_to_bgr_batch_dev(src.y_ptr, src.uv_ptr, dst.ptr, src.w, src.h, n, order, **kw)
    else:
        c.clahe_nv12_to_bgr_batch_dev(src.y_ptr, src.uv_ptr, dst.ptr, src.w, src.h, n, order, *cfg, **kw)


def stats(c):
    return c.get_stat("nv12_bgr_onepass"), c.get_stat("nv12_bgr_twopass")


def check(c, frames, w, h, op, order, src, dst, want_stats):
    """One call on uploaded `frames`: exact output, untouched guards and input, and the (onepass, twopass) counters moved by want_stats."""
    src.upload(frames)
    dst.clear()
    before = stats(c)
    run(c, op, src, dst, order)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same([expected(f, w, h, op, order) for f in frames])
    assert ok, (w, h, op, order, nbad, where)
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"
    after = stats(c)
    assert (after[0] - before[0], after[1] - before[1]) == want_stats, (op, before, after)


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


# ---- 1. fast path, tight ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_fast_path_tight(c, order):
    """32 x 16, three frames, everything 16-byte aligned: two 16-pixel groups per row pair; CLAHE 2 x 2 has tiles of 16 x 8."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 11)
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        check(c, frames, w, h, op, order, Nv12In(w, h, n), BgrOut(w, h, n), (1, 0))


# ---- 2. fast path, pitched with guards -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_fast_path_pitched_with_guards(c, order):
    """64 x 32, CLAHE 4 x 2, every pitch and stride a multiple of 16 and larger than its row: the pitch padding, the gap between the
    planes and the gaps between frames keep their pattern, in the output and in the input."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 12)
    src = Nv12In(w, h, n, y_pitch=80, uv_pitch=96, plane_gap=32, frame_gap=48, off=16)
    dst = BgrOut(w, h, n, pitch=208, frame_gap=64, off=32)
    check(c, frames, w, h, ("clahe", (2.0, 4, 2)), order, src, dst, (1, 0))
    check(c, frames, w, h, EQ, order, src, dst, (1, 0))


# ---- 3. general and fallback paths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_general_and_fallback_paths(c, order):
    """34 x 18 (W % 16 == 2, no tile grid divides it), pointers one byte past a 16-byte boundary, odd pitches: 2 x 2 blocks with byte
    accesses; CLAHE 3 x 2 pads by REFLECT_101 and takes the planar CLAHE + decode fallback."""
    w, h, n = 34, 18, 2
    frames = rand_frames(w, h, n, 13)
    src = Nv12In(w, h, n, y_pitch=35, uv_pitch=37, plane_gap=3, frame_gap=5, off=1)
    dst = BgrOut(w, h, n, pitch=103, frame_gap=7, off=1)
    check(c, frames, w, h, EQ, order, src, dst, (1, 0))
    check(c, frames, w, h, ("clahe", (2.0, 3, 2)), order, src, dst, (0, 1))


def test_fp_contract_takes_the_fallback(c):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    frames = rand_frames(w, h, n, 14)
    c.set_option("clahe_fp_contract", 1)
    prev = oracle.set_fp_contract(True)
    try:
        check(c, frames, w, h, ("clahe", (2.0, 4, 2)), ORDER_BGR, Nv12In(w, h, n), BgrOut(w, h, n), (0, 1))
    finally:
        oracle.set_fp_contract(prev)
        c.set_option("clahe_fp_contract", 0)


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------
def test_edges(c):
    """2 x 2: one block, one chroma pair.  A constant Y plane: equalizeHist's shortcut (every pixel keeps its value).  Two values."""
    f22 = rand_frames(2, 2, 2, 15)
    for op in (EQ, ("clahe", (2.0, 1, 1))):
        check(c, f22, 2, 2, op, ORDER_BGR, Nv12In(2, 2, 2), BgrOut(2, 2, 2), (1, 0) if op is EQ else (0, 1))
    w, h = 32, 16
    const, two = rand_frames(w, h, 2, 16)
    const[: w * h] = 9                                             # below 16: the decode clamps (Y - 16) at 0
    two[: w * h] = np.where(np.arange(w * h) % 3 == 0, 200, 3).astype(np.uint8)
    for order in ORDERS:
        for op in (EQ, ("clahe", (2.0, 2, 2))):
            check(c, [const, two], w, h, op, order, Nv12In(w, h, 2), BgrOut(w, h, 2), (1, 0))


# ---- 5. identity with the existing two-call composition --------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_two_call_composition(c, op):
    """The header's contract sentence as written: mi_*_nv12_batch_dev(MI_UV_COPY), then mi_cvt_color_420_u8_batch_dev(YUV2BGR_NV12)."""
    w, h, n = 64, 32, 3
    d_in = xfer.to_device(np.stack(rand_frames(w, h, n, 17)))
    d_mid = torch.empty_like(d_in)
    d_two = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0")
    d_one = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0")
    if op is EQ:
        c.equalize_hist_nv12_batch_dev(d_in, d_mid, w, h, n, UV_COPY, stream=stream())
        c.equalize_hist_nv12_to_bgr_batch_dev(d_in, None, d_one, w, h, n, ORDER_BGR, stream=stream())
    else:
        c.clahe_nv12_batch_dev(d_in, d_mid, w, h, n, UV_COPY, *op[1], stream=stream())
        c.clahe_nv12_to_bgr_batch_dev(d_in, None, d_one, w, h, n, ORDER_BGR, *op[1], stream=stream())
    c.cvt_color_420_batch_dev(d_mid, d_two, w, h, n, COLOR_YUV2BGR_NV12, stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(d_one, d_two), op


# ---- 6. chunking -----------------------------------------------------------------------------------------------------------------
def frames_per_launch():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "nv12_bgr.inc.hpp").read_text()
    return int(re.search(r"constexpr\s+int\s+kNv12BgrFramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1))


@pytest.mark.parametrize("op,want", [(EQ, (1, 0)), (("clahe", (2.0, 2, 2)), (1, 0)), (("clahe", (2.0, 3, 2)), (0, 1))],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, op, want):
    """One frame more than two full launch sequences: three chunks, the last of one frame; every frame distinct, every frame checked
    (the fallback reuses its scratch planes from chunk to chunk)."""
    w, h = 32, 16
    n = 2 * frames_per_launch() + 1
    frames = rand_frames(w, h, n, 18)
    check(c, frames, w, h, op, ORDER_RGB, Nv12In(w, h, n), BgrOut(w, h, n), want)


# ---- 7. host form ----------------------------------------------------------------------------------------------------------------
def aligned_bytes(n, align=4096):
    raw = np.full(n + align, SENT, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw, raw[o: o + n]


def test_host_form():
    w, h = 64, 32
    frame = rand_frames(w, h, 1, 19)[0]
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            for order in ORDERS:
                want = expected(frame, w, h, op, order)
                # pageable memory, rows padded: only the 3*W bytes of each row are written
                padded = np.full((h, 3 * w + 24), SENT, np.uint8)
                out = padded[:, : 3 * w].reshape(h, w, 3)
                assert np.shares_memory(out, padded)
                src = frame.copy()
                if op is EQ:
                    got = c.equalize_hist_nv12_to_bgr(src, w, h, order, out=out)
                else:
                    got = c.clahe_nv12_to_bgr(src, w, h, order, *op[1], out=out)
                assert got is out and np.array_equal(out, want), (op, order)
                assert (padded[:, 3 * w:] == SENT).all() and np.array_equal(src, frame)
        # registered (pinned) tight memory, page-aligned, each image one registration: both are DMA'd as they are
        raw_i, pin_in = aligned_bytes(w * h * 3 // 2)
        raw_o, pin_flat = aligned_bytes(w * h * 3)
        pin_in[:] = frame
        pin_out = pin_flat.reshape(h, w, 3)
        mi_lumaeq.host_register(pin_in)
        mi_lumaeq.host_register(pin_flat)
        try:
            for op in (EQ, ("clahe", (2.0, 4, 2))):
                pin_out[:] = SENT
                if op is EQ:
                    c.equalize_hist_nv12_to_bgr(pin_in, w, h, ORDER_BGR, out=pin_out)
                else:
                    c.clahe_nv12_to_bgr(pin_in, w, h, ORDER_BGR, *op[1], out=pin_out)
                assert np.array_equal(pin_out, expected(frame, w, h, op, ORDER_BGR)), op
                assert np.array_equal(pin_in, frame)
        finally:
            mi_lumaeq.host_unregister(pin_flat)
            mi_lumaeq.host_unregister(pin_in)
        assert c.get_stat("error_drains") == 0


# ---- 8. hipGraph -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then capture on a side stream and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    src = Nv12In(w, h, n, y_pitch=80, uv_pitch=96, plane_gap=32, frame_gap=48, off=16)
    dst = BgrOut(w, h, n, pitch=208, frame_gap=64, off=32)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            frames = rand_frames(w, h, n, 20)
            src.upload(frames)
            dst.clear()
            run(c, op, src, dst, ORDER_BGR)                         # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert dst.same([expected(f, w, h, op, ORDER_BGR) for f in frames])[0], ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, src, dst, ORDER_BGR, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                fresh = rand_frames(w, h, n, 21 + rep)
                src.upload(fresh)
                dst.clear()
                g.replay()
                torch.cuda.synchronize()
                assert dst.same([expected(f, w, h, op, ORDER_BGR) for f in fresh])[0], ("graph replay", op, rep)


# ---- 9. errors, zero sizes, launch accounting ------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    frames = rand_frames(w, h, n, 22)
    src = Nv12In(w, h, n, y_pitch=48, uv_pitch=48, frame_gap=16).upload(frames)
    dst = BgrOut(w, h, n, pitch=112)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        base = dict(ctx=hd, y=src.y_ptr, yp=src.y_pitch, uv=src.uv_ptr, up=src.uv_pitch, fi=src.fstride, o=dst.ptr, op=dst.pitch,
                    fo=dst.fstride, w=w, h=h, n=n, order=ORDER_BGR)

        def args(kw):
            a = dict(base)
            a.update(kw)
            return (a["ctx"], a["y"], a["yp"], a["uv"], a["up"], a["fi"], a["o"], a["op"], a["fo"], a["w"], a["h"], a["n"], a["order"])

        def eq(**kw):
            return L.mi_equalize_hist_nv12_to_bgr_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_nv12_to_bgr_batch_dev(*args(kw), 2.0, tx, ty, stream())
        bad = [dict(ctx=None), dict(y=None), dict(uv=None), dict(o=None),                  # a null ctx or plane pointer
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(w=-2), dict(h=-2), dict(n=-1),                                          # negative sizes
               dict(yp=w - 1), dict(up=w - 1), dict(op=3 * w - 1),                          # a pitch below its row
               dict(order=2), dict(order=-1),                                               # order other than the two
               dict(o=src.y_ptr), dict(o=src.uv_ptr)]                                       # no in-place form
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written
        for kw in (dict(w=0), dict(h=0), dict(n=0)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: their status
        big = dict(w=(1 << 24) + 2, h=2, yp=1 << 25, up=1 << 25, op=1 << 27)
        planar = L.mi_clahe_u8_batch_dev(hd, src.y_ptr, 1 << 25, 1 << 26, dst.ptr, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, src.y_ptr, src.y_pitch, src.fstride, dst.ptr, dst.pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0, 0)
        # launch accounting of the three sequences, by role; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (1, 0)),
                             (("clahe", (2.0, 2, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (1, 0)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (0, 1))):
            c.profile_read(reset=True)
            check(c, frames, w, h, op, ORDER_RGB, src, dst, st)
            got = launches(c)
            assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_host_form_errors():
    w, h = 32, 16
    frame = rand_frames(w, h, 1, 23)[0]
    out = np.full((h, w, 3), SENT, np.uint8)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        for a in ((None, frame.ctypes.data, out.ctypes.data, 3 * w, w, h, 0), (hd, None, out.ctypes.data, 3 * w, w, h, 0),
                  (hd, frame.ctypes.data, None, 3 * w, w, h, 0), (hd, frame.ctypes.data, out.ctypes.data, 3 * w - 1, w, h, 0),
                  (hd, frame.ctypes.data, out.ctypes.data, 3 * w, w - 1, h, 0), (hd, frame.ctypes.data, out.ctypes.data, 3 * w, w, h - 1, 0),
                  (hd, frame.ctypes.data, out.ctypes.data, 3 * w, -2, h, 0), (hd, frame.ctypes.data, out.ctypes.data, 3 * w, w, h, 2)):
            assert L.mi_equalize_hist_nv12_to_bgr(*a) == BAD_ARG, a
            assert L.mi_clahe_nv12_to_bgr(*a, 2.0, 2, 2) == BAD_ARG, a
        assert L.mi_clahe_nv12_to_bgr(hd, frame.ctypes.data, out.ctypes.data, 3 * w, w, h, 0, 2.0, 0, 2) == BAD_ARG
        assert L.mi_equalize_hist_nv12_to_bgr(hd, frame.ctypes.data, out.ctypes.data, 3 * w, 0, h, 0) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Nv12In(w, h, 1).upload(rand_frames(w, h, 1, 24))
    dst = BgrOut(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"
