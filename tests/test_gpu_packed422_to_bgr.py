"""Packed 4:2:2 frames in (YUY2 / UYVY), interleaved BGR / RGB images out on the GPU: mi_equalize_hist_packed422_to_bgr_batch_dev and
mi_clahe_packed422_to_bgr_batch_dev.  The expected image is tests/packed422_bgr_ref.py: oracle.equalize_hist / oracle.clahe on the
gathered luma (in the call's arithmetic mode), decoded with every row's OWN chroma through oracle.nv12_to_bgr on a row-doubled frame.
Inputs and outputs live in sentinel-filled allocations (padded pitches, gaps between frames, odd bases) and the WHOLE allocation is
compared: every comparison in this file is exact bytes."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import clahe_u8_rungs
import packed422_bgr_ref as ref
from mi_lumaeq import synth, UV_COPY, FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
DISTS = ["D1", "D2", "D3"]
N = 3
FMTS = [FMT_YUY2, FMT_UYVY]
ORDERS = [ORDER_BGR, ORDER_RGB]
# input, as the packed tests: (pitch - 2W, gap between frames, base offset from a 16-byte boundary)
LAYOUTS = [(4, 20, 4), (36, 0, 8), (0, 12, 12)]
# output: name -> how pitch, gap between frames and base offset are made from W.  Between them: base, pitch and frame stride all multiples
# of 16; multiples of 4 only (vector stores at 4-byte alignment); an odd base with pitch 3W + 1 (byte stores); a tight image, whose pitch
# is 2 mod 4 when W % 4 == 2 (byte stores again)
OUT_LAYOUTS = ["aligned16", "aligned4", "odd", "tight"]
WIDE_AND_NARROW = ["aligned4", "odd"]


def stream():
    return torch.cuda.current_stream().cuda_stream


class Batch:
    """n packed frames in one sentinel-filled allocation: rows of 2W bytes at `pitch`, frames `fstride` apart, first frame `off` in."""

    def __init__(self, w, h, n, layout=(0, 0, 0)):
        extra, gap, off = layout
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = 2 * w + extra
        self.fstride = self.pitch * h + gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, frames=None):
        a = np.full(self.total, SENT, np.uint8)
        if frames is not None:
            for k, f in enumerate(frames):
                o = self.off + k * self.fstride
                a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 2 * self.w] = f[:, : 2 * self.w]
        return a

    def upload(self, frames):
        self.buf.copy_(torch.from_numpy(self.image(frames)))
        return self

    def host(self):
        return self.buf.cpu().numpy()

    def kw(self):
        return {"in_pitch": self.pitch, "in_frame": self.fstride}


class BgrOut:
    """n images in one sentinel-filled allocation: rows of 3W bytes at `pitch`, images `fstride` apart, the first `off` bytes in."""

    def __init__(self, w, h, n, layout="aligned16"):
        self.w, self.h, self.n = w, h, n
        if layout == "aligned16":
            self.pitch, gap, self.off = (3 * w + 15) // 16 * 16 + 16, 32, 0
        elif layout == "aligned4":
            self.pitch, gap, self.off = (3 * w + 3) // 4 * 4 + 4, 8, 4
            if self.pitch % 16 == 0:
                self.pitch += 4
        elif layout == "odd":
            self.pitch, gap, self.off = 3 * w + 1, 3, 5
        else:
            self.pitch, gap, self.off = 3 * w, 0, 0
        self.fstride = self.pitch * h + gap
        self.total = self.off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        if layout == "aligned16":
            assert self.pitch % 16 == 0 and self.fstride % 16 == 0
        if layout == "aligned4":
            assert self.pitch % 4 == 0 and self.fstride % 4 == 0 and self.pitch % 16 != 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, images=None):
        a = np.full(self.total, SENT, np.uint8)
        if images is not None:
            for k, im in enumerate(images):
                o = self.off + k * self.fstride
                a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 3 * self.w] = im.reshape(self.h, 3 * self.w)
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def host(self):
        return self.buf.cpu().numpy()

    def same(self, images=None):
        return np.array_equal(self.host(), self.image(images))

    def kw(self):
        return {"out_pitch": self.pitch, "out_frame": self.fstride}


def run(c, op, cfg, src, dst, fmt, order, n=None, st=None):
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if op == "eq":
        c.equalize_hist_packed422_to_bgr_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, fmt, order, **kw)
    else:
        c.clahe_packed422_to_bgr_batch_dev(src.ptr, dst.ptr, src.w, src.h, n, fmt, order, *cfg, **kw)


_planar_cache = {}


def planar_status(c, w, h, n, op, cfg):
    """What the planar form answers for this size / grid pair (0 = accepted)."""
    k = (w, h, n, op, cfg)
    if k not in _planar_cache:
        a = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        status = 0
        try:
            if op == "eq":
                c.equalize_hist_batch_dev(a, b, w, h, n, stream=stream())
            else:
                c.clahe_batch_dev(a, b, w, h, n, *cfg, stream=stream())
        except mi_lumaeq.MiError as e:
            status = e.status
        finally:
            torch.cuda.synchronize()
        _planar_cache[k] = status
    return _planar_cache[k]


_frames, _luma = {}, {}


def frames_of(w, h, fmt, seed=100):
    k = (w, h, fmt, seed)
    if k not in _frames:
        _frames[k] = [synth.packed422_frame(w, h, fmt, d, seed + i) for i, d in enumerate(DISTS)]
    return _frames[k]


def mapped(key, frame, w, fmt, op, cfg, contract=False):
    """The oracle's luma plane of one frame, computed once per (content, op, arithmetic mode) and shared by both orders and all layouts."""
    k = (key, op, cfg, bool(contract))
    if k not in _luma:
        _luma[k] = ref.mapped_luma(ref.luma(frame, w, fmt), op, cfg, contract)
    return _luma[k]


def check_case(c, frames, w, h, fmt, order, op, cfg, li, lo, key, contract=False):
    n = len(frames)
    src = Batch(w, h, n, LAYOUTS[li]).upload(frames)
    dst = BgrOut(w, h, n, lo)
    why = (w, h, fmt, order, op, cfg, li, lo, contract)
    status = planar_status(c, w, h, n, op, cfg)
    if status != 0:                                   # a size / grid pair the planar form refuses: the same status, nothing written
        with pytest.raises(mi_lumaeq.MiError) as e:
            run(c, op, cfg, src, dst, fmt, order)
        torch.cuda.synchronize()
        assert e.value.status == status, (why, e.value.status, status)
        assert dst.same(), "a refused call wrote"
        return
    run(c, op, cfg, src, dst, fmt, order)
    torch.cuda.synchronize()
    want = dst.image([ref.expected(f, w, fmt, order, op, cfg, contract, mapped((key, w, h, fmt, k), f, w, fmt, op, cfg, contract))
                      for k, f in enumerate(frames)])
    got = dst.host()
    assert np.array_equal(got, want), (why, int((got != want).sum()), np.flatnonzero(got != want)[:8])
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


# ---- 1. groups and ragged tails, wide and narrow stores --------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 14, 16, 18, 30, 32, 50, 64])
def test_groups_and_tails(c, w):
    """W = 2, 14: no full 16-column group; 16, 32, 64: exact groups; 18, 30, 50: groups plus a ragged tail of 2, 14 and 2 columns (3 * n
    bytes = 6, 42, 6: whole dwords and a 2-byte rest, either parity of the dword count).  H = 1, 2, 3, 5: single rows and odd heights,
    which no other conversion form accepts.  Both formats x both orders x equalizeHist and CLAHE x all four output layouts (vector,
    dword and byte stores), 3 frames a call.  50, 18, 14 and 30 have W % 4 == 2: the tight layout is then 2 mod 4."""
    for h in (1, 2, 3, 5):
        for fi, fmt in enumerate(FMTS):
            frames = frames_of(w, h, fmt)
            for order in ORDERS:
                for oi, (op, cfg) in enumerate((("eq", None), ("clahe", (2.0, 2, 2)))):
                    for k, lo in enumerate(OUT_LAYOUTS):
                        check_case(c, frames, w, h, fmt, order, op, cfg, (k + oi + fi) % 3, lo, "tails")


# ---- 2. the apply kernel's item loop repeats -----------------------------------------------------------------------------------
def test_apply_loop_repeats(c):
    """64 x 130: a frame is 2 * 64 * 130 = 16640 bytes, so blocks_per_frame gives min(8 * CUs / 3, 16640 / 16384 = 1, rows, 2048) = 1
    workgroup per frame; a row has 64 / 16 = 4 groups, so the workgroup has 130 * 4 = 520 items for 256 lanes: every lane takes two,
    lanes 0..7 a third.  66 x 130 adds a ragged group to every row (5 groups, 650 items)."""
    for w, h in ((64, 130), (66, 130)):
        for fi, fmt in enumerate(FMTS):
            frames = frames_of(w, h, fmt, 300)
            for oi, order in enumerate(ORDERS):
                for k, lo in enumerate(WIDE_AND_NARROW):
                    check_case(c, frames, w, h, fmt, order, "eq", None, (fi + oi + k) % 3, lo, "loop")


# ---- 3. every rung of the CLAHE interpolation ladder -------------------------------------------------------------------------------
# tests/test_gpu_packed422_interp_paths.py derives these: plain float tables, column-segment float tables, quad fallback of a wide
# grid, global LUTs; then the last two again on tiles where the arithmetic mode shows
SHAPES = [(64, 48, 8, 8), (1792, 8, 16, 2), (64, 8, 16, 2), (128, 8, 64, 2), (96, 10, 16, 2), (192, 10, 64, 2)]
MODE_SHAPES = SHAPES[4:]
OPTIONS = [(1, 0), (0, 0), (1, 1), (0, 1)]           # (clahe_float_tables, clahe_fp_contract)


def rung_frame(shape, fmt, k):
    w, h = shape[:2]
    f = synth.packed422_frame(w, h, fmt, DISTS[k], 500 + k)
    if shape in MODE_SHAPES:
        f = f.copy()
        f[:, fmt - 2:2 * w:2] = clahe_u8_rungs.content(w, h, 100 + k)
    return f


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_every_rung(c, shape):
    """Three frames a call; both formats, both orders, clahe_float_tables and clahe_fp_contract both ways, vector and byte stores.  The
    bytes are the reference's in the call's arithmetic mode."""
    w, h, tx, ty = shape
    cfg = (2.0, tx, ty)
    try:
        for fmt in FMTS:
            frames = [rung_frame(shape, fmt, k) for k in range(N)]
            if shape in MODE_SHAPES:                                     # the two arithmetic modes are told apart on this shape
                assert any(not np.array_equal(mapped((("rung", shape), w, h, fmt, k), f, w, fmt, "clahe", cfg, 0),
                                              mapped((("rung", shape), w, h, fmt, k), f, w, fmt, "clahe", cfg, 1))
                           for k, f in enumerate(frames)), (shape, "both modes give the same bytes")
            for float_tables, contract in OPTIONS:
                c.set_option("clahe_float_tables", float_tables)
                c.set_option("clahe_fp_contract", contract)
                for oi, order in enumerate(ORDERS):
                    for k, lo in enumerate(WIDE_AND_NARROW):
                        check_case(c, frames, w, h, fmt, order, "clahe", cfg, (oi + k) % 3, lo, ("rung", shape), contract)
    finally:
        c.set_option("clahe_float_tables", 1)
        c.set_option("clahe_fp_contract", 0)


# ---- 4. tile grids that do not divide the frame ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,cfg", [(50, 13, (2.0, 3, 5)), (50, 13, (0.0, 3, 5)), (62, 47, (3.0, 4, 4))])
def test_non_dividing_grids(c, w, h, cfg):
    """50 x 13 at 3 x 5: tiles of 17 x 3 on a frame padded to 51 x 15 (REFLECT_101), tiles that start on odd columns, an odd height;
    clip_limit 0.0 is the unclipped histogram.  62 x 47 at 4 x 4: tiles of 16 x 12."""
    for fi, fmt in enumerate(FMTS):
        frames = frames_of(w, h, fmt, 400)
        for oi, order in enumerate(ORDERS):
            for k, lo in enumerate(OUT_LAYOUTS):
                check_case(c, frames, w, h, fmt, order, "clahe", cfg, (fi + oi + k) % 3, lo, "grids")


# ---- 5. every row keeps its own chroma -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_per_row_chroma(c, fmt):
    """Even rows with strong chroma, odd rows with chroma 128 (the frame of the ABI test), through both ops: the result is the 4:2:2
    reference and differs from what packed -> NV12 (MI_UV_COPY) followed by cvt_color_420(YUV2BGR_NV12) returns on the same frame."""
    w, h = 48, 6
    frame = ref.alternating_chroma_frame(w, h, fmt, 11)
    src = Batch(w, h, 1, LAYOUTS[0]).upload([frame])
    nv12 = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")
    two = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
    for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2))):
        dst = BgrOut(w, h, 1, "aligned4")
        run(c, op, cfg, src, dst, fmt, ORDER_BGR)
        if op == "eq":
            c.equalize_hist_packed422_to_nv12_batch_dev(src.ptr, nv12, None, w, h, 1, fmt, UV_COPY, stream=stream(), **src.kw())
        else:
            c.clahe_packed422_to_nv12_batch_dev(src.ptr, nv12, None, w, h, 1, fmt, UV_COPY, *cfg, stream=stream(), **src.kw())
        c.cvt_color_420_batch_dev(nv12, two, w, h, 1, mi_lumaeq.COLOR_YUV2BGR_NV12, stream=stream())
        torch.cuda.synchronize()
        want = ref.expected(frame, w, fmt, ORDER_BGR, op, cfg)
        assert dst.same([want]), (fmt, op)
        two_h = two.cpu().numpy()
        assert not np.array_equal(two_h, want), (fmt, op, "the two-call route kept every row's chroma?")
        assert not np.array_equal(two_h[0::2], want[0::2]) and not np.array_equal(two_h[1::2], want[1::2])


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    w, h, n = 64, 47, 2
    frames = frames_of(w, h, FMT_YUY2, 700)[:n]
    src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
    dst = BgrOut(w, h, n, "aligned4")
    L, hd = c._L, c._h
    ip, op_ = src.ptr, dst.ptr
    base = dict(i=ip, ipitch=src.pitch, ifs=src.fstride, o=op_, opitch=dst.pitch, ofs=dst.fstride, w=w, h=h, n=n, fmt=FMT_YUY2,
                order=ORDER_BGR)

    def args(kw):
        a = dict(base)
        a.update(kw)
        return (hd, a["i"], a["ipitch"], a["ifs"], a["o"], a["opitch"], a["ofs"], a["w"], a["h"], a["n"], a["fmt"], a["order"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_bgr_batch_dev(*args(kw), stream())

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_bgr_batch_dev(*args(kw), 2.0, tx, ty, stream())
    bad = [dict(i=None), dict(o=None),                                                            # null frame pointers
           dict(w=63), dict(w=63, h=0), dict(w=63, n=0), dict(w=1),                               # odd width, also next to a zero size
           dict(w=-2), dict(h=-2), dict(h=-1), dict(n=-1),                                        # negative sizes
           dict(ipitch=2 * w - 4), dict(opitch=3 * w - 1), dict(opitch=3 * w - 4),                # pitches too small
           dict(i=ip + 2), dict(i=ip + 1), dict(ipitch=2 * w + 2), dict(ifs=src.fstride + 2), dict(ifs=src.fstride + 1),   # input not multiples of 4
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(order=2), dict(order=-1),     # format, order
           dict(o=ip)]                                                                            # no in-place form
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert cl(tx, ty) == BAD_ARG
    # zero sizes: MI_OK, nothing written
    for kw in (dict(w=0), dict(h=0), dict(n=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    torch.cuda.synchronize()
    assert dst.same(), "a refused or empty call wrote"
    assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
    # the output side has no alignment rule: an odd pointer, pitch and frame stride are accepted (and an odd height)
    dst_odd = BgrOut(w, h, n, "odd")
    run(c, "eq", None, src, dst_odd, FMT_YUY2, ORDER_BGR)
    torch.cuda.synchronize()
    assert dst_odd.same([ref.expected(f, w, FMT_YUY2, ORDER_BGR, "eq") for f in frames])
    assert dst.same(), "a call on other buffers wrote"
    # and the context still works
    run(c, "clahe", (2.0, 8, 8), src, dst, FMT_YUY2, ORDER_RGB)
    torch.cuda.synchronize()
    assert dst.same([ref.expected(f, w, FMT_YUY2, ORDER_RGB, "clahe", (2.0, 8, 8)) for f in frames])


def test_sizes_the_planar_forms_refuse(c):
    """A tile grid the planar CLAHE refuses gives its status here, nothing written (check_case compares the statuses)."""
    w, h = 64, 8
    frames = frames_of(w, h, FMT_UYVY, 720)
    cfg = (2.0, 512, 256)                                                # 131072 tiles: more than a grid dimension holds
    assert planar_status(c, w, h, N, "clahe", cfg) != 0
    check_case(c, frames, w, h, FMT_UYVY, ORDER_BGR, "clahe", cfg, 0, "aligned4", "refused")


# ---- 7. streams, profiling, the pipe -----------------------------------------------------------------------------------------------
def test_streams(c):
    w, h = 64, 9
    frames = frames_of(w, h, FMT_UYVY, 900)
    src = Batch(w, h, N, LAYOUTS[1]).upload(frames)
    dst = BgrOut(w, h, N, "aligned16")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for st in (side.cuda_stream, mi_lumaeq.STREAM_CTX):
        for op, cfg in (("eq", None), ("clahe", (2.0, 4, 3))):
            dst.clear()
            torch.cuda.synchronize()
            run(c, op, cfg, src, dst, FMT_UYVY, ORDER_RGB, st=st)
            if st == side.cuda_stream:
                side.synchronize()
            else:
                c.synchronize(mi_lumaeq.STREAM_CTX)
            assert dst.same([ref.expected(f, w, FMT_UYVY, ORDER_RGB, op, cfg) for f in frames]), (st, op)


def test_launch_accounting():
    w, h = 64, 48
    frames = frames_of(w, h, FMT_YUY2, 1000)
    src = Batch(w, h, N, LAYOUTS[0]).upload(frames)
    dst = BgrOut(w, h, N, "aligned4")
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for order in ORDERS:
            c.profile_read(reset=True)
            run(c, "eq", None, src, dst, FMT_YUY2, order)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            assert len(prof) == 10
            for k in mi_lumaeq.KERNEL_NAMES:
                want = 1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0
                assert prof[k]["launches"] == want, (order, k, prof[k])
            assert dst.same([ref.expected(f, w, FMT_YUY2, order, "eq") for f in frames])
        for cfg in ((2.0, 8, 8), (2.0, 64, 2)):
            assert planar_status(c, w, h, N, "clahe", cfg) == 0
            c.profile_read(reset=True)
            run(c, "clahe", cfg, src, dst, FMT_YUY2, ORDER_BGR)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            for k in ("equalize_fused_kernel", "fused_finish_kernel", "color_kernel", "analyze_diff_kernel", "hist_partial_kernel",
                      "equalize_lut_kernel", "lut_apply_kernel"):
                assert prof[k]["launches"] == 0, (cfg, k, prof[k])
            assert prof["tile_hist_kernel"]["launches"] == 1 and prof["clahe_interp_kernel"]["launches"] == 1, (cfg, prof)
            assert prof["tile_lut_kernel"]["launches"] in (0, 1)
            assert dst.same([ref.expected(f, w, FMT_YUY2, ORDER_BGR, "clahe", cfg) for f in frames])
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Batch(w, h, 1).upload(frames_of(w, h, FMT_YUY2, 1100)[:1])
    dst = BgrOut(w, h, 1, "tight")
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, cfg, src, dst, FMT_YUY2, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same(), "a refused call wrote"
