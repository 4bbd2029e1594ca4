"""8-bit 4:2:0 frames whose two sides say where their planes lie (mi_*_yuv420*) on the GPU: I420 / YV12 / NV12 in, any of them out.
Expected bytes: oracle.equalize_hist / oracle.clahe on the Y plane, the chroma samples carried over by numpy slicing (MI_UV_COPY) or 128
(MI_UV_FILL128).  Planes hold full-range random bytes, U and V drawn independently, so an identity map, a swapped U / V order or a
mixed-up row cannot pass.  Every side of a call lives in a sentinel-filled allocation with 64 guard bytes and the WHOLE allocation is
compared, input and output: every comparison in this file is exact.

How many workgroups yuv420_chroma_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  yuv420_chroma_dev takes B = blocks_per_frame(bytes, H/2 rows, frames of the chunk,
2048) with bytes = W*H (copy: W*H/2 read and W*H/2 written per frame) or W*H/2 (fill), and blocks_per_frame never returns more than
max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which only lowers it.  So
B <= max(1, floor(W*H / 16384)),  B <= H/2,  and the 256 lanes of a workgroup step through a frame by stride = 256 * B items.  A layout
change on the vector path has W/32 * H/2 items (one chroma row x 32 output pixels), four of them in flight per lane: a lane takes a second
item when items > stride and a second round of its loop when items > 4 * stride; (row, slot) advance by (stride / slots, stride % slots)
with a wrap when slot >= slots = W/32.  On the byte path the items are the W/2 * H/2 sample pairs, one per step, walked the same way
with W/2 in the place of slots."""
import ctypes
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, UV_COPY, UV_FILL128, CHROMA_INTERLEAVED, CHROMA_PLANAR, Yuv420Planes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)
PAIRS = [("i420", "i420"), ("i420", "nv12"), ("nv12", "i420"), ("nv12", "nv12")]


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def content(w, h, n, seed):
    """n frames as (Y, U, V) arrays; computed once per shape and seed, never modified."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        planes = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
                  rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))
        for p in planes:
            p.setflags(write=False)
        out.append(planes)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def luma(w, h, n, seed, op):
    kind, cfg = op
    out = []
    for y, _, _ in content(w, h, n, seed):
        r = oracle.equalize_hist(y) if kind == "eq" else oracle.clahe(y, *cfg)
        r.setflags(write=False)
        out.append(r)
    return tuple(out)


def expected(w, h, n, seed, op, uv_mode):
    """The (Y, U, V) planes the call must produce for content(w, h, n, seed)."""
    fill = np.full((h // 2, w // 2), 128, np.uint8)
    return [(yy, u, v) if uv_mode == UV_COPY else (yy, fill, fill) for yy, (_, u, v) in zip(luma(w, h, n, seed, op), content(w, h, n, seed))]


class Side:
    """n frames of one side of a call in one sentinel-filled allocation (device memory, or host memory with dev=False).  A frame: the Y
    plane (H rows at y_pitch), gap0 bytes, the first chroma plane, [gap1 bytes, the second chroma plane,] frame_gap bytes; the first
    frame starts `off` bytes into the allocation.  fmt "nv12": one plane of W-byte rows; "i420": U then V, rows of W/2 bytes; "yv12": V
    then U.  c0 is always the U plane's address."""

    def __init__(self, w, h, n, fmt, y_pitch=None, c_pitch=None, gap0=0, gap1=0, frame_gap=0, off=0, dev=True):
        self.w, self.h, self.n, self.fmt, self.off = w, h, n, fmt, off
        self.planar = fmt != "nv12"
        self.row = w // 2 if self.planar else w
        self.y_pitch, self.c_pitch = y_pitch or w, c_pitch or self.row
        self.a_off = self.y_pitch * h + gap0
        self.b_off = self.a_off + self.c_pitch * (h // 2) + gap1
        self.fstride = (self.b_off + self.c_pitch * (h // 2) if self.planar else self.b_off - gap1) + frame_gap
        self.total = off + self.fstride * n + 64
        if dev:
            self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
            self.base = self.buf.data_ptr()
        else:
            self.raw = np.full(self.total + 16, SENT, np.uint8)          # the allocation proper starts at a multiple of 16 in it
            shift = (-self.raw.ctypes.data) % 16
            self.buf = self.raw[shift: shift + self.total]
            self.base = self.buf.ctypes.data
        assert self.base % 16 == 0
        self.dev = dev

    def offsets(self):
        """offsets of Y, c0 (U or UV) and c1 (V) of frame 0 in the allocation"""
        u, v = (self.a_off, self.b_off) if self.fmt != "yv12" else (self.b_off, self.a_off)
        return self.off, self.off + u, (self.off + v) if self.planar else None

    def planes(self, **over):
        y, c0, c1 = self.offsets()
        d = dict(y=self.base + y, y_pitch=self.y_pitch, c0=self.base + c0, c1=None if c1 is None else self.base + c1,
                 c_pitch=self.c_pitch, frame_stride=self.fstride, chroma=CHROMA_PLANAR if self.planar else CHROMA_INTERLEAVED)
        d.update(over)
        return Yuv420Planes(d["y"], d["y_pitch"], d["c0"], d["c1"], d["c_pitch"], d["frame_stride"], d["chroma"])

    def chroma_terms(self):
        """what the vector rule looks at on this side, relative to the (16-byte aligned) allocation"""
        _, c0, c1 = self.offsets()
        t = {"c0": c0, "c_pitch": self.c_pitch, "frame_stride": self.fstride}
        if c1 is not None:
            t["c1"] = c1
        return t

    def image(self, frames=None, chroma=True, luma=True):
        a = np.full(self.total, SENT, np.uint8)
        w, h = self.w, self.h
        for k, (y, u, v) in enumerate(frames or []):
            yo, c0, c1 = (o if o is None else o + k * self.fstride for o in self.offsets())
            for r in range(h if luma else 0):
                a[yo + r * self.y_pitch: yo + r * self.y_pitch + w] = y[r]
            if not chroma:
                continue
            for r in range(h // 2):
                if self.planar:
                    a[c0 + r * self.c_pitch: c0 + r * self.c_pitch + w // 2] = u[r]
                    a[c1 + r * self.c_pitch: c1 + r * self.c_pitch + w // 2] = v[r]
                else:
                    a[c0 + r * self.c_pitch: c0 + r * self.c_pitch + w: 2] = u[r]
                    a[c0 + r * self.c_pitch + 1: c0 + r * self.c_pitch + w: 2] = v[r]
        return a

    def upload(self, frames):
        img = self.image(frames)
        if self.dev:
            self.buf.copy_(xfer.to_device(img))
        else:
            self.buf[:] = img
        return self

    def clear(self):
        if self.dev:
            self.buf.fill_(SENT)
        else:
            self.buf[:] = SENT

    def host(self):
        return xfer.to_host(self.buf) if self.dev else self.buf.copy()

    def same(self, frames=None, chroma=True, luma=True):
        got, want = self.host(), self.image(frames, chroma, luma)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]


def run(c, op, src, dst, uv_mode, n=None, st=None, a=None, b=None):
    kind, cfg = op
    a, b = a or src.planes(), b or dst.planes()
    n = src.n if n is None else n
    st = stream() if st is None else st
    if kind == "eq":
        c.equalize_hist_yuv420_batch_dev(a, b, src.w, src.h, n, uv_mode, stream=st)
    else:
        c.clahe_yuv420_batch_dev(a, b, src.w, src.h, n, uv_mode, *cfg, stream=st)


def takes_vector_path(src, dst, uv_mode):
    """The header's rule, restated: a fill and a same-layout move always count as 16-byte launches; a layout change does when
    W % 32 == 0 and every chroma pointer, both c_pitch and both frame_stride are multiples of 16."""
    if uv_mode == UV_FILL128 or src.planar == dst.planar:
        return True
    return src.w % 32 == 0 and all(v % 16 == 0 for s in (src, dst) for v in s.chroma_terms().values())


def stats(c):
    return c.get_stat("yuv420_chroma_vec"), c.get_stat("yuv420_chroma_bytes")


def check(c, w, h, n, seed, op, uv_mode, src, dst, planar_y=None):
    """One call on the uploaded content: the whole output allocation is the oracle's image of it, the whole input allocation is what
    was uploaded, the counter of the path the rule names moved by one.  planar_y: an allocation laid out like dst into which
    mi_*_u8_batch_dev maps the same Y planes -- the same bytes."""
    frames = content(w, h, n, seed)
    src.upload(frames)
    dst.clear()
    before = stats(c)
    run(c, op, src, dst, uv_mode)
    torch.cuda.synchronize()
    want = expected(w, h, n, seed, op, uv_mode)
    ok, nbad, where = dst.same(want)
    assert ok, (w, h, src.fmt, dst.fmt, op, uv_mode, nbad, where)
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"
    vec = takes_vector_path(src, dst, uv_mode)
    assert stats(c) == (before[0] + vec, before[1] + (not vec)), (src.fmt, dst.fmt, uv_mode, vec)
    if planar_y is not None:
        planar_y.clear()
        kw = dict(src_step=src.y_pitch, src_frame=src.fstride, dst_step=planar_y.y_pitch, dst_frame=planar_y.fstride, stream=stream())
        ys, yd = src.base + src.offsets()[0], planar_y.base + planar_y.offsets()[0]
        if op[0] == "eq":
            c.equalize_hist_batch_dev(ys, yd, w, h, n, **kw)
        else:
            c.clahe_batch_dev(ys, yd, w, h, n, *op[1], **kw)
        torch.cuda.synchronize()
        assert planar_y.same(want, chroma=False)[0], "the Y plane is not what the planar form writes for the same layout"


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


def pitched16(fmt, w):
    """every pitch + 16, gaps between planes and frames, everything a multiple of 16"""
    row = w if fmt == "nv12" else w // 2
    return dict(y_pitch=w + 16, c_pitch=row + 16, gap0=16, gap1=32, frame_gap=48, off=16)


def pitched1(fmt, w):
    row = w if fmt == "nv12" else w // 2
    return dict(y_pitch=w + 1, c_pitch=row + 1)


def tight(fmt, w):
    return {}


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
PARITY = [
    # id, W, H, layout of both sides, the ops (CLAHE grids that divide the frame and that do not)
    ("2x2", 2, 2, tight, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 2))]),                       # one sample per chroma plane
    ("6x4", 6, 4, tight, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 4, 3))]),                       # W/2 = 3: odd planar rows, byte path
    ("32x4", 32, 4, tight, [EQ, ("clahe", (2.0, 2, 2)), ("clahe", (3.0, 3, 3))]),                     # the first vector shape: one item a row
    ("34x6", 34, 6, tight, [EQ, ("clahe", (2.0, 2, 3)), ("clahe", (2.0, 4, 4))]),                     # W % 32 != 0: byte path
    ("64x6-pitched16", 64, 6, pitched16, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 5, 4))]),       # padding and gaps, vector path
    ("64x6-pitched1", 64, 6, pitched1, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 5, 4))]),         # pitches + 1: byte path
]


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("name,w,h,lay,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, lay, ops, pair):
    n = 3
    src, dst = Side(w, h, n, pair[0], **lay(pair[0], w)), Side(w, h, n, pair[1], **lay(pair[1], w))
    py = Side(w, h, n, pair[1], **lay(pair[1], w))
    if pair[0] != pair[1]:
        assert takes_vector_path(src, dst, UV_COPY) == (name in ("32x4", "64x6-pitched16"))
    for op in ops:
        for uv_mode in UV_MODES:
            check(c, w, h, n, 51, op, uv_mode, src, dst, planar_y=py)


# ---- 2. YV12 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [("yv12", "nv12"), ("nv12", "yv12"), ("yv12", "i420"), ("i420", "yv12"), ("yv12", "yv12")],
                         ids=lambda p: "-".join(p))
@pytest.mark.parametrize("w,h", [(64, 6), (6, 4)])
def test_yv12_is_i420_with_the_chroma_addresses_exchanged(c, w, h, pair):
    """c0 is always U: a YV12 side passes its second chroma plane as c0.  U and V hold different bytes, a swap cannot pass."""
    n = 2
    u, v = content(w, h, n, 52)[0][1:]
    assert not np.array_equal(u, v)
    a, b = Side(w, h, n, "yv12"), Side(w, h, n, "i420")
    assert a.offsets()[1] == b.offsets()[2] and a.offsets()[2] == b.offsets()[1]
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        check(c, w, h, n, 52, op, UV_COPY, Side(w, h, n, pair[0]), Side(w, h, n, pair[1]))


# ---- 3. one alignment term at a time ---------------------------------------------------------------------------------------------
ONE_TERM = [
    # the side and term broken, its layout (from pitched16: 64 x 6, H/2 = 3 chroma rows)
    ("in", "c0", dict(gap0=17, gap1=31)),
    ("in", "c1", dict(gap1=33, frame_gap=47)),
    ("in", "c_pitch", dict(c_pitch=49, gap1=29, frame_gap=45)),            # 3 rows: each plane grows by 3
    ("in", "frame_stride", dict(frame_gap=49)),
    ("out", "c0", dict(gap0=17, gap1=31)),
    ("out", "c1", dict(gap1=33, frame_gap=47)),
    ("out", "c_pitch", dict(c_pitch=49, gap1=29, frame_gap=45)),
    ("out", "frame_stride", dict(frame_gap=49)),
]


@pytest.mark.parametrize("side,term,lay", ONE_TERM, ids=[f"{t[0]}-{t[1]}" for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, side, term, lay):
    """Exactly one chroma term of the planar side is no multiple of 16: the byte path, the same bytes, the same untouched guards."""
    w, h, n = 64, 6, 2
    for pair in (("i420", "nv12"), ("nv12", "i420")):
        planar_side = "in" if pair[0] == "i420" else "out"
        if planar_side != side and term == "c1":
            continue                                                                    # an interleaved side has no c1
        lays = [pitched16(pair[0], w), pitched16(pair[1], w)]
        k = 0 if side == "in" else 1
        if planar_side == side:
            lays[k].update(lay)
        elif term == "c0":
            lays[k].update(gap0=17, frame_gap=47)
        elif term == "c_pitch":
            lays[k].update(c_pitch=81, frame_gap=45)
        else:
            lays[k].update(frame_gap=49)
        src, dst = Side(w, h, n, pair[0], **lays[0]), Side(w, h, n, pair[1], **lays[1])
        broken = sorted(f"{s}-{t}" for s, sd in (("in", src), ("out", dst)) for t, v in sd.chroma_terms().items() if v % 16)
        assert broken == [f"{side}-{term}"], broken
        assert not takes_vector_path(src, dst, UV_COPY)
        check(c, w, h, n, 53, EQ, UV_COPY, src, dst)
        check(c, w, h, n, 53, ("clahe", (2.0, 2, 2)), UV_COPY, src, dst)


@pytest.mark.parametrize("pair", [("i420", "nv12"), ("nv12", "i420")], ids=lambda p: "-".join(p))
def test_a_misaligned_y_leaves_the_chroma_on_the_vector_path(c, pair):
    w, h, n = 64, 6, 2
    yb = (w + 17) * h                                                                   # Y at an odd address with an odd pitch ...
    gap0 = -(17 + yb) % 16                                                              # ... the chroma planes and the frame stride
    lays = [dict(pitched16(f, w), off=17, y_pitch=w + 17, gap0=gap0, frame_gap=48 + -(yb + gap0) % 16) for f in pair]   # multiples of 16
    src, dst = Side(w, h, n, pair[0], **lays[0]), Side(w, h, n, pair[1], **lays[1])
    for s in (src, dst):
        assert s.offsets()[0] % 16 and s.y_pitch % 16
    assert takes_vector_path(src, dst, UV_COPY)
    check(c, w, h, n, 54, EQ, UV_COPY, src, dst)


# ---- 4. loops past their first step ----------------------------------------------------------------------------------------------
LOOP_SHAPES = [
    # id, W, H, n, layout, vector path, items > 256 * min(bounds) * this (see the module docstring)
    # W*H/16384 = 1.02: B = 1, stride 256; slots 2, items 260: lanes 0..3 take a second item
    ("64x260", 64, 260, 1, tight, True, 1),
    # W*H/16384 = 1.05: B = 1, stride 256; slots 3, items 270, drow 85, dslot 1: the slot wraps on the second item of lanes with slot 2
    ("96x180", 96, 180, 1, pitched16, True, 1),
    # W*H/16384 = 16 but H/2 = 2 rows: B <= 2, stride <= 512; slots 2048, items 4096 > 4 * 512: a second round of the four-deep loop
    ("65536x4", 65536, 4, 1, tight, True, 4),
    # W*H/16384 = 4: B <= 4 (2 or more on a device with enough CUs; not asserted), slots 8, items 1024
    ("256x256", 256, 256, 2, pitched16, True, 0),
    # byte path, W*H/16384 = 0.07: B = 1; 17 x 16 = 272 pairs for 256 lanes, drow 15, dx 1: a second step that wraps
    ("34x32", 34, 32, 2, tight, False, 1),
    # byte path with B <= 4: 128 x 128 = 16384 pairs, stride <= 1024: sixteen steps or more
    ("256x256-pitched1", 256, 256, 1, pitched1, False, 1),
]


@pytest.mark.parametrize("pair", [("i420", "nv12"), ("nv12", "i420")], ids=lambda p: "-".join(p))
@pytest.mark.parametrize("name,w,h,n,lay,vec,rounds", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, lay, vec, rounds, pair):
    src, dst = Side(w, h, n, pair[0], **lay(pair[0], w)), Side(w, h, n, pair[1], **lay(pair[1], w))
    assert takes_vector_path(src, dst, UV_COPY) == vec
    bound = min(max(1, w * h // 16384), h // 2)
    items = (w // 32 if vec else w // 2) * (h // 2)
    assert items > 256 * bound * rounds, "the shape would not loop"
    check(c, w, h, n, 55, EQ, UV_COPY, src, dst)
    if w <= 256:
        check(c, w, h, n, 55, ("clahe", (2.0, 2, 2)), UV_COPY, src, dst)


def test_same_layout_moves_and_fills_past_one_workgroup(c):
    """uv_rows / uv_flat under the new kernel on more than one workgroup a frame: pitched and tight, both layouts, copy and fill."""
    w, h, n = 256, 256, 2
    for fmt in ("i420", "nv12"):
        for lay in (tight, pitched16, pitched1):
            for uv_mode in UV_MODES:
                check(c, w, h, n, 56, EQ, uv_mode, Side(w, h, n, fmt, **lay(fmt, w)), Side(w, h, n, fmt, **lay(fmt, w)))


# ---- 5. in place -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_in_place_on_the_same_planes(c, fmt, op):
    """The same planes on both sides: Y equalized, the chroma bytes untouched under COPY (no chroma launch: neither counter moves),
    128 under FILL128."""
    w, h, n = 64, 6, 3
    frames = content(w, h, n, 57)
    for lay in (tight, pitched16, pitched1):
        io = Side(w, h, n, fmt, **lay(fmt, w))
        for uv_mode in UV_MODES:
            io.upload(frames)
            before = stats(c)
            run(c, op, io, io, uv_mode)
            torch.cuda.synchronize()
            ok, nbad, where = io.same(expected(w, h, n, 57, op, uv_mode))
            assert ok, (fmt, op, uv_mode, nbad, where)
            assert stats(c) == ((before[0] + 1, before[1]) if uv_mode == UV_FILL128 else before)


def same_stride_pair(w, h, n, fa, fb):
    """two pitched sides whose frames lie equally far apart: what a plane shared between the two sides of a call needs"""
    la, lb = pitched16(fa, w), pitched16(fb, w)
    m = max(Side(w, h, n, fa, **la).fstride, Side(w, h, n, fb, **lb).fstride)
    la["frame_gap"] += m - Side(w, h, n, fa, **la).fstride
    lb["frame_gap"] += m - Side(w, h, n, fb, **lb).fstride
    a, b = Side(w, h, n, fa, **la), Side(w, h, n, fb, **lb)
    assert a.fstride == b.fstride
    return a, b


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_y_in_place_with_the_chroma_elsewhere_and_the_other_way_round(c, pair):
    w, h, n = 64, 6, 2
    frames = content(w, h, n, 58)
    op = ("clahe", (2.0, 2, 2))
    want = expected(w, h, n, 58, op, UV_COPY)
    src, dst = same_stride_pair(w, h, n, *pair)
    # Y in place, the chroma carried into the other allocation
    src.upload(frames)
    dst.clear()
    s = src.planes()
    run(c, op, src, dst, UV_COPY, b=dst.planes(y=s.y, y_pitch=s.y_pitch))
    torch.cuda.synchronize()
    assert src.same(want)[0], "Y in place: the input's Y is equalized, its chroma untouched"
    assert dst.same(want, luma=False)[0], "the chroma went into the other allocation, nothing else of it was written"
    if pair[0] == pair[1]:
        # the chroma in place, Y into the other allocation: nothing to move, no chroma launch
        src.upload(frames)
        dst.clear()
        before = stats(c)
        run(c, op, src, dst, UV_COPY, b=src.planes(y=dst.planes().y, y_pitch=dst.y_pitch))
        torch.cuda.synchronize()
        assert stats(c) == before
        assert np.array_equal(src.host(), src.image(frames))
        assert dst.same(want, chroma=False)[0]


# ---- 6. FILL128 without input chroma ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_fill128_with_null_input_chroma_pointers(c, pair):
    w, h, n = 34, 6, 2
    src, dst = Side(w, h, n, pair[0]), Side(w, h, n, pair[1], **pitched1(pair[1], w))
    frames = content(w, h, n, 59)
    src.upload(frames)
    for op in (EQ, ("clahe", (2.0, 2, 3))):
        dst.clear()
        run(c, op, src, dst, UV_FILL128, a=src.planes(c0=None, c1=None, c_pitch=0))
        torch.cuda.synchronize()
        assert dst.same(expected(w, h, n, 59, op, UV_FILL128))[0], (pair, op)
    assert np.array_equal(src.host(), src.image(frames))


# ---- 7. identity with the library's own pieces -----------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
@pytest.mark.parametrize("uv_mode", UV_MODES)
def test_interleaved_to_interleaved_equals_the_nv12_batch_form(c, op, uv_mode):
    w, h, n = 64, 32, 3
    frames = content(w, h, n, 60)
    src, dst, ref = Side(w, h, n, "nv12").upload(frames), Side(w, h, n, "nv12"), Side(w, h, n, "nv12")
    run(c, op, src, dst, uv_mode)
    if op is EQ:
        c.equalize_hist_nv12_batch_dev(src.base, ref.base, w, h, n, uv_mode, stream=stream())
    else:
        c.clahe_nv12_batch_dev(src.base, ref.base, w, h, n, uv_mode, *op[1], stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(dst.buf, ref.buf)
    assert dst.same(expected(w, h, n, 60, op, uv_mode))[0]


# ---- 8. chunking -----------------------------------------------------------------------------------------------------------------
def test_chunk_size_is_256():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "yuv420.inc.hpp").read_text()
    assert int(re.search(r"constexpr\s+int\s+kYuv420FramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1)) == 256


@pytest.mark.parametrize("w,h", [(2, 2), (32, 2)])
@pytest.mark.parametrize("pair", [("i420", "nv12"), ("nv12", "i420"), ("i420", "i420")], ids=lambda p: "-".join(p))
def test_chunking(c, w, h, pair):
    """Two frames past the chunk: two chroma launches, the second of two frames; every frame distinct, every frame checked."""
    n = 258
    check(c, w, h, n, 61, EQ, UV_COPY, Side(w, h, n, pair[0]), Side(w, h, n, pair[1]))
    check(c, w, h, n, 61, ("clahe", (2.0, 1, 1)), UV_COPY, Side(w, h, n, pair[0]), Side(w, h, n, pair[1]))


# ---- 9. errors, zero sizes -------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    frames = content(w, h, n, 62)
    src = Side(w, h, n, "i420", **pitched16("i420", w)).upload(frames)
    dst = Side(w, h, n, "nv12", **pitched16("nv12", w))
    pdst = Side(w, h, n, "i420", **pitched16("i420", w))          # a planar output with src's layout, for the in-place cases
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)

        def call(a, b, ctx=hd, w=w, h=h, n=n, uvm=UV_COPY, tiles=None):
            pa = None if a is None else ctypes.byref(a)
            pb = None if b is None else ctypes.byref(b)
            if tiles is None:
                return L.mi_equalize_hist_yuv420_batch_dev(ctx, pa, pb, w, h, n, uvm, stream())
            return L.mi_clahe_yuv420_batch_dev(ctx, pa, pb, w, h, n, uvm, 2.0, tiles[0], tiles[1], stream())

        def both(a, b, **kw):
            return call(a, b, **kw), call(a, b, tiles=(2, 2), **kw)
        A, B, P = src.planes, dst.planes, pdst.planes
        s = A()
        bad = [
            (A(), B(), dict(ctx=None)), (None, B(), {}), (A(), None, {}),                                  # a null ctx, in or out
            (A(y=None), B(), {}), (A(), B(y=None), {}),                                                    # a null y
            (A(), B(c0=None), {}), (A(), P(c1=None), {}),                                                  # a null out->c0; c1 of a PLANAR output
            (A(c0=None), B(), {}), (A(c1=None), B(), {}), (B(c0=None), P(), {}),                           # input chroma COPY needs
            (A(chroma=2), B(), {}), (A(), B(chroma=-1), {}), (A(chroma=2), B(), dict(uvm=UV_FILL128)),     # a chroma other than the two
            (A(), B(), dict(uvm=2)), (A(), B(), dict(uvm=-1)),                                             # a bad uv_mode
            (A(), B(), dict(w=-2)), (A(), B(), dict(h=-2)), (A(), B(), dict(n=-1)),                        # negative sizes
            (A(), B(), dict(w=31)), (A(), B(), dict(h=15)), (A(), B(), dict(w=31, h=0)), (A(), B(), dict(h=15, w=0)),
            (A(), B(), dict(h=15, n=0)),                                                                   # odd sizes, also next to a 0
            (A(y_pitch=w - 1), B(), {}), (A(), B(y_pitch=w - 1), {}),                                      # y_pitch < W
            (A(c_pitch=w // 2 - 1), B(), {}), (A(), B(c_pitch=w - 1), {}), (A(), P(c_pitch=w // 2 - 1), {}),   # c_pitch below its row
            (A(), B(c0=B().y), {}), (A(), P(c1=P().c0), {}), (A(), P(c1=P().y), {}),                       # two equal output pointers
            (A(), B(y=s.c0), {}), (A(), B(c0=s.y), {}), (A(), B(c0=s.c1), {}), (A(), P(c0=s.c1, c1=s.c0), {}),   # out == in, another plane
            (A(), B(y=s.y), {}),                                                                           # Y at in's address: another stride
            (A(), P(y=s.y, y_pitch=s.y_pitch + 16), {}),                                                   # ... another pitch
            (A(), P(c0=s.c0, frame_stride=s.frame_stride + 16), {}),                                       # U at in's address: another stride
            (A(), B(c0=s.c0), {}),                                                                         # ... another layout
            (A(), P(c0=s.c0, c_pitch=s.c_pitch + 16), {}),                                                 # ... another pitch
        ]
        assert B().y_pitch == s.y_pitch and B().frame_stride != s.frame_stride and P().frame_stride == s.frame_stride
        for a, b, kw in bad:
            assert both(a, b, **kw) == (BAD_ARG, BAD_ARG), (kw, None if a is None else bytes(a), None if b is None else bytes(b))
        for tiles in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert call(A(), B(), tiles=tiles) == BAD_ARG, tiles
            assert call(A(), B(), tiles=tiles, n=0) == BAD_ARG, tiles
        # zero sizes: MI_OK, nothing written
        for kw in (dict(w=0), dict(h=0), dict(n=0)):
            assert both(A(), B(), **kw) == (0, 0), kw
        # sizes and tile grids the planar forms refuse: their status
        bw = (1 << 24) + 2
        planar = L.mi_clahe_u8_batch_dev(hd, s.y, 1 << 25, 1 << 26, B().y, 1 << 25, 1 << 26, bw, 2, 1, 2.0, 2, 2, stream())
        big = (A(y_pitch=1 << 25, c_pitch=1 << 25), B(y_pitch=1 << 25, c_pitch=1 << 25))
        assert planar == UNSUPPORTED and both(*big, w=bw, h=2) == (planar, planar)
        planar = L.mi_clahe_u8_batch_dev(hd, s.y, s.y_pitch, s.frame_stride, B().y, dst.y_pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and call(A(), B(), tiles=(2048, 1024)) == planar
        torch.cuda.synchronize()
        assert dst.same()[0] and pdst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0, 0)
        c.set_profiling(0)
        # and the context still works
        check(c, w, h, n, 62, EQ, UV_COPY, src, dst)


def test_launch_contract():
    """The chroma is one MI_K_LUT_APPLY launch on top of what the planar form launches for the same Y planes; none for an in-place copy."""
    w, h, n = 64, 32, 3
    frames = content(w, h, n, 63)
    src, dst = same_stride_pair(w, h, n, "i420", "nv12")
    src.upload(frames)
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 5))):
            c.profile_read(reset=True)
            kw = dict(src_step=src.y_pitch, src_frame=src.fstride, dst_step=dst.y_pitch, dst_frame=dst.fstride, stream=stream())
            if op is EQ:
                c.equalize_hist_batch_dev(src.planes().y, dst.planes().y, w, h, n, **kw)
            else:
                c.clahe_batch_dev(src.planes().y, dst.planes().y, w, h, n, *op[1], **kw)
            torch.cuda.synchronize()
            planar = launches(c)
            assert sum(planar.values()) >= 2, planar
            for uv_mode in UV_MODES:
                c.profile_read(reset=True)
                check(c, w, h, n, 63, op, uv_mode, src, dst)
                assert launches(c) == dict(planar, lut_apply_kernel=planar["lut_apply_kernel"] + 1), (op, uv_mode)
            c.profile_read(reset=True)
            run(c, op, src, dst, UV_COPY, b=src.planes(y=dst.planes().y, y_pitch=dst.y_pitch))      # the chroma in place
            torch.cuda.synchronize()
            assert launches(c) == planar, "an in-place chroma copy launches no chroma kernel"
        c.set_profiling(0)


# ---- 10. busy --------------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Side(w, h, 1, "i420").upload(content(w, h, 1, 64))
    dst = Side(w, h, 1, "nv12")
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"


# ---- 11. hipGraph ----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist and one CLAHE call captured on a single stream (one linear chain, no parallel
    branches) and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    cl = ("clahe", (2.0, 4, 2))
    src = Side(w, h, n, "i420", **pitched16("i420", w))
    dst_eq, dst_cl = Side(w, h, n, "nv12", **pitched16("nv12", w)), Side(w, h, n, "yv12", **pitched1("yv12", w))
    with mi_lumaeq.Context(0) as c:
        src.upload(content(w, h, n, 65))
        for op, dst, uv_mode in ((EQ, dst_eq, UV_COPY), (cl, dst_cl, UV_FILL128)):        # the eager calls size the scratch
            dst.clear()
            run(c, op, src, dst, uv_mode)
            torch.cuda.synchronize()
            assert dst.same(expected(w, h, n, 65, op, uv_mode))[0], ("eager", op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            run(c, EQ, src, dst_eq, UV_COPY, st=st)
            run(c, cl, src, dst_cl, UV_FILL128, st=st)
        for rep in range(2):
            src.upload(content(w, h, n, 66 + rep))
            dst_eq.clear()
            dst_cl.clear()
            g.replay()
            torch.cuda.synchronize()
            assert dst_eq.same(expected(w, h, n, 66 + rep, EQ, UV_COPY))[0], ("graph replay", "eq", rep)
            assert dst_cl.same(expected(w, h, n, 66 + rep, cl, UV_FILL128))[0], ("graph replay", "clahe", rep)
            assert np.array_equal(src.host(), src.image(content(w, h, n, 66 + rep)))


# ---- 12. host forms --------------------------------------------------------------------------------------------------------------
def tight_frame(fmt, y, u, v):
    if fmt == "nv12":
        return np.concatenate([y.reshape(-1), np.stack([u, v], axis=-1).reshape(-1)])
    first, second = (u, v) if fmt == "i420" else (v, u)
    return np.concatenate([y.reshape(-1), first.reshape(-1), second.reshape(-1)])


HOST_PAIRS = [("i420", "nv12"), ("nv12", "i420"), ("yv12", "nv12"), ("i420", "i420")]


@pytest.mark.parametrize("w,h", [(6, 4), (48, 6), (66, 34)])
def test_host_forms(w, h):
    """Planes at odd addresses with padded rows, in and out, through the C entry points; tight numpy frames through the binding's
    methods: the layout-changing pairs and one that does not, both ops, both UV modes; the source is unchanged."""
    frames = content(w, h, 1, 67)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        for pair in HOST_PAIRS:
            src = Side(w, h, 1, pair[0], y_pitch=w + 5, c_pitch=w + 3, gap0=3, gap1=7, off=1, dev=False).upload(frames)
            dst = Side(w, h, 1, pair[1], y_pitch=w + 9, c_pitch=w + 1, gap0=5, gap1=1, off=3, dev=False)
            a, b = src.planes(frame_stride=12345), dst.planes(frame_stride=7)          # ignored by the host forms
            assert a.y % 2 == 1 and b.y % 2 == 1
            src0 = src.host()
            t_in = tight_frame(pair[0], *frames[0])
            for op in (EQ, ("clahe", (2.0, 3, 2))):
                for uv_mode in UV_MODES:
                    want = expected(w, h, 1, 67, op, uv_mode)
                    dst.clear()
                    if op is EQ:
                        st = L.mi_equalize_hist_yuv420(hd, ctypes.byref(a), ctypes.byref(b), w, h, uv_mode)
                    else:
                        st = L.mi_clahe_yuv420(hd, ctypes.byref(a), ctypes.byref(b), w, h, uv_mode, 2.0, 3, 2)
                    assert st == 0, (pair, op, uv_mode, st)
                    ok, nbad, where = dst.same(want)
                    assert ok, (pair, op, uv_mode, nbad, where)
                    assert np.array_equal(src.host(), src0), "the source was written"
                    t_want = tight_frame(pair[1], *want[0])
                    t0 = t_in.copy()
                    if op is EQ:
                        got = c.equalize_hist_yuv420(t_in, w, h, pair[0], pair[1], uv_mode)
                    else:
                        got = c.clahe_yuv420(t_in, w, h, pair[0], pair[1], uv_mode, *op[1])
                    assert got.shape == (w * h * 3 // 2,) and np.array_equal(got, t_want), (pair, op, uv_mode)
                    assert np.array_equal(t_in, t0), "the source was written"
        # a caller's own output buffer is filled and returned; a tight frame in place
        out = np.full(w * h * 3 // 2, SENT, np.uint8)
        t_in = tight_frame("i420", *frames[0])
        assert c.equalize_hist_yuv420(t_in, w, h, "i420", "nv12", out=out) is out
        assert np.array_equal(out, tight_frame("nv12", *expected(w, h, 1, 67, EQ, UV_COPY)[0]))
        io = t_in.copy()
        assert c.equalize_hist_yuv420(io, w, h, "i420", "i420", UV_FILL128, out=io) is io
        assert np.array_equal(io, tight_frame("i420", *expected(w, h, 1, 67, EQ, UV_FILL128)[0]))
        assert c.get_stat("error_drains") == 0


def test_host_form_errors():
    w, h = 32, 16
    src = Side(w, h, 1, "i420", dev=False).upload(content(w, h, 1, 68))
    dst = Side(w, h, 1, "nv12", dev=False)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        A, B = src.planes, dst.planes
        for ctx, a, b, ww, hh, uvm in ((None, A(), B(), w, h, 1), (hd, A(y=None), B(), w, h, 1), (hd, A(), B(c0=None), w, h, 1),
                                       (hd, A(c1=None), B(), w, h, 1), (hd, A(), B(), w - 1, h, 1), (hd, A(), B(), w, h - 1, 1),
                                       (hd, A(), B(), -2, h, 1), (hd, A(), B(), w, h, 2), (hd, A(chroma=3), B(), w, h, 1),
                                       (hd, A(), B(y=A().c0), w, h, 1), (hd, A(), B(c_pitch=w - 1), w, h, 1), (hd, A(), B(), w - 1, 0, 1)):
            assert L.mi_equalize_hist_yuv420(ctx, ctypes.byref(a), ctypes.byref(b), ww, hh, uvm) == BAD_ARG
            assert L.mi_clahe_yuv420(ctx, ctypes.byref(a), ctypes.byref(b), ww, hh, uvm, 2.0, 2, 2) == BAD_ARG
        a, b = A(), B()
        assert L.mi_clahe_yuv420(hd, ctypes.byref(a), ctypes.byref(b), w, h, 1, 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_yuv420(hd, ctypes.byref(a), ctypes.byref(b), w, h, 1, 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_yuv420(hd, ctypes.byref(a), ctypes.byref(b), 0, h, 1) == 0
        assert dst.same()[0] and c.get_stat("error_drains") == 0
