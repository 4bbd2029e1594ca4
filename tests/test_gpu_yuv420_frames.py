"""8-bit 4:2:0 frames given as a list of separately allocated, pitched planes (mi_*_yuv420_frames_dev) on the GPU: I420 / YV12 / NV12 in,
any of them out.  Expected bytes: oracle.equalize_hist / oracle.clahe on the Y plane, the chroma samples carried over by numpy slicing
(MI_UV_COPY) or 128 (MI_UV_FILL128), as in test_gpu_yuv420.py.  Planes hold full-range random bytes, U and V drawn independently.

Every plane of every frame is its own sentinel-filled allocation -- `off` bytes in front of it, rows * pitch bytes, 64 guard bytes
behind it -- unless a test says otherwise, and every comparison is exact and over WHOLE allocations, the inputs included: the sentinel
in front, the row padding and the guard bytes must still be there.

The shapes of test_loops_past_their_first_step are chosen by the walk of yuv420_relayout, which is the batch kernel's (see the
docstring of test_gpu_yuv420.py): B <= max(1, floor(W*H / 16384)) and B <= H/2 workgroups a frame, 256 * B items a step; the vector
path has W/32 * H/2 items, four in flight per lane, the byte path W/2 * H/2 sample pairs, one per step."""
import ctypes
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, UV_COPY, UV_FILL128, CHROMA_INTERLEAVED, CHROMA_PLANAR, Yuv420FrameDev, Yuv420Planes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
GUARD = 64
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)
PAIRS = [("i420", "i420"), ("i420", "nv12"), ("nv12", "i420"), ("nv12", "nv12")]
CHANGES = [("i420", "nv12"), ("nv12", "i420")]
LIST_STATS = ("yuv420_list_frames_vec", "yuv420_list_frames_bytes")
OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass",
               "yuv420_chroma_vec", "yuv420_chroma_bytes")
DEVICE = "cuda:0"


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- content and what it must become -------------------------------------------------------------------------------------------------
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


def map_luma(y, op):
    return oracle.equalize_hist(y) if op[0] == "eq" else oracle.clahe(y, *op[1])


@functools.lru_cache(maxsize=None)
def luma(w, h, n, seed, op):
    out = []
    for y, _, _ in content(w, h, n, seed):
        r = map_luma(y, op)
        r.setflags(write=False)
        out.append(r)
    return tuple(out)


def expected(w, h, n, seed, op, uv_mode):
    """The (Y, U, V) planes the call must produce for content(w, h, n, seed)."""
    fill = np.full((h // 2, w // 2), 128, np.uint8)
    return [(yy, u, v) if uv_mode == UV_COPY else (yy, fill, fill) for yy, (_, u, v) in zip(luma(w, h, n, seed, op), content(w, h, n, seed))]


# ---- planes, each in its own allocation ----------------------------------------------------------------------------------------------
class Plane:
    """`rows` rows of `row` bytes at `pitch`, `off` bytes into a sentinel-filled allocation of its own with GUARD bytes behind the last
    row's padding.  `want` is the image the allocation must hold: put() writes rows into it, load() sends it to the device."""

    def __init__(self, rows, row, pitch=None, off=0):
        self.rows, self.row, self.pitch, self.off = rows, row, pitch or row, off
        assert self.pitch >= row
        self.total = off + rows * self.pitch + GUARD
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device=DEVICE)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + off
        self.want = np.full(self.total, SENT, np.uint8)

    def put(self, data, x0=0):
        """rows of `data` (rows x k) at byte x0 of every row of the wanted image"""
        data = np.asarray(data, np.uint8).reshape(self.rows, -1)
        assert x0 + data.shape[1] <= self.row
        for r in range(self.rows):
            o = self.off + r * self.pitch + x0
            self.want[o: o + data.shape[1]] = data[r]
        return self

    def blank(self):
        self.want[:] = SENT
        return self


def load(planes):
    """the wanted images of `planes` up into their allocations: one transfer, then a device copy each"""
    planes = list(planes)
    if not planes:
        return
    staged = xfer.to_device(np.concatenate([p.want for p in planes]))
    o = 0
    for p in planes:
        p.buf.copy_(staged[o: o + p.total])
        o += p.total
    torch.cuda.synchronize()


def verify(planes, what=""):
    """every allocation, whole, against its wanted image: one transfer"""
    planes = list(planes)
    torch.cuda.synchronize()
    got = xfer.to_host(torch.cat([p.buf for p in planes]))
    want = np.concatenate([p.want for p in planes])
    if np.array_equal(got, want):
        return
    o = 0
    for k, p in enumerate(planes):
        g, wt = got[o: o + p.total], want[o: o + p.total]
        o += p.total
        assert np.array_equal(g, wt), (what, "plane", k, "rows x row @ pitch + off", (p.rows, p.row, p.pitch, p.off),
                                       int((g != wt).sum()), "bytes differ, first at", np.flatnonzero(g != wt)[:8])


def interleave(u, v):
    return np.stack([u, v], axis=-1).reshape(u.shape[0], -1)


class Side:
    """n frames of one side of a call: fmt "nv12": a Y and a UV plane a frame; "i420": Y, U, V; "yv12": the same planes with the chroma
    addresses exchanged -- the FIRST chroma plane of a frame holds V, and c0, which is always the U plane, is the second.  One y_pitch,
    one c_pitch for the side; offs = (Y, first chroma plane, second chroma plane): bytes in front of each plane in its allocation."""

    def __init__(self, w, h, n, fmt, y_pitch=None, c_pitch=None, offs=(0, 0, 0)):
        self.w, self.h, self.n, self.fmt = w, h, n, fmt
        self.planar = fmt != "nv12"
        self.chroma = CHROMA_PLANAR if self.planar else CHROMA_INTERLEAVED
        self.crow = w // 2 if self.planar else w
        self.y_pitch, self.c_pitch = y_pitch or w, c_pitch or self.crow
        self.y = [Plane(h, w, self.y_pitch, offs[0]) for _ in range(n)]
        self.a = [Plane(h // 2, self.crow, self.c_pitch, offs[1]) for _ in range(n)]
        self.b = [Plane(h // 2, self.crow, self.c_pitch, offs[2]) for _ in range(n)] if self.planar else [None] * n

    def u_plane(self, k):
        return self.b[k] if self.fmt == "yv12" else self.a[k]

    def v_plane(self, k):
        return self.a[k] if self.fmt == "yv12" else self.b[k]

    def c0(self, k):
        return self.u_plane(k).ptr

    def c1(self, k):
        return self.v_plane(k).ptr if self.planar else None

    def planes(self):
        return [p for k in range(self.n) for p in (self.y[k], self.a[k], self.b[k]) if p is not None]

    def put(self, k, frame, luma=True, chroma=True):
        """frame k must hold the (Y, U, V) arrays of `frame`"""
        y, u, v = frame
        if luma:
            self.y[k].put(y)
        if chroma and self.planar:
            self.u_plane(k).put(u)
            self.v_plane(k).put(v)
        elif chroma:
            self.a[k].put(interleave(u, v))
        return self

    def fill(self, frames):
        for k, f in enumerate(frames):
            self.put(k, f)
        return self

    def blank(self):
        for p in self.planes():
            p.blank()
        return self

    def chroma_ptrs(self, k):
        return [self.c0(k)] + ([self.c1(k)] if self.planar else [])


def entry(src, i, dst, k, **over):
    d = dict(y_in=src.y[i].ptr, c0_in=src.c0(i), c1_in=src.c1(i), y_out=dst.y[k].ptr, c0_out=dst.c0(k), c1_out=dst.c1(k))
    d.update(over)
    return Yuv420FrameDev(d["y_in"], d["c0_in"], d["c1_in"], d["y_out"], d["c0_out"], d["c1_out"])


def entries(src, dst):
    return [entry(src, k, dst, k) for k in range(src.n)]


def call(c, op, ents, src, dst, uv_mode, st=None):
    st = stream() if st is None else st
    a = (ents, src.w, src.h, src.y_pitch, src.c_pitch, src.chroma, dst.y_pitch, dst.c_pitch, dst.chroma, uv_mode)
    if op[0] == "eq":
        c.equalize_hist_yuv420_frames_dev(*a, stream=st)
    else:
        c.clahe_yuv420_frames_dev(*a, *op[1], stream=st)


def frame_takes_vector_path(src, i, dst, k):
    """The header's rule for one frame of a layout change: W % 32 == 0, both c_pitch and the frame's own chroma pointers multiples of 16."""
    return src.w % 32 == 0 and all(v % 16 == 0 for v in [src.c_pitch, dst.c_pitch] + src.chroma_ptrs(i) + dst.chroma_ptrs(k))


def stats(c, names=LIST_STATS):
    return tuple(c.get_stat(s) for s in names)


def check(c, w, h, n, seed, op, uv_mode, src, dst, want_vec=None):
    """One call on frames k -> k of two sides: every allocation of both sides holds what it must, the two list counters moved by the
    frames the rule names (layout changes under MI_UV_COPY only), the per-call counters of the batch form did not move."""
    frames = content(w, h, n, seed)
    src.blank().fill(frames)
    dst.blank()
    load(src.planes() + dst.planes())
    dst.fill(expected(w, h, n, seed, op, uv_mode))
    before, other = stats(c), stats(c, OTHER_STATS)
    call(c, op, entries(src, dst), src, dst, uv_mode)
    verify(src.planes() + dst.planes(), (w, h, n, src.fmt, dst.fmt, op, uv_mode))
    vec = nb = 0
    if uv_mode == UV_COPY and src.planar != dst.planar:
        vec = sum(frame_takes_vector_path(src, k, dst, k) for k in range(n))
        nb = n - vec
    if want_vec is not None:
        assert (vec, nb) == want_vec, "the test's own layout is not what it says"
    assert stats(c) == (before[0] + vec, before[1] + nb), (src.fmt, dst.fmt, uv_mode, vec, nb)
    assert stats(c, OTHER_STATS) == other


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small allocations leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def tight(fmt, w):
    return {}


def pitched16(fmt, w):
    """both pitches + 16 and 16 bytes in front of every plane: everything a multiple of 16"""
    return dict(y_pitch=w + 16, c_pitch=(w if fmt == "nv12" else w // 2) + 16, offs=(16, 16, 16))


def pitched1(fmt, w):
    return dict(y_pitch=w + 1, c_pitch=(w if fmt == "nv12" else w // 2) + 1)


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
PARITY = [
    # id, W, H, layout of both sides, the frames of a layout change on the vector path, the ops (grids that divide the frame and not)
    ("2x2", 2, 2, tight, 0, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 2))]),                       # one sample per chroma plane
    ("6x4", 6, 4, tight, 0, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 4, 3))]),                       # the byte path
    ("32x4", 32, 4, tight, 3, [EQ, ("clahe", (2.0, 2, 2)), ("clahe", (3.0, 3, 3))]),                     # the first vector shape
    ("34x6", 34, 6, tight, 0, [EQ, ("clahe", (2.0, 2, 3)), ("clahe", (2.0, 4, 4))]),                     # W % 32 != 0
    ("64x6-pitched16", 64, 6, pitched16, 3, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 5, 4))]),       # vector path with padding
    ("64x6-pitched1", 64, 6, pitched1, 0, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 5, 4))]),         # pitches + 1: byte path
]


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("name,w,h,lay,nvec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, lay, nvec, ops, pair):
    n = 3
    src, dst = Side(w, h, n, pair[0], **lay(pair[0], w)), Side(w, h, n, pair[1], **lay(pair[1], w))
    for op in ops:
        for uv_mode in UV_MODES:
            change = uv_mode == UV_COPY and pair[0] != pair[1]
            check(c, w, h, n, 71, op, uv_mode, src, dst, want_vec=(nvec, n - nvec) if change else (0, 0))


@pytest.mark.parametrize("pair", [("yv12", "nv12"), ("nv12", "yv12"), ("yv12", "i420"), ("i420", "yv12"), ("yv12", "yv12")],
                         ids=lambda p: "-".join(p))
@pytest.mark.parametrize("w,h", [(64, 6), (6, 4)])
def test_yv12_is_i420_with_the_chroma_addresses_exchanged(c, w, h, pair):
    """c0 is always U: a YV12 frame passes its second chroma plane as c0.  U and V hold different bytes, a swap cannot pass."""
    n = 3
    u, v = content(w, h, n, 72)[0][1:]
    assert not np.array_equal(u, v)
    s = Side(w, h, 1, "yv12")
    assert s.c0(0) == s.b[0].ptr and s.c1(0) == s.a[0].ptr
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        check(c, w, h, n, 72, op, UV_COPY, Side(w, h, n, pair[0]), Side(w, h, n, pair[1]))


# ---- 2. the path is chosen per frame ---------------------------------------------------------------------------------------------
class MiddleOff(Side):
    """a side whose MIDDLE frame (of three) has one plane 1 byte into its allocation: which = "c0" / "c1" / "y"."""

    def __init__(self, w, h, fmt, which):
        super().__init__(w, h, 3, fmt)
        if which == "y":
            self.y[1] = Plane(h, w, self.y_pitch, 1)
        elif which == "c0":
            self.a[1] = Plane(h // 2, self.crow, self.c_pitch, 1)
        elif which == "c1":
            self.b[1] = Plane(h // 2, self.crow, self.c_pitch, 1)


@pytest.mark.parametrize("pair", CHANGES, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("which", ["c0_in", "c1_in", "c0_out", "c1_out"])
def test_one_misaligned_frame_takes_the_byte_path_alone(c, pair, which):
    w, h, n = 64, 6, 3
    term, side = which.split("_")
    fmts = dict(zip(("in", "out"), pair))
    if term == "c1" and fmts[side] == "nv12":
        # an interleaved side has no c1: whatever the entry holds there is ignored, also by the alignment rule
        src, dst = Side(w, h, n, pair[0]), Side(w, h, n, pair[1])
        frames = content(w, h, n, 73)
        src.fill(frames)
        load(src.planes() + dst.planes())
        dst.fill(expected(w, h, n, 73, EQ, UV_COPY))
        ents = entries(src, dst)
        ents[1] = entry(src, 1, dst, 1, **{which: 0x1001})
        before = stats(c)
        call(c, EQ, ents, src, dst, UV_COPY)
        verify(src.planes() + dst.planes(), which)
        assert stats(c) == (before[0] + 3, before[1])
        return
    src = MiddleOff(w, h, pair[0], term) if side == "in" else Side(w, h, n, pair[0])
    dst = MiddleOff(w, h, pair[1], term) if side == "out" else Side(w, h, n, pair[1])
    assert [frame_takes_vector_path(src, k, dst, k) for k in range(n)] == [True, False, True]
    for op in (EQ, ("clahe", (2.0, 4, 2))):
        check(c, w, h, n, 73, op, UV_COPY, src, dst, want_vec=(2, 1))


@pytest.mark.parametrize("pair", CHANGES, ids=lambda p: "-".join(p))
def test_a_pitch_moves_every_frame_and_a_misaligned_y_none(c, pair):
    w, h, n = 64, 6, 3
    for k in (0, 1):                                   # one c_pitch + 1: all three frames on the byte path
        lays = [{}, {}]
        lays[k] = dict(c_pitch=(w if pair[k] == "nv12" else w // 2) + 1)
        check(c, w, h, n, 74, EQ, UV_COPY, Side(w, h, n, pair[0], **lays[0]), Side(w, h, n, pair[1], **lays[1]), want_vec=(0, 3))
    # every Y plane at an odd address with an odd pitch: the Y side plays no part
    lay = dict(y_pitch=w + 1, offs=(1, 0, 0))
    src, dst = Side(w, h, n, pair[0], **lay), Side(w, h, n, pair[1], **lay)
    assert all(p.ptr % 2 for s in (src, dst) for p in s.y)
    for op in (EQ, ("clahe", (2.0, 4, 2))):
        check(c, w, h, n, 74, op, UV_COPY, src, dst, want_vec=(3, 0))


# ---- 3. in place, per frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("uv_mode", UV_MODES)
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_in_place_is_decided_per_frame(c, fmt, uv_mode, op):
    """Frame 0: Y in place, the chroma elsewhere.  Frame 1: the chroma in place (MI_UV_COPY: nothing moves; MI_UV_FILL128: it becomes
    128), Y elsewhere.  Frame 2: everything elsewhere.  The planes of `dst` that an in-place plane stands in for stay untouched."""
    w, h, n = 64, 6, 3
    for lay in (tight, pitched16, pitched1):
        src, dst = Side(w, h, n, fmt, **lay(fmt, w)), Side(w, h, n, fmt, **lay(fmt, w))
        frames = content(w, h, n, 75)
        src.fill(frames)
        load(src.planes() + dst.planes())
        want = expected(w, h, n, 75, op, uv_mode)
        ents = [entry(src, 0, dst, 0, y_out=src.y[0].ptr),
                entry(src, 1, dst, 1, c0_out=src.c0(1), c1_out=src.c1(1)),
                entry(src, 2, dst, 2)]
        src.put(0, want[0], chroma=False)
        dst.put(0, want[0], luma=False)
        src.put(1, want[1], luma=False)
        dst.put(1, want[1], chroma=False)
        dst.put(2, want[2])
        before = stats(c) + stats(c, OTHER_STATS)
        call(c, op, ents, src, dst, uv_mode)
        verify(src.planes() + dst.planes(), (fmt, uv_mode, op, lay.__name__))
        assert stats(c) + stats(c, OTHER_STATS) == before, "a same-layout call counts no frame"


@pytest.mark.parametrize("pair", CHANGES, ids=lambda p: "-".join(p))
def test_layout_change_with_y_in_place_on_one_frame(c, pair):
    w, h, n = 64, 6, 3
    op = ("clahe", (2.0, 2, 2))
    src, dst = Side(w, h, n, pair[0]), Side(w, h, n, pair[1])
    src.fill(content(w, h, n, 76))
    load(src.planes() + dst.planes())
    want = expected(w, h, n, 76, op, UV_COPY)
    ents = entries(src, dst)
    ents[1] = entry(src, 1, dst, 1, y_out=src.y[1].ptr)
    dst.fill(want)
    dst.y[1].blank()
    src.put(1, want[1], chroma=False)
    before = stats(c)
    call(c, op, ents, src, dst, UV_COPY)
    verify(src.planes() + dst.planes(), pair)
    assert stats(c) == (before[0] + 3, before[1])


# ---- 4. U and V rows side by side in one pitched plane ---------------------------------------------------------------------------
class SideBySide(Side):
    """a planar side whose U and V rows share one plane of W-byte rows: c1 = c0 + W/2, c_pitch = W"""

    def __init__(self, w, h, n):
        super().__init__(w, h, n, "i420", c_pitch=w)
        self.a = [Plane(h // 2, w, w) for _ in range(n)]
        self.b = [None] * n

    def c1(self, k):
        return self.a[k].ptr + self.w // 2

    def put(self, k, frame, luma=True, chroma=True):
        y, u, v = frame
        if luma:
            self.y[k].put(y)
        if chroma:
            self.a[k].put(u).put(v, x0=self.w // 2)
        return self


@pytest.mark.parametrize("as_input", [True, False], ids=["input", "output"])
def test_side_by_side_chroma_is_legal_and_vectorised(c, as_input):
    w, h, n = 64, 6, 2
    for op in (EQ, ("clahe", (2.0, 4, 2))):
        src = SideBySide(w, h, n) if as_input else Side(w, h, n, "nv12")
        dst = Side(w, h, n, "nv12") if as_input else SideBySide(w, h, n)
        check(c, w, h, n, 77, op, UV_COPY, src, dst, want_vec=(2, 0))


# ---- 5. loops past their first step, through the table entry ---------------------------------------------------------------------
LOOP_SHAPES = [
    # W*H/16384 = 1.02: B = 1, stride 256; slots 2, items 260: lanes 0..3 take a second item
    ("64x260", 64, 260, tight, True),
    # W*H/16384 = 1.05: B = 1, stride 256; slots 3, items 270, drow 85, dslot 1: the slot wraps on the second item of lanes with slot 2
    ("96x180", 96, 180, pitched16, True),
    # byte path, B = 1: 17 x 16 = 272 pairs for 256 lanes, drow 15, dx 1: a second step that wraps
    ("34x32", 34, 32, tight, False),
]


@pytest.mark.parametrize("pair", CHANGES, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("name,w,h,lay,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, lay, vec, pair):
    n = 2
    src, dst = Side(w, h, n, pair[0], **lay(pair[0], w)), Side(w, h, n, pair[1], **lay(pair[1], w))
    bound = min(max(1, w * h // 16384), h // 2)
    items = (w // 32 if vec else w // 2) * (h // 2)
    assert items > 256 * bound, "the shape would not loop"
    check(c, w, h, n, 78, EQ, UV_COPY, src, dst, want_vec=(n, 0) if vec else (0, n))
    check(c, w, h, n, 78, ("clahe", (2.0, 2, 2)), UV_COPY, src, dst)


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_same_layout_moves_and_fills_past_one_workgroup(c, fmt):
    """256 x 256, pitched: uv_rows under the table entry on up to four workgroups a frame, copy and fill."""
    w, h, n = 256, 256, 2
    src, dst = Side(w, h, n, fmt, **pitched16(fmt, w)), Side(w, h, n, fmt, **pitched16(fmt, w))
    for uv_mode in UV_MODES:
        check(c, w, h, n, 79, EQ, uv_mode, src, dst)


# ---- 6. chunking -----------------------------------------------------------------------------------------------------------------
def frames_per_launch():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "common.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kFramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1))


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("w,h", [(2, 2), (32, 2)])
def test_chunking(c, w, h, n):
    """One frame past one and past two full chunks: frame 64 and frame 128 are the first of their chunk, so a table index that does
    not restart reads past the table.  Every frame is distinct and every frame is checked."""
    assert frames_per_launch() == 64
    for pair in CHANGES + [("i420", "i420")]:
        src, dst = Side(w, h, n, pair[0]), Side(w, h, n, pair[1])
        check(c, w, h, n, 80, EQ, UV_COPY, src, dst)
        check(c, w, h, n, 80, ("clahe", (2.0, 1, 1)), UV_COPY, src, dst)


# ---- 7. list order and aliasing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", CHANGES + [("i420", "i420")], ids=lambda p: "-".join(p))
def test_permuted_list_over_shuffled_pools(c, pair):
    """Entry k reads frame p[k] of the input pool and writes frame q[k] of the output pool."""
    w, h, n = 32, 4, 7
    rng = np.random.default_rng(81)
    p, q = rng.permutation(n), rng.permutation(n)
    src, dst = Side(w, h, n, pair[0]), Side(w, h, n, pair[1])
    src.fill(content(w, h, n, 81))
    load(src.planes() + dst.planes())
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        want = expected(w, h, n, 81, op, UV_COPY)
        for k in range(n):
            dst.put(int(q[k]), want[int(p[k])])
        call(c, op, [entry(src, int(p[k]), dst, int(q[k])) for k in range(n)], src, dst, UV_COPY)
        verify(src.planes() + dst.planes(), (pair, op))


def test_one_input_frame_listed_twice(c):
    w, h = 32, 4
    src, dst = Side(w, h, 1, "i420"), Side(w, h, 2, "nv12")
    src.fill(content(w, h, 1, 82))
    load(src.planes() + dst.planes())
    want = expected(w, h, 1, 82, EQ, UV_COPY)[0]
    dst.put(0, want).put(1, want)
    call(c, EQ, [entry(src, 0, dst, 0), entry(src, 0, dst, 1)], src, dst, UV_COPY)
    verify(src.planes() + dst.planes())


def test_histograms_do_not_leak_across_frames(c):
    w, h = 64, 32
    rng = np.random.default_rng(83)
    ys = [np.full((h, w), 77, np.uint8), np.tile(np.arange(w, dtype=np.uint8) * 3, (h, 1)), rng.integers(0, 256, (h, w), dtype=np.uint8),
          np.full((h, w), 200, np.uint8)]
    n = len(ys)
    chroma = content(w, h, n, 83)
    frames = [(ys[k], chroma[k][1], chroma[k][2]) for k in range(n)]
    src, dst = Side(w, h, n, "i420"), Side(w, h, n, "nv12")
    src.fill(frames)
    load(src.planes() + dst.planes())
    dst.fill([(oracle.equalize_hist(y), u, v) for y, u, v in frames])
    call(c, EQ, entries(src, dst), src, dst, UV_COPY)
    verify(src.planes() + dst.planes())


# ---- 8. identity with the existing forms -----------------------------------------------------------------------------------------
def arena_layout(w, h, fmt):
    """a pitched frame in an arena: offsets of Y, c0, c1 in the frame, the pitches, the frame stride (all multiples of 16)"""
    crow = w if fmt == "nv12" else w // 2
    yp, cp = w + 16, crow + 16
    c0 = yp * h + 32
    c1 = c0 + cp * (h // 2) + 16
    fs = (c1 + cp * (h // 2) if fmt != "nv12" else c1) + 48
    return dict(y=0, c0=c0, c1=c1 if fmt != "nv12" else None, yp=yp, cp=cp, fs=fs, chroma=CHROMA_INTERLEAVED if fmt == "nv12" else CHROMA_PLANAR)


def arena_image(w, h, fmt, frames, L, total, head):
    a = np.full(total, SENT, np.uint8)
    for k, (y, u, v) in enumerate(frames):
        b = head + k * L["fs"]
        for r in range(h):
            a[b + r * L["yp"]: b + r * L["yp"] + w] = y[r]
        for r in range(h // 2):
            if fmt == "nv12":
                a[b + L["c0"] + r * L["cp"]: b + L["c0"] + r * L["cp"] + w] = interleave(u, v)[r]
            else:
                a[b + L["c0"] + r * L["cp"]: b + L["c0"] + r * L["cp"] + w // 2] = u[r]
                a[b + L["c1"] + r * L["cp"]: b + L["c1"] + r * L["cp"] + w // 2] = v[r]
    return a


@pytest.mark.parametrize("pair", CHANGES, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_the_batch_form(c, op, pair):
    """The frames at a constant stride in ONE allocation a side, handed over as a list of their addresses: the whole output allocation is
    byte for byte what mi_*_yuv420_batch_dev leaves in its own copy of it, and what the oracle says."""
    w, h, n = 64, 32, 3
    head = 16
    Li, Lo = arena_layout(w, h, pair[0]), arena_layout(w, h, pair[1])
    ti, to = head + n * Li["fs"] + GUARD, head + n * Lo["fs"] + GUARD
    frames = content(w, h, n, 84)
    in_img = arena_image(w, h, pair[0], frames, Li, ti, head)
    src = xfer.to_device(in_img)
    out_list = torch.full((to,), SENT, dtype=torch.uint8, device=DEVICE)
    out_batch = torch.full((to,), SENT, dtype=torch.uint8, device=DEVICE)

    def addr(base, L, k, key):
        return None if L[key] is None else base + head + k * L["fs"] + L[key]
    ents = [Yuv420FrameDev(addr(src.data_ptr(), Li, k, "y"), addr(src.data_ptr(), Li, k, "c0"), addr(src.data_ptr(), Li, k, "c1"),
                           addr(out_list.data_ptr(), Lo, k, "y"), addr(out_list.data_ptr(), Lo, k, "c0"), addr(out_list.data_ptr(), Lo, k, "c1"))
            for k in range(n)]
    a = Yuv420Planes(addr(src.data_ptr(), Li, 0, "y"), Li["yp"], addr(src.data_ptr(), Li, 0, "c0"), addr(src.data_ptr(), Li, 0, "c1"), Li["cp"],
                     Li["fs"], Li["chroma"])
    b = Yuv420Planes(addr(out_batch.data_ptr(), Lo, 0, "y"), Lo["yp"], addr(out_batch.data_ptr(), Lo, 0, "c0"),
                     addr(out_batch.data_ptr(), Lo, 0, "c1"), Lo["cp"], Lo["fs"], Lo["chroma"])
    la = (ents, w, h, Li["yp"], Li["cp"], Li["chroma"], Lo["yp"], Lo["cp"], Lo["chroma"], UV_COPY)
    if op is EQ:
        c.equalize_hist_yuv420_frames_dev(*la, stream=stream())
        c.equalize_hist_yuv420_batch_dev(a, b, w, h, n, UV_COPY, stream=stream())
    else:
        c.clahe_yuv420_frames_dev(*la, *op[1], stream=stream())
        c.clahe_yuv420_batch_dev(a, b, w, h, n, UV_COPY, *op[1], stream=stream())
    torch.cuda.synchronize()
    got_list, got_batch = xfer.to_host(out_list), xfer.to_host(out_batch)
    assert np.array_equal(got_list, got_batch), np.flatnonzero(got_list != got_batch)[:8]
    assert np.array_equal(got_list, arena_image(w, h, pair[1], expected(w, h, n, 84, op, UV_COPY), Lo, to, head))
    assert np.array_equal(xfer.to_host(src), in_img), "the input allocation was written"


@pytest.mark.parametrize("uv_mode", UV_MODES)
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_interleaved_to_interleaved_equals_the_nv12_list_form(c, op, uv_mode):
    w, h, n = 64, 32, 3
    src = Side(w, h, n, "nv12", **pitched16("nv12", w))
    dst, ref = Side(w, h, n, "nv12", **pitched16("nv12", w)), Side(w, h, n, "nv12", **pitched16("nv12", w))
    src.fill(content(w, h, n, 85))
    load(src.planes() + dst.planes() + ref.planes())
    call(c, op, entries(src, dst), src, dst, uv_mode)
    ins = [(src.y[k].ptr, src.a[k].ptr) for k in range(n)]
    outs = [(ref.y[k].ptr, ref.a[k].ptr) for k in range(n)]
    kw = dict(y_in_pitch=src.y_pitch, uv_in_pitch=src.c_pitch, y_out_pitch=ref.y_pitch, uv_out_pitch=ref.c_pitch, stream=stream())
    if op is EQ:
        c.equalize_hist_nv12_frames(ins, outs, w, h, uv_mode, **kw)
    else:
        c.clahe_nv12_frames(ins, outs, w, h, uv_mode, *op[1], **kw)
    torch.cuda.synchronize()
    for p, r in zip(dst.planes(), ref.planes()):
        assert torch.equal(p.buf, r.buf)
    dst.fill(expected(w, h, n, 85, op, uv_mode))
    verify(src.planes() + dst.planes())


# ---- 9. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


@pytest.mark.parametrize("n", [2, 65])
def test_launch_contract(n):
    """With every chroma plane in place under MI_UV_COPY there is no chroma launch: the counts of that run are the luma's own.  Out of
    place -- a same-layout move, a fill, a layout change -- adds exactly one MI_K_LUT_APPLY launch per chunk of 64 frames and nothing
    else; the statistics of other forms do not move."""
    w, h = 32, 4
    chunks = (n + 63) // 64
    frames = content(w, h, n, 86)
    src, same, other = Side(w, h, n, "i420"), Side(w, h, n, "i420"), Side(w, h, n, "nv12")
    src.fill(frames)
    load(src.planes() + same.planes() + other.planes())
    with mi_lumaeq.Context(0) as c:
        before = stats(c, OTHER_STATS)
        c.set_profiling(1)
        for op in (EQ, ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 3, 1))):
            want = expected(w, h, n, 86, op, UV_COPY)
            c.profile_read(reset=True)
            same.blank()
            for k in range(n):
                same.put(k, want[k], chroma=False)
            call(c, op, [entry(src, k, same, k, c0_out=src.c0(k), c1_out=src.c1(k)) for k in range(n)], src, same, UV_COPY)
            verify(src.planes() + same.planes(), "chroma in place")
            own = launches(c)
            assert len(own) == 10 and sum(own.values()) >= 2 * chunks, own
            load(same.planes())                                                       # Y back to the sentinel
            for dst, uv_mode in ((same, UV_COPY), (same, UV_FILL128), (other, UV_COPY), (other, UV_FILL128)):
                c.profile_read(reset=True)
                dst.blank()
                load(dst.planes())
                dst.fill(expected(w, h, n, 86, op, uv_mode))
                call(c, op, entries(src, dst), src, dst, uv_mode)
                verify(src.planes() + dst.planes(), (op, dst.fmt, uv_mode))
                assert launches(c) == dict(own, lut_apply_kernel=own["lut_apply_kernel"] + chunks), (op, dst.fmt, uv_mode, own)
            same.blank()
            load(same.planes())
        c.set_profiling(0)
        assert stats(c, OTHER_STATS) == before


# ---- 10. errors, zero sizes ------------------------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    frames = content(w, h, n, 87)
    src = Side(w, h, n, "i420", **pitched16("i420", w)).fill(frames)
    dst = Side(w, h, n, "nv12", **pitched16("nv12", w))
    pdst = Side(w, h, n, "i420", **pitched16("i420", w))              # a planar output with src's pitches, for the in-place cases
    everything = src.planes() + dst.planes() + pdst.planes()
    load(everything)
    NULL_LIST = object()
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)

        def run(out, tiles=None, ctx=hd, lst=None, n=n, w=w, h=h, uvm=UV_COPY, last=None, yip=None, cip=None, ich=None, yop=None,
                cop=None, och=None):
            """the list src -> out with the fields of `last` replacing those of its LAST entry: the first two frames are good"""
            ents = entries(src, out)
            if last:
                ents[-1] = entry(src, src.n - 1, out, out.n - 1, **last)
            arr = (Yuv420FrameDev * len(ents))(*ents)
            a = (ctx, None if lst is NULL_LIST else arr, n, w, h, src.y_pitch if yip is None else yip, src.c_pitch if cip is None else cip,
                 src.chroma if ich is None else ich, out.y_pitch if yop is None else yop, out.c_pitch if cop is None else cop,
                 out.chroma if och is None else och, uvm)
            if tiles is None:
                return L.mi_equalize_hist_yuv420_frames_dev(*a, stream())
            return L.mi_clahe_yuv420_frames_dev(*a, 2.0, tiles[0], tiles[1], stream())

        def both(out, **kw):
            return run(out, **kw), run(out, tiles=(2, 2), **kw)
        s_y, s_u, s_v = src.y[-1].ptr, src.c0(n - 1), src.c1(n - 1)
        bad = [
            (dst, dict(ctx=None)), (dst, dict(lst=NULL_LIST)), (dst, dict(lst=NULL_LIST, n=1)),           # a null ctx, a null list with n_frames > 0
            (dst, dict(last=dict(y_in=None))), (dst, dict(last=dict(y_out=None))),                        # a null y
            (dst, dict(last=dict(c0_out=None))), (pdst, dict(last=dict(c1_out=None))),                    # a null out c0; c1 of a PLANAR output
            (dst, dict(last=dict(c0_in=None))), (dst, dict(last=dict(c1_in=None))),                       # input chroma COPY needs
            (dst, dict(ich=2)), (dst, dict(och=-1)), (dst, dict(ich=2, uvm=UV_FILL128)),                  # a chroma other than the two
            (dst, dict(uvm=2)), (dst, dict(uvm=-1)),                                                      # a bad uv_mode
            (dst, dict(w=-2)), (dst, dict(h=-2)), (dst, dict(n=-1)),                                      # negative sizes
            (dst, dict(w=31)), (dst, dict(h=15)), (dst, dict(w=31, h=0)), (dst, dict(h=15, w=0)), (dst, dict(h=15, n=0)),   # odd, also next to a 0
            (dst, dict(yip=w - 1)), (dst, dict(yop=w - 1)),                                               # a y pitch < W
            (dst, dict(cip=w // 2 - 1)), (dst, dict(cop=w - 1)), (pdst, dict(cop=w // 2 - 1)),            # a c pitch below its row
            (dst, dict(last=dict(c0_out=dst.y[-1].ptr))),                                                 # two equal output pointers
            (pdst, dict(last=dict(c1_out=pdst.c0(n - 1)))), (pdst, dict(last=dict(c1_out=pdst.y[-1].ptr))),
            (dst, dict(last=dict(y_out=s_u))), (dst, dict(last=dict(c0_out=s_y))), (dst, dict(last=dict(c0_out=s_v))),   # out == in, another plane
            (pdst, dict(last=dict(c0_out=s_v, c1_out=s_u))),
            (dst, dict(last=dict(y_out=s_y), yop=src.y_pitch + 16)),                                      # Y at in's address: another pitch
            (dst, dict(last=dict(c0_out=s_u))),                                                           # U at in's address: another layout
            (pdst, dict(last=dict(c0_out=s_u), cop=src.c_pitch + 16)),                                    # ... another pitch
        ]
        assert dst.y_pitch == src.y_pitch and pdst.c_pitch == src.c_pitch
        for out, kw in bad:
            assert both(out, **kw) == (BAD_ARG, BAD_ARG), (out.fmt, kw)
        for tiles in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert run(dst, tiles=tiles) == BAD_ARG, tiles
            assert run(dst, tiles=tiles, n=0) == BAD_ARG, tiles
        # zero sizes: MI_OK, nothing written -- a null list is fine when there are no frames
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, lst=NULL_LIST)):
            assert both(dst, **kw) == (0, 0), kw
        # sizes and tile grids the planar forms refuse: their status
        bw = (1 << 24) + 2
        planar = L.mi_clahe_u8_batch_dev(hd, s_y, 1 << 25, 1 << 26, dst.y[0].ptr, 1 << 25, 1 << 26, bw, 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and both(dst, w=bw, h=2, yip=1 << 25, cip=1 << 25, yop=1 << 25, cop=1 << 25) == (planar, planar)
        planar = L.mi_clahe_u8_batch_dev(hd, s_y, src.y_pitch, 0, dst.y[0].ptr, dst.y_pitch, 0, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and run(dst, tiles=(2048, 1024)) == planar
        verify(everything, "a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0, 0)
        c.set_profiling(0)
        # MI_UV_FILL128 with null input chroma pointers, and a c_in_pitch of 0, is accepted: the context still works
        for out in (dst, pdst):
            for op, tiles in ((EQ, None), (("clahe", (2.0, 2, 2)), (2, 2))):
                out.blank()
                load(out.planes())
                ents = [entry(src, k, out, k, c0_in=None, c1_in=None) for k in range(n)]
                arr = (Yuv420FrameDev * n)(*ents)
                a = (hd, arr, n, w, h, src.y_pitch, 0, src.chroma, out.y_pitch, out.c_pitch, out.chroma, UV_FILL128)
                st = L.mi_equalize_hist_yuv420_frames_dev(*a, stream()) if tiles is None else \
                    L.mi_clahe_yuv420_frames_dev(*a, 2.0, 2, 2, stream())
                assert st == 0, (out.fmt, op)
                out.fill(expected(w, h, n, 87, op, UV_FILL128))
                verify(src.planes() + out.planes(), ("fill128 without input chroma", out.fmt, op))


# ---- 11. busy, hipGraph ----------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src, dst = Side(w, h, 1, "i420").fill(content(w, h, 1, 88)), Side(w, h, 1, "nv12")
    load(src.planes() + dst.planes())
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, entries(src, dst), src, dst, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        verify(src.planes() + dst.planes(), "a refused call wrote")


def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist and one CLAHE call captured on a single stream (one linear chain, no parallel
    branches) and two replays onto fresh inputs at the captured addresses: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    cl = ("clahe", (2.0, 4, 2))
    src = Side(w, h, n, "i420", **pitched16("i420", w))
    dst_eq, dst_cl = Side(w, h, n, "nv12", **pitched16("nv12", w)), Side(w, h, n, "yv12", **pitched1("yv12", w))
    everything = src.planes() + dst_eq.planes() + dst_cl.planes()
    jobs = ((EQ, dst_eq, UV_COPY), (cl, dst_cl, UV_FILL128))
    with mi_lumaeq.Context(0) as c:
        for op, dst, uv_mode in jobs:                                                    # the eager calls size the scratch
            check(c, w, h, n, 89, op, uv_mode, src, dst)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            for op, dst, uv_mode in jobs:
                call(c, op, entries(src, dst), src, dst, uv_mode, st=st)
        for rep in range(2):
            src.blank().fill(content(w, h, n, 90 + rep))
            dst_eq.blank()
            dst_cl.blank()
            load(everything)
            for op, dst, uv_mode in jobs:
                dst.fill(expected(w, h, n, 90 + rep, op, uv_mode))
            g.replay()
            verify(everything, ("graph replay", rep))
