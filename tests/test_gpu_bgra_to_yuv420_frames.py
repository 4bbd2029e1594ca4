"""Four-channel BGRA / RGBA (CV_8UC4) in, planar 4:2:0 (I420 / YV12) or NV12 out on a LIST of pitched device frames on the GPU:
mi_equalize_hist_bgra_to_yuv420_frames_dev and mi_clahe_bgra_to_yuv420_frames_dev.  Expected bytes are bgra_yuv420_layouts.expected4
(the three-channel builder on the image with its fourth byte removed), computed once per (image, op, order, uv_mode) and shared
read-only; pixels are full-range random bytes, the fourth byte included, and the frames of a list have distinct content.  Every image
is its own sentinel-filled torch allocation and so is every output surface (a Y plane and, behind gaps, its U and its V plane, or its
UV plane) unless a test says otherwise, with guard bytes before, between and behind the planes; every allocation is compared WHOLE,
inputs included: pitch padding, gaps and guards keep their sentinel.  Every comparison in this file is exact.  After every call the
deltas of all four "bgra_yuv420*" counters are asserted: a list call, planar or interleaved, moves only
"bgra_yuv420_list_frames_vec" / "bgra_yuv420_list_frames_bytes", by the FRAMES that took each walk under the header's rule restated
in Pool.frame_vec.

How many workgroups a frame gets (B) is not observable and no test asserts it, but the shapes of test_loops_past_their_first_step are
chosen by it, as in tests/test_gpu_bgra_to_yuv420.py (its docstring has the arithmetic of each shape): the list form takes
launch_bgra_to_yuv420's grid, B = min(blocks_per_frame(W*H*11/4 bytes, H/2 rows, n, 2048), ceil(items / 256)) with items counted by
what the SHAPE allows, so B <= max(1, floor(W*H*11/4 / 16384)), B <= H/2, and the 256 lanes of a workgroup step through the frame by
stride = 256 * B items.  A shape with more items than 256 * min(both bounds) makes at least one lane take a second step.  B comes from
the shape alone, so a frame that takes the byte walk inside a vector-shaped call steps through its 2 x 2 blocks with the vector walk's
stride: 8 times as many steps."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, CHROMA_PLANAR, CHROMA_INTERLEAVED, BgrYuv420FrameDev
import bgra_yuv420_layouts as layouts
from bgra_yuv420_layouts import BgraIn, Nv12Out, Yuv420Out, as_fmt, rand_images4

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = layouts.SENT
HEAD = 32                 # guard bytes in front of the first plane of an allocation
ORDERS = [ORDER_BGR, ORDER_RGB]
UV_MODES = [UV_COPY, UV_FILL128]
FMTS = ["i420", "yv12", "nv12", "side"]
EQ = ("eq", None)
COUNTERS = layouts.COUNTERS + layouts.LIST_COUNTERS


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in COUNTERS)


def moved(c, before):
    return tuple(a - b for a, b in zip(counters(c), before))


@functools.lru_cache(maxsize=None)
def _expected(img_bytes, w, h, op, order, uv_mode):
    out = layouts.expected4(np.frombuffer(img_bytes, np.uint8).reshape(h, w, 4), op, order, uv_mode)
    out.setflags(write=False)
    return out


def expected4(img, op, order, uv_mode):
    """The tight I420 frame the call must produce for `img` (H x W x 4): computed once per (image, op, order, uv_mode), read-only."""
    h, w = img.shape[:2]
    return _expected(img.tobytes(), w, h, op, order, uv_mode)


class Arena:
    """One sentinel-filled torch allocation and the host image of what it must hold."""

    def __init__(self, nbytes, head=HEAD):
        self.buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.img = np.full(nbytes, SENT, np.uint8)
        self.top = head

    def carve(self, nbytes, skew=0, gap=0):
        """The next nbytes, `skew` bytes past a 16-byte boundary, at least `gap` bytes behind the previous piece."""
        off = (self.top + gap + 15) // 16 * 16 + skew
        self.top = off + nbytes
        assert self.top <= self.img.size
        return off

    def upload(self):
        self.buf.copy_(xfer.to_device(self.img))

    def clear(self):
        self.buf.fill_(SENT)
        self.img[:] = SENT

    def diff(self):
        got = xfer.to_host(self.buf)
        return int((got != self.img).sum()), np.flatnonzero(got != self.img)[:8]


def span(rows, row_bytes, pitch):
    return (rows - 1) * pitch + row_bytes


class Plane:
    """`rows` rows of `row_bytes` bytes at `pitch`: carved out of `arena`, or (at: a byte offset) laid over bytes carved before."""

    def __init__(self, arena, rows, row_bytes, pitch=None, skew=0, gap=0, at=None):
        self.rows, self.row_bytes, self.pitch, self.arena = rows, row_bytes, pitch or row_bytes, arena
        self.off = arena.carve(span(rows, row_bytes, self.pitch), skew, gap) if at is None else at
        assert self.off + span(rows, row_bytes, self.pitch) <= arena.img.size

    @property
    def ptr(self):
        return self.arena.buf.data_ptr() + self.off

    def put(self, data):
        """The bytes the plane's rows must hold, into the arena's host image."""
        a = self.arena.img
        d = np.asarray(data, np.uint8).reshape(self.rows, self.row_bytes)
        for r in range(self.rows):
            a[self.off + r * self.pitch: self.off + r * self.pitch + self.row_bytes] = d[r]


class Pool:
    """n frames of one shape: a pool of four-byte-per-pixel surfaces (ins) and an encoder's frame pool (ys, us, vs: the planes of a
    surface share one allocation, at least 32 guard bytes apart).  fmt: "i420" (U before V), "yv12" (the V plane lies before the U
    plane; us is still U), "side" (ONE chroma plane of H/2 rows at c_pitch >= W holds the U rows and, W/2 bytes further, the V rows)
    or "nv12" (us is the interleaved UV plane of H/2 rows of W bytes, vs holds None).  skew(k) -> the offsets of frame k's four
    addresses (in, y, c0, c1) past a 16-byte boundary.  arenas: (in, out) allocations to carve the images / the surfaces from instead
    (None: one each, as usual), `gaps` bytes in front of every image, Y plane, first and second chroma plane."""

    def __init__(self, w, h, n, fmt="i420", in_pitch=None, y_pitch=None, c_pitch=None, skew=lambda k: (0, 0, 0, 0), alloc_order=None,
                 arenas=None, gaps=(0, 0, 32, 32)):
        self.w, self.h, self.n, self.fmt = w, h, n, fmt
        self.planar = fmt != "nv12"
        wide = fmt in ("side", "nv12")
        ip, yp, cp = in_pitch or 4 * w, y_pitch or w, c_pitch or (w if wide else w // 2)
        assert cp >= (w if wide else w // 2)
        self.ins, self.ys, self.us, self.vs = [None] * n, [None] * n, [None] * n, [None] * n
        for k in (alloc_order or range(n)):
            si, sy, su, sv = skew(k)
            ain, aout = arenas or (None, None)
            ain = ain or Arena(HEAD + 16 + si + span(h, 4 * w, ip) + 48)
            aout = aout or Arena(HEAD + 16 + sy + span(h, w, yp) + 2 * (48 + 16 + max(su, sv) + span(h // 2, w, cp)) + 48)
            self.ins[k] = Plane(ain, h, 4 * w, ip, si, gaps[0])
            self.ys[k] = Plane(aout, h, w, yp, sy, gaps[1])
            if fmt == "nv12":
                self.us[k] = Plane(aout, h // 2, w, cp, su, gaps[2])
            elif fmt == "side":
                both = Plane(aout, h // 2, w, cp, su, gaps[2])
                self.us[k] = Plane(aout, h // 2, w // 2, cp, at=both.off)
                self.vs[k] = Plane(aout, h // 2, w // 2, cp, at=both.off + w // 2)
            elif fmt == "yv12":
                self.vs[k] = Plane(aout, h // 2, w // 2, cp, sv, gaps[2])
                self.us[k] = Plane(aout, h // 2, w // 2, cp, su, gaps[3])
            else:
                self.us[k] = Plane(aout, h // 2, w // 2, cp, su, gaps[2])
                self.vs[k] = Plane(aout, h // 2, w // 2, cp, sv, gaps[3])
        self.pitches = (ip, yp, cp)

    @property
    def chroma(self):
        return CHROMA_PLANAR if self.planar else CHROMA_INTERLEAVED

    def shape_vec(self):
        """The header's rule, the shape's part: W % 16 == 0, in_pitch and y_pitch multiples of 16, c_pitch a multiple of 16
        (interleaved) or 8 (planar)."""
        ip, yp, cp = self.pitches
        return self.w % 16 == 0 and ip % 16 == 0 and yp % 16 == 0 and cp % (8 if self.planar else 16) == 0

    def frame_vec(self, k):
        """... and the frame's part: in and y multiples of 16, c0 a multiple of 16 (interleaved) or c0 and c1 multiples of 8 (planar)."""
        if not (self.shape_vec() and self.ins[k].ptr % 16 == 0 and self.ys[k].ptr % 16 == 0):
            return False
        return (self.us[k].ptr % 8 == 0 and self.vs[k].ptr % 8 == 0) if self.planar else self.us[k].ptr % 16 == 0

    def in_arenas(self):
        return list({id(p.arena): p.arena for p in self.ins}.values())

    def out_arenas(self):
        return list({id(p.arena): p.arena for p in self.ys}.values())

    def load(self, images):
        """Upload `images` into the image pool; every surface back to the sentinel."""
        for k, img in enumerate(images):
            self.ins[k].put(img)
        for a in self.in_arenas():
            a.upload()
        return self.clear()

    def clear(self):
        for a in self.out_arenas():
            a.clear()
        return self

    def expect(self, k, frame):
        """The tight I420 `frame` of expected4() into surface k."""
        w, h = self.w, self.h
        ysz, csz = w * h, w * h // 4
        self.ys[k].put(frame[:ysz])
        if self.planar:
            self.us[k].put(frame[ysz: ysz + csz])
            self.vs[k].put(frame[ysz + csz:])
        else:
            self.us[k].put(as_fmt(frame, w, h, "nv12")[ysz:])

    def entries(self, idx=None, ins=None):
        idx = range(self.n) if idx is None else idx
        ins = self.ins if ins is None else ins
        return [BgrYuv420FrameDev.of(ins[k].ptr, self.ys[k].ptr, self.us[k].ptr, self.vs[k].ptr if self.planar else None) for k in idx]

    def verify(self, what):
        for a in self.in_arenas():
            nbad, where = a.diff()
            assert nbad == 0, ("an input allocation was written", what, nbad, where)
        for i, a in enumerate(self.out_arenas()):
            nbad, where = a.diff()
            assert nbad == 0, (what, "output allocation", i, nbad, where)


def call(c, op, frames, w, h, pitches, order, uv_mode, chroma=CHROMA_PLANAR, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = (frames, w, h, *pitches, chroma, order, uv_mode)
    st = stream() if st is None else st
    if kind == "eq":
        c.equalize_hist_bgra_to_yuv420_frames_dev(*a, stream=st)
    else:
        c.clahe_bgra_to_yuv420_frames_dev(*a, *cfg, stream=st)


def check(c, images, pool, op, order, uv_mode, perm=None, loaded=False):
    """One call on `images`: every surface is the oracle's frame for its own image, guards and inputs untouched, and the two list
    counters moved by the frames of each walk.  perm: the order in which the frames appear in the list.  loaded: the images are in
    the pool already."""
    w, h = pool.w, pool.h
    pool.clear() if loaded else pool.load(images)
    for k, img in enumerate(images):
        pool.expect(k, expected4(img, op, order, uv_mode))
    idx = list(range(pool.n)) if perm is None else list(perm)
    before = counters(c)
    call(c, op, pool.entries(idx), w, h, pool.pitches, order, uv_mode, chroma=pool.chroma)
    torch.cuda.synchronize()
    pool.verify((w, h, pool.fmt, op, order, uv_mode))
    n_vec = sum(pool.frame_vec(k) for k in idx)
    assert moved(c, before) == (0, 0, n_vec, len(idx) - n_vec), (moved(c, before), n_vec, len(idx))


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


def layout(lay, fmt):
    """The Pool arguments of a layout for `fmt`: c_pitch is given per kind of chroma row (narrow: W/2 bytes; wide: W bytes)."""
    kw = dict(lay)
    narrow, wide = kw.pop("c_pitch", None), kw.pop("c_pitch_wide", None)
    kw["c_pitch"] = wide if fmt in ("side", "nv12") else narrow
    return kw


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
ODD_66 = dict(in_pitch=265, y_pitch=67, c_pitch=35, c_pitch_wide=67, skew=lambda k: (1, 1, 1, 1))
# planar: c0 and c1 at a multiple of 8 that is not a multiple of 16 and c_pitch 40 / 72: the chroma stores are 8-byte stores;
# interleaved: the UV plane at a multiple of 16, c_pitch 96
PITCHED_64 = dict(in_pitch=272, y_pitch=80, c_pitch=40, c_pitch_wide=72, skew=lambda k: (0, 0, 8, 8))
PITCHED_64_NV12 = dict(in_pitch=272, y_pitch=80, c_pitch_wide=96)
PARITY = [
    # id, W, H, n, layout, frames on the vector walk, the non-dividing CLAHE grid (REFLECT_101 padding) behind 1 x 1 and 2 x 1
    ("2x2", 2, 2, 1, {}, False, (2.0, 3, 1)),                        # one byte block
    ("16x2", 16, 2, 2, {}, True, (2.0, 3, 1)),                       # one vector group
    ("48x6", 48, 6, 2, {}, True, (2.0, 5, 4)),                       # gx_n = 3: the row walk wraps
    ("64x32-pitched", 64, 32, 3, PITCHED_64, True, (4.0, 5, 3)),     # padding; planar chroma addresses and pitch at 8 (mod 16)
    ("66x34-odd", 66, 34, 2, ODD_66, False, (3.0, 4, 3)),            # odd pitches, every address at offset 1: bytes throughout
]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,w,h,n,lay,vec,odd_grid", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, lay, vec, odd_grid, fmt):
    if name == "64x32-pitched" and fmt == "nv12":
        lay = PITCHED_64_NV12
    pool = Pool(w, h, n, fmt, **layout(lay, fmt))
    assert [pool.frame_vec(k) for k in range(n)] == [vec] * n
    if fmt == "yv12":
        assert all(pool.vs[k].ptr < pool.us[k].ptr for k in range(n))
    if fmt == "side":
        assert all(pool.vs[k].ptr == pool.us[k].ptr + w // 2 for k in range(n)) and pool.pitches[2] >= w
    if name == "66x34-odd":
        assert all(p.ptr % 16 == 1 for p in pool.ins + pool.ys + pool.us) and all(v % 2 for v in pool.pitches)
    if name == "64x32-pitched" and pool.planar:
        assert pool.pitches[2] % 16 == 8 and all(p.ptr % 16 == 8 for p in pool.us + pool.vs)
    assert w % odd_grid[1] or h % odd_grid[2]
    images = rand_images4(w, h, n, 31)
    pool.load(images)
    for op in (EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1)), ("clahe", odd_grid)):
        for order in ORDERS:
            for uv_mode in UV_MODES:
                check(c, images, pool, op, order, uv_mode, loaded=True)


# ---- 2. per-frame alignment ------------------------------------------------------------------------------------------------------
ALIGN_OPS = ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, UV_FILL128))
ONE_ADDRESS = [("i420", "in", 0, 1), ("i420", "y", 1, 1), ("i420", "c0", 2, 4), ("i420", "c1", 3, 4),
               ("nv12", "in", 0, 1), ("nv12", "y", 1, 1), ("nv12", "c0", 2, 8)]


@pytest.mark.parametrize("fmt,which,slot,by", ONE_ADDRESS, ids=[f"{a[0]}-{a[1]}" for a in ONE_ADDRESS])
def test_one_address_misaligned(c, fmt, which, slot, by):
    """64 x 32 at pitches the shape's rule allows.  The middle frame of three has ONE address off its modulus (in, y: 1 past a multiple
    of 16; planar c0, c1: 4 past a multiple of 8; the interleaved c0: 8 past a multiple of 16): it alone takes the 2 x 2 byte walk
    inside the same launch and counts as bytes, its neighbours keep the groups and count as vec."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, fmt, in_pitch=272, y_pitch=80, c_pitch=40 if fmt == "i420" else 96,
                skew=lambda k: tuple(by * int(k == 1 and i == slot) for i in range(4)))
    assert pool.shape_vec() and [pool.frame_vec(k) for k in range(n)] == [True, False, True]
    planes = [pool.ins[1], pool.ys[1], pool.us[1]] + ([pool.vs[1]] if pool.planar else [])
    mods = [16, 16] + ([8, 8] if pool.planar else [16])
    assert [p.ptr % m for p, m in zip(planes, mods)] == [by * int(i == slot) for i in range(len(planes))]
    images = rand_images4(w, h, n, 32)
    for op, order, uv_mode in ALIGN_OPS:
        check(c, images, pool, op, order, uv_mode)


ONE_PITCH = [("i420", "in_pitch", (264, 80, 40)), ("i420", "y_pitch", (272, 72, 40)), ("i420", "c_pitch", (272, 80, 36)),
             ("nv12", "in_pitch", (264, 80, 96)), ("nv12", "y_pitch", (272, 72, 96)), ("nv12", "c_pitch", (272, 80, 72))]


@pytest.mark.parametrize("fmt,which,pitches", ONE_PITCH, ids=[f"{p[0]}-{p[1]}" for p in ONE_PITCH])
def test_one_pitch_misaligned(c, fmt, which, pitches):
    """Every address a multiple of 16 and ONE pitch off its modulus (in_pitch, y_pitch: a multiple of 8 only; the planar c_pitch: 36, a
    multiple of 4 only; the interleaved c_pitch: 72, a multiple of 8 only): every frame of the call takes bytes and counts as bytes;
    the same bytes, the same guards."""
    w, h, n = 64, 32, 3
    ip, yp, cp = pitches
    planar = fmt == "i420"
    assert ip >= 4 * w and yp >= w and cp >= (w // 2 if planar else w) and (ip % 16, yp % 16, cp % (8 if planar else 16)).count(0) == 2
    pool = Pool(w, h, n, fmt, in_pitch=ip, y_pitch=yp, c_pitch=cp)
    assert all(p.ptr % 16 == 0 for p in pool.ins + pool.ys + pool.us + (pool.vs if planar else []))
    assert not pool.shape_vec() and not any(pool.frame_vec(k) for k in range(n))
    images = rand_images4(w, h, n, 32)
    for op, order, uv_mode in ALIGN_OPS:
        check(c, images, pool, op, order, uv_mode)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
PITCHED_112 = dict(in_pitch=464, y_pitch=128, c_pitch=72, c_pitch_wide=128, skew=lambda k: (0, 0, 8, 8))
PITCHED_16000 = dict(in_pitch=64016, y_pitch=16016, c_pitch=8008, c_pitch_wide=16016, skew=lambda k: (0, 0, 8, 8))
LOOP_SHAPES = [
    # id, W, H, n, layout, items of a frame by the shape (16 x 2 groups or 2 x 2 blocks), vector shape -- LOOP_SHAPES of
    # tests/test_gpu_bgra_to_yuv420.py, whose docstring has the arithmetic
    ("112x80-pitched", 112, 80, 2, PITCHED_112, 280, True),              # B = 1: 280 groups for 256 lanes
    ("16000x6-pitched", 16000, 6, 2, PITCHED_16000, 3000, True),         # B <= 3: gx wraps on more than one step of a lane
    ("66x34-odd", 66, 34, 2, ODD_66, 561, False),                        # the byte walk: three steps
    # the pitched vector shape with the second of two frames one byte off: B is sized for 280 groups (B = 1), so that frame's
    # 56 x 40 = 2240 blocks of 2 x 2 take 9 steps of 256 lanes while frame 0 walks its groups
    ("112x80-one-frame-bytes", 112, 80, 2, dict(PITCHED_112, skew=lambda k: (k, 0, 8, 8)), 280, True),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("name,w,h,n,lay,items,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, lay, items, vec, fmt, order):
    """The conversion where a lane owns more than one group / block: with the histogram (equalizeHist, U and V computed) and without
    it (CLAHE 2 x 2, chroma filled)."""
    kw = layout(lay, fmt)
    if fmt == "nv12" and vec:
        kw["skew"] = (lambda k: (k, 0, 0, 0)) if name == "112x80-one-frame-bytes" else (lambda k: (0, 0, 0, 0))
    pool = Pool(w, h, n, fmt, **kw)
    assert pool.shape_vec() == vec and items == (w * h // 32 if vec else w * h // 4)
    assert items > 256 * min(max(1, w * h * 11 // 4 // 16384), h // 2), "the shape would not loop"
    if name == "112x80-one-frame-bytes":
        assert [pool.frame_vec(k) for k in range(n)] == [True, False] and w * h // 4 == 2240
    else:
        assert [pool.frame_vec(k) for k in range(n)] == [vec] * n
    images = rand_images4(w, h, n, 33)
    pool.load(images)
    check(c, images, pool, EQ, order, UV_COPY, loaded=True)
    check(c, images, pool, ("clahe", (2.0, 2, 2)), order, UV_FILL128, loaded=True)


# ---- 4. a table, not a stride ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_permuted_list_of_shuffled_pools(c, fmt):
    """The pools are allocated in a shuffled order and the list names the frames in another one: the addresses are neither monotonic
    nor at one stride, and every frame equals the oracle's result for its own image."""
    w, h, n = 48, 6, 5
    pool = Pool(w, h, n, fmt, in_pitch=208, y_pitch=64, c_pitch=32 if fmt == "i420" else 64, alloc_order=(3, 0, 4, 1, 2))
    perm = (2, 4, 0, 3, 1)
    images = rand_images4(w, h, n, 34)
    for op, order, uv_mode in ((EQ, ORDER_RGB, UV_COPY), (("clahe", (2.0, 3, 2)), ORDER_BGR, UV_COPY)):
        check(c, images, pool, op, order, uv_mode, perm=perm)


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_one_image_two_surfaces(c, fmt):
    """The same image in two entries with different output surfaces: inputs are only read, both surfaces are exact (hence equal)."""
    w, h = 48, 6
    img = rand_images4(w, h, 1, 35)[0]
    pool = Pool(w, h, 2, fmt)
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        pool.load([img, img])
        for k in range(2):
            pool.expect(k, expected4(img, op, ORDER_BGR, UV_COPY))
        before = counters(c)
        call(c, op, pool.entries(ins=[pool.ins[0]] * 2), w, h, pool.pitches, ORDER_BGR, UV_COPY, chroma=pool.chroma)
        torch.cuda.synchronize()
        pool.verify(("one image, two surfaces", op))
        assert moved(c, before) == (0, 0, 2, 0)


# ---- 5. the fourth byte is ignored -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_the_fourth_byte_is_ignored(c, fmt):
    """A list that mixes the two walks (the middle frame's image one byte off), uploaded twice with every fourth byte complemented
    in between: the surfaces are byte-identical and both are expected4's."""
    w, h, n = 48, 6, 3
    pool = Pool(w, h, n, fmt, skew=lambda k: (int(k == 1), 0, 0, 0))
    assert [pool.frame_vec(k) for k in range(n)] == [True, False, True]
    images = rand_images4(w, h, n, 46)
    flipped = layouts.complement_x(images)
    for op, order in ((EQ, ORDER_BGR), (("clahe", (2.0, 3, 2)), ORDER_RGB)):
        check(c, images, pool, op, order, UV_COPY)
        one = [xfer.to_host(a.buf) for a in pool.out_arenas()]
        check(c, flipped, pool, op, order, UV_COPY)
        two = [xfer.to_host(a.buf) for a in pool.out_arenas()]
        assert all(np.array_equal(a, b) for a, b in zip(one, two)), op


# ---- 6. chunking -----------------------------------------------------------------------------------------------------------------
def frames_per_launch():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "common.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kFramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1))


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("n", [65, 129])
def test_chunking(c, n, fmt):
    """One frame past one and past two full launch sequences: the last sequence is of one frame.  Every frame is distinct and every
    frame is checked, and the list counters count FRAMES; here the images lie in one allocation, every surface is its own."""
    assert frames_per_launch() == 64
    w, h = 16, 2
    images = rand_images4(w, h, n, 37)
    pool = Pool(w, h, n, fmt, arenas=(Arena(HEAD + n * (4 * w * h + 32) + 64), None), gaps=(16, 0, 32, 32))
    assert len(pool.out_arenas()) == n and all(pool.frame_vec(k) for k in range(n))
    pool.load(images)
    for op in (EQ, ("clahe", (2.0, 1, 1))):
        check(c, images, pool, op, ORDER_RGB, UV_COPY, loaded=True)


# ---- 7. identity with the batch form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_the_batch_form(c, op, fmt):
    """The same frames in ONE strided input and ONE strided output allocation (the batch form's pitched layout with gaps): the batch
    call, and the list call over the same addresses in a second, equal pair of allocations, leave equal allocations."""
    w, h, n = 64, 32, 3
    si = dict(pitch=272, frame_gap=64, off=32)
    do = (dict(y_pitch=80, c_pitch=40, u_gap=24, v_gap=16, frame_gap=8, off=16) if fmt == "i420" else
          dict(y_pitch=80, c_pitch=96, uv_gap=32, frame_gap=48, off=16))
    mk = Yuv420Out if fmt == "i420" else Nv12Out
    images = rand_images4(w, h, n, 38)
    src = BgraIn(w, h, n, **si).upload(images)
    bat, lst = mk(w, h, n, **do), mk(w, h, n, **do)
    assert not layouts.misaligned(w, src, bat)
    before = counters(c)
    kw = dict(src.kw(), stream=stream())
    if op is EQ:
        c.equalize_hist_bgra_to_yuv420_batch_dev(src.ptr, bat.planes(), w, h, n, ORDER_BGR, UV_COPY, **kw)
    else:
        c.clahe_bgra_to_yuv420_batch_dev(src.ptr, bat.planes(), w, h, n, ORDER_BGR, UV_COPY, *op[1], **kw)
    assert moved(c, before) == (1, 0, 0, 0)
    before = counters(c)
    if fmt == "i420":
        frames = [BgrYuv420FrameDev(src.ptr + k * src.fstride, lst.y_ptr + k * lst.fstride, lst.u_ptr + k * lst.fstride,
                                    lst.v_ptr + k * lst.fstride) for k in range(n)]
        chroma = CHROMA_PLANAR
    else:
        frames = [BgrYuv420FrameDev.of(src.ptr + k * src.fstride, lst.y_ptr + k * lst.fstride, lst.uv_ptr + k * lst.fstride, None)
                  for k in range(n)]
        chroma = CHROMA_INTERLEAVED
    call(c, op, frames, w, h, (src.pitch, lst.y_pitch, lst.c_pitch), ORDER_BGR, UV_COPY, chroma=chroma)
    torch.cuda.synchronize()
    assert moved(c, before) == (0, 0, n, 0)
    got_list, got_batch = xfer.to_host(lst.buf), xfer.to_host(bat.buf)
    assert np.array_equal(got_list, got_batch), (op, np.flatnonzero(got_list != got_batch)[:8])
    ok, nbad, where = lst.same([expected4(img, op, ORDER_BGR, UV_COPY) for img in images])
    assert ok, (op, nbad, where)
    assert np.array_equal(src.host(), src.image(images)), "the input allocation was written"


# ---- 8. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "bgr_yuv420_list_frames_vec",
               "bgr_yuv420_list_frames_bytes")


@pytest.mark.parametrize("fmt,n", [("i420", 2), ("i420", 65), ("nv12", 65)])
def test_launch_contract(fmt, n):
    """Per chunk of 64 frames.  equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch -- at n = 2
    too, where the planar form would take hist_lut_kernel.  CLAHE: one MI_K_COLOR launch per chunk plus what mi_clahe_nv12_frames_dev
    launches in place on the same Y planes (with a scratch UV plane that MI_UV_COPY leaves alone in place), measured here."""
    w, h = 32, 4
    chunks = (n + 63) // 64
    images = rand_images4(w, h, n, 39)
    pool = Pool(w, h, n, fmt, in_pitch=144, y_pitch=48, c_pitch=24 if fmt == "i420" else 48,
                arenas=(Arena(HEAD + n * (144 * h + 32) + 64), None), gaps=(16, 0, 32, 32)).load(images)
    uv = torch.zeros((n, 48 * (h // 2)), dtype=torch.uint8, device="cuda:0")
    with mi_lumaeq.Context(0) as c:
        before = {k: c.get_stat(k) for k in OTHER_STATS}
        c.set_profiling(1)
        c.profile_read(reset=True)
        check(c, images, pool, EQ, ORDER_BGR, UV_COPY, loaded=True)
        got = launches(c)
        want = {"color_kernel": chunks, "equalize_lut_kernel": chunks, "lut_apply_kernel": chunks}
        assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, got
        for cfg in ((2.0, 2, 2), (2.0, 3, 1)):
            c.profile_read(reset=True)
            planes = [(pool.ys[k].ptr, uv[k].data_ptr()) for k in range(n)]
            c.clahe_nv12_frames(planes, None, w, h, UV_COPY, *cfg, y_in_pitch=48, uv_in_pitch=48, y_out_pitch=48, uv_out_pitch=48,
                                stream=stream())
            torch.cuda.synchronize()
            planar = launches(c)
            assert planar["color_kernel"] == 0 and sum(planar.values()) >= 2 * chunks, planar
            c.profile_read(reset=True)
            check(c, images, pool, ("clahe", cfg), ORDER_RGB, UV_FILL128, loaded=True)
            got = launches(c)
            assert got == dict(planar, color_kernel=chunks), (cfg, got, planar)
        c.set_profiling(0)
        assert {k: c.get_stat(k) for k in OTHER_STATS} == before


# ---- 9. errors, zero sizes -------------------------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    ip, yp, cp = 144, 48, 24
    images = rand_images4(w, h, n, 40)
    pool = Pool(w, h, n, "i420", in_pitch=ip, y_pitch=yp, c_pitch=cp).load(images)
    nv = Pool(w, h, n, "nv12", in_pitch=ip, y_pitch=yp, c_pitch=yp).load(images)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(pool.ins[k].ptr, pool.ys[k].ptr, pool.us[k].ptr, pool.vs[k].ptr) for k in range(n)]
        good_il = [(nv.ins[k].ptr, nv.ys[k].ptr, nv.us[k].ptr, None) for k in range(n)]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, ip=ip, yp=yp, cp=cp, chroma=CHROMA_PLANAR, order=ORDER_BGR, uvm=UV_COPY)
        il = dict(entries=good_il, chroma=CHROMA_INTERLEAVED, cp=yp)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (BgrYuv420FrameDev * max(1, len(a["entries"])))(*[BgrYuv420FrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["ip"], a["yp"], a["cp"], a["chroma"], a["order"], a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgra_to_yuv420_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgra_to_yuv420_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(src=good, i=None, y=None, u=None, v=None):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = list(src[-1])
            for k, val in enumerate((i, y, u, v)):
                if val is not None:
                    e[k] = None if val == "null" else val
            return dict(entries=src[:-1] + [tuple(e)])
        i2, y2, u2, v2 = good[-1]
        j2, z2, uv2, _ = good_il[-1]
        in_span, y_span, c_span, uv_span = span(h, 4 * w, ip), span(h, w, yp), span(h // 2, w // 2, cp), span(h // 2, w, yp)
        before = counters(c)
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(i="null"), last(y="null"), last(u="null"), last(v="null"),               # a null address in the last entry
               dict(il, **last(good_il, i="null")), dict(il, **last(good_il, y="null")), dict(il, **last(good_il, u="null")),
               dict(chroma=2), dict(chroma=-1),                                              # a chroma other than the two
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(il, w=31, h=0), dict(il, h=15, n=0),
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(ip=4 * w - 1), dict(ip=3 * w), dict(yp=w - 1), dict(cp=w // 2 - 1), dict(il, cp=w - 1),   # a pitch below its row
               dict(order=2), dict(order=-1), dict(uvm=2), dict(uvm=-1),                     # an order, a uv_mode other than the two
               # no in-place form, compared as address ranges with an image row of 4*W bytes.  The image's rows meeting its own Y plane:
               # the same address, and ending one byte inside it; its own U plane: the same address, and U ending on the image's first
               # byte; its own V plane: the same address, and V starting on the image's last byte
               last(y=i2), last(y=i2 + in_span - 1), last(u=i2), last(u=i2 - c_span + 1), last(v=i2), last(v=i2 + in_span - 1),
               # a plane starting in the fourth quarter of the image's rows: outside a 3*W-byte row range, inside the 4*W-byte one
               last(y=i2 + (h - 1) * ip + 3 * w + 1), last(u=i2 + (h - 1) * ip + 3 * w + 1),
               # Y meeting its own U: the same address, U starting on the last byte of the Y rows; its own V: the same address, V ending
               # on the first byte of the Y rows
               last(u=y2), last(u=y2 + y_span - 1), last(v=y2), last(v=y2 - c_span + 1),
               # c0 == c1 on a planar list
               last(v=u2), last(u=v2),
               # interleaved: the image meeting its own Y or UV plane, Y meeting its own UV plane
               dict(il, **last(good_il, y=j2)), dict(il, **last(good_il, u=j2 + in_span - 1)), dict(il, **last(good_il, u=j2 - uv_span + 1)),
               dict(il, **last(good_il, u=z2)), dict(il, **last(good_il, u=z2 + y_span - 1))]
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, **il) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written -- a null list is fine when there are no frames
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, lst=NULL_LIST), dict(il, n=0, lst=NULL_LIST), dict(il, w=0)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar form refuses: its status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, yp=1 << 25, cp=1 << 24)
        planar = L.mi_clahe_u8_batch_dev(hd, y2, 1 << 25, 1 << 26, y2, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, y2, yp, 0, y2, yp, 0, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar and cl(2048, 1024, **il) == planar
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        nv.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert moved(c, before) == (0, 0, 0, 0), "a refused or empty call moved a counter"
        c.set_profiling(0)
        # and the context still works; on an interleaved list c1 is ignored, whatever it is (here: the frame's own Y plane)
        check(c, images, pool, EQ, ORDER_RGB, UV_FILL128, loaded=True)
        for k, img in enumerate(images):
            nv.expect(k, expected4(img, EQ, ORDER_BGR, UV_COPY))
        frames = [BgrYuv420FrameDev(nv.ins[k].ptr, nv.ys[k].ptr, nv.us[k].ptr, nv.ys[k].ptr) for k in range(n)]
        call(c, EQ, frames, w, h, nv.pitches, ORDER_BGR, UV_COPY, chroma=CHROMA_INTERLEAVED)
        torch.cuda.synchronize()
        nv.verify("an interleaved list with a c1")


# ---- 10. pipe pending ------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(rand_images4(w, h, 1, 41))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            before = counters(c)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, pool.entries(), w, h, pool.pitches, ORDER_BGR, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert moved(c, before) == (0, 0, 0, 0)
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")


# ---- 11. streams and hipGraph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_stream_and_graph_capture(fmt):
    """A call on a non-default stream.  Then one eager call of the shape, ONE capture of that call on a single stream (one linear
    chain, no parallel branches) and ONE replay onto fresh input bytes at the same addresses: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    lay = PITCHED_64_NV12 if fmt == "nv12" else PITCHED_64
    pool = Pool(w, h, n, fmt, **layout(lay, fmt))
    with mi_lumaeq.Context(0) as c:
        images = rand_images4(w, h, n, 42)
        pool.load(images)
        cl = ("clahe", (2.0, 4, 2))
        for k, img in enumerate(images):
            pool.expect(k, expected4(img, cl, ORDER_RGB, UV_COPY))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(c, cl, pool.entries(), w, h, pool.pitches, ORDER_RGB, UV_COPY, chroma=pool.chroma, st=side.cuda_stream)
        side.synchronize()
        pool.verify("side stream")
        for op, uv_mode in ((EQ, UV_COPY), (cl, UV_FILL128)):
            check(c, images, pool, op, ORDER_BGR, uv_mode)                                    # sizes the scratch
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(c, op, pool.entries(), w, h, pool.pitches, ORDER_BGR, uv_mode, chroma=pool.chroma,
                     st=torch.cuda.current_stream().cuda_stream)
            fresh = rand_images4(w, h, n, 43)
            pool.load(fresh)
            for k, img in enumerate(fresh):
                pool.expect(k, expected4(img, op, ORDER_BGR, uv_mode))
            g.replay()
            torch.cuda.synchronize()
            pool.verify(("graph replay", op))
