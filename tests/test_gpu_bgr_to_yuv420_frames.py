"""Interleaved BGR / RGB in, planar 4:2:0 (I420 / YV12) out on a LIST of pitched device frames on the GPU:
mi_equalize_hist_bgr_to_yuv420_frames_dev and mi_clahe_bgr_to_yuv420_frames_dev.  Expected bytes are bgr_yuv420_layouts.expected (the
tight I420 frame of the batch form's tests: Y of oracle.nv12_frame(oracle.bgr_to_nv12(img), ...), its chroma de-interleaved), computed
once per (image, op, order, uv_mode) and shared read-only; pixels are full-range random bytes unless a test says otherwise, and the
frames of a list have distinct content.  Every image is its own sentinel-filled torch allocation and so is every output surface (a Y
plane and, behind gaps, its U and its V plane) unless a test says otherwise, with guard bytes before, between and behind the planes;
every allocation is compared WHOLE, inputs included: pitch padding, gaps and guards keep their sentinel.  Every comparison in this
file is exact.  After every call the deltas of all four "bgr_yuv420*" counters are asserted: a PLANAR list call moves only
"bgr_yuv420_list_frames_vec" / "bgr_yuv420_list_frames_bytes", by the FRAMES that took each walk under the header's rule restated in
Pool.frame_vec.

How many workgroups a frame gets (B) is not observable and no test asserts it, but the shapes of test_loops_past_their_first_step are
chosen by it, as in tests/test_gpu_bgr_to_yuv420.py: the list form takes launch_bgr_to_yuv420's grid,
B = min(blocks_per_frame(W*H*9/4 bytes, H/2 rows, n, 2048), ceil(items / 256)) with items counted by what the SHAPE allows, and
blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which
only lowers it.  So B <= max(1, floor(W*H*9/4 / 16384)), B <= H/2, and the 256 lanes of a workgroup step through the frame by
stride = 256 * B items: 16 x 2 pixel groups on the vector walk (gx_n = W/16 per row pair, the carried walk by += dby, gx += dgx with
dby = stride / gx_n, dgx = stride % gx_n and a wrap when gx >= gx_n), 2 x 2 pixel blocks on the byte walk.  A shape with more items
than 256 * min(both bounds) makes at least one lane take a second step.  B comes from the shape alone, so a frame that takes the byte
walk inside a vector-shaped call steps through its 2 x 2 blocks with the vector walk's stride: 8 times as many steps."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, CHROMA_PLANAR, CHROMA_INTERLEAVED, BgrYuv420FrameDev
import bgr_yuv420_layouts as layouts
from bgr_yuv420_layouts import BgrIn, Yuv420Out, as_fmt, rand_images

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = layouts.SENT
HEAD = 32                 # guard bytes in front of the first plane of an allocation
ORDERS = [ORDER_BGR, ORDER_RGB]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)
COUNTERS = ("bgr_yuv420_vec", "bgr_yuv420_bytes", "bgr_yuv420_list_frames_vec", "bgr_yuv420_list_frames_bytes")
assert COUNTERS[:2] == layouts.COUNTERS


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in COUNTERS)


def moved(c, before):
    return tuple(a - b for a, b in zip(counters(c), before))


@functools.lru_cache(maxsize=None)
def _expected(img_bytes, w, h, op, order, uv_mode):
    out = layouts.expected(np.frombuffer(img_bytes, np.uint8).reshape(h, w, 3), op, order, uv_mode)
    out.setflags(write=False)
    return out


def expected(img, op, order, uv_mode):
    """The tight I420 frame the call must produce for `img` (H x W x 3, in the order the call is told): computed once per (image, op,
    order, uv_mode) and shared, read-only, by the tests that need it."""
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
    """n frames of one shape: an image pool (ins) and a software encoder's frame pool (ys, us, vs: the three planes of a surface share
    one allocation, at least 32 guard bytes apart).  skew(k) -> the offsets of frame k's four addresses (in, y, u, v) past a 16-byte
    boundary.  v_first: the V plane lies before the U plane (YV12 address order; us is still U).  side_by_side: ONE chroma plane of H/2
    rows at c_pitch >= W holds the U rows and, W/2 bytes further, the V rows (the v skew is not used).  alloc_order: the order in which
    the frames' allocations are made; arenas: (in, out) allocations to carve the images / the surfaces from instead (None: one each,
    as usual), `gaps` bytes in front of every image, Y plane, first and second chroma plane."""

    def __init__(self, w, h, n, in_pitch=None, y_pitch=None, c_pitch=None, skew=lambda k: (0, 0, 0, 0), v_first=False, side_by_side=False,
                 alloc_order=None, arenas=None, gaps=(0, 0, 32, 32)):
        self.w, self.h, self.n = w, h, n
        ip, yp, cp = in_pitch or 3 * w, y_pitch or w, c_pitch or (w if side_by_side else w // 2)
        assert cp >= (w if side_by_side else w // 2)
        self.ins, self.ys, self.us, self.vs = [None] * n, [None] * n, [None] * n, [None] * n
        for k in (alloc_order or range(n)):
            si, sy, su, sv = skew(k)
            ain, aout = arenas or (None, None)
            ain = ain or Arena(HEAD + 16 + si + span(h, 3 * w, ip) + 48)
            aout = aout or Arena(HEAD + 16 + sy + span(h, w, yp) + 2 * (48 + 16 + max(su, sv) + span(h // 2, w, cp)) + 48)
            self.ins[k] = Plane(ain, h, 3 * w, ip, si, gaps[0])
            self.ys[k] = Plane(aout, h, w, yp, sy, gaps[1])
            if side_by_side:
                both = Plane(aout, h // 2, w, cp, su, gaps[2])
                self.us[k] = Plane(aout, h // 2, w // 2, cp, at=both.off)
                self.vs[k] = Plane(aout, h // 2, w // 2, cp, at=both.off + w // 2)
            elif v_first:
                self.vs[k] = Plane(aout, h // 2, w // 2, cp, sv, gaps[2])
                self.us[k] = Plane(aout, h // 2, w // 2, cp, su, gaps[3])
            else:
                self.us[k] = Plane(aout, h // 2, w // 2, cp, su, gaps[2])
                self.vs[k] = Plane(aout, h // 2, w // 2, cp, sv, gaps[3])
        self.pitches = (ip, yp, cp)

    def shape_vec(self):
        """The header's rule, the shape's part: W % 16 == 0, in_pitch and y_pitch multiples of 16, c_pitch a multiple of 8."""
        ip, yp, cp = self.pitches
        return self.w % 16 == 0 and ip % 16 == 0 and yp % 16 == 0 and cp % 8 == 0

    def frame_vec(self, k):
        """... and the frame's part: in and y multiples of 16, c0 and c1 multiples of 8."""
        return (self.shape_vec() and self.ins[k].ptr % 16 == 0 and self.ys[k].ptr % 16 == 0 and self.us[k].ptr % 8 == 0
                and self.vs[k].ptr % 8 == 0)

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
        """The tight I420 `frame` of expected() into surface k."""
        ysz, csz = self.w * self.h, self.w * self.h // 4
        self.ys[k].put(frame[:ysz])
        self.us[k].put(frame[ysz: ysz + csz])
        self.vs[k].put(frame[ysz + csz:])

    def verify(self, what):
        for a in self.in_arenas():
            nbad, where = a.diff()
            assert nbad == 0, ("an input allocation was written", what, nbad, where)
        for i, a in enumerate(self.out_arenas()):
            nbad, where = a.diff()
            assert nbad == 0, (what, "output allocation", i, nbad, where)


def entries(ins, ys, us, vs):
    return [BgrYuv420FrameDev(i.ptr, y.ptr, u.ptr, v.ptr) for i, y, u, v in zip(ins, ys, us, vs)]


def call(c, op, frames, w, h, pitches, order, uv_mode, chroma=CHROMA_PLANAR, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = (frames, w, h, *pitches, chroma, order, uv_mode)
    st = stream() if st is None else st
    if kind == "eq":
        c.equalize_hist_bgr_to_yuv420_frames_dev(*a, stream=st)
    else:
        c.clahe_bgr_to_yuv420_frames_dev(*a, *cfg, stream=st)


def check(c, images, pool, op, order, uv_mode, perm=None, loaded=False):
    """One call on `images`: every surface is the oracle's frame for its own image, guards and inputs untouched, and the two list
    counters moved by the frames of each walk.  perm: the order in which the frames appear in the list.  loaded: the images are in
    the pool already."""
    w, h = pool.w, pool.h
    pool.clear() if loaded else pool.load(images)
    for k, img in enumerate(images):
        pool.expect(k, expected(img, op, order, uv_mode))
    idx = list(range(pool.n)) if perm is None else list(perm)
    before = counters(c)
    call(c, op, entries(*([p[k] for k in idx] for p in (pool.ins, pool.ys, pool.us, pool.vs))), w, h, pool.pitches, order, uv_mode)
    torch.cuda.synchronize()
    pool.verify((w, h, op, order, uv_mode))
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


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
ODD_66 = dict(in_pitch=201, y_pitch=67, c_pitch=35, skew=lambda k: (1, 1, 1, 1))
# c0 and c1 at a multiple of 8 that is not a multiple of 16: the chroma stores are 8-byte stores
PITCHED_64 = dict(in_pitch=208, y_pitch=80, c_pitch=40, skew=lambda k: (0, 0, 8, 8))
PARITY = [
    # id, W, H, n, layout, frames on the vector walk, the non-dividing CLAHE grid (REFLECT_101 padding) behind 1 x 1 and 2 x 1
    ("2x2", 2, 2, 1, {}, False, (2.0, 3, 1)),                        # one byte-path block
    ("16x2", 16, 2, 2, {}, True, (2.0, 3, 1)),                       # one vector group
    ("64x32-tight", 64, 32, 3, {}, True, (4.0, 5, 3)),
    ("64x32-pitched", 64, 32, 3, PITCHED_64, True, (4.0, 5, 3)),     # padding; chroma addresses and pitch at 8 (mod 16)
    ("66x34-odd", 66, 34, 2, ODD_66, False, (3.0, 4, 3)),            # odd pitches, every address at offset 1: bytes throughout
]


@pytest.mark.parametrize("v_first", [False, True], ids=["i420", "yv12"])
@pytest.mark.parametrize("name,w,h,n,layout,vec,odd_grid", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, layout, vec, odd_grid, v_first):
    pool = Pool(w, h, n, v_first=v_first, **layout)
    assert [pool.frame_vec(k) for k in range(n)] == [vec] * n
    assert all((pool.vs[k].ptr < pool.us[k].ptr) == v_first for k in range(n))
    if name == "66x34-odd":
        assert all(p.ptr % 16 == 1 for p in pool.ins + pool.ys + pool.us + pool.vs) and all(v % 2 for v in pool.pitches)
    if name == "64x32-pitched":
        assert pool.pitches == (208, 80, 40) and all(p.ptr % 16 == 8 for p in pool.us + pool.vs)
    assert w % odd_grid[1] or h % odd_grid[2]
    images = rand_images(w, h, n, 31)
    pool.load(images)
    for op in (EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1)), ("clahe", odd_grid)):
        for order in ORDERS:
            for uv_mode in UV_MODES:
                check(c, images, pool, op, order, uv_mode, loaded=True)


# ---- 2. per-frame alignment ------------------------------------------------------------------------------------------------------
ALIGN_OPS = ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, UV_FILL128))
ONE_ADDRESS = [("in", 0, 1), ("y", 1, 1), ("c0", 2, 4), ("c1", 3, 4)]


@pytest.mark.parametrize("which,slot,by", ONE_ADDRESS, ids=[a[0] for a in ONE_ADDRESS])
def test_one_address_misaligned(c, which, slot, by):
    """64 x 32 at pitches 208 / 80 / 40: the shape allows the 16 x 2 groups.  The middle frame of three has ONE address off its modulus
    (in, y: 1 past a multiple of 16; c0, c1: 4 past a multiple of 8): it alone takes the 2 x 2 byte walk inside the same launch and
    counts as bytes, its neighbours keep the groups and count as vec."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, in_pitch=208, y_pitch=80, c_pitch=40, skew=lambda k: tuple(by * int(k == 1 and i == slot) for i in range(4)))
    assert pool.shape_vec() and [pool.frame_vec(k) for k in range(n)] == [True, False, True]
    planes = (pool.ins[1], pool.ys[1], pool.us[1], pool.vs[1])
    assert [p.ptr % (16 if i < 2 else 8) for i, p in enumerate(planes)] == [by * int(i == slot) for i in range(4)]
    images = rand_images(w, h, n, 32)
    for op, order, uv_mode in ALIGN_OPS:
        check(c, images, pool, op, order, uv_mode)


@pytest.mark.parametrize("which,pitches", [("in_pitch", (200, 80, 40)), ("y_pitch", (208, 72, 40)), ("c_pitch", (208, 80, 36))],
                         ids=["in_pitch", "y_pitch", "c_pitch"])
def test_one_pitch_misaligned(c, which, pitches):
    """Every address a multiple of 16 and ONE pitch off its modulus (in_pitch, y_pitch: a multiple of 8 only; c_pitch: 36, a multiple of
    4 only): every frame of the call takes bytes and counts as bytes; the same bytes, the same guards."""
    w, h, n = 64, 32, 3
    ip, yp, cp = pitches
    assert ip >= 3 * w and yp >= w and cp >= w // 2 and (ip % 16, yp % 16, cp % 8).count(0) == 2
    pool = Pool(w, h, n, in_pitch=ip, y_pitch=yp, c_pitch=cp)
    assert all(p.ptr % 16 == 0 for p in pool.ins + pool.ys + pool.us + pool.vs)
    assert not pool.shape_vec() and not any(pool.frame_vec(k) for k in range(n))
    images = rand_images(w, h, n, 32)
    for op, order, uv_mode in ALIGN_OPS:
        check(c, images, pool, op, order, uv_mode)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
PITCHED_112 = dict(in_pitch=352, y_pitch=128, c_pitch=72, skew=lambda k: (0, 0, 8, 8))
LOOP_SHAPES = [
    # id, W, H, n, layout, items of a frame by the shape (16 x 2 groups or 2 x 2 blocks), vector shape -- LOOP_SHAPES of
    # tests/test_gpu_bgr_to_yuv420.py, see the module docstring for the bound on B
    # bytes/16384 = 1.9: B = 1, stride 256; gx_n 6, groups 432, dby 42, dgx 4: the wrap fires whenever gx >= 2, the second step is partial
    ("96x144", 96, 144, 1, {}, 432, True),
    # bytes/16384 = 2.46: B <= 2, stride <= 512; gx_n 7, groups 560, dby 73, dgx 1; pitches and chroma bases at their moduli
    ("112x160-pitched", 112, 160, 2, PITCHED_112, 560, True),
    # bytes/16384 = 4.5, H/2 = 4: B <= 4, stride <= 1024; gx_n 257, groups 1028, dby 3, dgx 253: four lanes take a second step, and wrap
    ("4112x8", 4112, 8, 1, {}, 1028, True),
    # bytes/16384 = 4.5 but H/2 = 2 rows: B <= 2, stride <= 512; gx_n 512, groups 1024, dby 1, dgx 0: every lane steps straight down a row pair
    ("8192x4", 8192, 4, 1, {}, 1024, True),
    # byte walk, bytes/16384 = 0.3: B = 1; 33 x 17 = 561 blocks of 2 x 2 for 256 lanes: three steps, the last of 49 lanes
    ("66x34-odd", 66, 34, 2, ODD_66, 561, False),
    # the pitched vector shape with the second of two frames one byte off: B is sized for 560 groups (B <= 2), so that frame's
    # 56 x 80 = 4480 blocks of 2 x 2 take at least 9 steps of 512 lanes while frame 0 walks its groups
    ("112x160-one-frame-bytes", 112, 160, 2, dict(PITCHED_112, skew=lambda k: (k, 0, 8, 8)), 560, True),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,w,h,n,layout,items,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, layout, items, vec, order):
    """The conversion where a lane owns more than one group / block: with the histogram (equalizeHist, U and V computed) and without
    it (CLAHE 2 x 2, chroma filled)."""
    pool = Pool(w, h, n, **layout)
    assert pool.shape_vec() == vec and items == (w * h // 32 if vec else w * h // 4)
    assert items > 256 * min(max(1, w * h * 9 // 4 // 16384), h // 2), "the shape would not loop"
    if name == "112x160-one-frame-bytes":
        assert [pool.frame_vec(k) for k in range(n)] == [True, False] and w * h // 4 == 4480
    else:
        assert [pool.frame_vec(k) for k in range(n)] == [vec] * n
    images = rand_images(w, h, n, 33)
    pool.load(images)
    check(c, images, pool, EQ, order, UV_COPY, loaded=True)
    check(c, images, pool, ("clahe", (2.0, 2, 2)), order, UV_FILL128, loaded=True)


# ---- 4. a table, not a stride ----------------------------------------------------------------------------------------------------
def test_permuted_list_of_shuffled_pools(c):
    """The pools are allocated in a shuffled order and the list names the frames in another one: the addresses are neither monotonic
    nor at one stride, and every frame equals the oracle's result for its own image."""
    w, h, n = 48, 6, 5
    pool = Pool(w, h, n, in_pitch=160, y_pitch=64, c_pitch=32, alloc_order=(3, 0, 4, 1, 2))
    perm = (2, 4, 0, 3, 1)
    d = [pool.ys[perm[k + 1]].ptr - pool.ys[perm[k]].ptr for k in range(n - 1)]
    assert len(set(d)) > 1 and min(d) < 0 < max(d), "the listed Y planes must not lie at one stride"
    images = rand_images(w, h, n, 34)
    for op, order, uv_mode in ((EQ, ORDER_RGB, UV_COPY), (("clahe", (2.0, 3, 2)), ORDER_BGR, UV_COPY)):
        check(c, images, pool, op, order, uv_mode, perm=perm)


def test_one_image_two_surfaces(c):
    """The same image in two entries with different output surfaces: inputs are only read, both surfaces are exact (hence equal)."""
    w, h = 48, 6
    img = rand_images(w, h, 1, 35)[0]
    pool = Pool(w, h, 2)
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        pool.load([img, img])
        for k in range(2):
            pool.expect(k, expected(img, op, ORDER_BGR, UV_COPY))
        before = counters(c)
        call(c, op, entries([pool.ins[0]] * 2, pool.ys, pool.us, pool.vs), w, h, pool.pitches, ORDER_BGR, UV_COPY)
        torch.cuda.synchronize()
        pool.verify(("one image, two surfaces", op))
        assert moved(c, before) == (0, 0, 2, 0)


# ---- 5. histogram isolation ------------------------------------------------------------------------------------------------------
def test_histograms_do_not_leak_across_frames(c):
    """Noise, a constant colour (equalizeHist's single-bin shortcut: every pixel keeps its luma), noise and a horizontal ramp in one
    call: each frame equals its own oracle result."""
    w, h = 48, 6
    const = np.empty((h, w, 3), np.uint8)
    const[:] = (200, 31, 7)
    ramp = np.empty((h, w, 3), np.uint8)
    ramp[:] = (np.arange(w) * 255 // (w - 1)).astype(np.uint8)[None, :, None]
    ramp[:, :, 1] //= 2
    noise = rand_images(w, h, 2, 36)
    images = [noise[0], const, noise[1], ramp]
    pool = Pool(w, h, 4).load(images)
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        for order in ORDERS:
            check(c, images, pool, op, order, UV_COPY, loaded=True)


# ---- 6. chunking -----------------------------------------------------------------------------------------------------------------
def frames_per_launch():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "common.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kFramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1))


@pytest.mark.parametrize("n", [65, 129])
def test_chunking(c, n):
    """One frame past one and past two full launch sequences: the last sequence is of one frame.  Every frame is distinct and every
    frame is checked; here the images lie in one allocation, every surface is its own."""
    assert frames_per_launch() == 64
    w, h = 16, 2
    images = rand_images(w, h, n, 37)
    pool = Pool(w, h, n, arenas=(Arena(HEAD + n * (3 * w * h + 32) + 64), None), gaps=(16, 0, 32, 32))
    assert len(pool.out_arenas()) == n
    pool.load(images)
    for op in (EQ, ("clahe", (2.0, 1, 1))):
        check(c, images, pool, op, ORDER_RGB, UV_COPY, loaded=True)


# ---- 7. U and V rows side by side ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v_first", [False, True], ids=["u-left", "v-left"])
def test_u_and_v_side_by_side(c, v_first):
    """ONE pitched chroma plane of H/2 rows of W bytes: the U rows and, W/2 bytes further, the V rows (c1 = c0 + W/2, c_pitch = W; for
    v-left the list names the right half as c0).  The address ranges of U and V interleave and the call is accepted and exact."""
    w, h, n = 64, 32, 2
    pool = Pool(w, h, n, c_pitch=w, side_by_side=True)
    if v_first:
        pool.us, pool.vs = pool.vs, pool.us
    assert all(abs(pool.vs[k].ptr - pool.us[k].ptr) == w // 2 for k in range(n)) and pool.pitches[2] == w
    assert all(pool.frame_vec(k) for k in range(n))
    images = rand_images(w, h, n, 44)
    for op in (EQ, ("clahe", (2.0, 4, 2))):
        check(c, images, pool, op, ORDER_BGR, UV_COPY)


# ---- 8. identity with the batch form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_the_batch_form(c, op):
    """The same frames in ONE strided input and ONE strided output allocation (the batch form's pitched layout with gaps): the batch
    call, and the list call over the same addresses in a second, equal pair of allocations, leave equal allocations."""
    w, h, n = 64, 32, 3
    si = dict(pitch=208, frame_gap=64, off=32)
    do = dict(y_pitch=80, c_pitch=40, u_gap=32, v_gap=8, frame_gap=40, off=16)
    images = rand_images(w, h, n, 38)
    src = BgrIn(w, h, n, **si).upload(images)
    bat, lst = Yuv420Out(w, h, n, **do), Yuv420Out(w, h, n, **do)
    assert not layouts.misaligned(w, src, bat)
    before = counters(c)
    kw = dict(src.kw(), stream=stream())
    if op is EQ:
        c.equalize_hist_bgr_to_yuv420_batch_dev(src.ptr, bat.planes(), w, h, n, ORDER_BGR, UV_COPY, **kw)
    else:
        c.clahe_bgr_to_yuv420_batch_dev(src.ptr, bat.planes(), w, h, n, ORDER_BGR, UV_COPY, *op[1], **kw)
    assert moved(c, before) == (1, 0, 0, 0)
    before = counters(c)
    frames = [BgrYuv420FrameDev(src.ptr + k * src.fstride, lst.y_ptr + k * lst.fstride, lst.u_ptr + k * lst.fstride,
                                lst.v_ptr + k * lst.fstride) for k in range(n)]
    call(c, op, frames, w, h, (src.pitch, lst.y_pitch, lst.c_pitch), ORDER_BGR, UV_COPY)
    torch.cuda.synchronize()
    assert moved(c, before) == (0, 0, n, 0)
    got_list, got_batch = xfer.to_host(lst.buf), xfer.to_host(bat.buf)
    assert np.array_equal(got_list, got_batch), (op, np.flatnonzero(got_list != got_batch)[:8])
    ok, nbad, where = lst.same([expected(img, op, ORDER_BGR, UV_COPY) for img in images])
    assert ok, (op, nbad, where)
    assert np.array_equal(src.host(), src.image(images)), "the input allocation was written"


# ---- 9. the interleaved hand-over ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_interleaved_is_the_nv12_list_form(c, op):
    """chroma = INTERLEAVED with c1 = None: the bytes of mi_*_bgr_to_nv12_frames_dev on {in, y, c0}, on surfaces of their own; none of
    the four counters moves."""
    w, h, n = 64, 32, 3
    ip, yp, up = 208, 80, 96
    images = rand_images(w, h, n, 45)
    ins, surf = [], {"list": [], "nv12": []}
    for img in images:
        a = Arena(HEAD + 16 + span(h, 3 * w, ip) + 48)
        ins.append(Plane(a, h, 3 * w, ip))
        ins[-1].put(img)
        a.upload()
        for key in surf:
            o = Arena(HEAD + 16 + span(h, w, yp) + 48 + 16 + span(h // 2, w, up) + 48)
            surf[key].append((Plane(o, h, w, yp), Plane(o, h // 2, w, up, gap=32)))
    for key in surf:
        for (y, uv), img in zip(surf[key], images):
            nv12 = as_fmt(expected(img, op, ORDER_RGB, UV_COPY), w, h, "nv12")
            y.put(nv12[: w * h])
            uv.put(nv12[w * h:])
    before = counters(c)
    frames = [BgrYuv420FrameDev.of(i.ptr, y.ptr, uv.ptr, None) for i, (y, uv) in zip(ins, surf["list"])]
    assert all(f.c1 is None for f in frames)
    call(c, op, frames, w, h, (ip, yp, up), ORDER_RGB, UV_COPY, chroma=CHROMA_INTERLEAVED)
    a = ([i.ptr for i in ins], [y.ptr for y, _ in surf["nv12"]], [uv.ptr for _, uv in surf["nv12"]], w, h, ORDER_RGB, UV_COPY)
    kw = dict(in_pitch=ip, y_pitch=yp, uv_pitch=up, stream=stream())
    if op is EQ:
        c.equalize_hist_bgr_to_nv12_frames(*a, **kw)
    else:
        c.clahe_bgr_to_nv12_frames(*a, *op[1], **kw)
    torch.cuda.synchronize()
    assert moved(c, before) == (0, 0, 0, 0)
    for k in range(n):
        one, two = surf["list"][k][0].arena, surf["nv12"][k][0].arena
        assert np.array_equal(xfer.to_host(one.buf), xfer.to_host(two.buf)), k
        for a in (one, two, ins[k].arena):
            nbad, where = a.diff()
            assert nbad == 0, (op, k, nbad, where)


# ---- 10. launch contract ---------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass")


@pytest.mark.parametrize("n", [2, 65])
def test_launch_contract(n):
    """Per chunk of 64 frames.  equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch -- at n = 2
    too, where the planar form would take hist_lut_kernel.  CLAHE: one MI_K_COLOR launch per chunk plus what mi_clahe_nv12_frames_dev
    launches in place on the same Y planes (with a scratch UV plane that MI_UV_COPY leaves alone in place), measured here."""
    w, h = 32, 4
    chunks = (n + 63) // 64
    images = rand_images(w, h, n, 39)
    pool = Pool(w, h, n, in_pitch=112, y_pitch=48, c_pitch=24, arenas=(Arena(HEAD + n * (112 * h + 32) + 64), None),
                gaps=(16, 0, 32, 32)).load(images)
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


# ---- 11. errors, zero sizes ------------------------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    ip, yp, cp = 112, 48, 24
    images = rand_images(w, h, n, 40)
    pool = Pool(w, h, n, in_pitch=ip, y_pitch=yp, c_pitch=cp).load(images)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(pool.ins[k].ptr, pool.ys[k].ptr, pool.us[k].ptr, pool.vs[k].ptr) for k in range(n)]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, ip=ip, yp=yp, cp=cp, chroma=CHROMA_PLANAR, order=ORDER_BGR, uvm=UV_COPY)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (BgrYuv420FrameDev * max(1, len(a["entries"])))(*[BgrYuv420FrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["ip"], a["yp"], a["cp"], a["chroma"], a["order"], a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgr_to_yuv420_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgr_to_yuv420_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(i=None, y=None, u=None, v=None):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = list(good[-1])
            for k, val in enumerate((i, y, u, v)):
                if val is not None:
                    e[k] = None if val == "null" else val
            return dict(entries=good[:-1] + [tuple(e)])
        i2, y2, u2, v2 = good[-1]
        in_span, y_span, c_span = span(h, 3 * w, ip), span(h, w, yp), span(h // 2, w // 2, cp)
        before = counters(c)
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(i="null"), last(y="null"), last(u="null"), last(v="null"),               # a null address in the last entry
               dict(chroma=2), dict(chroma=-1),                                              # a chroma other than the two
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(ip=3 * w - 1), dict(yp=w - 1), dict(cp=w // 2 - 1),                      # a pitch below its row
               dict(order=2), dict(order=-1), dict(uvm=2), dict(uvm=-1),                     # an order, a uv_mode other than the two
               # no in-place form, compared as address ranges.  The image's rows meeting its own Y plane: the same address, and ending
               # one byte inside it; its own U plane: the same address, and U ending on the image's first byte; its own V plane: the
               # same address, and V starting on the image's last byte
               last(y=i2), last(y=i2 + in_span - 1), last(u=i2), last(u=i2 - c_span + 1), last(v=i2), last(v=i2 + in_span - 1),
               # Y meeting its own U: the same address, U starting on the last byte of the Y rows; its own V: the same address, V ending
               # on the first byte of the Y rows
               last(u=y2), last(u=y2 + y_span - 1), last(v=y2), last(v=y2 - c_span + 1),
               # c0 == c1
               last(v=u2), last(u=v2)]
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written -- a null list is fine when there are no frames
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, lst=NULL_LIST)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar form refuses: its status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, yp=1 << 25, cp=1 << 24)
        planar = L.mi_clahe_u8_batch_dev(hd, y2, 1 << 25, 1 << 26, y2, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, y2, yp, 0, y2, yp, 0, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert moved(c, before) == (0, 0, 0, 0), "a refused or empty call moved a counter"
        c.set_profiling(0)
        # and the context still works
        check(c, images, pool, EQ, ORDER_RGB, UV_FILL128, loaded=True)


# ---- 12. pipe pending ------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(rand_images(w, h, 1, 41))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            before = counters(c)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, entries(pool.ins, pool.ys, pool.us, pool.vs), w, h, pool.pitches, ORDER_BGR, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert moved(c, before) == (0, 0, 0, 0)
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")


# ---- 13. hipGraph ----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then ONE capture of that call on a single stream (one linear chain, no parallel branches) and ONE
    replay onto fresh input bytes at the same addresses: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, **PITCHED_64)
    with mi_lumaeq.Context(0) as c:
        for op, uv_mode in ((EQ, UV_COPY), (("clahe", (2.0, 4, 2)), UV_FILL128)):
            check(c, rand_images(w, h, n, 42), pool, op, ORDER_BGR, uv_mode)                  # sizes the scratch
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(c, op, entries(pool.ins, pool.ys, pool.us, pool.vs), w, h, pool.pitches, ORDER_BGR, uv_mode,
                     st=torch.cuda.current_stream().cuda_stream)
            fresh = rand_images(w, h, n, 43)
            pool.load(fresh)
            for k, img in enumerate(fresh):
                pool.expect(k, expected(img, op, ORDER_BGR, uv_mode))
            g.replay()
            torch.cuda.synchronize()
            pool.verify(("graph replay", op))
