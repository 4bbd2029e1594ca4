"""Interleaved BGR / RGB in, NV12 out on a LIST of pitched device frames on the GPU: mi_equalize_hist_bgr_to_nv12_frames_dev and
mi_clahe_bgr_to_nv12_frames_dev.  Expected bytes are oracle.nv12_frame(oracle.bgr_to_nv12(img), W, H, uv_mode, op, ...), the image's
last axis reversed first for MI_ORDER_RGB, as tests/test_gpu_bgr_to_nv12.py computes them; pixels are full-range random bytes unless a
test says otherwise.  Every output surface (a Y plane and, behind a gap, its UV plane) is its own sentinel-filled torch allocation with
guard bytes before, between and behind the planes, and so is every image unless a test says otherwise; every allocation is compared
WHOLE, inputs included: pitch padding and guards keep their sentinel.  Every comparison in this file is exact.

The shapes follow tests/test_gpu_bgr_to_nv12.py (see its module docstring for the bound on the workgroups per frame, B): the list form
computes B from the shape alone, so a frame that takes the byte path inside a vector-shaped call steps through its 2 x 2 blocks with the
vector path's stride."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, BgrNv12FrameDev

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
HEAD = 32                 # guard bytes in front of the first plane of an allocation
ORDERS = [ORDER_BGR, ORDER_RGB]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def rand_images(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _expected(img_bytes, w, h, op, order, uv_mode):
    kind, cfg = op
    img = np.frombuffer(img_bytes, np.uint8).reshape(h, w, 3)
    bgr = img if order == ORDER_BGR else np.ascontiguousarray(img[:, :, ::-1])
    nv12 = oracle.bgr_to_nv12(bgr)
    out = oracle.nv12_frame(nv12, w, h, uv_mode, 0) if kind == "eq" else oracle.nv12_frame(nv12, w, h, uv_mode, 1, *cfg)
    out.setflags(write=False)
    return out


def expected(img, op, order, uv_mode):
    """The tight NV12 frame the call must produce for `img` (H x W x 3, in the order the call is told): computed once per (image, op,
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
    """`rows` rows of `row_bytes` bytes at `pitch`, carved out of `arena`."""

    def __init__(self, arena, rows, row_bytes, pitch=None, skew=0, gap=0):
        self.rows, self.row_bytes, self.pitch, self.arena = rows, row_bytes, pitch or row_bytes, arena
        self.off = arena.carve(span(rows, row_bytes, self.pitch), skew, gap)

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
    """n frames of one shape: an image pool (ins) and an encoder's surface pool (ys, uvs: the two planes of a surface share one
    allocation, 32 guard bytes apart).  skew(k) -> the offsets of frame k's three addresses past a 16-byte boundary; alloc_order: the
    order in which the frames' allocations are made; arenas: (in, out) allocations to carve the images / the surfaces from instead
    (None: one each, as usual), `gaps` bytes in front of every image, Y plane and UV plane."""

    def __init__(self, w, h, n, in_pitch=None, y_pitch=None, uv_pitch=None, skew=lambda k: (0, 0, 0), alloc_order=None, arenas=None,
                 gaps=(0, 0, 32)):
        self.w, self.h, self.n = w, h, n
        ip, yp, up = in_pitch or 3 * w, y_pitch or w, uv_pitch or w
        self.ins, self.ys, self.uvs = [None] * n, [None] * n, [None] * n
        for k in (alloc_order or range(n)):
            si, sy, su = skew(k)
            ain, aout = arenas or (None, None)
            ain = ain or Arena(HEAD + 16 + si + span(h, 3 * w, ip) + 48)
            aout = aout or Arena(HEAD + 16 + sy + span(h, w, yp) + 48 + 16 + su + span(h // 2, w, up) + 48)
            self.ins[k] = Plane(ain, h, 3 * w, ip, si, gaps[0])
            self.ys[k] = Plane(aout, h, w, yp, sy, gaps[1])
            self.uvs[k] = Plane(aout, h // 2, w, up, su, gaps[2])
        self.pitches = dict(in_pitch=ip, y_pitch=yp, uv_pitch=up)

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
        wh = self.w * self.h
        self.ys[k].put(frame[:wh])
        self.uvs[k].put(frame[wh:])

    def verify(self, what):
        for a in self.in_arenas():
            nbad, where = a.diff()
            assert nbad == 0, ("an input allocation was written", what, nbad, where)
        for i, a in enumerate(self.out_arenas()):
            nbad, where = a.diff()
            assert nbad == 0, (what, "output allocation", i, nbad, where)


def call(c, op, ins, ys, uvs, w, h, order, uv_mode, pitches, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = ([p.ptr for p in ins], [p.ptr for p in ys], [p.ptr for p in uvs], w, h, order, uv_mode)
    kw = dict(pitches, stream=stream() if st is None else st)
    if kind == "eq":
        c.equalize_hist_bgr_to_nv12_frames(*a, **kw)
    else:
        c.clahe_bgr_to_nv12_frames(*a, *cfg, **kw)


def check(c, images, pool, op, order, uv_mode, perm=None, loaded=False):
    """One call on `images`: every surface is the oracle's frame for its own image, guards and inputs untouched.  perm: the order in
    which the frames appear in the list.  loaded: the images are in the pool already."""
    w, h = pool.w, pool.h
    pool.clear() if loaded else pool.load(images)
    for k, img in enumerate(images):
        pool.expect(k, expected(img, op, order, uv_mode))
    idx = list(range(pool.n)) if perm is None else list(perm)
    call(c, op, [pool.ins[k] for k in idx], [pool.ys[k] for k in idx], [pool.uvs[k] for k in idx], w, h, order, uv_mode, pool.pitches)
    torch.cuda.synchronize()
    pool.verify((w, h, op, order, uv_mode))


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
ODD_66 = dict(in_pitch=201, y_pitch=67, uv_pitch=69, skew=lambda k: (1, 1, 1))
PITCHED_64 = dict(in_pitch=208, y_pitch=80, uv_pitch=96)
PARITY = [
    # id, W, H, n, layout, vector path, the two CLAHE grids: one divides the frame, one does not (REFLECT_101 padding)
    ("16x2", 16, 2, 1, {}, True, [(2.0, 1, 1), (2.0, 3, 1)]),                   # one vector group
    ("48x6", 48, 6, 3, {}, True, [(2.0, 3, 2), (2.0, 5, 4)]),                   # gx_n = 3: the row walk wraps
    ("2x2", 2, 2, 1, {}, False, [(2.0, 1, 1), (2.0, 3, 1)]),                    # one byte-path block
    ("66x34-odd", 66, 34, 2, ODD_66, False, [(2.0, 3, 2), (3.0, 4, 3)]),        # odd pitches, addresses at offset 1: nothing aligned
    ("64x32-pitched", 64, 32, 3, PITCHED_64, True, [(2.0, 4, 2), (4.0, 5, 3)]),  # padding, aligned
]


@pytest.mark.parametrize("name,w,h,n,layout,vec,grids", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, layout, vec, grids):
    pool = Pool(w, h, n, **layout)
    aligned = all(p.ptr % 16 == 0 for p in pool.ins + pool.ys + pool.uvs) and all(v % 16 == 0 for v in pool.pitches.values())
    assert (w % 16 == 0 and aligned) == vec
    if name == "66x34-odd":
        assert all(p.ptr % 16 == 1 for p in pool.ins + pool.ys + pool.uvs)
    assert (w % grids[0][1], h % grids[0][2]) == (0, 0) and (w % grids[1][1] or h % grids[1][2])
    images = rand_images(w, h, n, 31)
    pool.load(images)
    for op in [EQ] + [("clahe", g) for g in grids]:
        for order in ORDERS:
            for uv_mode in UV_MODES:
                check(c, images, pool, op, order, uv_mode, loaded=True)


# ---- 2. per-frame alignment ------------------------------------------------------------------------------------------------------
ALIGN_OPS = ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, UV_FILL128))


@pytest.mark.parametrize("which", [0, 1, 2], ids=["in", "y", "uv"])
def test_one_frame_misaligned(c, which):
    """32 x 4 at pitches 112 / 48 / 48: the shape allows 16-byte accesses.  The middle frame of three has ONE address 8 bytes past a
    16-byte boundary: it alone takes the 2 x 2 byte path inside the same launch, its neighbours keep the 16 x 2 groups."""
    w, h, n = 32, 4, 3
    pool = Pool(w, h, n, in_pitch=112, y_pitch=48, uv_pitch=48, skew=lambda k: tuple(8 * int(k == 1 and i == which) for i in range(3)))
    for k in range(n):
        assert [p.ptr % 16 for p in (pool.ins[k], pool.ys[k], pool.uvs[k])] == [8 * int(k == 1 and i == which) for i in range(3)]
    images = rand_images(w, h, n, 32)
    for op, order, uv_mode in ALIGN_OPS:
        check(c, images, pool, op, order, uv_mode)


@pytest.mark.parametrize("which", ["in_pitch", "y_pitch", "uv_pitch"])
def test_one_pitch_misaligned(c, which):
    """Every address a multiple of 16 and ONE pitch a multiple of 8 only: the whole call takes bytes; the same bytes, the same guards."""
    w, h, n = 32, 4, 3
    pitches = dict(in_pitch=112, y_pitch=48, uv_pitch=48)
    pitches[which] -= 8
    assert pitches[which] % 16 == 8 and pitches["in_pitch"] >= 3 * w and min(pitches["y_pitch"], pitches["uv_pitch"]) >= w
    pool = Pool(w, h, n, **pitches)
    assert all(p.ptr % 16 == 0 for p in pool.ins + pool.ys + pool.uvs)
    images = rand_images(w, h, n, 32)
    for op, order, uv_mode in ALIGN_OPS:
        check(c, images, pool, op, order, uv_mode)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
LOOP_SHAPES = [
    # id, W, H, n, layout, items of a frame (16 x 2 groups or 2 x 2 blocks), vector shape -- LOOP_SHAPES of tests/test_gpu_bgr_to_nv12.py
    # bytes/16384 = 1.9: B = 1, stride 256; gx_n 6, groups 432, dby 42, dgx 4: the wrap fires whenever gx >= 2, the second step is partial
    ("96x144", 96, 144, 1, {}, 432, True),
    # byte path, bytes/16384 = 0.3: B = 1; 33 x 17 = 561 blocks of 2 x 2 for 256 lanes: three steps, the last of 49 lanes
    ("66x34-odd", 66, 34, 2, ODD_66, 561, False),
    # the vector shape above with the second of two frames 8 bytes off: B is sized for 432 groups (B = 1), so that frame's 3456 blocks
    # take 14 steps of 256 lanes while frame 0 walks its groups
    ("96x144-one-frame-bytes", 96, 144, 2, dict(skew=lambda k: (8 * k, 0, 0)), 432, True),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,w,h,n,layout,items,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, layout, items, vec, order):
    """The conversion where a lane owns more than one group / block: with the histogram (equalizeHist, U and V computed) and without
    it (CLAHE 2 x 2, chroma filled)."""
    assert items == (w * h // 32 if vec else w * h // 4)
    assert items > 256 * min(max(1, w * h * 9 // 4 // 16384), h // 2), "the shape would not loop"
    pool = Pool(w, h, n, **layout)
    images = rand_images(w, h, n, 33)
    pool.load(images)
    check(c, images, pool, EQ, order, UV_COPY, loaded=True)
    check(c, images, pool, ("clahe", (2.0, 2, 2)), order, UV_FILL128, loaded=True)


# ---- 4. a table, not a stride ----------------------------------------------------------------------------------------------------
def test_permuted_list_of_shuffled_pools(c):
    """The pools are allocated in a shuffled order and the list names the frames in another one: the addresses are neither monotonic
    nor at one stride, and every frame equals the oracle's result for its own image."""
    w, h, n = 48, 6, 5
    pool = Pool(w, h, n, in_pitch=160, y_pitch=64, uv_pitch=64, alloc_order=(3, 0, 4, 1, 2))
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
        call(c, op, [pool.ins[0]] * 2, pool.ys, pool.uvs, w, h, ORDER_BGR, UV_COPY, pool.pitches)
        torch.cuda.synchronize()
        pool.verify(("one image, two surfaces", op))


# ---- 5. histogram isolation ------------------------------------------------------------------------------------------------------
def test_histograms_do_not_leak_across_frames(c):
    """A constant colour (equalizeHist's single-bin shortcut: every pixel keeps its luma), noise and a horizontal ramp in one call: each
    frame equals its own oracle result."""
    w, h = 48, 6
    const = np.empty((h, w, 3), np.uint8)
    const[:] = (200, 31, 7)
    ramp = np.empty((h, w, 3), np.uint8)
    ramp[:] = (np.arange(w) * 255 // (w - 1)).astype(np.uint8)[None, :, None]
    ramp[:, :, 1] //= 2
    images = [const, rand_images(w, h, 1, 36)[0], ramp]
    pool = Pool(w, h, 3).load(images)
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
    frame is checked; the images lie in one allocation, every surface is its own."""
    assert frames_per_launch() == 64
    w, h = 16, 2
    images = rand_images(w, h, n, 37)
    pool = Pool(w, h, n, arenas=(Arena(HEAD + n * (3 * w * h + 32) + 64), None), gaps=(16, 0, 32))
    assert len(pool.out_arenas()) == n
    pool.load(images)
    for op in (EQ, ("clahe", (2.0, 1, 1))):
        check(c, images, pool, op, ORDER_RGB, UV_COPY, loaded=True)


# ---- 7. identity with the batch form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_the_batch_form(c, op):
    """The pools are views into ONE input and ONE output allocation at a fixed frame stride, so the batch form can take the same
    layout: the batch call and the list call, each on its own sentinel-filled copy of the output allocation, leave equal allocations."""
    w, h, n = 64, 32, 3
    ip, yp, up = 208, 80, 96
    in_frame = ip * h + 64                                       # 64 bytes between the images
    out_frame = yp * h + 32 + up * (h // 2) + 48                 # 32 bytes between the planes, 48 between the frames
    in_bytes, out_bytes = HEAD + n * in_frame + 64, HEAD + n * out_frame + 64
    images = rand_images(w, h, n, 38)

    def layout():
        # gaps that reproduce the strides: carve() rounds up to 16, every term here is a multiple of 16
        pool = Pool(w, h, n, ip, yp, up, arenas=(Arena(in_bytes), Arena(out_bytes)),
                    gaps=(in_frame - span(h, 3 * w, ip), out_frame - (yp * h + 32) - span(h // 2, w, up), yp * h - span(h, w, yp) + 32))
        for k in range(n):
            assert pool.ins[k].off == pool.ins[0].off + k * in_frame, k
            assert (pool.ys[k].off, pool.uvs[k].off) == (pool.ys[0].off + k * out_frame, pool.uvs[0].off + k * out_frame), k
        return pool.load(images)
    lst, bat = layout(), layout()
    call(c, op, lst.ins, lst.ys, lst.uvs, w, h, ORDER_BGR, UV_COPY, lst.pitches)
    a = (bat.ins[0].ptr, bat.ys[0].ptr, bat.uvs[0].ptr, w, h, n, ORDER_BGR, UV_COPY)
    kw = dict(in_pitch=ip, in_frame=in_frame, y_pitch=yp, uv_pitch=up, out_frame=out_frame, stream=stream())
    if op is EQ:
        c.equalize_hist_bgr_to_nv12_batch_dev(*a, **kw)
    else:
        c.clahe_bgr_to_nv12_batch_dev(*a, *op[1], **kw)
    torch.cuda.synchronize()
    got_list, got_batch = xfer.to_host(lst.ys[0].arena.buf), xfer.to_host(bat.ys[0].arena.buf)
    assert np.array_equal(got_list, got_batch), (op, np.flatnonzero(got_list != got_batch)[:8])
    for k, img in enumerate(images):
        lst.expect(k, expected(img, op, ORDER_BGR, UV_COPY))
    lst.verify(("list form on the batch layout", op))


# ---- 8. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass")


@pytest.mark.parametrize("n", [2, 65])
def test_launch_contract(n):
    """Per chunk of 64 frames.  equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch -- at n = 2
    too, where the planar form would take hist_lut_kernel.  CLAHE: one MI_K_COLOR launch per chunk plus what mi_clahe_nv12_frames_dev
    launches in place on the same Y planes, measured here."""
    w, h = 32, 4
    chunks = (n + 63) // 64
    images = rand_images(w, h, n, 39)
    pool = Pool(w, h, n, in_pitch=112, y_pitch=48, uv_pitch=48).load(images)
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
            planes = [(pool.ys[k].ptr, pool.uvs[k].ptr) for k in range(n)]
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
    ip, yp, up = 112, 48, 48
    images = rand_images(w, h, n, 40)
    pool = Pool(w, h, n, in_pitch=ip, y_pitch=yp, uv_pitch=up).load(images)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(pool.ins[k].ptr, pool.ys[k].ptr, pool.uvs[k].ptr) for k in range(n)]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, ip=ip, yp=yp, up=up, order=ORDER_BGR, uvm=UV_COPY)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (BgrNv12FrameDev * max(1, len(a["entries"])))(*[BgrNv12FrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["ip"], a["yp"], a["up"], a["order"], a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgr_to_nv12_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgr_to_nv12_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(i=None, y=None, uv=None):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = list(good[-1])
            for k, v in enumerate((i, y, uv)):
                if v is not None:
                    e[k] = None if v == "null" else v
            return dict(entries=good[:-1] + [tuple(e)])
        i2, y2, uv2 = good[-1]
        in_span, y_span = span(h, 3 * w, ip), span(h, w, yp)
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(i="null"), last(y="null"), last(uv="null"),                              # a null address in the last entry
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(ip=3 * w - 1), dict(yp=w - 1), dict(up=w - 1),                           # a pitch below its row
               dict(order=2), dict(order=-1), dict(uvm=2), dict(uvm=-1),                     # an order, a uv_mode other than the two
               # no in-place form, compared as address ranges.  The image's rows meeting its own Y plane: the same address, and ending
               # one byte inside it; meeting its own UV plane: the same address, and starting on the last byte of its last row
               last(y=i2), last(y=i2 + in_span - 1), last(uv=i2), last(uv=i2 - span(h // 2, w, up) + 1),
               # Y meeting its own UV: the same address, UV starting on the last byte of the Y rows, UV ending on the first
               last(uv=y2), last(uv=y2 + y_span - 1), last(uv=y2 - span(h // 2, w, up) + 1)]
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
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, yp=1 << 25, up=1 << 25)
        planar = L.mi_clahe_u8_batch_dev(hd, y2, 1 << 25, 1 << 26, y2, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, y2, yp, 0, y2, yp, 0, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        c.set_profiling(0)
        # and the context still works
        check(c, images, pool, EQ, ORDER_RGB, UV_FILL128, loaded=True)


# ---- 10. pipe pending ------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(rand_images(w, h, 1, 41))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, pool.ins, pool.ys, pool.uvs, w, h, ORDER_BGR, UV_COPY, pool.pitches)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")


# ---- 11. hipGraph ----------------------------------------------------------------------------------------------------------------
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
                call(c, op, pool.ins, pool.ys, pool.uvs, w, h, ORDER_BGR, uv_mode, pool.pitches, st=torch.cuda.current_stream().cuda_stream)
            fresh = rand_images(w, h, n, 43)
            pool.load(fresh)
            for k, img in enumerate(fresh):
                pool.expect(k, expected(img, op, ORDER_BGR, uv_mode))
            g.replay()
            torch.cuda.synchronize()
            pool.verify(("graph replay", op))
