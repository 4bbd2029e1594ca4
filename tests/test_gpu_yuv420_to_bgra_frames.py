"""Planar 4:2:0 (I420 / YV12) or NV12 in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out on a LIST of pitched device frames on the GPU:
mi_equalize_hist_yuv420_to_bgra_frames_dev and mi_clahe_yuv420_to_bgra_frames_dev.  Expected bytes are the `expected` of
tests/test_gpu_nv12_to_bgr_frames.py -- oracle.nv12_to_bgr(oracle.nv12_frame(...)), the last axis reversed for MI_ORDER_RGB, computed
once per frame and shared -- with a fourth byte of 255 appended (tests/yuv420_bgra_layouts.py).  Y, U and V are full-range random
bytes.  Every Y, U, V or UV plane and every image is its own sentinel-filled torch allocation with guard bytes unless a test says
otherwise, and every allocation is compared WHOLE, inputs included.  Every call asserts the exact deltas of the six yuv420_bgra_*
counters -- onepass / twopass (one count a call), vec / bytes (never moved by a list call), list_frames_vec / list_frames_bytes (FRAMES
by their walk) -- and that no nv12_bgr_* / yuv420_bgr_* counter moved.  Every comparison in this file is exact.

A frame pool has no layout of its own: "i420" and "yv12" say which of a frame's two chroma allocations (data[1], data[2]) holds U; the
entry always carries U in c0 and V in c1.  "nv12" frames have one UV allocation in c0 and c1 = NULL."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
import yuv420_bgra_layouts as lay
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, CHROMA_PLANAR, CHROMA_INTERLEAVED, Yuv420BgrFrameDev, Yuv420Planes
from test_gpu_nv12_to_bgr_frames import Arena, Plane, SENT, EQ, ORDERS, BAD_ARG, UNSUPPORTED, stream, rand_frames, expected, launches
from test_gpu_yuv420_to_bgr_frames import Half
from test_gpu_nv12_to_bgr_geometry import K

pytestmark = pytest.mark.gpu
FMTS = ["i420", "yv12", "nv12"]
CL22 = ("clahe", (2.0, 2, 2))


def expected4(frame, w, h, op, order, contract=False):
    return lay.with_alpha(expected(frame, w, h, op, order, contract))


class Pool:
    """n frames of one shape: a decoder's frame pool (ys; us and vs, carried by the frame's two chroma allocations in the order fmt
    says; or uvs for "nv12") and a pool of four-byte-per-pixel images (outs).  skew(k) -> the offsets of frame k's (y, c0, c1, out)
    past a 16-byte boundary; arenas: (Y, data[1], data[2], out) allocations to carve the planes from instead of one allocation each;
    side_by_side: data[1] and data[2] are the two halves of the rows of ONE plane of W-byte rows at c_pitch."""

    def __init__(self, w, h, n, fmt="i420", y_pitch=None, c_pitch=None, out_pitch=None, skew=lambda k: (0, 0, 0, 0), arenas=None,
                 gap=lambda k: 0, side_by_side=False):
        self.w, self.h, self.n, self.fmt, self.planar = w, h, n, fmt, fmt != "nv12"
        ay, a1, a2, ao = arenas or (None, None, None, None)
        self.ys, self.us, self.vs, self.uvs, self.outs = [], [], [], [], []
        for k in range(n):
            sy, s0, s1, so = skew(k)
            self.ys.append(Plane(h, w, y_pitch, sy, ay, gap(k)))
            if not self.planar:
                self.uvs.append(Plane(h // 2, w, c_pitch, s0, a1, gap(k)))
            elif side_by_side:
                assert (s0, s1) == (0, 0)
                both = Plane(h // 2, w, c_pitch, 0, a1, gap(k))
                first, second = Half(both, 0), Half(both, w // 2)
            else:
                sa, sb = (s0, s1) if fmt == "i420" else (s1, s0)
                first = Plane(h // 2, w // 2, c_pitch, sa, a1, gap(k))
                second = Plane(h // 2, w // 2, c_pitch, sb, a2, gap(k))
            if self.planar:
                u, v = (first, second) if fmt == "i420" else (second, first)
                self.us.append(u)
                self.vs.append(v)
            self.outs.append(Plane(h, 4 * w, out_pitch, so, ao, gap(k)))
        self.pitches = dict(y_pitch=self.ys[0].pitch, c_pitch=(self.us if self.planar else self.uvs)[0].pitch, out_pitch=self.outs[0].pitch)
        self.chroma = CHROMA_PLANAR if self.planar else CHROMA_INTERLEAVED

    def in_arenas(self):
        return list({id(p.arena): p.arena for p in self.ys + self.us + self.vs + self.uvs}.values())

    def out_arenas(self):
        return list({id(p.arena): p.arena for p in self.outs}.values())

    def entries(self, idx=None):
        idx = range(self.n) if idx is None else idx
        if self.planar:
            return [Yuv420BgrFrameDev(self.ys[k].ptr, self.us[k].ptr, self.vs[k].ptr, self.outs[k].ptr) for k in idx]
        return [Yuv420BgrFrameDev(self.ys[k].ptr, self.uvs[k].ptr, None, self.outs[k].ptr) for k in idx]

    def load(self, frames):
        """Upload `frames` (tight NV12; for a planar pool the U, V pairs are split into the two planes); every image back to the
        sentinel."""
        w, h = self.w, self.h
        for k, f in enumerate(frames):
            self.ys[k].put(f[: w * h])
            if self.planar:
                uv = f[w * h:].reshape(h // 2, w)
                self.us[k].put(uv[:, 0::2])
                self.vs[k].put(uv[:, 1::2])
            else:
                self.uvs[k].put(f[w * h:])
        for a in self.in_arenas():
            a.upload()
        for a in self.out_arenas():
            a.clear()
        return self

    def verify(self, what):
        for a in self.in_arenas():
            nbad, where = a.diff()
            assert nbad == 0, ("an input allocation was written", what, nbad, where)
        for a in self.out_arenas():
            nbad, where = a.diff()
            assert nbad == 0, (what, nbad, where)


def call(c, op, entries, w, h, order, pitches, chroma, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = (entries, w, h, pitches["y_pitch"], pitches["c_pitch"], chroma, order)
    kw = dict(out_pitch=pitches["out_pitch"], stream=stream() if st is None else st)
    if kind == "eq":
        c.equalize_hist_yuv420_to_bgra_frames_dev(*a, **kw)
    else:
        c.clahe_yuv420_to_bgra_frames_dev(*a, *cfg, **kw)


def stats(c):
    return tuple(c.get_stat(s) for s in lay.COUNTERS)


def foreign(c):
    return tuple(c.get_stat(s) for s in lay.FOREIGN)


def delta(before, after):
    return tuple(a - b for a, b in zip(after, before))


def check(c, frames, pool, op, order, want, perm=None, contract=False, entries=None):
    """One call on uploaded `frames`: exact images, untouched guards and inputs, the counters moved by `want` = (onepass, twopass,
    list_frames_vec, list_frames_bytes) with the per-call vec / bytes pair at rest, and no counter of another form moved."""
    w, h = pool.w, pool.h
    pool.load(frames)
    for k, f in enumerate(frames):
        pool.outs[k].put(expected4(f, w, h, op, order, contract))
    before, fbefore = stats(c), foreign(c)
    call(c, op, entries or pool.entries(perm), w, h, order, pool.pitches, pool.chroma)
    torch.cuda.synchronize()
    pool.verify((w, h, pool.fmt, op, order))
    assert delta(before, stats(c)) == tuple(want[:2]) + (0, 0) + tuple(want[2:]), (op, want, delta(before, stats(c)))
    assert foreign(c) == fbefore, "a counter of another form moved"


def image_bytes(plane):
    """what the device holds in the rows of `plane`"""
    got = xfer.to_host(plane.arena.buf)
    return np.stack([got[plane.off + r * plane.pitch: plane.off + r * plane.pitch + plane.row_bytes] for r in range(plane.rows)])


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


# ---- 1. four frames, each with its own allocations -------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FMTS)
def test_four_frames_against_four_batch_calls_and_the_oracle(c, fmt, order):
    """64 x 32 at pitches 80 / 40 (96 interleaved) / 272, every plane and image an allocation of its own: the oracle's bytes, and the
    bytes of four n_frames = 1 batch calls on the same addresses.  CLAHE 4 x 2 in one pass, 3 x 2 (REFLECT_101) in two; an all-aligned
    list counts four frames on the 16 x 2 groups."""
    w, h, n = 64, 32, 4
    frames = rand_frames(w, h, n, 231)
    cp = 40 if fmt != "nv12" else 96
    pool = Pool(w, h, n, fmt, y_pitch=80, c_pitch=cp, out_pitch=272)
    ref = Pool(w, h, n, fmt, y_pitch=80, c_pitch=cp, out_pitch=272)
    for op, one in ((EQ, 1), (("clahe", (2.0, 4, 2)), 1), (("clahe", (2.0, 3, 2)), 0)):
        check(c, frames, pool, op, order, (one, 1 - one, 4, 0), perm=None)
        ref.load(frames)
        for k, e in enumerate(ref.entries()):
            planes = Yuv420Planes(e.y, 80, e.c0, e.c1, cp, 0, ref.chroma)
            if op is EQ:
                c.equalize_hist_yuv420_to_bgra_batch_dev(planes, e.out, w, h, 1, order, out_pitch=272, out_frame=0, stream=stream())
            else:
                c.clahe_yuv420_to_bgra_batch_dev(planes, e.out, w, h, 1, order, *op[1], out_pitch=272, out_frame=0, stream=stream())
        torch.cuda.synchronize()
        for k in range(n):
            ref.outs[k].put(image_bytes(pool.outs[k]))
        ref.verify(("four batch calls against the list call", fmt, op))


# ---- 2. mixed calls: per-frame alignment, one term at a time ---------------------------------------------------------------------
BROKEN = [("i420", "y", 0, 8), ("i420", "c0", 1, 4), ("yv12", "c1", 2, 4), ("i420", "out", 3, 8),
          ("nv12", "y", 0, 8), ("nv12", "c0", 1, 8), ("nv12", "out", 3, 8)]


@pytest.mark.parametrize("fmt,name,which,by", BROKEN, ids=[f"{b[0]}-{b[1]}+{b[3]}" for b in BROKEN])
def test_mixed_calls(c, fmt, name, which, by):
    """32 x 16 at pitches 48 / 24 (48 interleaved) / 144: the shape allows the 16 x 2 groups.  Frames 0 and 2 are aligned, frames 1 and
    3 have ONE address broken -- y or out by 8 (rule: 16), a planar c0 or c1 by 4 (rule: 8), an interleaved c0 by 8 (rule: 16): they
    alone take the byte walk inside the same launch, and equalizeHist stays one pass.  CLAHE 2 x 2, whose blend + decode kernel has no
    byte path, goes two-pass for the whole call; its decode reads the luma from the context's aligned scratch planes, so a broken y
    leaves every frame on the vector walk there."""
    w, h, n = 32, 16, 4
    frames = rand_frames(w, h, n, 232)
    planar = fmt != "nv12"
    pool = Pool(w, h, n, fmt, y_pitch=48, c_pitch=24 if planar else 48, out_pitch=144,
                skew=lambda k: tuple(by * int(k % 2 == 1 and i == which) for i in range(4)))
    for k, e in enumerate(pool.entries()):
        got = [e.y % 16, e.c0 % 16, (e.c1 or 0) % 16, e.out % 16]
        assert got == [by * int(k % 2 == 1 and i == which) for i in range(4)]
        assert lay.frame_vec(True, planar, e.y, e.c0, e.c1 or 0, e.out) == (k % 2 == 0)
    for order in ORDERS:
        check(c, frames, pool, EQ, order, (1, 0, 2, 2))
        check(c, frames, pool, CL22, order, (0, 1, 4, 0) if name == "y" else (0, 1, 2, 2))


@pytest.mark.parametrize("fmt", FMTS)
def test_all_aligned_list_is_one_pass(c, fmt):
    """The control, with the planar chroma planes of the odd frames 8 past a 16-byte boundary: four frames on the groups, CLAHE one-pass."""
    w, h, n = 32, 16, 4
    frames = rand_frames(w, h, n, 232)
    planar = fmt != "nv12"
    pool = Pool(w, h, n, fmt, y_pitch=48, c_pitch=24 if planar else 48, out_pitch=144,
                skew=lambda k: (0, 8 * (k % 2), 8 * (k % 2), 0) if planar else (0, 0, 0, 0))
    check(c, frames, pool, EQ, ORDER_BGR, (1, 0, 4, 0))
    check(c, frames, pool, CL22, ORDER_RGB, (1, 0, 4, 0))


@pytest.mark.parametrize("fmt,pitch", [("i420", dict(c_pitch=20)), ("i420", dict(y_pitch=40)), ("nv12", dict(c_pitch=56)),
                                       ("yv12", dict(out_pitch=136))], ids=["c_pitch-20", "y_pitch-40", "uv_pitch-56", "out_pitch-136"])
def test_shape_term(c, fmt, pitch):
    """A pitch the shape rule refuses: every frame takes the byte walk although all its addresses are aligned (in the CLAHE fallback
    too: the shape is judged on the caller's pitches)."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 233)
    base = dict(y_pitch=48, c_pitch=24 if fmt != "nv12" else 48, out_pitch=144)
    pool = Pool(w, h, n, fmt, **dict(base, **pitch))
    assert all((e.y | e.c0 | (e.c1 or 0) | e.out) % 16 == 0 for e in pool.entries())
    check(c, frames, pool, EQ, ORDER_BGR, (1, 0, 0, 3))
    check(c, frames, pool, CL22, ORDER_RGB, (0, 1, 0, 3))


@pytest.mark.parametrize("fmt", FMTS)
def test_general_and_fallback(c, fmt):
    """66 x 34, odd pitches, addresses at odd offsets: 2 x 2 blocks with byte accesses, three steps a lane; CLAHE 3 x 2 in two passes."""
    w, h, n = 66, 34, 2
    frames = rand_frames(w, h, n, 234)
    pool = Pool(w, h, n, fmt, y_pitch=67, c_pitch=35 if fmt != "nv12" else 69, out_pitch=269, skew=lambda k: (1 + 2 * k, 3, 7 + 2 * k, 5 + 6 * k))
    check(c, frames, pool, EQ, ORDER_RGB, (1, 0, 0, 2))
    check(c, frames, pool, ("clahe", (2.0, 3, 2)), ORDER_BGR, (0, 1, 0, 2))


@pytest.mark.parametrize("fmt", ["yv12", "nv12"])
def test_loops_and_straddling_bands(c, fmt):
    """112 x 80 (280 groups for the 256 lanes of one workgroup: the carried walk wraps) through the table kernels, LUT apply and decode
    alone (5 x 3 pads); 48 x 30 CLAHE 3 x 2 (tile 16 x 15: a row pair straddles two bands) through the blend + decode table kernel."""
    w, h, n = 112, 80, 2
    frames = rand_frames(w, h, n, 235)
    pool = Pool(w, h, n, fmt, skew=lambda k: (0, 0, 0, 0))
    check(c, frames, pool, EQ, ORDER_BGR, (1, 0, 2, 0))
    check(c, frames, pool, ("clahe", (2.0, 5, 3)), ORDER_RGB, (0, 1, 2, 0))
    w, h = 48, 30
    planar = fmt != "nv12"
    pool = Pool(w, h, n, fmt, y_pitch=64, c_pitch=40 if planar else 64, out_pitch=208, skew=lambda k: (0, 8, 8, 0) if planar else (0, 0, 0, 0))
    check(c, rand_frames(w, h, n, 236), pool, ("clahe", (2.0, 3, 2)), ORDER_BGR, (1, 0, 2, 0))


def test_fp_contract_takes_the_fallback(c):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    frames = rand_frames(w, h, n, 237)
    pool = Pool(w, h, n, "nv12")
    c.set_option("clahe_fp_contract", 1)
    prev = oracle.set_fp_contract(True)
    try:
        check(c, frames, pool, ("clahe", (2.0, 4, 2)), ORDER_BGR, (0, 1, 2, 0), contract=True)
    finally:
        oracle.set_fp_contract(prev)
        c.set_option("clahe_fp_contract", 0)
    check(c, frames, pool, ("clahe", (2.0, 4, 2)), ORDER_BGR, (1, 0, 2, 0))


# ---- 3. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,op,one", [("i420", EQ, 1), ("nv12", ("clahe", (2.0, 1, 1)), 1), ("yv12", ("clahe", (2.0, 3, 1)), 0)],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, fmt, op, one):
    """65 frames of 16 x 2: two launch sequences, the second of one frame.  The planes are carved at irregular (16-byte aligned)
    distances out of four large allocations; every frame is distinct and every frame is checked (the fallback reuses its scratch planes
    from chunk to chunk)."""
    w, h, n = 16, 2, 65

    def gap(k):
        return 16 * ((k * 7) % 5)
    arenas = tuple(Arena(n * (sz + 96) + 64) for sz in (w * h, w * h // 2, w * h // 4, 4 * w * h))
    pool = Pool(w, h, n, fmt, arenas=arenas, gap=gap)
    frames = rand_frames(w, h, n, 238)
    assert len({f.tobytes() for f in frames}) == n
    assert len({pool.ys[k + 1].ptr - pool.ys[k].ptr for k in range(n - 1)}) > 1, "the Y planes are not at one stride"
    check(c, frames, pool, op, ORDER_RGB, (one, 1 - one, n, 0))


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------
def test_one_input_two_outputs(c):
    """The same {y, c0, c1} in two entries with different images: inputs are only read, both images are exact (hence equal)."""
    w, h = 32, 16
    frame = rand_frames(w, h, 1, 239)[0]
    for fmt in ("i420", "nv12"):
        pool = Pool(w, h, 2, fmt)
        for op in (EQ, CL22):
            e = pool.entries()
            e[1] = Yuv420BgrFrameDev(e[0].y, e[0].c0, e[0].c1, e[1].out)
            check(c, [frame, frame], pool, op, ORDER_BGR, (1, 0, 2, 0), entries=e)


@pytest.mark.parametrize("order", ORDERS)
def test_u_and_v_rows_side_by_side_in_one_plane(c, order):
    """c1 = c0 + W/2, c_pitch = W: legal (input planes are not compared with each other) and, both being multiples of 8, on the groups."""
    w, h, n = 16, 2, 3
    for fmt in ("i420", "yv12"):
        pool = Pool(w, h, n, fmt, side_by_side=True)
        e = pool.entries()[0]
        assert abs(e.c1 - e.c0) == 8 and (e.c1 > e.c0) == (fmt == "i420") and pool.pitches["c_pitch"] == 16
        frames = rand_frames(w, h, n, 240)
        for op in (EQ, ("clahe", (2.0, 1, 1))):
            check(c, frames, pool, op, order, (1, 0, n, 0))


def test_interleaved_list_with_null_and_junk_c1(c):
    """chroma = MI_CHROMA_INTERLEAVED: c1 is ignored -- NULL in one entry, junk in another, the image's own address in a third."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 241)
    pool = Pool(w, h, n, "nv12", y_pitch=48, c_pitch=64, out_pitch=160)
    e = pool.entries()
    entries = [Yuv420BgrFrameDev(e[k].y, e[k].c0, (None, 1, e[k].out)[k], e[k].out) for k in range(n)]
    for op, one in ((EQ, 1), (CL22, 1), (("clahe", (2.0, 3, 2)), 0)):
        check(c, frames, pool, op, ORDER_BGR, (one, 1 - one, 3, 0), entries=entries)


def test_constant_and_two_valued_planes(c):
    """A constant Y plane below 16: equalizeHist's shortcut and the decode's clamp of (Y - 16) at 0.  Two values."""
    w, h = 32, 16
    const, two = rand_frames(w, h, 2, 242)
    const[: w * h] = 9
    two[: w * h] = np.where(np.arange(w * h) % 3 == 0, 200, 3).astype(np.uint8)
    for order, fmt in zip(ORDERS, ("yv12", "nv12")):
        pool = Pool(w, h, 2, fmt)
        for op in (EQ, CL22):
            check(c, [const, two], pool, op, order, (1, 0, 2, 0))


# ---- 5. hipGraph -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_graph_capture_and_two_replays(fmt):
    """One eager call of the shape, then capture and two replays, each onto fresh input bytes at the same addresses."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, fmt, y_pitch=80, c_pitch=40 if fmt != "nv12" else 96, out_pitch=272)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            one = int(op[1] != (2.0, 3, 2))
            check(c, rand_frames(w, h, n, 243), pool, op, ORDER_BGR, (one, 1 - one, 3, 0))   # sizes the scratch
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(c, op, pool.entries(), w, h, ORDER_BGR, pool.pitches, pool.chroma, st=torch.cuda.current_stream().cuda_stream)
            for seed in (244, 245):
                fresh = rand_frames(w, h, n, seed)
                pool.load(fresh)
                for k, f in enumerate(fresh):
                    pool.outs[k].put(expected4(f, w, h, op, ORDER_BGR))
                g.replay()
                torch.cuda.synchronize()
                pool.verify(("graph replay", op, seed))


# ---- 6. refusals, zero sizes, launch accounting ----------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 246)
    pool = Pool(w, h, n, y_pitch=48, c_pitch=24, out_pitch=144).load(frames)
    ipool = Pool(w, h, n, "nv12", y_pitch=48, c_pitch=48, out_pitch=144).load(frames)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(e.y, e.c0, e.c1, e.out) for e in pool.entries()]
        igood = [(e.y, e.c0, None, e.out) for e in ipool.entries()]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, yp=48, cp=24, chroma=CHROMA_PLANAR, op=144, order=ORDER_BGR)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (Yuv420BgrFrameDev * max(1, len(a["entries"])))(*[Yuv420BgrFrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["yp"], a["cp"], a["chroma"], a["op"], a["order"])

        def eq(**kw):
            return L.mi_equalize_hist_yuv420_to_bgra_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_yuv420_to_bgra_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(src=good, **over):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = dict(zip(("y", "c0", "c1", "out"), src[-1]))
            e.update({k: (None if v == "null" else v) for k, v in over.items()})
            return dict(entries=src[:-1] + [(e["y"], e["c0"], e["c1"], e["out"])])
        y2, u2, v2, _ = good[-1]
        iy2, iuv2, _, _ = igood[-1]
        img = (h - 1) * 144 + 4 * w                                                           # the bytes an image spans
        INTER = dict(chroma=CHROMA_INTERLEAVED, cp=48, entries=igood)                         # the interleaved list
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(y="null"), last(c0="null"), last(c1="null"), last(out="null"),           # a null plane address in the last entry
               dict(entries=[(None,) + good[0][1:]] + good[1:]),                             # ... and in the first
               dict(chroma=2), dict(chroma=-1),                                              # a chroma other than the two
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(yp=w - 1), dict(cp=w // 2 - 1), dict(op=4 * w - 1), dict(op=3 * w),      # a pitch below its row
               dict(INTER, cp=w - 1),                                                        # ... W for an interleaved chroma plane
               dict(order=2), dict(order=-1),                                                # an order other than the two
               # no in-place form, compared as address ranges: the image of the last frame on its own Y, U and V plane, ending one
               # byte inside its V plane, and starting on the last byte of its Y plane's last row
               last(out=y2), last(out=u2), last(out=v2), last(out=v2 - img + 1), last(out=y2 + (h - 1) * 48 + w - 1),
               # the interleaved list has the same checks on {y, c0, out}
               dict(INTER, lst=NULL_LIST), dict(INTER, **last(igood, y="null")), dict(INTER, **last(igood, c0="null")),
               dict(INTER, **last(igood, out="null")), dict(INTER, w=31), dict(INTER, order=2),
               dict(INTER, **last(igood, out=iy2)), dict(INTER, **last(igood, out=iuv2)),
               dict(INTER, **last(igood, out=iuv2 + (h // 2 - 1) * 48 + w - 1))]
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, **INTER) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written -- a null list is fine when there are no frames
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, lst=NULL_LIST), dict(INTER, n=0)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: the batch form's status
        big = dict(w=(1 << 24) + 2, h=2, yp=1 << 25, cp=1 << 24, op=1 << 27)
        y0, u0, v0, o0 = good[0]
        planes = Yuv420Planes(y0, 1 << 25, u0, v0, 1 << 24, 1 << 27, CHROMA_PLANAR)
        batch = L.mi_equalize_hist_yuv420_to_bgra_batch_dev(hd, planes, o0, 1 << 27, 1 << 28, big["w"], 2, 1, 0, stream())
        assert batch == UNSUPPORTED and eq(**big) == batch and cl(**big) == batch
        planes = Yuv420Planes(y0, 48, u0, v0, 24, 0, CHROMA_PLANAR)
        batch = L.mi_clahe_yuv420_to_bgra_batch_dev(hd, planes, o0, 144, 0, w, h, 1, 0, 2.0, 2048, 1024, stream())
        assert batch == UNSUPPORTED and cl(2048, 1024) == batch
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        ipool.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0,) * 6 and foreign(c) == (0,) * 8
        # launch accounting of the three sequences, by role: the batch form's slots; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (1, 0, 3, 0)),
                             (CL22, {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (1, 0, 3, 0)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (0, 1, 3, 0))):
            for p in (pool, ipool):
                c.profile_read(reset=True)
                check(c, frames, p, op, ORDER_RGB, st)
                got = launches(c)
                assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(rand_frames(w, h, 1, 247))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, CL22):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, pool.entries(), w, h, ORDER_BGR, pool.pitches, pool.chroma)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")
        assert stats(c) == (0,) * 6


# ---- 7. seeded sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["eq", "clahe"])
def test_seeded_sweep(c, kind):
    """The 32 cases per op of tests/yuv420_bgra_layouts.py (tests/test_yuv420_to_bgra_frames_abi.py asserts the census of their classes
    on the CPU): exact bytes, whole allocations, and the six counter deltas the documented rule gives.  No case is skipped."""
    sweep = lay.sweep_cases(kind)
    assert len(sweep) == 32 and lay.census(sweep, K)["refused"] == 0
    c.set_option("clahe_fp_contract", 0)
    ran = 0
    for i, k in enumerate(sweep):
        w, h, n, order, sk = k["w"], k["h"], k["n"], k["order"], k["skews"]
        op = EQ if kind == "eq" else ("clahe", (k["clip"], k["tx"], k["ty"]))
        frames = rand_frames(w, h, n, 600 + i)
        want = lay.classify(k, K)[0]
        pool = Pool(w, h, n, k["fmt"], y_pitch=k["y_pitch"], c_pitch=k["c_pitch"], out_pitch=k["out_pitch"], skew=lambda f: sk[f]).load(frames)
        entries = pool.entries()
        for f in range(n):
            e = entries[f]
            got, drawn = [e.y % 16, e.c0 % 16, (e.c1 or 0) % 16, e.out % 16], [s % 16 for s in sk[f]]
            if not pool.planar:
                got[2] = drawn[2] = 0                 # c1 is NULL and ignored
            assert got == drawn, (i, f)
            pool.outs[f].put(expected4(frames[f], w, h, op, order))
        before, fbefore = stats(c), foreign(c)
        call(c, op, entries, w, h, order, pool.pitches, pool.chroma)
        torch.cuda.synchronize()
        pool.verify((i, k))
        assert delta(before, stats(c)) == want, (i, k, want, delta(before, stats(c)))
        assert foreign(c) == fbefore
        ran += 1
    assert ran == 32
