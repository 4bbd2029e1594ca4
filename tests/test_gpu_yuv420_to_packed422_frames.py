"""4:2:0 (NV12 / I420 / YV12) in, packed 4:2:2 (YUY2 / UYVY) out on a LIST of pitched device frames on the GPU:
mi_equalize_hist_yuv420_to_packed422_frames_dev and mi_clahe_yuv420_to_packed422_frames_dev.  Expected bytes are
yuv420_packed422_ref.expected_frame: the Y plane mapped by oracle.equalize_hist / oracle.clahe, input chroma row r under output rows 2r
and 2r+1 (MI_UV_COPY) or 128 (MI_UV_FILL128), interleaved by format -- not the code under test.  Y, U and V are full-range random bytes,
U and V drawn independently.  Every Y, U, V (or UV) plane and every packed frame is its own sentinel-filled torch allocation with guard
bytes unless a test says otherwise, and every allocation is compared WHOLE, inputs included.  Every call asserts the deltas of six
counters: yuv420_packed422_onepass / yuv420_packed422_twopass (one count a call), yuv420_packed422_list_frames_vec /
yuv420_packed422_list_frames_bytes (FRAMES by their walk) and yuv420_packed422_vec / yuv420_packed422_bytes (never moved by a list
call).  Every comparison in this file is exact.

A frame pool has no layout of its own: "i420" and "yv12" say which of a frame's two chroma allocations comes first.  The entry always
carries U in c0 and V in c1; an "nv12" frame carries its UV plane in c0 and None in c1.

How many workgroups yuv420_to_packed422_frames_kernel gets per frame (B) is not observable, but the shapes of the tests that loop are
chosen by it: launch_yuv420_to_packed422 takes B = min(blocks_per_frame(W*H*7/4 bytes, H/2 rows, n, 2048), ceil(items / 256)), and
blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which
only lowers it.  So B <= max(1, floor(W*H*7/4 / 16384)) and B <= H/2, and the 256 lanes of a workgroup step through the frame by
256 * B items: 16 x 2 pixel groups on the vector walk (W*H/32 items), 2 x 2 blocks on the byte walk (W*H/4 items)."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import yuv420_packed422_frames_cases as cases
from mi_lumaeq import xfer, UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY, CHROMA_PLANAR, CHROMA_INTERLEAVED, Yuv420Packed422FrameDev, Yuv420Planes
from test_gpu_nv12_to_bgr_frames import Arena, Plane, SENT, BAD_ARG, UNSUPPORTED, stream, frames_per_launch, launches
from test_yuv420_to_packed422_frames_abi import max_pairs_lds_f32
from yuv420_packed422_ref import content, expected_frame, uv_rows, _ref

pytestmark = pytest.mark.gpu
SRCS = ["nv12", "i420", "yv12"]
FMTS = [FMT_YUY2, FMT_UYVY]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)


class Half:
    """The left or the right W/2 bytes of every row of a plane of W-byte rows: U and V rows side by side in one pitched plane."""

    def __init__(self, plane, xoff):
        self.plane, self.xoff, self.arena, self.pitch = plane, xoff, plane.arena, plane.pitch

    @property
    def ptr(self):
        return self.plane.ptr + self.xoff

    def put(self, data):
        p, half = self.plane, self.plane.row_bytes // 2
        d = np.asarray(data, np.uint8).reshape(p.rows, half)
        for r in range(p.rows):
            o = p.off + r * p.pitch + self.xoff
            p.arena.img[o: o + half] = d[r]


class Pool:
    """n frames of one shape: a decoder's surface pool (ys; us and vs, or the UV planes in us with vs None) and a playout buffer pool
    (outs).  skew(k) -> the offsets of frame k's (y, c0, c1, out) past a 16-byte boundary; arenas: (Y, first chroma, second chroma, out)
    allocations to carve the planes from instead of one allocation each; side_by_side: U and V are the two halves of the rows of ONE
    plane of W-byte rows at c_pitch."""

    def __init__(self, w, h, n, src="i420", y_pitch=None, c_pitch=None, out_pitch=None, skew=lambda k: (0, 0, 0, 0), arenas=None,
                 gap=lambda k: 0, side_by_side=False):
        self.w, self.h, self.n, self.src = w, h, n, src
        ay, a1, a2, ao = arenas or (None, None, None, None)
        self.ys, self.us, self.vs, self.outs = [], [], [], []
        for k in range(n):
            sy, s0, s1, so = skew(k)
            self.ys.append(Plane(h, w, y_pitch, sy, ay, gap(k)))
            if src == "nv12":
                u, v = Plane(h // 2, w, c_pitch, s0, a1, gap(k)), None
            elif side_by_side:
                assert (s0, s1) == (0, 0)
                both = Plane(h // 2, w, c_pitch, 0, a1, gap(k))
                u, v = (Half(both, 0), Half(both, w // 2)) if src == "i420" else (Half(both, w // 2), Half(both, 0))
            elif src == "i420":
                u = Plane(h // 2, w // 2, c_pitch, s0, a1, gap(k))
                v = Plane(h // 2, w // 2, c_pitch, s1, a2, gap(k))
            else:
                v = Plane(h // 2, w // 2, c_pitch, s1, a1, gap(k))
                u = Plane(h // 2, w // 2, c_pitch, s0, a2, gap(k))
            self.us.append(u)
            self.vs.append(v)
            self.outs.append(Plane(h, 2 * w, out_pitch, so, ao, gap(k)))
        self.pitches = dict(y_pitch=self.ys[0].pitch, c_pitch=self.us[0].pitch, out_pitch=self.outs[0].pitch)
        self.chroma = CHROMA_INTERLEAVED if src == "nv12" else CHROMA_PLANAR

    def in_arenas(self):
        return list({id(p.arena): p.arena for p in self.ys + self.us + [v for v in self.vs if v is not None]}.values())

    def out_arenas(self):
        return list({id(p.arena): p.arena for p in self.outs}.values())

    def entries(self, idx=None, chroma=True):
        idx = range(self.n) if idx is None else idx
        return [Yuv420Packed422FrameDev(self.ys[k].ptr, self.us[k].ptr if chroma else None,
                                        self.vs[k].ptr if chroma and self.vs[k] is not None else None, self.outs[k].ptr) for k in idx]

    def load(self, frames):
        """Upload `frames` ((Y, U, V) of content()); every packed frame back to the sentinel."""
        for k, (y, u, v) in enumerate(frames):
            self.ys[k].put(y)
            if self.src == "nv12":
                self.us[k].put(uv_rows(u, v))
            else:
                self.us[k].put(u)
                self.vs[k].put(v)
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


def call(c, op, entries, w, h, fmt, uv_mode, pitches, chroma, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = (entries, w, h, pitches["y_pitch"], pitches["c_pitch"], chroma, fmt, uv_mode)
    kw = dict(out_pitch=pitches["out_pitch"], stream=stream() if st is None else st)
    if kind == "eq":
        c.equalize_hist_yuv420_to_packed422_frames_dev(*a, **kw)
    else:
        c.clahe_yuv420_to_packed422_frames_dev(*a, *cfg, **kw)


def stats(c):
    return tuple(c.get_stat(s) for s in cases.COUNTERS)


def delta(before, after):
    return tuple(a - b for a, b in zip(after, before))


def check(c, frames, pool, op, fmt, uv_mode, want, perm=None, contract=False, entries=None, pitches=None):
    """One call on uploaded `frames`: exact packed frames, untouched guards and inputs, and the counters moved by `want` = (onepass,
    twopass, list_frames_vec, list_frames_bytes) and by nothing else.  perm: the order in which the frames appear in the list;
    entries / pitches: what the call is given instead of the pool's own."""
    w, h = pool.w, pool.h
    pool.load(frames)
    for k, f in enumerate(frames):
        pool.outs[k].put(expected_frame(f, op, fmt, uv_mode, contract))
    before = stats(c)
    call(c, op, entries or pool.entries(perm), w, h, fmt, uv_mode, pitches or pool.pitches, pool.chroma)
    torch.cuda.synchronize()
    pool.verify((w, h, pool.src, op, fmt, uv_mode))
    assert delta(before, stats(c)) == tuple(want) + (0, 0), (pool.src, op, fmt, uv_mode, want, delta(before, stats(c)))


def would_loop(w, h, vec):
    """more items than the lanes of the largest grid the launcher takes (the bound on B of the module docstring)"""
    bound = max(1, w * h * 7 // 4 // 16384)
    return (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2)


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small allocations leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    _ref.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. the smallest frames ------------------------------------------------------------------------------------------------------
SMALLEST = [
    # W, H, the CLAHE grids, (onepass, twopass, vec frames, byte frames) of equalizeHist and of each grid, n = 3
    (2, 2, [(2.0, 1, 1)], (1, 0, 0, 3), [(0, 1, 0, 3)]),                          # one 2 x 2 block; no grid gives 16-column tiles
    (16, 2, [(2.0, 1, 1)], (1, 0, 3, 0), [(1, 0, 3, 0)]),                         # one 16 x 2 group; planar: U and V 8 bytes each, V at 8 mod 16
    (18, 4, [(2.0, 1, 2)], (1, 0, 0, 3), [(0, 1, 0, 3)]),                         # ragged rows: bytes
    (48, 6, [(2.0, 3, 3), (2.0, 2, 2)], (1, 0, 3, 0), [(1, 0, 3, 0), (0, 1, 3, 0)]),   # 3 x 3: tile 16 x 2, one-pass; 2 x 2: tile_w 24, two-pass
]


@pytest.mark.parametrize("src", SRCS)
@pytest.mark.parametrize("w,h,grids,want_eq,want_cl", SMALLEST, ids=[f"{s[0]}x{s[1]}" for s in SMALLEST])
def test_smallest_frames(c, w, h, grids, want_eq, want_cl, src):
    """Each layout, both formats, both UV modes.  16 x 2 planar: the U and V rows lie side by side in one 16-byte row (c1 = c0 + 8), both
    multiples of 8: still the groups."""
    n = 3
    pool = Pool(w, h, n, src, side_by_side=(w == 16 and src != "nv12"))
    if w == 16 and src != "nv12":
        e = pool.entries()[0]
        assert abs(e.c1 - e.c0) == 8 and (e.c1 > e.c0) == (src == "i420") and pool.pitches["c_pitch"] == 16
    frames = content(w, h, n, 61)
    for fmt in FMTS:
        for uv_mode in UV_MODES:
            check(c, frames, pool, EQ, fmt, uv_mode, want_eq)
            for cfg, want in zip(grids, want_cl):
                check(c, frames, pool, ("clahe", cfg), fmt, uv_mode, want)


# ---- 2. mixed walks in one launch ------------------------------------------------------------------------------------------------
CL21 = ("clahe", (2.0, 2, 1))
#          id           src     the middle frame's (y, c0, c1, out) skew   bytes?
BROKEN = [("y+1", "i420", (1, 0, 0, 0), True), ("y+1-nv12", "nv12", (1, 0, 0, 0), True), ("out+4", "yv12", (0, 0, 0, 4), True),
          ("c0+8-interleaved", "nv12", (0, 8, 0, 0), True), ("c0c1+8-planar", "i420", (0, 8, 8, 0), False),
          ("c1+4-planar", "i420", (0, 0, 4, 0), True), ("c0+4-planar", "yv12", (0, 4, 0, 0), True)]


@pytest.mark.parametrize("name,src,bad,breaks", BROKEN, ids=[b[0] for b in BROKEN])
def test_per_frame_alignment(c, name, src, bad, breaks):
    """32 x 4, n = 3, pitches 48 / 24 (planar) or 48 (interleaved) / 80: the shape allows the groups.  The middle frame has ONE term of
    its rule broken: it alone takes the byte walk inside the same launch and equalizeHist stays one pass.  CLAHE 2 x 1 (tiles of 16 x 4),
    whose blend + pack kernel has no byte path, then takes the fallback for the whole call; its pack reads the luma from the context's
    aligned scratch planes, so a broken y alone leaves all three frames on the groups there.  Planar chroma 8 past a 16-byte boundary
    breaks nothing."""
    w, h, n = 32, 4, 3
    frames = content(w, h, n, 62)
    pool = Pool(w, h, n, src, y_pitch=48, c_pitch=48 if src == "nv12" else 24, out_pitch=80, skew=lambda k: bad if k == 1 else (0, 0, 0, 0))
    e = pool.entries()[1]
    assert [e.y % 16, e.c0 % 16, (e.c1 or 0) % 16, e.out % 16] == list(bad)
    for fmt in FMTS:
        if not breaks:
            check(c, frames, pool, EQ, fmt, UV_COPY, (1, 0, 3, 0))
            check(c, frames, pool, CL21, fmt, UV_COPY, (1, 0, 3, 0))
            continue
        check(c, frames, pool, EQ, fmt, UV_COPY, (1, 0, 2, 1))
        check(c, frames, pool, CL21, fmt, UV_COPY, (0, 1, 3, 0) if bad[0] else (0, 1, 2, 1))
    # under MI_UV_FILL128 a chroma address decides nothing
    chroma_only = breaks and not bad[0] and not bad[3]
    check(c, frames, pool, EQ, FMT_YUY2, UV_FILL128, (1, 0, 3, 0) if chroma_only or not breaks else (1, 0, 2, 1))
    if chroma_only:
        check(c, frames, pool, CL21, FMT_UYVY, UV_FILL128, (1, 0, 3, 0))


# ---- 3. the shape term -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,pitch", [("i420", dict(c_pitch=20)), ("i420", dict(y_pitch=40)), ("nv12", dict(c_pitch=40)), ("nv12", dict(y_pitch=40))],
                         ids=["planar-c_pitch-20", "planar-y_pitch-40", "interleaved-c_pitch-40", "interleaved-y_pitch-40"])
def test_shape_term(c, src, pitch):
    """The same pool with a chroma pitch that is no multiple of 8 (planar) or 16 (interleaved), or a Y pitch that is no multiple of 16:
    every frame takes the byte walk although all its addresses are aligned (in the CLAHE fallback too: the shape is judged on the
    caller's pitches).  Under MI_UV_FILL128 the chroma pitch decides nothing."""
    w, h, n = 32, 4, 3
    frames = content(w, h, n, 63)
    pool = Pool(w, h, n, src, **dict(dict(y_pitch=48, c_pitch=48 if src == "nv12" else 24, out_pitch=80), **pitch))
    assert all((e.y | e.c0 | (e.c1 or 0) | e.out) % 16 == 0 for e in pool.entries())
    for fmt in FMTS:
        check(c, frames, pool, EQ, fmt, UV_COPY, (1, 0, 0, 3))
        check(c, frames, pool, CL21, fmt, UV_COPY, (0, 1, 0, 3))
    if "c_pitch" in pitch:
        check(c, frames, pool, EQ, FMT_UYVY, UV_FILL128, (1, 0, 3, 0))
        check(c, frames, pool, CL21, FMT_YUY2, UV_FILL128, (1, 0, 3, 0))


# ---- 4. MI_UV_FILL128 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["nv12", "i420"])
def test_fill128_ignores_the_chroma_arguments(c, src):
    """c0 = c1 = NULL with c_pitch 0, and c0 / c1 / c_pitch set to odd junk: c0 an odd address inside the frame's OWN output buffer (so
    it would fail the overlap check if it took part), c1 an odd address inside its Y plane, c_pitch 7 (below its row).  Same bytes as
    with the real planes, every frame on the groups, CLAHE one-pass, and the chroma planes -- guarded allocations next to the others --
    are untouched."""
    w, h, n = 32, 4, 3
    frames = content(w, h, n, 64)
    pool = Pool(w, h, n, src, y_pitch=48, c_pitch=48 if src == "nv12" else 24, out_pitch=80)
    null = pool.entries(chroma=False)
    assert all(e.c0 is None and e.c1 is None for e in null)
    junk = [Yuv420Packed422FrameDev(e.y, e.out + 5, e.y + 3, e.out) for e in pool.entries()]
    for fmt in FMTS:
        for op in (EQ, CL21):
            check(c, frames, pool, op, fmt, UV_FILL128, (1, 0, 3, 0))
            check(c, frames, pool, op, fmt, UV_FILL128, (1, 0, 3, 0), entries=null, pitches=dict(pool.pitches, c_pitch=0))
            check(c, frames, pool, op, fmt, UV_FILL128, (1, 0, 3, 0), entries=junk, pitches=dict(pool.pitches, c_pitch=7))


# ---- 5. a lane past its first item -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", SRCS)
def test_equalize_loops_past_first_step(c, src):
    """yuv420_to_packed422_frames_kernel<.., LUT = true> where a lane owns more than one item.  96 x 144 x 2 on the vector walk:
    B <= max(1, floor(96*144*7/4 / 16384)) = 1, so 432 groups for 256 lanes: the carried (by, gx) walk wraps, the second step is
    partial.  66 x 34 at y_pitch 67, c_pitch 35 (planar) / 67 (interleaved), out_pitch 136 on the byte walk: B <= 1, 561 blocks."""
    n = 2
    w, h = 96, 144
    assert would_loop(w, h, True), "the shape would not loop"
    fmt = FMTS[SRCS.index(src) % 2]
    check(c, content(w, h, n, 65), Pool(w, h, n, src), EQ, fmt, UV_COPY, (1, 0, 2, 0))
    w, h = 66, 34
    assert would_loop(w, h, False), "the shape would not loop"
    pool = Pool(w, h, n, src, y_pitch=67, c_pitch=67 if src == "nv12" else 35, out_pitch=136, skew=lambda k: (1, 3, 5 if src != "nv12" else 0, 4))
    check(c, content(w, h, n, 66), pool, EQ, FMT_UYVY if fmt == FMT_YUY2 else FMT_YUY2, UV_COPY, (1, 0, 0, 2))


@pytest.mark.parametrize("src", ["nv12", "yv12"])
@pytest.mark.parametrize("broken", [False, True], ids=["aligned", "one-frame-out+4"])
def test_pack_only_loops_past_first_step(c, broken, src):
    """yuv420_to_packed422_frames_kernel<.., LUT = false>, the second pass of the CLAHE fallback, at 96 x 144 (B <= 1: 432 groups or
    3456 blocks for 256 lanes): 144 % 5 != 0, so a 4 x 5 grid pads by REFLECT_101 and the call goes two-pass.  The luma comes from the
    context's scratch planes.  Aligned: both frames on the groups; with the output of ONE frame 4 past a 16-byte boundary both walks
    run in one launch."""
    w, h, n = 96, 144, 2
    assert would_loop(w, h, True) and would_loop(w, h, False), "the shape would not loop"
    pool = Pool(w, h, n, src, skew=lambda k: (0, 0, 0, 4 * int(broken and k == 1)))
    check(c, content(w, h, n, 67), pool, ("clahe", (2.0, 4, 5)), FMT_YUY2 if src == "nv12" else FMT_UYVY, UV_COPY,
          (0, 1, 1, 1) if broken else (0, 1, 2, 0))


# ---- 6. one-pass kernel geometry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", SRCS)
def test_clahe_onepass_odd_tile_height(c, src):
    """48 x 30, 3 x 2 (tile 16 x 15: an odd tile height, so a row pair straddles two bands; three groups a row), every pitch larger than
    its row and planar chroma planes 8 past a 16-byte boundary: yuv420_packed422_clahe_interp_frames_kernel with guards."""
    w, h, n = 48, 30, 2
    planar = src != "nv12"
    pool = Pool(w, h, n, src, y_pitch=64, c_pitch=40 if planar else 64, out_pitch=112, skew=lambda k: (0, 8, 8, 0) if planar else (0, 0, 0, 0))
    frames = content(w, h, n, 68)
    for fmt, uv_mode in ((FMT_YUY2, UV_COPY), (FMT_UYVY, UV_COPY), (FMT_UYVY, UV_FILL128)):
        check(c, frames, pool, ("clahe", (2.0, 3, 2)), fmt, uv_mode, (1, 0, 2, 0))


@pytest.mark.parametrize("src", ["nv12", "i420"])
def test_clahe_onepass_two_column_segments(c, src):
    """4112 x 4 at 1 x 2, n = 2: 257 groups a row, so two column segments, the second of one group; 64 x 32 at 4 x 4."""
    w, h, n = 4112, 4, 2
    check(c, content(w, h, n, 69), Pool(w, h, n, src), ("clahe", (2.0, 1, 2)), FMT_YUY2, UV_COPY, (1, 0, 2, 0))
    w, h = 64, 32
    check(c, content(w, h, n, 70), Pool(w, h, n, src), ("clahe", (2.0, 4, 4)), FMT_UYVY, UV_COPY, (1, 0, 2, 0))


# ---- 7. clahe_fp_contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["nv12", "i420"])
def test_fp_contract_takes_the_fallback_and_back(src):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    frames = content(w, h, n, 71)
    pool = Pool(w, h, n, src)
    with mi_lumaeq.Context(0) as c:
        c.set_option("clahe_fp_contract", 1)
        try:
            check(c, frames, pool, ("clahe", (2.0, 4, 2)), FMT_YUY2, UV_COPY, (0, 1, 2, 0), contract=True)
        finally:
            c.set_option("clahe_fp_contract", 0)
        check(c, frames, pool, ("clahe", (2.0, 4, 2)), FMT_YUY2, UV_COPY, (1, 0, 2, 0))


# ---- 8. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,one,src", [(EQ, 1, "yv12"), (("clahe", (2.0, 2, 2)), 1, "nv12"), (("clahe", (2.0, 3, 2)), 0, "i420")],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, op, one, src):
    """One frame more than two full launches: three chunks, the last of one frame.  The planes are carved at irregular (16-byte
    aligned) distances out of a few large allocations, which keeps the allocation count small; every frame is distinct and every frame
    is checked (the fallback reuses its scratch planes from chunk to chunk)."""
    w, h = 32, 16
    per = frames_per_launch()
    assert per == 64
    n = 2 * per + 1
    frames = content(w, h, n, 72)

    def gap(k):
        return 16 * ((k * 7) % 5)
    crow = w * h // 2 if src == "nv12" else w * h // 4
    arenas = (Arena(n * (w * h + 96) + 64), Arena(n * (crow + 96) + 64), Arena(n * (crow + 96) + 64), Arena(n * (2 * w * h + 96) + 64))
    pool = Pool(w, h, n, src, arenas=arenas, gap=gap)
    assert len({pool.us[k + 1].ptr - pool.us[k].ptr for k in range(n - 1)}) > 1, "the chroma planes are not at one stride"
    assert len({f[0].tobytes() for f in frames}) == n
    check(c, frames, pool, op, FMT_UYVY, UV_COPY, (one, 1 - one, n, 0))


# ---- 9. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["nv12", "i420"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))], ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_identity_with_the_batch_form(c, op, src):
    """The list call on separate allocations and mi_*_yuv420_to_packed422_batch_dev on the same pixels in one allocation: byte-equal."""
    w, h, n = 64, 32, 3
    frames = content(w, h, n, 73)
    pool = Pool(w, h, n, src).load(frames)
    tight = np.stack([np.concatenate([y.ravel(), uv_rows(u, v).ravel()] if src == "nv12" else [y.ravel(), u.ravel(), v.ravel()]) for y, u, v in frames])
    d_in = xfer.to_device(tight)
    d_batch = torch.full((n, h, 2 * w), SENT, dtype=torch.uint8, device="cuda:0")
    call(c, op, pool.entries(), w, h, FMT_YUY2, UV_COPY, pool.pitches, pool.chroma)
    planes = (Yuv420Planes.nv12 if src == "nv12" else Yuv420Planes.i420)(d_in, w, h)
    if op is EQ:
        c.equalize_hist_yuv420_to_packed422_batch_dev(planes, d_batch, w, h, n, FMT_YUY2, UV_COPY, stream=stream())
    else:
        c.clahe_yuv420_to_packed422_batch_dev(planes, d_batch, w, h, n, FMT_YUY2, UV_COPY, *op[1], stream=stream())
    torch.cuda.synchronize()
    batch = xfer.to_host(d_batch)
    for k in range(n):
        assert np.array_equal(batch[k], expected_frame(frames[k], op, FMT_YUY2, UV_COPY)), ("batch form", op, k)
        pool.outs[k].put(batch[k])
    pool.verify(("list form against batch form", op))


# ---- 10. edges -------------------------------------------------------------------------------------------------------------------
def test_one_input_two_outputs(c):
    """The same {y, c0, c1} in two entries with different outputs: inputs are only read, both frames are exact (hence equal)."""
    w, h = 32, 16
    frame = content(w, h, 1, 74)[0]
    pool = Pool(w, h, 2)
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        pool.load([frame, frame])
        for k in range(2):
            pool.outs[k].put(expected_frame(frame, op, FMT_UYVY, UV_COPY))
        e = pool.entries()
        e[1] = Yuv420Packed422FrameDev(e[0].y, e[0].c0, e[0].c1, e[1].out)
        before = stats(c)
        call(c, op, e, w, h, FMT_UYVY, UV_COPY, pool.pitches, pool.chroma)
        torch.cuda.synchronize()
        pool.verify(("one input, two outputs", op))
        assert delta(before, stats(c)) == (1, 0, 2, 0, 0, 0)


@pytest.mark.parametrize("src", SRCS)
def test_permuted_list_on_pitched_frames(c, src):
    """64 x 32 at pitches 80 / 40 (planar: every second chroma row 8 past a 16-byte boundary) or 96 / 144: the list is a permutation of
    the pool, so its addresses are not monotonic.  Pitch padding and allocation tails keep their sentinel."""
    w, h, n = 64, 32, 3
    frames = content(w, h, n, 75)
    pool = Pool(w, h, n, src, y_pitch=80, c_pitch=96 if src == "nv12" else 40, out_pitch=144)
    check(c, frames, pool, ("clahe", (2.0, 4, 2)), FMT_YUY2, UV_COPY, (1, 0, 3, 0), perm=(2, 0, 1))
    check(c, frames, pool, EQ, FMT_UYVY, UV_COPY, (1, 0, 3, 0), perm=(1, 2, 0))
    check(c, frames, pool, ("clahe", (2.0, 3, 2)), FMT_UYVY, UV_COPY, (0, 1, 3, 0), perm=(0, 2, 1))


@pytest.mark.parametrize("src", ["i420", "yv12"])
def test_u_and_v_as_two_halves_of_one_plane(c, src):
    """c1 = c0 + W/2 (or c0 = c1 + W/2) at c_pitch = W: U and V are not compared with each other.  32 x 16: both are multiples of 16."""
    w, h, n = 32, 16, 2
    pool = Pool(w, h, n, src, side_by_side=True)
    e = pool.entries()[0]
    assert abs(e.c1 - e.c0) == w // 2 and pool.pitches["c_pitch"] == w
    frames = content(w, h, n, 76)
    for op in (EQ, ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 3, 2))):
        one = int(op[1] != (2.0, 3, 2))
        check(c, frames, pool, op, FMT_YUY2, UV_COPY, (one, 1 - one, 2, 0))


# ---- 11. hipGraph ----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_two_replays():
    """One eager call of the shape, then capture on a side stream and two replays, each onto fresh input bytes at the same addresses."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, "i420", y_pitch=80, c_pitch=40, out_pitch=144)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            one = int(op[1] != (2.0, 3, 2))
            check(c, content(w, h, n, 77), pool, op, FMT_YUY2, UV_COPY, (one, 1 - one, 3, 0))   # sizes the scratch
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(c, op, pool.entries(), w, h, FMT_YUY2, UV_COPY, pool.pitches, pool.chroma, st=torch.cuda.current_stream().cuda_stream)
            for seed in (78, 79):
                fresh = content(w, h, n, seed)
                pool.load(fresh)
                for k, f in enumerate(fresh):
                    pool.outs[k].put(expected_frame(f, op, FMT_YUY2, UV_COPY))
                g.replay()
                torch.cuda.synchronize()
                pool.verify(("graph replay", op, seed))


# ---- 12. refusals, zero sizes, launch accounting ---------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    frames = content(w, h, n, 80)
    pool = Pool(w, h, n, y_pitch=48, c_pitch=24, out_pitch=80).load(frames)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(e.y, e.c0, e.c1, e.out) for e in pool.entries()]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, yp=48, cp=24, chroma=CHROMA_PLANAR, op=80, fmt=FMT_YUY2, uv=UV_COPY)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (Yuv420Packed422FrameDev * max(1, len(a["entries"])))(*[Yuv420Packed422FrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["yp"], a["cp"], a["chroma"], a["op"], a["fmt"], a["uv"])

        def eq(**kw):
            return L.mi_equalize_hist_yuv420_to_packed422_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_yuv420_to_packed422_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(**over):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = dict(zip(("y", "c0", "c1", "out"), good[-1]))
            e.update({k: (None if v == "null" else v) for k, v in over.items()})
            return dict(entries=good[:-1] + [(e["y"], e["c0"], e["c1"], e["out"])])
        y2, u2, v2, o2 = good[-1]
        img = (h - 1) * 80 + 2 * w                                                             # the bytes a packed frame spans
        INTER = dict(chroma=CHROMA_INTERLEAVED, cp=48)                                        # a valid interleaved shape on the same addresses
        FILL = dict(uv=UV_FILL128)
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(y="null"), last(out="null"), last(c0="null"), last(c1="null"),           # a null address in the last entry
               dict(INTER, **last(c0="null")), dict(FILL, **last(y="null")), dict(FILL, **last(out="null")),
               dict(entries=[(None,) + good[0][1:]] + good[1:]),                             # ... and in the first
               last(out=o2 + 2), last(out=o2 + 1), dict(FILL, **last(out=o2 + 2)), dict(op=82), dict(op=81),   # out / out_pitch no multiple of 4
               dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1),                          # a format other than the two
               dict(chroma=2), dict(chroma=-1),                                              # a chroma other than the two
               dict(uv=2), dict(uv=-1),                                                      # a bad uv_mode
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(yp=w - 1), dict(cp=w // 2 - 1), dict(op=2 * w - 4),                      # a pitch below its row
               dict(chroma=CHROMA_INTERLEAVED, cp=w - 1),                                    # ... W for an interleaved chroma plane
               # no in-place form, compared as address ranges: the output of the last frame on its own Y, U and V plane, ending four
               # bytes inside its V plane, and starting on the last dword of its Y plane's last row
               last(out=y2), last(out=u2), last(out=v2), last(out=v2 - img + 4), last(out=y2 + (h - 1) * 48 + w - 4),
               dict(INTER, **last(out=u2)), dict(FILL, **last(out=y2))]
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, **INTER) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written -- a null list is fine when there are no frames
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, lst=NULL_LIST), dict(INTER, n=0), dict(FILL, w=0)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: the batch form's status
        big = dict(w=(1 << 24) + 2, h=2, yp=1 << 25, cp=1 << 24, op=1 << 27)
        y0, u0, v0, o0 = good[0]
        planes = Yuv420Planes(y0, 1 << 25, u0, v0, 1 << 24, 1 << 27, CHROMA_PLANAR)
        batch = L.mi_equalize_hist_yuv420_to_packed422_batch_dev(hd, planes, o0, 1 << 27, 1 << 28, big["w"], 2, 1, FMT_YUY2, UV_COPY, stream())
        assert batch == UNSUPPORTED and eq(**big) == batch and cl(**big) == batch
        planes = Yuv420Planes(y0, 48, u0, v0, 24, 0, CHROMA_PLANAR)
        batch = L.mi_clahe_yuv420_to_packed422_batch_dev(hd, planes, o0, 80, 0, w, h, 1, FMT_YUY2, UV_COPY, 2.0, 2048, 1024, stream())
        assert batch == UNSUPPORTED and cl(2048, 1024) == batch
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0,) * 6
        # launch accounting of the three sequences, by role: the batch form's slots; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (1, 0, 3, 0)),
                             (("clahe", (2.0, 2, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (1, 0, 3, 0)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (0, 1, 3, 0))):
            c.profile_read(reset=True)
            check(c, frames, pool, op, FMT_UYVY, UV_COPY, st)
            got = launches(c)
            assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 13. pipe pending ------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(content(w, h, 1, 81))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, pool.entries(), w, h, FMT_YUY2, UV_COPY, pool.pitches, pool.chroma)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")
        assert stats(c) == (0,) * 6


# ---- 14. seeded sweep ------------------------------------------------------------------------------------------------------------
def test_seeded_sweep(c):
    """The 32 cases of tests/yuv420_packed422_frames_cases.py (tests/test_yuv420_to_packed422_frames_abi.py asserts their class counts on
    the CPU): exact bytes, whole allocations, and the six counter deltas the documented rule gives.  No case is skipped."""
    K = max_pairs_lds_f32()
    sweep = cases.sweep_cases()
    assert len(sweep) == 32 and min(cases.class_counts(sweep, K).values()) >= 4
    c.set_option("clahe_fp_contract", 0)
    ran = 0
    for i, k in enumerate(sweep):
        w, h, n, sk = k["w"], k["h"], k["n"], k["skews"]
        op = EQ if k["kind"] == "eq" else ("clahe", (k["clip"], k["tx"], k["ty"]))
        frames = content(w, h, n, 500 + i)
        want = cases.classify(k, K)[1]
        pool = Pool(w, h, n, k["src"], y_pitch=k["y_pitch"], c_pitch=k["c_pitch"], out_pitch=k["out_pitch"], skew=lambda f: sk[f]).load(frames)
        entries = pool.entries()
        for f in range(n):
            e = entries[f]
            assert [e.y % 16, e.c0 % 16, (e.c1 or 0) % 16, e.out % 16] == [s % 16 for s in sk[f]], (i, f)
            pool.outs[f].put(expected_frame(frames[f], op, k["fmt"], k["uv_mode"]))
        before = stats(c)
        call(c, op, entries, w, h, k["fmt"], k["uv_mode"], pool.pitches, pool.chroma)
        torch.cuda.synchronize()
        pool.verify((i, k))
        assert delta(before, stats(c)) == want, (i, k, want, delta(before, stats(c)))
        ran += 1
    assert ran == 32
