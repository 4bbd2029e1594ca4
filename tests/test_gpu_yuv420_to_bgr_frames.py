"""Planar 4:2:0 (I420 / YV12) in, interleaved BGR / RGB out on a LIST of pitched device frames on the GPU:
mi_equalize_hist_yuv420_to_bgr_frames_dev and mi_clahe_yuv420_to_bgr_frames_dev.  Expected bytes are
oracle.nv12_to_bgr(oracle.nv12_frame(<Y, then U and V interleaved>, W, H, 1, op...), W, H), the last axis reversed for MI_ORDER_RGB
(the `expected` of tests/test_gpu_nv12_to_bgr_frames.py, computed once per frame and shared).  Y, U and V are full-range random bytes.
Every Y, U and V plane and every image is its own sentinel-filled torch allocation with guard bytes unless a test says otherwise, and
every allocation is compared WHOLE, inputs included.  Every call asserts the deltas of eight counters: yuv420_bgr_onepass /
yuv420_bgr_twopass (one count a call), yuv420_bgr_list_frames_vec / yuv420_bgr_list_frames_bytes (FRAMES by their walk),
yuv420_bgr_vec / yuv420_bgr_bytes (never moved by a list call) and nv12_bgr_onepass / nv12_bgr_twopass (moved by INTERLEAVED lists
only).  Every comparison in this file is exact.

A frame pool has no layout of its own: "i420" and "yv12" say which of a frame's two chroma allocations (data[1], data[2]) holds U.
The entry always carries U in c0 and V in c1, so a YV12 frame passes data[2] as c0."""
import re

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
import yuv420_bgr_frames_cases as cases
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, CHROMA_PLANAR, CHROMA_INTERLEAVED, Yuv420BgrFrameDev, Yuv420Planes
from test_gpu_nv12_to_bgr_frames import (Arena, Plane, Pool as Nv12Pool, SENT, EQ, ORDERS, BAD_ARG, UNSUPPORTED, ROOT, stream, rand_frames,
                                         expected, frames_per_launch, launches, call as nv12_call)

pytestmark = pytest.mark.gpu
FMTS = ["i420", "yv12"]
CL22 = ("clahe", (2.0, 2, 2))


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
    """n frames of one shape: a software decoder's frame pool (ys; us and vs, carried by the frame's two chroma allocations in the order
    fmt says) and an image pool (outs).  skew(k) -> the offsets of frame k's (y, c0, c1, out) past a 16-byte boundary; arenas:
    (Y, data[1], data[2], out) allocations to carve the planes from instead of one allocation each; side_by_side: data[1] and data[2]
    are the two halves of the rows of ONE plane of W-byte rows at c_pitch."""

    def __init__(self, w, h, n, fmt="i420", y_pitch=None, c_pitch=None, out_pitch=None, skew=lambda k: (0, 0, 0, 0), arenas=None,
                 gap=lambda k: 0, side_by_side=False):
        self.w, self.h, self.n, self.fmt = w, h, n, fmt
        ay, a1, a2, ao = arenas or (None, None, None, None)
        self.ys, self.us, self.vs, self.outs = [], [], [], []
        for k in range(n):
            sy, s0, s1, so = skew(k)
            self.ys.append(Plane(h, w, y_pitch, sy, ay, gap(k)))
            if side_by_side:
                assert (s0, s1) == (0, 0)
                both = Plane(h // 2, w, c_pitch, 0, a1, gap(k))
                first, second = Half(both, 0), Half(both, w // 2)
            else:
                sa, sb = (s0, s1) if fmt == "i420" else (s1, s0)
                first = Plane(h // 2, w // 2, c_pitch, sa, a1, gap(k))
                second = Plane(h // 2, w // 2, c_pitch, sb, a2, gap(k))
            u, v = (first, second) if fmt == "i420" else (second, first)
            self.us.append(u)
            self.vs.append(v)
            self.outs.append(Plane(h, 3 * w, out_pitch, so, ao, gap(k)))
        self.pitches = dict(y_pitch=self.ys[0].pitch, c_pitch=self.us[0].pitch, out_pitch=self.outs[0].pitch)

    def in_arenas(self):
        return list({id(p.arena): p.arena for p in self.ys + self.us + self.vs}.values())

    def out_arenas(self):
        return list({id(p.arena): p.arena for p in self.outs}.values())

    def entries(self, idx=None):
        idx = range(self.n) if idx is None else idx
        return [Yuv420BgrFrameDev(self.ys[k].ptr, self.us[k].ptr, self.vs[k].ptr, self.outs[k].ptr) for k in idx]

    def load(self, frames):
        """Upload `frames` (tight NV12: the U, V pairs are split into the two planes); every image back to the sentinel."""
        w, h = self.w, self.h
        for k, f in enumerate(frames):
            uv = f[w * h:].reshape(h // 2, w)
            self.ys[k].put(f[: w * h])
            self.us[k].put(uv[:, 0::2])
            self.vs[k].put(uv[:, 1::2])
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


def call(c, op, entries, w, h, order, pitches, chroma=CHROMA_PLANAR, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = (entries, w, h, pitches["y_pitch"], pitches["c_pitch"], chroma, order)
    kw = dict(out_pitch=pitches["out_pitch"], stream=stream() if st is None else st)
    if kind == "eq":
        c.equalize_hist_yuv420_to_bgr_frames_dev(*a, **kw)
    else:
        c.clahe_yuv420_to_bgr_frames_dev(*a, *cfg, **kw)


def stats(c):
    return tuple(c.get_stat(s) for s in cases.COUNTERS)


def delta(before, after):
    return tuple(a - b for a, b in zip(after, before))


def check(c, frames, pool, op, order, want, perm=None, contract=False):
    """One call on uploaded `frames`: exact images, untouched guards and inputs, and the counters moved by `want` = (onepass, twopass,
    list_frames_vec, list_frames_bytes) and by nothing else.  perm: the order in which the frames appear in the list."""
    w, h = pool.w, pool.h
    pool.load(frames)
    for k, f in enumerate(frames):
        pool.outs[k].put(expected(f, w, h, op, order, contract))
    before = stats(c)
    call(c, op, pool.entries(perm), w, h, order, pool.pitches)
    torch.cuda.synchronize()
    pool.verify((w, h, pool.fmt, op, order))
    assert delta(before, stats(c)) == tuple(want) + (0, 0, 0, 0), (op, want, delta(before, stats(c)))


def would_loop(w, h, vec):
    """tests/test_gpu_yuv420_to_bgr_geometry.py's own assertion: more items than the lanes of the largest grid the launcher takes"""
    bound = max(1, w * h * 9 // 4 // 16384)
    return (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2)


def max_pairs_lds_f32():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "clahe.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kMaxPairsLdsF32\s*=\s*(\d+)\s*;", src).group(1))


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


# ---- 1. fast path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FMTS)
def test_fast_path(c, fmt, order):
    """32 x 16, three frames, tight (chroma rows of 16 bytes), every allocation 16-byte aligned: 16 x 2 groups; CLAHE 2 x 2 (tiles of
    16 x 8) in one pass."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 131)
    pool = Pool(w, h, n, fmt)
    for op in (EQ, CL22):
        check(c, frames, pool, op, order, (1, 0, 3, 0))


# ---- 2. the smallest frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FMTS)
def test_smallest_frames(c, fmt, order):
    """16 x 2: one 16 x 2 group a frame, with the U and V rows side by side in one plane (c1 = c0 + 8, c_pitch = 16): legal, and both
    chroma addresses are multiples of 8; CLAHE 1 x 1 (one tile of 16 columns) is one-pass.  2 x 2: one block, one sample per chroma
    plane; no grid gives 16-column tiles, so CLAHE 1 x 1 takes the fallback."""
    n = 3
    pool = Pool(16, 2, n, fmt, side_by_side=True)
    e = pool.entries()[0]
    assert abs(e.c1 - e.c0) == 8 and (e.c1 > e.c0) == (fmt == "i420") and pool.pitches["c_pitch"] == 16
    frames = rand_frames(16, 2, n, 132)
    for op in (EQ, ("clahe", (2.0, 1, 1))):
        check(c, frames, pool, op, order, (1, 0, n, 0))
    pool = Pool(2, 2, 2, fmt)
    frames = rand_frames(2, 2, 2, 133)
    check(c, frames, pool, EQ, order, (1, 0, 0, 2))
    check(c, frames, pool, ("clahe", (2.0, 1, 1)), order, (0, 1, 0, 2))


# ---- 3. pitched with guards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FMTS)
def test_pitched_with_guards(c, fmt, order):
    """64 x 32 at pitches 80 / 40 / 208: the chroma pitch is a multiple of 8 and not of 16, so every second chroma row starts 8 past a
    16-byte boundary.  The list is a permutation of the pool, so its addresses are not monotonic.  CLAHE 4 x 2 stays one-pass; pitch
    padding and allocation tails keep their sentinel, in the images and in the planes."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 134)
    pool = Pool(w, h, n, fmt, y_pitch=80, c_pitch=40, out_pitch=208)
    assert pool.pitches["c_pitch"] % 16 == 8
    check(c, frames, pool, ("clahe", (2.0, 4, 2)), order, (1, 0, 3, 0), perm=(2, 0, 1))
    check(c, frames, pool, EQ, order, (1, 0, 3, 0), perm=(1, 2, 0))


# ---- 4. per-frame alignment ------------------------------------------------------------------------------------------------------
BROKEN = [("y", 0, 1), ("c0", 1, 4), ("c1", 2, 4), ("out", 3, 8)]


@pytest.mark.parametrize("name,which,by", BROKEN, ids=[f"{b[0]}+{b[2]}" for b in BROKEN])
def test_per_frame_alignment(c, name, which, by):
    """32 x 16 at pitches 48 / 24 / 112: the shape allows the 16 x 2 groups.  The middle frame of three has ONE address broken -- y by
    1 (rule: 16), c0 or c1 by 4 (rule: 8), out by 8 (rule: 16): it alone takes the byte walk inside the same launch, and equalizeHist
    stays one pass.  CLAHE 2 x 2, whose blend + decode kernel has no byte path, takes the fallback for the whole call; its decode reads
    the luma from the context's aligned scratch planes, so a broken y leaves every frame on the vector walk there."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 135)
    for order, fmt in zip(ORDERS, FMTS):
        pool = Pool(w, h, n, fmt, y_pitch=48, c_pitch=24, out_pitch=112, skew=lambda k: tuple(by * int(k == 1 and i == which) for i in range(4)))
        e = pool.entries()[1]
        assert [e.y % 16, e.c0 % 16, e.c1 % 16, e.out % 16] == [by * int(i == which) for i in range(4)]
        check(c, frames, pool, EQ, order, (1, 0, 2, 1))
        check(c, frames, pool, CL22, order, (0, 1, 3, 0) if name == "y" else (0, 1, 2, 1))


@pytest.mark.parametrize("order", ORDERS)
def test_chroma_at_multiples_of_8_stays_vector(c, order):
    """The control: the middle frame's c0 and c1 are 8 past a 16-byte boundary.  Three frames on the vector walk, CLAHE one-pass."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 135)
    pool = Pool(w, h, n, "i420", y_pitch=48, c_pitch=24, out_pitch=112, skew=lambda k: (0, 8 * (k == 1), 8 * (k == 1), 0))
    e = pool.entries()[1]
    assert (e.c0 % 16, e.c1 % 16) == (8, 8)
    check(c, frames, pool, EQ, order, (1, 0, 3, 0))
    check(c, frames, pool, CL22, order, (1, 0, 3, 0))


# ---- 5. the shape term -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", [dict(c_pitch=20), dict(y_pitch=40)], ids=["c_pitch-20", "y_pitch-40"])
def test_shape_term(c, pitch):
    """The same pool with a chroma pitch that is no multiple of 8, or a Y pitch that is no multiple of 16: every frame takes the byte
    walk although all its addresses are aligned (in the CLAHE fallback too: the shape is judged on the caller's pitches)."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 135)
    for order, fmt in zip(ORDERS, FMTS):
        pool = Pool(w, h, n, fmt, **dict(dict(y_pitch=48, c_pitch=24, out_pitch=112), **pitch))
        assert all((e.y | e.c0 | e.c1 | e.out) % 16 == 0 for e in pool.entries())
        check(c, frames, pool, EQ, order, (1, 0, 0, 3))
        check(c, frames, pool, CL22, order, (0, 1, 0, 3))


# ---- 6. general and fallback -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FMTS)
def test_general_and_fallback(c, fmt, order):
    """34 x 18 (W % 16 == 2, no tile grid divides it), odd pitches 35 / 19 / 103, addresses at odd offsets: 2 x 2 blocks with byte
    accesses; CLAHE 3 x 2 pads by REFLECT_101 and takes the planar CLAHE + decode fallback."""
    w, h, n = 34, 18, 2
    frames = rand_frames(w, h, n, 136)
    pool = Pool(w, h, n, fmt, y_pitch=35, c_pitch=19, out_pitch=103, skew=lambda k: (1 + 2 * k, 3, 7 + 2 * k, 5 + 6 * k))
    check(c, frames, pool, EQ, order, (1, 0, 0, 2))
    check(c, frames, pool, ("clahe", (2.0, 3, 2)), order, (0, 1, 0, 2))


# ---- 7. loops past their first step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_equalize_loops_past_first_step(c, order):
    """yuv420_to_bgr_frames_kernel<ORDER, true> where a lane owns more than one item: 96 x 144 x 2 on the vector walk (432 groups for
    256 lanes: the carried (by, gx) walk wraps, the second step is partial), 66 x 34 at odd pitches on the byte walk (561 blocks)."""
    fmt = FMTS[order]
    w, h, n = 96, 144, 2
    assert would_loop(w, h, True), "the shape would not loop"
    check(c, rand_frames(w, h, n, 137), Pool(w, h, n, fmt), EQ, order, (1, 0, 2, 0))
    w, h = 66, 34
    assert would_loop(w, h, False), "the shape would not loop"
    pool = Pool(w, h, n, fmt, y_pitch=67, c_pitch=35, out_pitch=201, skew=lambda k: (1, 3, 5, 7))
    check(c, rand_frames(w, h, n, 138), pool, EQ, order, (1, 0, 0, 2))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("broken", [False, True], ids=["aligned", "one-frame-out+1"])
def test_decode_only_loops_past_first_step(c, broken, order):
    """yuv420_to_bgr_frames_kernel<ORDER, false>, the second pass of the CLAHE fallback, at 96 x 144: 144 % 5 != 0, so a 4 x 5 grid
    pads by REFLECT_101 and the call goes two-pass.  The luma comes from the context's scratch planes.  Aligned: both frames on the
    vector walk; with the image of ONE frame one byte past a 16-byte boundary both walks run in one launch."""
    w, h, n = 96, 144, 2
    assert would_loop(w, h, True) and would_loop(w, h, False), "the shape would not loop"
    pool = Pool(w, h, n, FMTS[order], skew=lambda k: (0, 0, 0, int(broken and k == 1)))
    check(c, rand_frames(w, h, n, 139), pool, ("clahe", (2.0, 4, 5)), order, (0, 1, 1, 1) if broken else (0, 1, 2, 0))


@pytest.mark.parametrize("order", ORDERS)
def test_clahe_onepass_odd_tile_height(c, order):
    """48 x 30, 3 x 2 (tile 16 x 15: an odd tile height, so a row pair straddles two bands; three groups a row), every pitch larger than
    its row and the chroma planes 8 past a 16-byte boundary: yuv420_bgr_clahe_interp_frames_kernel with guards."""
    w, h, n = 48, 30, 2
    pool = Pool(w, h, n, FMTS[order], y_pitch=64, c_pitch=40, out_pitch=160, skew=lambda k: (0, 8, 8, 0))
    check(c, rand_frames(w, h, n, 140), pool, ("clahe", (2.0, 3, 2)), order, (1, 0, 2, 0))


# ---- 8. clahe_fp_contract --------------------------------------------------------------------------------------------------------
def test_fp_contract_takes_the_fallback(c):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    frames = rand_frames(w, h, n, 141)
    pool = Pool(w, h, n)
    c.set_option("clahe_fp_contract", 1)
    prev = oracle.set_fp_contract(True)
    try:
        check(c, frames, pool, ("clahe", (2.0, 4, 2)), ORDER_BGR, (0, 1, 2, 0), contract=True)
    finally:
        oracle.set_fp_contract(prev)
        c.set_option("clahe_fp_contract", 0)
    check(c, frames, pool, ("clahe", (2.0, 4, 2)), ORDER_BGR, (1, 0, 2, 0))


# ---- 9. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,one", [(EQ, 1), (CL22, 1), (("clahe", (2.0, 3, 2)), 0)], ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, op, one):
    """One frame more than two full launches: three chunks, the last of one frame.  The planes are carved at irregular (16-byte
    aligned) distances out of four large allocations (Y, data[1], data[2], images), which keeps the allocation count small; every frame
    is distinct and every frame is checked (the fallback reuses its scratch planes from chunk to chunk)."""
    w, h = 32, 16
    per = frames_per_launch()
    n = 2 * per + 1
    frames = rand_frames(w, h, n, 142)

    def gap(k):
        return 16 * ((k * 7) % 5)
    arenas = (Arena(n * (w * h + 96) + 64), Arena(n * (w * h // 4 + 96) + 64), Arena(n * (w * h // 4 + 96) + 64), Arena(n * (3 * w * h + 96) + 64))
    pool = Pool(w, h, n, "yv12", arenas=arenas, gap=gap)
    assert len({pool.us[k + 1].ptr - pool.us[k].ptr for k in range(n - 1)}) > 1, "the U planes are not at one stride"
    assert len({f.tobytes() for f in frames}) == n
    check(c, frames, pool, op, ORDER_RGB, (one, 1 - one, n, 0))


# ---- 10. identities --------------------------------------------------------------------------------------------------------------
def image_bytes(plane):
    """what the device holds in the rows of `plane`"""
    got = xfer.to_host(plane.arena.buf)
    return np.stack([got[plane.off + r * plane.pitch: plane.off + r * plane.pitch + plane.row_bytes] for r in range(plane.rows)])


@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))], ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_identity_with_the_batch_form(c, op):
    """The list call on separate allocations and mi_*_yuv420_to_bgr_batch_dev on the same pixels in one allocation: byte-equal."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 143)
    pool = Pool(w, h, n).load(frames)
    i420 = np.stack([np.concatenate([f[: w * h], f[w * h:][0::2], f[w * h:][1::2]]) for f in frames])
    d_in = xfer.to_device(i420)
    d_batch = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0")
    call(c, op, pool.entries(), w, h, ORDER_BGR, pool.pitches)
    src = Yuv420Planes.i420(d_in, w, h)
    if op is EQ:
        c.equalize_hist_yuv420_to_bgr_batch_dev(src, d_batch, w, h, n, ORDER_BGR, stream=stream())
    else:
        c.clahe_yuv420_to_bgr_batch_dev(src, d_batch, w, h, n, ORDER_BGR, *op[1], stream=stream())
    torch.cuda.synchronize()
    batch = xfer.to_host(d_batch)
    for k in range(n):
        assert np.array_equal(batch[k], expected(frames[k], w, h, op, ORDER_BGR)), ("batch form", op, k)
        pool.outs[k].put(batch[k])
    pool.verify(("list form against batch form", op))


@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_the_nv12_list_form(c, op):
    """The planar list call and mi_*_nv12_to_bgr_frames_dev on the same pixels with U and V interleaved: byte-equal images."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 144)
    pool = Pool(w, h, n, "yv12").load(frames)
    nv = Nv12Pool(w, h, n).load(frames)
    call(c, op, pool.entries(), w, h, ORDER_RGB, pool.pitches)
    nv12_call(c, op, nv.ys, nv.uvs, nv.outs, w, h, ORDER_RGB, nv.pitches)
    torch.cuda.synchronize()
    for k in range(n):
        pool.outs[k].put(image_bytes(nv.outs[k]))
    pool.verify(("planar list form against NV12 list form", op))


@pytest.mark.parametrize("op,want", [(EQ, (1, 0)), (("clahe", (2.0, 4, 2)), (1, 0)), (("clahe", (2.0, 3, 2)), (0, 1))],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_interleaved_list_is_the_nv12_list_form(c, op, want):
    """chroma = MI_CHROMA_INTERLEAVED: {y, c0, out} go to the NV12 list form -- c1 is ignored (None in one entry, junk in another) --
    with its bytes and its counters; none of the six planar counters moves."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 145)
    a, b = Nv12Pool(w, h, n, y_pitch=80, uv_pitch=96, out_pitch=208).load(frames), Nv12Pool(w, h, n, y_pitch=80, uv_pitch=96, out_pitch=208).load(frames)
    entries = [Yuv420BgrFrameDev(a.ys[k].ptr, a.uvs[k].ptr, (None, 1, a.outs[k].ptr)[k], a.outs[k].ptr) for k in range(n)]
    before = stats(c)
    call(c, op, entries, w, h, ORDER_BGR, dict(y_pitch=80, c_pitch=96, out_pitch=208), chroma=CHROMA_INTERLEAVED)
    torch.cuda.synchronize()
    assert delta(before, stats(c)) == (0, 0, 0, 0, 0, 0) + want
    nv12_call(c, op, b.ys, b.uvs, b.outs, w, h, ORDER_BGR, b.pitches)
    torch.cuda.synchronize()
    for k in range(n):
        a.outs[k].put(image_bytes(b.outs[k]))
        b.outs[k].put(expected(frames[k], w, h, op, ORDER_BGR))
    a.verify(("interleaved list against the NV12 list form", op))
    b.verify(("the NV12 list form", op))


# ---- 11. edges -------------------------------------------------------------------------------------------------------------------
def test_one_input_two_outputs(c):
    """The same {y, c0, c1} in two entries with different images: inputs are only read, both images are exact (hence equal)."""
    w, h = 32, 16
    frame = rand_frames(w, h, 1, 146)[0]
    pool = Pool(w, h, 2)
    for op in (EQ, CL22):
        pool.load([frame, frame])
        for k in range(2):
            pool.outs[k].put(expected(frame, w, h, op, ORDER_BGR))
        e = pool.entries()
        e[1] = Yuv420BgrFrameDev(e[0].y, e[0].c0, e[0].c1, e[1].out)
        before = stats(c)
        call(c, op, e, w, h, ORDER_BGR, pool.pitches)
        torch.cuda.synchronize()
        pool.verify(("one input, two outputs", op))
        assert delta(before, stats(c)) == (1, 0, 2, 0, 0, 0, 0, 0)


def test_constant_and_two_valued_planes(c):
    """A constant Y plane below 16: equalizeHist's shortcut and the decode's clamp of (Y - 16) at 0.  Two values."""
    w, h = 32, 16
    const, two = rand_frames(w, h, 2, 147)
    const[: w * h] = 9
    two[: w * h] = np.where(np.arange(w * h) % 3 == 0, 200, 3).astype(np.uint8)
    for order, fmt in zip(ORDERS, FMTS):
        pool = Pool(w, h, 2, fmt)
        for op in (EQ, CL22):
            check(c, [const, two], pool, op, order, (1, 0, 2, 0))


# ---- 12. hipGraph ----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_two_replays():
    """One eager call of the shape, then capture on a side stream and two replays, each onto fresh input bytes at the same addresses."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, y_pitch=80, c_pitch=40, out_pitch=208)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            one = int(op[1] != (2.0, 3, 2))
            check(c, rand_frames(w, h, n, 148), pool, op, ORDER_BGR, (one, 1 - one, 3, 0))   # sizes the scratch
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(c, op, pool.entries(), w, h, ORDER_BGR, pool.pitches, st=torch.cuda.current_stream().cuda_stream)
            for seed in (149, 150):
                fresh = rand_frames(w, h, n, seed)
                pool.load(fresh)
                for k, f in enumerate(fresh):
                    pool.outs[k].put(expected(f, w, h, op, ORDER_BGR))
                g.replay()
                torch.cuda.synchronize()
                pool.verify(("graph replay", op, seed))


# ---- 13. refusals, zero sizes, launch accounting ---------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 151)
    pool = Pool(w, h, n, y_pitch=48, c_pitch=24, out_pitch=112).load(frames)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(e.y, e.c0, e.c1, e.out) for e in pool.entries()]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, yp=48, cp=24, chroma=CHROMA_PLANAR, op=112, order=ORDER_BGR)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (Yuv420BgrFrameDev * max(1, len(a["entries"])))(*[Yuv420BgrFrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["yp"], a["cp"], a["chroma"], a["op"], a["order"])

        def eq(**kw):
            return L.mi_equalize_hist_yuv420_to_bgr_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_yuv420_to_bgr_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(**over):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = dict(zip(("y", "c0", "c1", "out"), good[-1]))
            e.update({k: (None if v == "null" else v) for k, v in over.items()})
            return dict(entries=good[:-1] + [(e["y"], e["c0"], e["c1"], e["out"])])
        y2, u2, v2, _ = good[-1]
        img = (h - 1) * 112 + 3 * w                                                           # the bytes an image spans
        INTER = dict(chroma=CHROMA_INTERLEAVED, cp=48)                                        # a valid interleaved shape on the same addresses
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(y="null"), last(c0="null"), last(c1="null"), last(out="null"),           # a null plane address in the last entry
               dict(entries=[(None,) + good[0][1:]] + good[1:]),                             # ... and in the first
               dict(chroma=2), dict(chroma=-1),                                              # a chroma other than the two
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(yp=w - 1), dict(cp=w // 2 - 1), dict(op=3 * w - 1),                      # a pitch below its row
               dict(chroma=CHROMA_INTERLEAVED, cp=w - 1),                                    # ... W for an interleaved chroma plane
               dict(order=2), dict(order=-1),                                                # an order other than the two
               # no in-place form, compared as address ranges: the image of the last frame on its own Y, U and V plane, ending one
               # byte inside its V plane, and starting on the last byte of its Y plane's last row
               last(out=y2), last(out=u2), last(out=v2), last(out=v2 - img + 1), last(out=y2 + (h - 1) * 48 + w - 1),
               # the interleaved route has the NV12 list form's checks
               dict(INTER, lst=NULL_LIST), dict(INTER, **last(y="null")), dict(INTER, **last(c0="null")), dict(INTER, **last(out="null")),
               dict(INTER, w=31), dict(INTER, order=2), dict(INTER, **last(out=u2))]
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
        batch = L.mi_equalize_hist_yuv420_to_bgr_batch_dev(hd, planes, o0, 1 << 27, 1 << 28, big["w"], 2, 1, 0, stream())
        assert batch == UNSUPPORTED and eq(**big) == batch and cl(**big) == batch
        planes = Yuv420Planes(y0, 48, u0, v0, 24, 0, CHROMA_PLANAR)
        batch = L.mi_clahe_yuv420_to_bgr_batch_dev(hd, planes, o0, 112, 0, w, h, 1, 0, 2.0, 2048, 1024, stream())
        assert batch == UNSUPPORTED and cl(2048, 1024) == batch
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0,) * 8
        # launch accounting of the three sequences, by role: the batch form's slots; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (1, 0, 3, 0)),
                             (CL22, {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (1, 0, 3, 0)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (0, 1, 3, 0))):
            c.profile_read(reset=True)
            check(c, frames, pool, op, ORDER_RGB, st)
            got = launches(c)
            assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 14. pipe pending ------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(rand_frames(w, h, 1, 152))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, CL22):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, pool.entries(), w, h, ORDER_BGR, pool.pitches)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")
        assert stats(c) == (0,) * 8


# ---- 15. seeded sweep ------------------------------------------------------------------------------------------------------------
def test_seeded_sweep(c):
    """The 32 cases of tests/yuv420_bgr_frames_cases.py (tests/test_yuv420_to_bgr_frames_abi.py asserts their class counts on the CPU):
    exact bytes, whole allocations, and the eight counter deltas the documented rule gives.  No case is skipped."""
    K = max_pairs_lds_f32()
    sweep = cases.sweep_cases()
    assert len(sweep) == 32 and min(cases.class_counts(sweep, K).values()) >= 6
    c.set_option("clahe_fp_contract", 0)
    ran = 0
    for i, k in enumerate(sweep):
        w, h, n, order, sk = k["w"], k["h"], k["n"], k["order"], k["skews"]
        op = EQ if k["kind"] == "eq" else ("clahe", (k["clip"], k["tx"], k["ty"]))
        frames = rand_frames(w, h, n, 500 + i)
        want = cases.classify(k, K)[1]
        pitches = dict(y_pitch=k["y_pitch"], c_pitch=k["c_pitch"], out_pitch=k["out_pitch"])
        if k["fmt"] == "nv12":
            pool = Nv12Pool(w, h, n, y_pitch=k["y_pitch"], uv_pitch=k["c_pitch"], out_pitch=k["out_pitch"],
                            skew=lambda f: (sk[f][0], sk[f][1], sk[f][3])).load(frames)
            entries = [Yuv420BgrFrameDev(pool.ys[f].ptr, pool.uvs[f].ptr, None, pool.outs[f].ptr) for f in range(n)]
            chroma = CHROMA_INTERLEAVED
        else:
            pool = Pool(w, h, n, k["fmt"], skew=lambda f: sk[f], **pitches).load(frames)
            entries, chroma = pool.entries(), CHROMA_PLANAR
        for f in range(n):
            e = entries[f]
            got, drawn = [e.y % 16, e.c0 % 16, (e.c1 or 0) % 16, e.out % 16], [s % 16 for s in sk[f]]
            if chroma == CHROMA_INTERLEAVED:
                got[2] = drawn[2] = 0                 # c1 is ignored
            assert got == drawn, (i, f)
            pool.outs[f].put(expected(frames[f], w, h, op, order))
        before = stats(c)
        call(c, op, entries, w, h, order, pitches, chroma=chroma)
        torch.cuda.synchronize()
        pool.verify((i, k))
        assert delta(before, stats(c)) == want, (i, k, want, delta(before, stats(c)))
        ran += 1
    assert ran == 32
