"""NV12 in, interleaved BGR / RGB out on a LIST of pitched device frames on the GPU: mi_equalize_hist_nv12_to_bgr_frames_dev and
mi_clahe_nv12_to_bgr_frames_dev.  Expected bytes are oracle.nv12_to_bgr(oracle.nv12_frame(frame, W, H, 1, op...), W, H), the last axis
reversed for MI_ORDER_RGB.  Y, U and V are full-range random bytes, as tests/test_gpu_nv12_to_bgr.py computes them.  Every Y plane, UV
plane and image is its own sentinel-filled torch allocation unless a test says otherwise, and every allocation is compared WHOLE, inputs
included: pitch padding and allocation tails keep their sentinel.  Every comparison in this file is exact."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, Nv12BgrFrameDev

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


@functools.lru_cache(maxsize=None)
def _expected(frame_bytes, w, h, op, order, contract):
    kind, cfg = op
    frame = np.frombuffer(frame_bytes, np.uint8)
    nv12 = oracle.nv12_frame(frame, w, h, 1, 0) if kind == "eq" else oracle.nv12_frame(frame, w, h, 1, 1, *cfg)
    bgr = oracle.nv12_to_bgr(nv12, w, h)
    out = bgr if order == ORDER_BGR else np.ascontiguousarray(bgr[:, :, ::-1])
    out.setflags(write=False)
    return out


def expected(frame, w, h, op, order, contract=False):
    """Computed once per (frame, op, order, oracle flavour) and shared, read-only, by the tests that need it."""
    return _expected(frame.tobytes(), w, h, op, order, contract)


class Arena:
    """One sentinel-filled torch allocation and the host image of what it must hold."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.img = np.full(nbytes, SENT, np.uint8)
        self.top = 0

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


class Plane:
    """`rows` rows of `row_bytes` bytes at `pitch`: an allocation of its own (with a tail behind the last row), or a piece of `arena`."""

    def __init__(self, rows, row_bytes, pitch=None, skew=0, arena=None, gap=0, tail=48):
        self.rows, self.row_bytes, self.pitch = rows, row_bytes, pitch or row_bytes
        span = (rows - 1) * self.pitch + row_bytes
        self.arena = arena or Arena(skew + span + tail)
        self.off = self.arena.carve(span, skew, gap)

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
    """n frames of one shape: a decoder's surface pool (ys, uvs) and an image pool (outs).  skew(k) -> the three addresses' offsets
    past a 16-byte boundary for frame k; arenas: (Y, UV, out) allocations to carve the planes from instead of one allocation each."""

    def __init__(self, w, h, n, y_pitch=None, uv_pitch=None, out_pitch=None, skew=lambda k: (0, 0, 0), arenas=None, gap=lambda k: 0):
        self.w, self.h, self.n = w, h, n
        ay, au, ao = arenas or (None, None, None)
        self.ys = [Plane(h, w, y_pitch, skew(k)[0], ay, gap(k)) for k in range(n)]
        self.uvs = [Plane(h // 2, w, uv_pitch, skew(k)[1], au, gap(k)) for k in range(n)]
        self.outs = [Plane(h, 3 * w, out_pitch, skew(k)[2], ao, gap(k)) for k in range(n)]
        self.pitches = dict(y_pitch=self.ys[0].pitch, uv_pitch=self.uvs[0].pitch, out_pitch=self.outs[0].pitch)

    def in_arenas(self):
        return list({id(p.arena): p.arena for p in self.ys + self.uvs}.values())

    def out_arenas(self):
        return list({id(p.arena): p.arena for p in self.outs}.values())

    def load(self, frames):
        """Upload `frames` (tight NV12) into the input planes; every image back to the sentinel."""
        w, h = self.w, self.h
        for k, f in enumerate(frames):
            self.ys[k].put(f[: w * h])
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


def call(c, op, ys, uvs, outs, w, h, order, pitches, st=None):
    """The list form through the binding, on raw device addresses."""
    kind, cfg = op
    a = ([p.ptr for p in ys], [p.ptr for p in uvs], [p.ptr for p in outs], w, h, order)
    kw = dict(pitches, stream=stream() if st is None else st)
    if kind == "eq":
        c.equalize_hist_nv12_to_bgr_frames(*a, **kw)
    else:
        c.clahe_nv12_to_bgr_frames(*a, *cfg, **kw)


def stats(c):
    return c.get_stat("nv12_bgr_onepass"), c.get_stat("nv12_bgr_twopass")


def check(c, frames, pool, op, order, want_stats, perm=None, contract=False):
    """One call on uploaded `frames`: exact images, untouched guards and inputs, and the (onepass, twopass) counters moved by
    want_stats.  perm: the order in which the frames appear in the list."""
    w, h = pool.w, pool.h
    pool.load(frames)
    for k, f in enumerate(frames):
        pool.outs[k].put(expected(f, w, h, op, order, contract))
    idx = list(range(pool.n)) if perm is None else list(perm)
    before = stats(c)
    call(c, op, [pool.ys[k] for k in idx], [pool.uvs[k] for k in idx], [pool.outs[k] for k in idx], w, h, order, pool.pitches)
    torch.cuda.synchronize()
    pool.verify((w, h, op, order))
    after = stats(c)
    assert (after[0] - before[0], after[1] - before[1]) == want_stats, (op, before, after)


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
def test_fast_path(c, order):
    """32 x 16, three frames, tight, every allocation 16-byte aligned: 16 x 2 groups; CLAHE 2 x 2 (tiles of 16 x 8) in one pass."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 31)
    pool = Pool(w, h, n)
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        check(c, frames, pool, op, order, (1, 0))


# ---- 2. pitched with guards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_pitched_with_guards(c, order):
    """64 x 32, every pitch a multiple of 16 and larger than its row; the list is a permutation of the pool, so its addresses are not
    monotonic.  Pitch padding and allocation tails keep their sentinel, in the images and in the planes."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 32)
    pool = Pool(w, h, n, y_pitch=80, uv_pitch=96, out_pitch=208)
    check(c, frames, pool, ("clahe", (2.0, 4, 2)), order, (1, 0), perm=(2, 0, 1))
    check(c, frames, pool, EQ, order, (1, 0), perm=(1, 2, 0))


# ---- 3. per-frame alignment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2], ids=["y", "uv", "out"])
def test_per_frame_alignment(c, which):
    """32 x 16 at pitches 48 / 48 / 112: the shape allows 16-byte accesses.  The middle frame of three has ONE address one byte past a
    16-byte boundary: it alone runs the byte path inside the same launch.  equalizeHist stays one pass; CLAHE 2 x 2, whose blend +
    decode kernel has no byte path, takes the fallback for the whole call."""
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 33)
    pool = Pool(w, h, n, y_pitch=48, uv_pitch=48, out_pitch=112,
                skew=lambda k: tuple(int(k == 1 and i == which) for i in range(3)))
    assert [p.ptr % 16 for p in (pool.ys[1], pool.uvs[1], pool.outs[1])] == [int(i == which) for i in range(3)]
    for order in ORDERS:
        check(c, frames, pool, EQ, order, (1, 0))
        check(c, frames, pool, ("clahe", (2.0, 2, 2)), order, (0, 1))


# ---- 4. general and fallback -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_general_and_fallback(c, order):
    """34 x 18 (W % 16 == 2, no tile grid divides it), odd pitches, addresses at odd offsets: 2 x 2 blocks with byte accesses; CLAHE
    3 x 2 pads by REFLECT_101 and takes the planar CLAHE + decode fallback."""
    w, h, n = 34, 18, 2
    frames = rand_frames(w, h, n, 34)
    pool = Pool(w, h, n, y_pitch=35, uv_pitch=37, out_pitch=103, skew=lambda k: (1 + 2 * k, 3, 5 + 6 * k))
    check(c, frames, pool, EQ, order, (1, 0))
    check(c, frames, pool, ("clahe", (2.0, 3, 2)), order, (0, 1))


# ---- 5. clahe_fp_contract --------------------------------------------------------------------------------------------------------
def test_fp_contract_takes_the_fallback(c):
    """64 x 32 CLAHE 4 x 2 is the one-pass shape; with clahe_fp_contract on it runs the planar kernels' contracted arithmetic."""
    w, h, n = 64, 32, 2
    frames = rand_frames(w, h, n, 35)
    pool = Pool(w, h, n)
    c.set_option("clahe_fp_contract", 1)
    prev = oracle.set_fp_contract(True)
    try:
        check(c, frames, pool, ("clahe", (2.0, 4, 2)), ORDER_BGR, (0, 1), contract=True)
    finally:
        oracle.set_fp_contract(prev)
        c.set_option("clahe_fp_contract", 0)


# ---- 6. chunking -----------------------------------------------------------------------------------------------------------------
def frames_per_launch():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "common.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kFramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1))


@pytest.mark.parametrize("op,want", [(EQ, (1, 0)), (("clahe", (2.0, 2, 2)), (1, 0)), (("clahe", (2.0, 3, 2)), (0, 1))],
                         ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_chunking(c, op, want):
    """One frame more than two full launches: three chunks, the last of one frame.  The planes are carved at irregular (16-byte
    aligned) distances out of three large allocations, which keeps the allocation count small; every frame is distinct and every frame
    is checked (the fallback reuses its scratch planes from chunk to chunk)."""
    w, h = 32, 16
    n = 2 * frames_per_launch() + 1
    frames = rand_frames(w, h, n, 36)

    def gap(k):
        return 16 * ((k * 7) % 5)
    arenas = (Arena(n * (w * h + 96) + 64), Arena(n * (w * h // 2 + 96) + 64), Arena(n * (3 * w * h + 96) + 64))
    pool = Pool(w, h, n, arenas=arenas, gap=gap)
    assert len({pool.ys[k + 1].ptr - pool.ys[k].ptr for k in range(n - 1)}) > 1, "the Y planes are not at one stride"
    check(c, frames, pool, op, ORDER_RGB, want)


# ---- 7. identity with the batch form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_identity_with_the_batch_form(c, op):
    """The list call on separate allocations and the batch call on the same pixels in one allocation: byte-equal images."""
    w, h, n = 64, 32, 3
    frames = rand_frames(w, h, n, 37)
    pool = Pool(w, h, n).load(frames)
    d_in = xfer.to_device(np.stack(frames))
    d_batch = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0")
    call(c, op, pool.ys, pool.uvs, pool.outs, w, h, ORDER_BGR, pool.pitches)
    if op is EQ:
        c.equalize_hist_nv12_to_bgr_batch_dev(d_in, None, d_batch, w, h, n, ORDER_BGR, stream=stream())
    else:
        c.clahe_nv12_to_bgr_batch_dev(d_in, None, d_batch, w, h, n, ORDER_BGR, *op[1], stream=stream())
    torch.cuda.synchronize()
    batch = xfer.to_host(d_batch)
    for k in range(n):
        assert np.array_equal(batch[k], expected(frames[k], w, h, op, ORDER_BGR)), ("batch form", op, k)
        pool.outs[k].put(batch[k])
    pool.verify(("list form against batch form", op))


# ---- 8. one input, two outputs ---------------------------------------------------------------------------------------------------
def test_one_input_two_outputs(c):
    """The same {y, uv} in two entries with different images: inputs are only read, both images are exact (hence equal)."""
    w, h = 32, 16
    frame = rand_frames(w, h, 1, 38)[0]
    pool = Pool(w, h, 2)
    for op in (EQ, ("clahe", (2.0, 2, 2))):
        pool.load([frame, frame])
        for k in range(2):
            pool.outs[k].put(expected(frame, w, h, op, ORDER_BGR))
        call(c, op, [pool.ys[0]] * 2, [pool.uvs[0]] * 2, pool.outs, w, h, ORDER_BGR, pool.pitches)
        torch.cuda.synchronize()
        pool.verify(("one input, two outputs", op))


# ---- 9. edges --------------------------------------------------------------------------------------------------------------------
def test_edges(c):
    """2 x 2: one block, one chroma pair (CLAHE 1 x 1 takes the fallback).  A constant Y plane below 16: equalizeHist's shortcut and
    the decode's clamp of (Y - 16) at 0.  Two values."""
    f22 = rand_frames(2, 2, 2, 39)
    pool = Pool(2, 2, 2)
    check(c, f22, pool, EQ, ORDER_BGR, (1, 0))
    check(c, f22, pool, ("clahe", (2.0, 1, 1)), ORDER_BGR, (0, 1))
    w, h = 32, 16
    const, two = rand_frames(w, h, 2, 40)
    const[: w * h] = 9
    two[: w * h] = np.where(np.arange(w * h) % 3 == 0, 200, 3).astype(np.uint8)
    pool = Pool(w, h, 2)
    for order in ORDERS:
        for op in (EQ, ("clahe", (2.0, 2, 2))):
            check(c, [const, two], pool, op, order, (1, 0))


# ---- 10. hipGraph ----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then capture on a side stream and a replay onto fresh input bytes at the same addresses."""
    w, h, n = 64, 32, 3
    pool = Pool(w, h, n, y_pitch=80, uv_pitch=96, out_pitch=208)
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 4, 2)), ("clahe", (2.0, 3, 2))):
            check(c, rand_frames(w, h, n, 41), pool, op, ORDER_BGR, (0, 1) if op[1] == (2.0, 3, 2) else (1, 0))   # sizes the scratch
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call(c, op, pool.ys, pool.uvs, pool.outs, w, h, ORDER_BGR, pool.pitches, st=torch.cuda.current_stream().cuda_stream)
            fresh = rand_frames(w, h, n, 42)
            pool.load(fresh)
            for k, f in enumerate(fresh):
                pool.outs[k].put(expected(f, w, h, op, ORDER_BGR))
            g.replay()
            torch.cuda.synchronize()
            pool.verify(("graph replay", op))


# ---- 11. errors, zero sizes, launch accounting -----------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 3
    frames = rand_frames(w, h, n, 43)
    pool = Pool(w, h, n, y_pitch=48, uv_pitch=48, out_pitch=112).load(frames)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        good = [(pool.ys[k].ptr, pool.uvs[k].ptr, pool.outs[k].ptr) for k in range(n)]
        base = dict(ctx=hd, entries=good, n=n, w=w, h=h, yp=48, up=48, op=112, order=ORDER_BGR)
        NULL_LIST = object()

        def args(kw):
            a = dict(base)
            a.update(kw)
            arr = (Nv12BgrFrameDev * max(1, len(a["entries"])))(*[Nv12BgrFrameDev(*e) for e in a["entries"]])
            lst = None if a.get("lst") is NULL_LIST else arr
            return (a["ctx"], lst, a["n"], a["w"], a["h"], a["yp"], a["up"], a["op"], a["order"])

        def eq(**kw):
            return L.mi_equalize_hist_nv12_to_bgr_frames_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_nv12_to_bgr_frames_dev(*args(kw), 2.0, tx, ty, stream())

        def last(y=None, uv=None, out=None):
            """The list with its LAST entry replaced: the first two frames are good."""
            e = list(good[-1])
            for i, v in enumerate((y, uv, out)):
                if v is not None:
                    e[i] = None if v == "null" else v
            return dict(entries=good[:-1] + [tuple(e)])
        y2, uv2 = pool.ys[2].ptr, pool.uvs[2].ptr
        bad = [dict(ctx=None), dict(lst=NULL_LIST), dict(lst=NULL_LIST, n=1),                # a null ctx, a null list with n_frames > 0
               last(y="null"), last(uv="null"), last(out="null"),                            # a null plane address in the last entry
               dict(entries=[(None, good[0][1], good[0][2])] + good[1:]),                    # ... and in the first
               dict(w=-2), dict(h=-2), dict(n=-1),                                           # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),    # odd sizes, also when another size is 0
               dict(yp=w - 1), dict(up=w - 1), dict(op=3 * w - 1),                           # a pitch below its row
               dict(order=2), dict(order=-1),                                                # an order other than the two
               # no in-place form, compared as address ranges: the image of the last frame on its own Y plane, on its own UV plane,
               # ending one byte inside its UV plane, and starting on the last byte of its Y plane's last row
               last(out=y2), last(out=uv2), last(out=uv2 - ((h - 1) * 112 + 3 * w) + 1), last(out=y2 + (h - 1) * 48 + w - 1)]
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written -- a null list is fine when there are no frames
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, lst=NULL_LIST)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the batch form refuses: its status
        big = dict(w=(1 << 24) + 2, h=2, yp=1 << 25, up=1 << 25, op=1 << 27)
        y0, uv0, o0 = good[0]
        batch = L.mi_equalize_hist_nv12_to_bgr_batch_dev(hd, y0, 1 << 25, uv0, 1 << 25, 1 << 27, o0, 1 << 27, 1 << 28, big["w"], 2, 1, 0, stream())
        assert batch == UNSUPPORTED and eq(**big) == batch and cl(**big) == batch
        batch = L.mi_clahe_nv12_to_bgr_batch_dev(hd, y0, 48, uv0, 48, 0, o0, 112, 0, w, h, 1, 0, 2.0, 2048, 1024, stream())
        assert batch == UNSUPPORTED and cl(2048, 1024) == batch
        torch.cuda.synchronize()
        pool.verify("a refused or empty call wrote")
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert stats(c) == (0, 0)
        # launch accounting of the three sequences, by role: the batch form's slots; and the context still works
        for op, want, st in ((EQ, {"hist_partial_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}, (1, 0)),
                             (("clahe", (2.0, 2, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1}, (1, 0)),
                             (("clahe", (2.0, 3, 2)), {"tile_hist_kernel": 1, "clahe_interp_kernel": 1, "color_kernel": 1}, (0, 1))):
            c.profile_read(reset=True)
            check(c, frames, pool, op, ORDER_RGB, st)
            got = launches(c)
            assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (op, got)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 12. pipe pending ------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 1).load(rand_frames(w, h, 1, 44))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    call(c, op, pool.ys, pool.uvs, pool.outs, w, h, ORDER_BGR, pool.pitches)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        pool.verify("a refused call wrote")
