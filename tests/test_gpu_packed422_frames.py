"""Lists of pitched packed 4:2:2 frames (mi_equalize_hist_packed422_frames_dev, mi_clahe_packed422_frames_dev) on the GPU.  Every
frame lives in its own allocation filled with a sentinel byte -- rows of 2W bytes at a padded pitch, the frame `off` bytes into the
allocation, so that each frame has its own alignment modulo 16 -- and the WHOLE allocation is compared: pitch padding and guard bytes
are checked, and inputs are shown unwritten.  Expected frames are built on the CPU as "gather the luma -> oracle.equalize_hist /
oracle.clahe -> scatter it back, chroma copied or 128".  Every comparison in this file is exact bytes."""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import capi, synth, UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
DISTS = ["D1", "D2", "D3", "D4", "D5"]
CLAHE_CONFIGS = [(2.0, 8, 8), (0.0, 3, 5), (2.0, 64, 2)]       # 8x8; reflection on both axes at 62x47; the wide-grid kernel
OPS = [("eq", None)] + [("clahe", cfg) for cfg in CLAHE_CONFIGS]
IN_OFFS = [0, 4, 8, 12, 20]
OUT_OFFS = IN_OFFS[1:] + IN_OFFS[:1]                              # source and destination of a frame differ modulo 16
EXTRAS = [0, 4, 36]
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]


def stream():
    return torch.cuda.current_stream().cuda_stream


def align(x, a):
    return (x + a - 1) // a * a


def luma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, fmt - 2:2 * w:2])


_ref_cache = {}


def y_ref(y, op, cfg, key=None):
    """The oracle's plane; `key` names the content so that one plane is computed once per op (default arithmetic mode only)."""
    k = None if key is None else (key, op, cfg)
    if k in _ref_cache:
        return _ref_cache[k]
    r = oracle.equalize_hist(y) if op == "eq" else oracle.clahe(y, *cfg)
    if k is not None:
        _ref_cache[k] = r
    return r


def expected_frame(frame, w, fmt, op, cfg, uv_mode, key=None):
    off = fmt - 2
    out = frame[:, :2 * w].copy() if uv_mode == UV_COPY else np.full((frame.shape[0], 2 * w), 128, np.uint8)
    out[:, off::2] = y_ref(luma(frame, w, fmt), op, cfg, key)
    return out


class Frame:
    """One packed frame in its own sentinel-filled allocation: rows of 2W bytes at `pitch` = 2W + extra, the frame `off` bytes in,
    `slack` spare rows and 64 guard bytes behind it."""

    def __init__(self, w, h, extra=0, off=0, pitch=None, slack=0):
        self.w, self.h, self.off = w, h, off
        self.pitch = 2 * w + extra if pitch is None else pitch
        self.total = off + self.pitch * (h + slack) + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, frame=None):
        """The allocation as it must read with `frame` in it (None: untouched)."""
        a = np.full(self.total, SENT, np.uint8)
        if frame is not None:
            np.lib.stride_tricks.as_strided(a[self.off:], (self.h, 2 * self.w), (self.pitch, 1))[:] = frame[:, : 2 * self.w]
        return a

    def upload(self, frame):
        self.buf.copy_(torch.from_numpy(self.image(frame)))
        return self

    def clear(self):
        self.buf.fill_(SENT)

    def host(self):
        return self.buf.cpu().numpy()


def run(c, op, cfg, srcs, dsts, w, h, fmt, uv_mode, st=None):
    """The list form on Frame lists (dsts None: in place); the pitches are the first frames'."""
    kw = dict(in_pitch=srcs[0].pitch, out_pitch=(srcs if dsts is None else dsts)[0].pitch, stream=stream() if st is None else st)
    ins, outs = [f.ptr for f in srcs], None if dsts is None else [f.ptr for f in dsts]
    if op == "eq":
        c.equalize_hist_packed422_frames(ins, outs, w, h, fmt, uv_mode, **kw)
    else:
        c.clahe_packed422_frames(ins, outs, w, h, fmt, uv_mode, *cfg, **kw)


def planar_status(c, w, h, n, op, cfg):
    """What the planar form answers for this size / grid pair (0 = accepted)."""
    a = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    try:
        if op == "eq":
            c.equalize_hist_batch_dev(a, b, w, h, n, stream=stream())
        else:
            c.clahe_batch_dev(a, b, w, h, n, *cfg, stream=stream())
    except mi_lumaeq.MiError as e:
        return e.status
    finally:
        torch.cuda.synchronize()
    return 0


def assert_frames(got_frames, want_images, why):
    for k, (f, want) in enumerate(zip(got_frames, want_images)):
        got = f.host()
        assert np.array_equal(got, want), (why, k, int((got != want).sum()), np.flatnonzero(got != want)[:8])


def make_frames(w, h, fmt, dists, first):
    return [synth.packed422_frame(w, h, fmt, d, first + k) for k, d in enumerate(dists)]


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


# ---- 1. small full matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (62, 47), (2, 1), (4098, 3)])
def test_small_sizes_full_matrix(c, w, h):
    """Every format x uv_mode x op x pitch padding on five frames (D1-D5), each in its own allocation at its own offset, input and
    output of a frame at different alignments modulo 16.  (0.0, 3, 5) on 62 x 47 pads by reflection on both axes, (2.0, 64, 2) takes
    the wide-grid kernel, 2 x 1 and 4098 x 3 have tiles narrower than a macropixel / rows of one ragged slot.  A size / grid pair the
    planar form refuses gets the same status and writes nothing."""
    n = len(DISTS)
    status = {(op, cfg): planar_status(c, w, h, n, op, cfg) for op, cfg in OPS}
    for fmt in FMTS:
        frames = make_frames(w, h, fmt, DISTS, 100)
        for extra in EXTRAS:
            srcs = [Frame(w, h, extra, IN_OFFS[k]).upload(frames[k]) for k in range(n)]
            src_images = [s.image(f) for s, f in zip(srcs, frames)]
            dsts = [Frame(w, h, extra, OUT_OFFS[k]) for k in range(n)]
            assert all((s.ptr - d.ptr) % 16 != 0 for s, d in zip(srcs, dsts))
            for uv_mode in UVS:
                for op, cfg in OPS:
                    why = (w, h, fmt, extra, uv_mode, op, cfg)
                    for d in dsts:
                        d.clear()
                    if status[(op, cfg)] != 0:
                        with pytest.raises(mi_lumaeq.MiError) as e:
                            run(c, op, cfg, srcs, dsts, w, h, fmt, uv_mode)
                        torch.cuda.synchronize()
                        assert e.value.status == status[(op, cfg)], (why, e.value.status)
                        assert_frames(dsts, [d.image() for d in dsts], ("a refused call wrote", why))
                        continue
                    run(c, op, cfg, srcs, dsts, w, h, fmt, uv_mode)
                    torch.cuda.synchronize()
                    want = [d.image(expected_frame(f, w, fmt, op, cfg, uv_mode, ("small", w, h, k, fmt)))
                            for k, (d, f) in enumerate(zip(dsts, frames))]
                    assert_frames(dsts, want, why)
                    assert_frames(srcs, src_images, ("an input allocation was written", why))


# ---- 2. identity with the batch form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 64, 65, 128, 129, 258])
def test_identity_with_batch_form(c, n):
    """Lists laid over one tight batch, out of place and in place, against mi_*_packed422_batch_dev on the same bytes: both ops, both
    CLAHE arithmetic modes, across the boundary of a chunk whichever table size the library was built with."""
    w, h = 64, 36
    g = torch.Generator(device="cuda:0")
    g.manual_seed(4220 + n)
    x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
    x[: n // 2 + 1] = (x[: n // 2 + 1] // 3) + 40                                  # half of the frames low-contrast
    try:
        for fmt in FMTS:
            for contract in (0, 1):
                c.set_option("clahe_fp_contract", contract)
                for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
                    why = (n, fmt, contract, op)
                    want = torch.full_like(x, SENT)
                    got = torch.full_like(x, SENT)
                    want_ip, got_ip = x.clone(), x.clone()
                    if op == "eq":
                        c.equalize_hist_packed422_batch_dev(x, want, w, h, n, fmt, UV_COPY, stream=stream())
                        c.equalize_hist_packed422_batch_dev(want_ip, want_ip, w, h, n, fmt, UV_FILL128, stream=stream())
                        c.equalize_hist_packed422_frames(list(x), list(got), w, h, fmt, UV_COPY, stream=stream())
                        c.equalize_hist_packed422_frames(list(got_ip), None, w, h, fmt, UV_FILL128, stream=stream())
                    else:
                        c.clahe_packed422_batch_dev(x, want, w, h, n, fmt, UV_COPY, *cfg, stream=stream())
                        c.clahe_packed422_batch_dev(want_ip, want_ip, w, h, n, fmt, UV_FILL128, *cfg, stream=stream())
                        c.clahe_packed422_frames(list(x), list(got), w, h, fmt, UV_COPY, *cfg, stream=stream())
                        c.clahe_packed422_frames(list(got_ip), None, w, h, fmt, UV_FILL128, *cfg, stream=stream())
                    torch.cuda.synchronize()
                    assert torch.equal(got, want), ("out of place", why)
                    assert torch.equal(got_ip, want_ip), ("in place", why)
                    assert not torch.equal(want, torch.full_like(x, SENT)) and not torch.equal(want_ip, x), "the batch form did nothing"
    finally:
        c.set_option("clahe_fp_contract", 0)


# ---- 3. order and aliasing -------------------------------------------------------------------------------------------------------
def test_order_and_aliasing(c):
    w, h, extra = 62, 47, 4
    for fmt, uv_mode in ((FMT_YUY2, UV_COPY), (FMT_UYVY, UV_FILL128)):
        frames = make_frames(w, h, fmt, DISTS, 300)
        for op, cfg in (("eq", None), ("clahe", (0.0, 3, 5))):
            def exp(k):
                return expected_frame(frames[k], w, fmt, op, cfg, uv_mode, ("order", k, fmt))

            # a list whose entries name allocations in shuffled, non-monotonic address order
            pool = sorted((Frame(w, h, extra, IN_OFFS[k % 5]) for k in range(10)), key=lambda f: f.ptr)
            perm = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]
            srcs = [pool[perm[k]].upload(frames[k]) for k in range(5)]
            dsts = [pool[perm[5 + k]] for k in range(5)]
            for ptrs in ([f.ptr for f in srcs], [f.ptr for f in dsts]):
                assert ptrs != sorted(ptrs) and ptrs != sorted(ptrs, reverse=True)
            run(c, op, cfg, srcs, dsts, w, h, fmt, uv_mode)
            torch.cuda.synchronize()
            assert_frames(dsts, [d.image(exp(k)) for k, d in enumerate(dsts)], ("shuffled", fmt, op))
            assert_frames(srcs, [s.image(frames[k]) for k, s in enumerate(srcs)], ("shuffled: input written", fmt, op))

            # one input in two entries, with two outputs
            src = Frame(w, h, extra, 8).upload(frames[1])
            other = Frame(w, h, extra, 4).upload(frames[2])
            outs = [Frame(w, h, extra, 12), Frame(w, h, extra, 0), Frame(w, h, extra, 20)]
            run(c, op, cfg, [src, other, src], outs, w, h, fmt, uv_mode)
            torch.cuda.synchronize()
            assert_frames(outs, [outs[0].image(exp(1)), outs[1].image(exp(2)), outs[2].image(exp(1))], ("aliased input", fmt, op))
            assert_frames([src, other], [src.image(frames[1]), other.image(frames[2])], ("aliased input written", fmt, op))

            # a mixed list: even entries in place, odd entries out of place, equal pitches
            srcs = [Frame(w, h, extra, IN_OFFS[k]).upload(frames[k]) for k in range(5)]
            dsts = [srcs[k] if k % 2 == 0 else Frame(w, h, extra, OUT_OFFS[k]) for k in range(5)]
            run(c, op, cfg, srcs, dsts, w, h, fmt, uv_mode)
            torch.cuda.synchronize()
            assert_frames(dsts, [d.image(exp(k)) for k, d in enumerate(dsts)], ("mixed", fmt, op))
            assert_frames(srcs[1::2], [srcs[k].image(frames[k]) for k in (1, 3)], ("mixed: input of an out-of-place frame written", fmt, op))


# ---- 4. 1080p --------------------------------------------------------------------------------------------------------------------
def test_1080p(c):
    w, h, n = 1920, 1080, 3
    pitch = align(2 * w, 256)
    for fmt, uv_mode in ((FMT_YUY2, UV_COPY), (FMT_UYVY, UV_FILL128)):
        frames = make_frames(w, h, fmt, DISTS[1:1 + n], 400)
        srcs = [Frame(w, h, off=IN_OFFS[k], pitch=pitch).upload(frames[k]) for k in range(n)]
        dsts = [Frame(w, h, off=OUT_OFFS[k], pitch=pitch) for k in range(n)]
        for op, cfg in (("clahe", (2.0, 8, 8)), ("eq", None)):
            for d in dsts:
                d.clear()
            run(c, op, cfg, srcs, dsts, w, h, fmt, uv_mode)
            torch.cuda.synchronize()
            assert_frames(dsts, [d.image(expected_frame(f, w, fmt, op, cfg, uv_mode)) for d, f in zip(dsts, frames)], (fmt, op))
        assert_frames(srcs, [s.image(f) for s, f in zip(srcs, frames)], "an input allocation was written")


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    """Every MI_ERR_BAD_ARG row of the contract, the offending frame last in a three-frame list; the zero-size calls answer MI_OK.
    Nothing is written by any of them."""
    w, h, n, extra = 64, 48, 3, 4
    frames = make_frames(w, h, FMT_YUY2, DISTS[:n], 500)
    # 8 spare rows: every address range named below, refused or not, lies inside an allocation of this test
    srcs = [Frame(w, h, extra, IN_OFFS[k], slack=8).upload(frames[k]) for k in range(n)]
    dsts = [Frame(w, h, extra, OUT_OFFS[k], slack=8) for k in range(n)]
    pitch = srcs[0].pitch
    L, hd = c._L, c._h

    def call(which, last=None, null_list=False, tx=8, ty=8, **kw):
        a = dict(n=n, w=w, h=h, ip=pitch, op=pitch, fmt=FMT_YUY2, uv=UV_COPY, ctx=hd)
        a.update(kw)
        arr = (capi.Packed422FrameDev * n)()
        for k in range(n):
            arr[k] = capi.Packed422FrameDev(srcs[k].ptr, dsts[k].ptr)
        if last is not None:
            arr[n - 1] = capi.Packed422FrameDev(*last)
        lst = None if null_list else arr
        head = (a["ctx"], lst, a["n"], a["w"], a["h"], a["ip"], a["op"], a["fmt"], a["uv"])
        if which == "eq":
            return L.mi_equalize_hist_packed422_frames_dev(*head, stream())
        return L.mi_clahe_packed422_frames_dev(*head, ctypes.c_double(2.0), tx, ty, stream())

    si, do = srcs[n - 1].ptr, dsts[n - 1].ptr
    bad = [dict(ctx=None), dict(null_list=True),
           dict(w=-2), dict(h=-1), dict(n=-1), dict(w=63),
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uv=2), dict(uv=-1),
           dict(ip=2 * w - 4), dict(op=2 * w - 4), dict(ip=2 * w + 2), dict(op=2 * w + 6),
           dict(last=(si + 2, do)), dict(last=(si, do + 2)), dict(last=(si + 1, do)),
           dict(last=(None, do)), dict(last=(si, None)),
           dict(last=(si, si), op=pitch + 4),                                 # in place with unequal pitches
           dict(last=(si, si + 4)), dict(last=(si, si + pitch)), dict(last=(si + 8 * pitch, si)),   # partial overlap with its own input
           dict(last=(si, si - 4))]
    for kw in bad:
        assert call("eq", **kw) == BAD_ARG, kw
        assert call("clahe", **kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call("clahe", tx=tx, ty=ty) == BAD_ARG, (tx, ty)
    # zero sizes: MI_OK, nothing written (a null list is fine with no frames)
    for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, null_list=True)):
        assert call("eq", **kw) == 0 and call("clahe", **kw) == 0, kw
    torch.cuda.synchronize()
    assert_frames(dsts, [d.image() for d in dsts], "a refused or empty call wrote")
    assert_frames(srcs, [s.image(f) for s, f in zip(srcs, frames)], "a refused or empty call wrote an input")
    # and the context still works
    run(c, "eq", None, srcs, dsts, w, h, FMT_YUY2, UV_COPY)
    torch.cuda.synchronize()
    assert_frames(dsts, [d.image(expected_frame(f, w, FMT_YUY2, "eq", None, UV_COPY)) for d, f in zip(dsts, frames)], "after the refusals")


# ---- 6. streams, graph capture, profiling, pipe ----------------------------------------------------------------------------------
def test_stream_graph_profiling_and_busy():
    w, h, n = 1280, 720, 4
    fmt = FMT_UYVY
    frames = make_frames(w, h, fmt, DISTS[:n], 600)
    srcs = [Frame(w, h, 36, IN_OFFS[k]).upload(frames[k]) for k in range(n)]
    dsts = [Frame(w, h, 36, OUT_OFFS[k]) for k in range(n)]

    def check(fr, op, cfg, uv_mode, why):
        assert_frames(dsts, [d.image(expected_frame(f, w, fmt, op, cfg, uv_mode)) for d, f in zip(dsts, fr)], why)

    def clear():
        for d in dsts:
            d.clear()
        torch.cuda.synchronize()

    with mi_lumaeq.Context(0) as c:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            run(c, "clahe", (2.0, 8, 8), srcs, dsts, w, h, fmt, UV_COPY, st=side.cuda_stream)
        side.synchronize()
        check(frames, "clahe", (2.0, 8, 8), UV_COPY, "side stream")

        clear()
        run(c, "eq", None, srcs, dsts, w, h, fmt, UV_FILL128, st=mi_lumaeq.STREAM_CTX)
        c.synchronize(mi_lumaeq.STREAM_CTX)
        check(frames, "eq", None, UV_FILL128, "MI_STREAM_CTX")

        fresh = [make_frames(w, h, fmt, [DISTS[(k + 2 + r) % 5] for k in range(n)], 650 + 10 * r) for r in range(2)]
        for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
            clear()
            run(c, op, cfg, srcs, dsts, w, h, fmt, UV_FILL128)            # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                                     # a linear chain of launches: no parallel branches
                run(c, op, cfg, srcs, dsts, w, h, fmt, UV_FILL128, st=torch.cuda.current_stream().cuda_stream)
            for r in range(2):
                for s, f in zip(srcs, fresh[r]):
                    s.upload(f)
                clear()
                g.replay()
                torch.cuda.synchronize()
                check(fresh[r], op, cfg, UV_FILL128, ("graph replay", op, r))
            for s, f in zip(srcs, frames):
                s.upload(f)

        c.set_profiling(1)
        c.profile_read(reset=True)
        run(c, "eq", None, srcs, dsts, w, h, fmt, UV_COPY)
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
        c.set_profiling(0)
        assert len(prof) == 10
        for k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel"):
            assert prof[k]["launches"] == 1, (k, prof[k])
        for k in ("equalize_fused_kernel", "fused_finish_kernel", "tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel"):
            assert prof[k]["launches"] == 0, (k, prof[k])
        check(frames, "eq", None, UV_COPY, "profiled call")

        # MI_ERR_BUSY while a pipe of the context has a frame pending; nothing is written by the refused calls
        f = synth.nv12_frame(w, h, "D2", 3)
        o = np.zeros_like(f)
        clear()
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(f, o, 1)
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, cfg, srcs, dsts, w, h, fmt, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert_frames(dsts, [d.image() for d in dsts], "a busy context wrote")
        run(c, "clahe", (2.0, 8, 8), srcs, dsts, w, h, fmt, UV_COPY)       # nothing pending any more
        torch.cuda.synchronize()
        check(frames, "clahe", (2.0, 8, 8), UV_COPY, "after the pipe")
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 7. the fused path's counters ------------------------------------------------------------------------------------------------
def test_zz_fused_counters_stay_zero(c):
    torch.cuda.synchronize()
    assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
