"""Packed 4:2:2 frames (YUY2 / UYVY) on the GPU: mi_equalize_hist_packed422*, mi_clahe_packed422*, and the pipe formats.  Expected
frames are built on the CPU as "gather the luma -> oracle.equalize_hist / oracle.clahe -> scatter it back, chroma copied or 128".
Frames of a batch live in one allocation filled with a sentinel byte (padded pitch, a gap between frames, a base that is only 4-byte
aligned), and the WHOLE allocation is compared: every comparison in this file is exact bytes."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY, OP_EQUALIZE, OP_CLAHE, OP_CHANNELS

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
DISTS = ["D1", "D2", "D3", "D4", "D5"]
CLAHE_CONFIGS = [(2.0, 8, 8), (3.0, 4, 4), (0.0, 3, 5), (2.0, 16, 16), (2.0, 64, 2)]
OPS = [("eq", None)] + [("clahe", cfg) for cfg in CLAHE_CONFIGS]
# (pitch - 2W, gap between frames, base offset from a 16-byte boundary)
LAYOUTS = [(4, 20, 4), (36, 0, 8), (0, 12, 12)]
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]


def stream():
    return torch.cuda.current_stream().cuda_stream


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


class Batch:
    """n packed frames in one sentinel-filled allocation: rows of 2W bytes at `pitch`, frames `fstride` apart, first frame `off` in."""

    def __init__(self, w, h, n, layout=(0, 0, 0)):
        extra, gap, off = layout
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = 2 * w + extra
        self.fstride = self.pitch * h + gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def dev(self):
        return self.buf[self.off:]

    def image(self, frames=None):
        """The allocation as it must read with `frames` in it (None: untouched)."""
        a = np.full(self.total, SENT, np.uint8)
        if frames is not None:
            for k, f in enumerate(frames):
                o = self.off + k * self.fstride
                a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 2 * self.w] = f[:, : 2 * self.w]
        return a

    def upload(self, frames):
        self.buf.copy_(torch.from_numpy(self.image(frames)))
        return self

    def clear(self):
        self.buf.fill_(SENT)

    def host(self):
        return self.buf.cpu().numpy()

    def kw(self, prefix):
        return {prefix + "_pitch": self.pitch, prefix + "_frame": self.fstride}


def run(c, op, cfg, src, dst, fmt, uv_mode, n=None, st=None):
    kw = dict(src.kw("in"), **dst.kw("out"), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if op == "eq":
        c.equalize_hist_packed422_batch_dev(src.dev, dst.dev, src.w, src.h, n, fmt, uv_mode, **kw)
    else:
        c.clahe_packed422_batch_dev(src.dev, dst.dev, src.w, src.h, n, fmt, uv_mode, *cfg, **kw)


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


def check_case(c, frames, w, h, fmt, uv_mode, op, cfg, layout, key):
    n = len(frames)
    src = Batch(w, h, n, layout).upload(frames)
    dst = Batch(w, h, n, layout)
    status = planar_status(c, w, h, n, op, cfg)
    if status != 0:                                   # a size / grid pair the planar form refuses: the same status, nothing written
        with pytest.raises(mi_lumaeq.MiError) as e:
            run(c, op, cfg, src, dst, fmt, uv_mode)
        torch.cuda.synchronize()
        assert e.value.status == status, (w, h, op, cfg, e.value.status, status)
        assert np.array_equal(dst.host(), dst.image()), "a refused call wrote"
        return
    run(c, op, cfg, src, dst, fmt, uv_mode)
    torch.cuda.synchronize()
    want = dst.image([expected_frame(f, w, fmt, op, cfg, uv_mode, (key, k, fmt)) for k, f in enumerate(frames)])
    got = dst.host()
    assert np.array_equal(got, want), (w, h, fmt, uv_mode, op, cfg, layout, int((got != want).sum()), np.flatnonzero(got != want)[:8])
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


def make_frames(w, h, fmt, dists, first):
    return [synth.packed422_frame(w, h, fmt, d, first + k) for k, d in enumerate(dists)]


# ---- 1. device batch, out of place -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (62, 47), (2, 1), (4098, 3)])
def test_small_sizes_full_matrix(c, w, h):
    """Every format x uv_mode x op x layout on D1-D5; (0.0, 3, 5) on 62 x 47 pads by reflection on both axes, (2.0, 64, 2) takes the
    wide-grid kernel, 2 x 1 and 4098 x 3 have tiles narrower than a macropixel / rows of one ragged slot."""
    for fmt in FMTS:
        frames = make_frames(w, h, fmt, DISTS, 100)
        for uv_mode in UVS:
            for op, cfg in OPS:
                for layout in LAYOUTS:
                    check_case(c, frames, w, h, fmt, uv_mode, op, cfg, layout, ("small", w, h))


@pytest.mark.parametrize("w,h", [(1918, 1079), (1920, 1080)])
def test_hd_sizes(c, w, h):
    """D1-D5 at 1080p and at a size no tile grid divides: every format x uv_mode x op, the layouts in rotation."""
    i = 0
    for fmt in FMTS:
        frames = make_frames(w, h, fmt, DISTS, 200)
        for uv_mode in UVS:
            for op, cfg in OPS:
                check_case(c, frames, w, h, fmt, uv_mode, op, cfg, LAYOUTS[i % 3], ("hd", w, h))
                i += 1


@pytest.mark.parametrize("dist,fmt", [("D1", FMT_YUY2), ("D2", FMT_UYVY)])
def test_4k(c, dist, fmt):
    w, h = 3840, 2160
    frames = make_frames(w, h, fmt, [dist], 300)
    i = 0
    for uv_mode in UVS:
        for op, cfg in OPS:
            check_case(c, frames, w, h, fmt, uv_mode, op, cfg, LAYOUTS[i % 3], ("4k", dist))
            i += 1


# ---- 2. identity with the planar forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 64, 65, 130])
def test_identity_with_planar_forms(c, n):
    """The luma gathered from the packed output is the planar form's output on the gathered input, across chunk boundaries, in both
    CLAHE arithmetic modes and with the single-launch histogram + LUT path of the planar form on and off."""
    w, h = 320, 90
    g = torch.Generator(device="cuda:0")
    g.manual_seed(422 + n)
    x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
    x[: n // 2 + 1, :, :] = (x[: n // 2 + 1, :, :] // 3) + 40                      # half of the frames low-contrast
    out = torch.empty_like(x)
    try:
        for fmt in FMTS:
            off = fmt - 2
            y = x[:, :, off::2].contiguous()
            yo = torch.empty_like(y)
            for contract in (0, 1):
                for k2 in (0, 64):
                    c.set_option("clahe_fp_contract", contract)
                    c.set_option("two_kernel_max_frames", k2)
                    for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (3.0, 5, 3))):
                        out.fill_(SENT)
                        if op == "eq":
                            c.equalize_hist_batch_dev(y, yo, w, h, n, stream=stream())
                            c.equalize_hist_packed422_batch_dev(x, out, w, h, n, fmt, UV_COPY, stream=stream())
                        else:
                            c.clahe_batch_dev(y, yo, w, h, n, *cfg, stream=stream())
                            c.clahe_packed422_batch_dev(x, out, w, h, n, fmt, UV_COPY, *cfg, stream=stream())
                        torch.cuda.synchronize()
                        assert torch.equal(out[:, :, off::2], yo), (n, fmt, contract, k2, op, cfg)
                        assert torch.equal(out[:, :, 1 - off::2], x[:, :, 1 - off::2]), "chroma not passed through"
    finally:
        c.set_option("clahe_fp_contract", 0)
        c.set_option("two_kernel_max_frames", 8)


# ---- 3. in place -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(62, 47), (1280, 720)])
def test_in_place(c, w, h):
    for fmt in FMTS:
        frames = make_frames(w, h, fmt, DISTS[:3], 400)
        for uv_mode in UVS:
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (2.0, 64, 2))):
                b = Batch(w, h, len(frames), LAYOUTS[0]).upload(frames)
                run(c, op, cfg, b, b, fmt, uv_mode)
                torch.cuda.synchronize()
                want = b.image([expected_frame(f, w, fmt, op, cfg, uv_mode) for f in frames])
                assert np.array_equal(b.host(), want), (w, h, fmt, uv_mode, op, cfg)


# ---- 4. host forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(62, 47), (1280, 720)])
def test_host_forms(c, w, h):
    for fmt in FMTS:
        f = synth.packed422_frame(w, h, fmt, "D2", 500)
        for uv_mode in UVS:
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
                want = expected_frame(f, w, fmt, op, cfg, uv_mode)

                def call(src, out):
                    if op == "eq":
                        return c.equalize_hist_packed422(src, w, fmt, uv_mode, out=out)
                    return c.clahe_packed422(src, w, fmt, uv_mode, *cfg, out=out)
                # unpinned, tight
                src = f.copy()
                got = call(src, None)
                assert np.array_equal(got, want) and np.array_equal(src, f), ("unpinned", fmt, uv_mode, op)
                # registered (pinned) frames, DMA'd as they are
                pin_in, pin_out = f.copy(), np.full_like(f, SENT)
                mi_lumaeq.capi.host_register(pin_in)
                mi_lumaeq.capi.host_register(pin_out)
                try:
                    call(pin_in, pin_out)
                    assert np.array_equal(pin_out, want) and np.array_equal(pin_in, f), ("registered", fmt, uv_mode, op)
                finally:
                    mi_lumaeq.capi.host_unregister(pin_in)
                    mi_lumaeq.capi.host_unregister(pin_out)
                # pitched: only the 2W bytes of each row are read and written
                big_in = np.full((h, 2 * w + 12), SENT, np.uint8)
                big_out = np.full((h, 2 * w + 20), SENT, np.uint8)
                big_in[:, : 2 * w] = f
                call(big_in[:, : 2 * w], big_out[:, : 2 * w])
                assert np.array_equal(big_out[:, : 2 * w], want), ("pitched", fmt, uv_mode, op)
                assert (big_out[:, 2 * w:] == SENT).all() and (big_in[:, 2 * w:] == SENT).all() and np.array_equal(big_in[:, : 2 * w], f)
                # in == out
                io = f.copy()
                call(io, io)
                assert np.array_equal(io, want), ("in place", fmt, uv_mode, op)


# ---- 5. pipe ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("op", [OP_EQUALIZE, OP_CLAHE])
def test_pipe(c, fmt, op):
    w, h, n = 640, 359, 12
    ins = [synth.packed422_frame(w, h, fmt, DISTS[k % 5], 600 + k) for k in range(n)]
    outs = [np.full_like(f, SENT) for f in ins]
    tags = []
    with mi_lumaeq.Pipe(c, w, h, op=op, uv_mode=UV_COPY, clip_limit=2.0, tiles_x=8, tiles_y=8, depth=3, format=fmt) as pipe:
        assert pipe.depth == 3 and pipe.frame_bytes == 2 * w * h
        for k in range(n):
            while not pipe.submit(ins[k], outs[k], 1000 + k):
                tags.append(pipe.wait()[0])
        while pipe.pending:
            tags.append(pipe.wait()[0])
    assert tags == [1000 + k for k in range(n)]
    for k in range(n):
        want = expected_frame(ins[k], w, fmt, "eq" if op == OP_EQUALIZE else "clahe", (2.0, 8, 8), UV_COPY)
        assert np.array_equal(outs[k], want), (fmt, op, k)


def test_pipe_refusals(c):
    def status(**kw):
        a = dict(op=OP_EQUALIZE, format=FMT_YUY2)
        a.update(kw)
        w = a.pop("w", 64)
        try:
            mi_lumaeq.Pipe(c, w, 48, **a).close()
        except mi_lumaeq.MiError as e:
            return e.status
        return 0
    assert status() == 0 and status(format=FMT_UYVY, op=OP_CLAHE, uv_policy=mi_lumaeq.PIPE_UV_DEVICE) == 0
    assert status(op=OP_CHANNELS) == UNSUPPORTED and status(op=OP_CHANNELS, format=FMT_UYVY) == UNSUPPORTED
    assert status(uv_policy=mi_lumaeq.PIPE_UV_HOST) == UNSUPPORTED
    assert status(format=7) == BAD_ARG
    assert status(w=63) == BAD_ARG and status(w=63, format=FMT_UYVY) == BAD_ARG


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    w, h, n = 64, 48, 2
    frames = make_frames(w, h, FMT_YUY2, DISTS[:n], 700)
    src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
    dst = Batch(w, h, n, LAYOUTS[0])
    L, hd = c._L, c._h
    ip, of = src.dev.data_ptr(), dst.dev.data_ptr()

    def eq(**kw):
        a = dict(i=ip, ipitch=src.pitch, ifs=src.fstride, o=of, opitch=dst.pitch, ofs=dst.fstride, w=w, h=h, n=n, fmt=FMT_YUY2, uv=UV_COPY)
        a.update(kw)
        return L.mi_equalize_hist_packed422_batch_dev(hd, a["i"], a["ipitch"], a["ifs"], a["o"], a["opitch"], a["ofs"], a["w"], a["h"],
                                                      a["n"], a["fmt"], a["uv"], stream())

    def cl(tx=8, ty=8, **kw):
        a = dict(i=ip, ipitch=src.pitch, ifs=src.fstride, o=of, opitch=dst.pitch, ofs=dst.fstride, w=w, h=h, n=n, fmt=FMT_YUY2, uv=UV_COPY)
        a.update(kw)
        return L.mi_clahe_packed422_batch_dev(hd, a["i"], a["ipitch"], a["ifs"], a["o"], a["opitch"], a["ofs"], a["w"], a["h"],
                                              a["n"], a["fmt"], a["uv"], 2.0, tx, ty, stream())
    bad = [dict(i=None), dict(o=None), dict(w=63), dict(w=-2), dict(h=-1), dict(n=-1), dict(ipitch=2 * w - 4), dict(opitch=2 * w - 4),
           dict(i=ip + 2), dict(o=of + 1), dict(ipitch=2 * w + 2), dict(opitch=2 * w + 6), dict(ifs=src.fstride + 2), dict(ofs=dst.fstride + 1),
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uv=2), dict(uv=-1)]
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert cl(tx, ty) == BAD_ARG
    # host forms: the same checks
    f, o = frames[0].copy(), np.full((h, 2 * w), SENT, np.uint8)
    for fmt, uv, ww, pi in ((5, 0, w, 2 * w), (2, 3, w, 2 * w), (2, 0, w - 1, 2 * w), (2, 0, w, 2 * w - 4), (2, 0, w, 2 * w + 2)):
        assert L.mi_equalize_hist_packed422(hd, f.ctypes.data, pi, o.ctypes.data, 2 * w, ww, h, fmt, uv) == BAD_ARG
        assert L.mi_clahe_packed422(hd, f.ctypes.data, pi, o.ctypes.data, 2 * w, ww, h, fmt, uv, 2.0, 8, 8) == BAD_ARG
    assert L.mi_equalize_hist_packed422(hd, None, 2 * w, o.ctypes.data, 2 * w, w, h, 2, 0) == BAD_ARG
    assert L.mi_clahe_packed422(hd, f.ctypes.data, 2 * w, o.ctypes.data, 2 * w, w, h, 2, 0, 2.0, 0, 8) == BAD_ARG
    # zero sizes: MI_OK, nothing written
    for kw in (dict(w=0), dict(h=0), dict(n=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    assert L.mi_equalize_hist_packed422(hd, f.ctypes.data, 2 * w, o.ctypes.data, 2 * w, 0, h, 2, 0) == 0
    assert L.mi_clahe_packed422(hd, f.ctypes.data, 2 * w, o.ctypes.data, 2 * w, w, 0, 3, 1, 2.0, 8, 8) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.host(), dst.image()), "a refused or empty call wrote"
    assert np.array_equal(src.host(), src.image(frames))
    assert (o == SENT).all() and np.array_equal(f, frames[0])
    # and the context still works
    run(c, "eq", None, src, dst, FMT_YUY2, UV_COPY)
    torch.cuda.synchronize()
    assert np.array_equal(dst.host(), dst.image([expected_frame(x, w, FMT_YUY2, "eq", None, UV_COPY) for x in frames]))


# ---- 7. streams, graph capture, profiling ----------------------------------------------------------------------------------------
def test_stream_graph_and_profiling():
    w, h, n = 1280, 720, 4
    fmt = FMT_UYVY
    frames = make_frames(w, h, fmt, DISTS[:n], 800)
    src = Batch(w, h, n, LAYOUTS[1]).upload(frames)
    dst = Batch(w, h, n, LAYOUTS[1])

    def check(fr, op, cfg, uv_mode, why):
        want = dst.image([expected_frame(f, w, fmt, op, cfg, uv_mode) for f in fr])
        assert np.array_equal(dst.host(), want), why

    with mi_lumaeq.Context(0) as c:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            run(c, "clahe", (2.0, 8, 8), src, dst, fmt, UV_COPY, st=side.cuda_stream)
        side.synchronize()
        check(frames, "clahe", (2.0, 8, 8), UV_COPY, "side stream")

        dst.clear()
        torch.cuda.synchronize()
        run(c, "eq", None, src, dst, fmt, UV_FILL128, st=mi_lumaeq.STREAM_CTX)
        c.synchronize(mi_lumaeq.STREAM_CTX)
        check(frames, "eq", None, UV_FILL128, "MI_STREAM_CTX")

        for op, cfg in (("eq", None), ("clahe", (3.0, 4, 4))):
            dst.clear()
            run(c, op, cfg, src, dst, fmt, UV_FILL128)                 # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, cfg, src, dst, fmt, UV_FILL128, st=torch.cuda.current_stream().cuda_stream)
            fresh = make_frames(w, h, fmt, [DISTS[(k + 2) % 5] for k in range(n)], 850)
            src.upload(fresh)
            dst.clear()
            g.replay()
            torch.cuda.synchronize()
            check(fresh, op, cfg, UV_FILL128, ("graph replay", op))
            src.upload(frames)

        c.set_profiling(1)
        c.profile_read(reset=True)
        run(c, "eq", None, src, dst, fmt, UV_COPY)
        run(c, "clahe", (2.0, 8, 8), src, dst, fmt, UV_COPY)
        run(c, "clahe", (2.0, 64, 2), src, dst, fmt, UV_COPY)
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
        c.set_profiling(0)
        assert len(prof) == 10
        # the new kernels are charged by role; the two LUT kernels between them are the planar forms' own, in their own slots
        for k, want in (("hist_partial_kernel", 1), ("lut_apply_kernel", 1), ("tile_hist_kernel", 2), ("clahe_interp_kernel", 2),
                        ("equalize_lut_kernel", 1)):
            assert prof[k]["launches"] == want, (k, prof[k])
        for k in ("equalize_fused_kernel", "fused_finish_kernel", "color_kernel", "analyze_diff_kernel"):
            assert prof[k]["launches"] == 0, (k, prof[k])
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 8. the fused path's counters ------------------------------------------------------------------------------------------------
def test_zz_fused_counters_stay_zero(c):
    torch.cuda.synchronize()
    assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
