"""P010 frame lists on the GPU (mi_clahe_p010_frames_dev).  Frames live in separately allocated 16-bit "surfaces" laid out like a
Main10 decoder's: rows padded to a pitch, the UV plane after a vertical stride, every sample outside the pixels set to a sentinel.
Every comparison is exact bytes: Y against oracle.clahe16 per frame, UV against the fill / copy rule, the sentinels against
themselves, and lists over one tight batch against mi_clahe_p010_batch_dev.  The mixed lists -- in-place and out-of-place frames of
wide content in one launch -- are what shows that the interpolation kernels decide who writes an in-place pixel per frame."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5AA5                                   # sentinel sample (bytes A5 5A)
CONTENTS = ["p010", "p012", "p016", "14-bit", "hot", "full"]


def align(x, a):
    return (x + a - 1) // a * a


def stream():
    return torch.cuda.current_stream().cuda_stream


def content(kind, w, h, idx):
    """(Y, UV) uint16 arrays: synth's P010 / P012 / P016 frames, or wide content (14-bit noise, 12-bit noise with one hot pixel,
    full-range noise) with synth's chroma."""
    fr = synth.p010_frame(w, h, kind if kind in ("p010", "p012", "p016") else "p010", idx)
    y, uv = fr[:h].copy(), fr[h:].reshape(h // 2, w).copy()
    rng = np.random.default_rng(9000 + idx)
    if kind == "14-bit":
        y = rng.integers(0, 16384, (h, w), dtype=np.uint16)
    elif kind == "hot":
        y = rng.integers(0, 4096, (h, w), dtype=np.uint16)
        y[h // 2 + 3, w // 3 + 5] = 65535
    elif kind == "full":
        y = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    return y, uv


class Surface:
    """One allocation holding a P010 frame as int16 samples: Y rows at `pitch` bytes, the UV plane at off + pitch * vstride, the
    sentinel everywhere else.  `off` in samples (an odd count: 2-byte but not 16-byte aligned planes)."""

    def __init__(self, w, h, pitch, vstride, off=0):
        assert pitch % 2 == 0
        self.w, self.h, self.ps, self.vstride, self.off = w, h, pitch // 2, vstride, off
        self.pitch = pitch
        self.total = off + self.ps * vstride + self.ps * (h // 2) + 24
        self.buf = torch.full((self.total,), SENT, dtype=torch.int16, device="cuda:0")
        self.y, self.uv = self._views(self.buf)

    def _views(self, buf):
        p, o = self.ps, self.off
        y = buf[o: o + p * self.h].view(self.h, p)[:, : self.w]
        u0 = o + p * self.vstride
        return y, buf[u0: u0 + p * (self.h // 2)].view(self.h // 2, p)[:, : self.w]

    def fill(self, y, uv):
        self.y.copy_(torch.from_numpy(y.view(np.int16)))
        self.uv.copy_(torch.from_numpy(uv.view(np.int16)))
        return self

    def expected(self, y, uv):
        cpu = torch.full((self.total,), SENT, dtype=torch.int16)
        vy, vuv = self._views(cpu)
        vy.copy_(torch.from_numpy(np.ascontiguousarray(y).view(np.int16)))
        vuv.copy_(torch.from_numpy(np.ascontiguousarray(uv).view(np.int16)))
        return cpu.numpy()

    def planes(self):
        return (self.y, self.uv)


def uv_ref(uv, uv_mode):
    return np.full_like(uv, 0x8000) if uv_mode == UV_FILL128 else uv


_want_cache = {}


def y_want(y, cfg, key):
    k = (key, cfg, y.shape, hash(y[::7, ::5].tobytes()))             # the content itself, sampled: keys repeat across tests
    if k not in _want_cache:
        _want_cache[k] = oracle.clahe16(np.ascontiguousarray(y), *cfg)
    return _want_cache[k]


def check(dst, y, uv, cfg, uv_mode, key, why):
    got = dst.buf.cpu().numpy()
    want = dst.expected(y_want(y, cfg, key), uv_ref(uv, uv_mode))
    assert np.array_equal(got, want), (why, key, cfg, uv_mode, int((got != want).sum()))


@pytest.mark.parametrize("w,h,cfgs", [(3840, 2160, [(2.0, 8, 8)]), (1920, 1080, [(2.0, 8, 8), (3.0, 5, 3), (40.0, 7, 5)])])
def test_decoder_surfaces(w, h, cfgs):
    """Pitch align(2W, 256), vertical stride align(H, 64), UV at pitch x vstride; every content, both chroma modes; 7 x 5 tiles at 1080p
    pad the tiles (careful histogram path)."""
    pitch, vs = align(2 * w, 256), align(h, 64)
    data = [content(k, w, h, 10 + i) for i, k in enumerate(CONTENTS)]
    srcs = [Surface(w, h, pitch, vs).fill(y, uv) for y, uv in data]
    dsts = [Surface(w, h, pitch, vs) for _ in data]
    with mi_lumaeq.Context(0) as c:
        for cfg in cfgs:
            for uv_mode in (UV_COPY, UV_FILL128):
                c.clahe_p010_frames([s.planes() for s in srcs], [d.planes() for d in dsts], w, h, uv_mode, *cfg, stream=stream())
                torch.cuda.synchronize()
                for k, (s, d, (y, uv)) in enumerate(zip(srcs, dsts, data)):
                    check(d, y, uv, cfg, uv_mode, (w, CONTENTS[k]), "surfaces")
                    assert np.array_equal(s.buf.cpu().numpy(), s.expected(y, uv)), ("input written", k)


@pytest.mark.parametrize("n", [1, 16, 64, 65, 130])
def test_same_bytes_as_batch_form(n):
    """A list over one tight batch (frame k at base + k * 3WH) returns exactly what mi_clahe_p010_batch_dev returns, across the
    64-frame chunks, out of place and in place."""
    w, h = 320, 180
    fb = w * h * 3                                                      # bytes per frame
    kinds = ["p010", "p012", "p016"]
    batch = np.stack([synth.p010_frame(w, h, kinds[k % 3], 100 + k) for k in range(n)])
    with mi_lumaeq.Context(0) as c:
        d_in = torch.from_numpy(batch.reshape(-1).view(np.int16)).to("cuda:0")
        base = d_in.data_ptr()
        ins = [(base + k * fb, base + k * fb + 2 * w * h) for k in range(n)]
        for uv_mode in (UV_FILL128, UV_COPY):
            for cfg in ((2.0, 8, 8), (0.0, 3, 5)):
                want = torch.full_like(d_in, SENT)
                got = torch.full_like(d_in, SENT)
                ob = got.data_ptr()
                c.clahe_p010_batch_dev(d_in, want, w, h, n, uv_mode, *cfg, stream=stream())
                c.clahe_p010_frames(ins, [(ob + k * fb, ob + k * fb + 2 * w * h) for k in range(n)], w, h, uv_mode, *cfg, stream=stream())
                torch.cuda.synchronize()
                assert torch.equal(got, want), (n, cfg, uv_mode)
                io = d_in.clone()
                b = io.data_ptr()
                c.clahe_p010_frames([(b + k * fb, b + k * fb + 2 * w * h) for k in range(n)], None, w, h, uv_mode, *cfg, stream=stream())
                torch.cuda.synchronize()
                assert torch.equal(io, want), ("in place", n, cfg, uv_mode)
        g = want.cpu().numpy().view(np.uint16).reshape(n, 3 * h // 2, w)
        for k in {0, n - 1}:                                            # and the batch form is right
            assert np.array_equal(g[k][:h], oracle.clahe16(np.ascontiguousarray(batch[k][:h]), 0.0, 3, 5))


@pytest.mark.parametrize("off,pad", [(3, 2), (1, 18), (0, 32)])
def test_alignment(off, pad):
    """Planes at 2-byte aligned offsets that are not 16-byte aligned and pitches 2W + 2 / 2W + 18 (the careful tile histogram), and
    16-byte aligned planes at a pitch that is a multiple of 16 (the vector path and the 12-bit bet); the chroma copy from a source at
    another alignment than its destination."""
    w, h = 1280, 720
    data = [content(k, w, h, 30 + i) for i, k in enumerate(CONTENTS)]
    srcs = [Surface(w, h, 2 * w + pad, h + 2 * k, off=off * (k + 1) % 16 if off else 0).fill(y, uv) for k, (y, uv) in enumerate(data)]
    dsts = [Surface(w, h, 2 * w + pad, h + 4, off=(off * (k + 3)) % 16 if off else 8 * (k % 2)) for k in range(len(data))]
    with mi_lumaeq.Context(0) as c:
        for cfg in ((2.0, 8, 8), (2.0, 4, 6)):
            for uv_mode in (UV_COPY, UV_FILL128):
                c.clahe_p010_frames([s.planes() for s in srcs], [d.planes() for d in dsts], w, h, uv_mode, *cfg, stream=stream())
                torch.cuda.synchronize()
                for k, (d, (y, uv)) in enumerate(zip(dsts, data)):
                    check(d, y, uv, cfg, uv_mode, (w, CONTENTS[k]), ("align", off, pad))


def test_mixed_in_place_lists():
    """One list, one launch: wide content (14-bit, hot pixel, full range) and P010 content, each both IN PLACE and out of place.  In
    place, the rectangles that need several windows belong to the mid or the gathering kernel; out of place to the table kernels.
    Under clahe16_wide 0 / 1 / 2, clahe16_fast12 0 and clahe16_transposed 1; lists where every frame is in place too."""
    w, h = 1920, 1080
    cfg = (2.0, 8, 8)
    kinds = ["14-bit", "hot", "full", "p010"]
    data = [content(k, w, h, 50 + i) for i, k in enumerate(kinds)]
    pitch, vs = align(2 * w, 256), align(h, 64)
    with mi_lumaeq.Context(0) as c:
        settings = [("clahe16_wide", 2), ("clahe16_wide", 0), ("clahe16_wide", 1), ("clahe16_wide", 1), ("clahe16_fast12", 0),
                    ("clahe16_transposed", 1)]
        try:
            for name, value in settings:
                c.set_option(name, value)
                for all_in_place in (False, True):
                    io = [Surface(w, h, pitch, vs).fill(y, uv) for y, uv in data]
                    srcs = [Surface(w, h, pitch, vs).fill(y, uv) for y, uv in data]
                    dsts = [Surface(w, h, pitch, vs) for _ in data]
                    # interleaved: in-place frame k, then out-of-place frame k
                    ins, outs = [], []
                    for k in range(len(data)):
                        ins.append(io[k].planes()); outs.append(io[k].planes())
                        if not all_in_place:
                            ins.append(srcs[k].planes()); outs.append(dsts[k].planes())
                    for uv_mode in (UV_COPY, UV_FILL128):
                        if uv_mode == UV_FILL128:
                            for k, (y, uv) in enumerate(data):
                                io[k].fill(y, uv)
                        c.clahe_p010_frames(ins, outs, w, h, uv_mode, *cfg, stream=stream())
                        torch.cuda.synchronize()
                        for k, (y, uv) in enumerate(data):
                            check(io[k], y, uv, cfg, uv_mode, (w, kinds[k]), ("in place", name, value, all_in_place))
                            if not all_in_place:
                                check(dsts[k], y, uv, cfg, uv_mode, (w, kinds[k]), ("out of place", name, value))
                                assert np.array_equal(srcs[k].buf.cpu().numpy(), srcs[k].expected(y, uv))
                c.set_option(name, {"clahe16_wide": 1, "clahe16_fast12": 1, "clahe16_transposed": 0}[name])
            assert c.get_stat("clahe16_mid_launches") > 0
        finally:
            c.set_option("clahe16_wide", 1)
            c.set_option("clahe16_fast12", 1)
            c.set_option("clahe16_transposed", 0)


def test_argument_errors_write_nothing():
    w, h = 64, 32
    pitch = 256
    data = [content("p010", w, h, 70 + k) for k in range(2)]
    srcs = [Surface(w, h, pitch, 48).fill(y, uv) for y, uv in data]
    dsts = [Surface(w, h, pitch, 48) for _ in data]
    s0, d0 = srcs[0], dsts[0]
    P = mi_lumaeq.Nv12FrameDev
    y_in, uv_in, y_out, uv_out = s0.y.data_ptr(), s0.uv.data_ptr(), d0.y.data_ptr(), d0.uv.data_ptr()
    with mi_lumaeq.Context(0) as c:
        L, hc, st = c._L, c._h, stream()

        def cl(fr, n=None, ww=w, hh=h, p=(pitch,) * 4, uv=UV_COPY, tx=8, ty=8):
            arr = (P * max(1, len(fr)))(*fr)
            return L.mi_clahe_p010_frames_dev(hc, arr if fr else None, len(fr) if n is None else n, ww, hh, *p, uv, 2.0, tx, ty, st)

        good = P(y_in, uv_in, y_out, uv_out)
        assert L.mi_clahe_p010_frames_dev(None, (P * 1)(good), 1, w, h, pitch, pitch, pitch, pitch, UV_COPY, 2.0, 8, 8, st) == BAD_ARG
        assert cl([], n=1) == BAD_ARG                                  # null list, n > 0
        assert cl([good], n=-1) == BAD_ARG
        assert cl([good], ww=62 + 1) == BAD_ARG and cl([good], hh=31) == BAD_ARG
        for k in range(4):
            p = [pitch] * 4
            p[k] = 2 * w - 2                                           # each pitch < 2W (>= W: the NV12 bound would pass)
            assert cl([good], p=tuple(p)) == BAD_ARG, k
            p[k] = pitch + 1                                           # each pitch odd
            assert cl([good], p=tuple(p)) == BAD_ARG, k
        for bad in (P(y_in + 1, uv_in, y_out, uv_out), P(y_in, uv_in + 1, y_out, uv_out), P(y_in, uv_in, y_out + 1, uv_out),
                    P(y_in, uv_in, y_out, uv_out + 1)):
            assert cl([good, bad]) == BAD_ARG                          # a plane that is not 2-byte aligned
        assert cl([P(None, uv_in, y_out, uv_out)]) == BAD_ARG
        assert cl([P(y_in, uv_in, None, uv_out)]) == BAD_ARG
        assert cl([P(y_in, uv_in, y_out, None)]) == BAD_ARG
        assert cl([P(y_in, None, y_out, uv_out)]) == BAD_ARG           # null uv_in with MI_UV_COPY
        assert cl([P(y_in, uv_in, y_in + 2, uv_out)]) == BAD_ARG       # partial overlaps of an output with an input plane
        assert cl([P(y_in, uv_in, y_out, uv_in + 16)]) == BAD_ARG
        assert cl([P(y_in, uv_in, y_out, y_in + pitch)]) == BAD_ARG
        assert cl([P(y_in, uv_in, uv_in, uv_out)]) == BAD_ARG
        assert cl([P(y_in, uv_in, y_in, uv_out)], p=(pitch, pitch, pitch + 2, pitch)) == BAD_ARG   # "in place" at another pitch
        assert cl([good], uv=7) == BAD_ARG
        assert cl([good], tx=0) == BAD_ARG and cl([good], ty=-1) == BAD_ARG
        # a bad frame deep in a long list: the first chunks are not enqueued either
        assert cl([good] * 100 + [P(y_in, uv_in, y_out + 1, uv_out)] + [good] * 20) == BAD_ARG
        assert cl([good], ww=65536, hh=16384, p=(131072,) * 4) == UNSUPPORTED      # beyond mi_clahe_u16's sizes
        torch.cuda.synchronize()
        for s, d, (y, uv) in zip(srcs, dsts, data):
            assert np.array_equal(s.buf.cpu().numpy(), s.expected(y, uv))
            assert np.array_equal(d.buf.cpu().numpy(), np.full(d.total, SENT, np.int16)), "a refused call wrote"
        assert cl([], n=0) == 0 and cl([good], ww=0) == 0 and cl([good], hh=0) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d0.buf.cpu().numpy(), np.full(d0.total, SENT, np.int16))
        assert cl([P(y_in, None, y_out, uv_out)], uv=UV_FILL128) == 0   # MI_UV_FILL128 reads no chroma
        torch.cuda.synchronize()
        check(d0, data[0][0], data[0][1], (2.0, 8, 8), UV_FILL128, ("err", 0), "fill without uv_in")


def test_stream_graph_and_profiling():
    """A non-default torch stream; one torch.cuda.graph capture after an eager call, replayed on new pixels; with profiling on the
    launches land in the existing slots (the chroma in lut_apply_kernel's)."""
    w, h, n = 1280, 720, 5
    pitch, vs = align(2 * w, 256), align(h, 16)
    data = [content(CONTENTS[k], w, h, 80 + k) for k in range(n)]
    srcs = [Surface(w, h, pitch, vs).fill(y, uv) for y, uv in data]
    dsts = [Surface(w, h, pitch, vs) for _ in data]
    ins, outs = [s.planes() for s in srcs], [d.planes() for d in dsts]
    cfg = (3.0, 4, 4)
    with mi_lumaeq.Context(0) as c:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c.clahe_p010_frames(ins, outs, w, h, UV_COPY, *cfg, stream=side.cuda_stream)
        side.synchronize()
        for k, (y, uv) in enumerate(data):
            check(dsts[k], y, uv, cfg, UV_COPY, ("g", k), "side stream")

        c.clahe_p010_frames(ins, outs, w, h, UV_FILL128, *cfg, stream=stream())     # eager call of the captured shape sizes the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.clahe_p010_frames(ins, outs, w, h, UV_FILL128, *cfg, stream=torch.cuda.current_stream().cuda_stream)
        fresh = [content(CONTENTS[(k + 2) % len(CONTENTS)], w, h, 90 + k) for k in range(n)]
        for s, (y, uv) in zip(srcs, fresh):
            s.fill(y, uv)
        for d in dsts:
            d.buf.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        for k, (y, uv) in enumerate(fresh):
            check(dsts[k], y, uv, cfg, UV_FILL128, ("fresh", k), "graph replay")

        c.set_profiling(1)
        c.profile_read(reset=True)
        c.clahe_p010_frames(ins, outs, w, h, UV_COPY, 2.0, 8, 8, stream=stream())
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
        c.set_profiling(0)
        assert len(prof) == 10
        for k, want in (("tile_hist_kernel", 1), ("tile_lut_kernel", 1), ("lut_apply_kernel", 1)):
            assert prof[k]["launches"] == want, (k, prof[k])
        assert prof["clahe_interp_kernel"]["launches"] >= 1
