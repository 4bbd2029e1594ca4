"""NV12 frame lists on the GPU (mi_equalize_hist_nv12_frames_dev, mi_clahe_nv12_frames_dev).  Frames live in separately allocated
"surfaces" laid out like a decoder's: rows padded to a pitch, the UV plane after a vertical stride, every byte outside the pixels set
to a sentinel.  Every comparison is exact bytes: Y against oracle.equalize_hist / oracle.clahe per frame, UV against the fill / copy
rule, the sentinel bytes against themselves, and lists over one tight batch against the existing mi_*_nv12_batch_dev forms."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY

pytestmark = pytest.mark.gpu
BAD_ARG = 1
SENT = 0x5A
DISTS = ["D1", "D2", "D3", "D4", "D5"]
CLAHE_CONFIGS = [(2.0, 8, 8), (3.0, 4, 4), (0.0, 3, 5), (2.0, 16, 16), (2.0, 64, 2)]


def align(x, a):
    return (x + a - 1) // a * a


def stream():
    return torch.cuda.current_stream().cuda_stream


class Surface:
    """One allocation holding an NV12 frame: Y rows at `pitch`, the UV plane at off + pitch * vstride, sentinel everywhere else."""

    def __init__(self, w, h, pitch, vstride, off=0, device="cuda:0"):
        self.w, self.h, self.pitch, self.vstride, self.off = w, h, pitch, vstride, off
        self.total = off + pitch * vstride + pitch * (h // 2) + 48
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device=device)
        self.y, self.uv = self._views(self.buf)

    def _views(self, buf):
        p, o = self.pitch, self.off
        y = buf[o: o + p * self.h].view(self.h, p)[:, : self.w]
        u0 = o + p * self.vstride
        uv = buf[u0: u0 + p * (self.h // 2)].view(self.h // 2, p)[:, : self.w]
        return y, uv

    def fill(self, frame):
        y, uv = split(frame, self.w, self.h)
        self.y.copy_(torch.from_numpy(y))
        self.uv.copy_(torch.from_numpy(uv))
        return self

    def expected(self, y, uv):
        """The whole buffer as it must read: sentinel outside the pixels."""
        cpu = torch.full((self.total,), SENT, dtype=torch.uint8)
        vy, vuv = self._views(cpu)
        vy.copy_(torch.from_numpy(np.ascontiguousarray(y)))
        vuv.copy_(torch.from_numpy(np.ascontiguousarray(uv)))
        return cpu.numpy()

    def planes(self):
        return (self.y, self.uv)


def split(frame, w, h):
    frame = np.asarray(frame).reshape(-1)
    return frame[: w * h].reshape(h, w), frame[w * h: w * h * 3 // 2].reshape(h // 2, w)


def y_ref(y, op, cfg):
    return oracle.equalize_hist(np.ascontiguousarray(y)) if op == "eq" else oracle.clahe(np.ascontiguousarray(y), *cfg)


def uv_ref(uv, uv_mode):
    return np.full_like(uv, 128) if uv_mode == UV_FILL128 else uv


def run(c, op, ins, outs, w, h, uv_mode, cfg=(2.0, 8, 8), **kw):
    if op == "eq":
        c.equalize_hist_nv12_frames(ins, outs, w, h, uv_mode, stream=kw.pop("stream", stream()), **kw)
    else:
        c.clahe_nv12_frames(ins, outs, w, h, uv_mode, *cfg, stream=kw.pop("stream", stream()), **kw)


def check_surfaces(srcs, dsts, frames, w, h, op, uv_mode, cfg=(2.0, 8, 8), why=()):
    torch.cuda.synchronize()
    for k, (s, d, f) in enumerate(zip(srcs, dsts, frames)):
        y, uv = split(f, w, h)
        want = d.expected(y_ref(y, op, cfg), uv_ref(uv, uv_mode))
        got = d.buf.cpu().numpy()
        assert np.array_equal(got, want), (why, op, uv_mode, cfg, k, int((got != want).sum()))
        assert np.array_equal(s.buf.cpu().numpy(), s.expected(y, uv)), (why, "input written", k)


def surfaces(w, h, n, vstride_align, dists=DISTS, first=0, pitch_align=256):
    pitch, vs = align(w, pitch_align), align(h, vstride_align)
    frames = [synth.nv12_frame(w, h, dists[k % len(dists)], first + k) for k in range(n)]
    return frames, [Surface(w, h, pitch, vs).fill(f) for f in frames], [Surface(w, h, pitch, vs) for f in frames]


@pytest.mark.parametrize("w,h,va", [(1280, 720, 16), (1280, 720, 64), (1920, 1080, 64)])
def test_decoder_surfaces(w, h, va):
    """Pitch align(W, 256), vertical stride align(H, 16 / 64), UV at pitch x vstride: both ops, both UV modes, every CLAHE config
    (the segmented float tables at 1920 16x16, the global-LUT kernel at 64x2) in both arithmetic modes."""
    frames, srcs, dsts = surfaces(w, h, 3, va, first=10)
    ins, outs = [s.planes() for s in srcs], [d.planes() for d in dsts]
    with mi_lumaeq.Context(0) as c:
        for uv_mode in (UV_FILL128, UV_COPY):
            run(c, "eq", ins, outs, w, h, uv_mode)
            check_surfaces(srcs, dsts, frames, w, h, "eq", uv_mode)
        for contract in (False, True):
            old = oracle.set_fp_contract(contract)
            try:
                c.set_option("clahe_fp_contract", int(contract))
                for cfg in CLAHE_CONFIGS:
                    uv_mode = UV_COPY if cfg[1] % 2 == 0 else UV_FILL128
                    run(c, "clahe", ins, outs, w, h, uv_mode, cfg)
                    check_surfaces(srcs, dsts, frames, w, h, "clahe", uv_mode, cfg, why=("contract", contract))
            finally:
                oracle.set_fp_contract(old)
                c.set_option("clahe_fp_contract", 0)


@pytest.mark.parametrize("n", [1, 8, 9, 63, 64, 65, 130])
def test_same_bytes_as_batch_form(n):
    """A list over one tight contiguous batch (frame k at base + k * 1.5WH) returns exactly what mi_*_nv12_batch_dev returns:
    across the 64-frame chunks and both equalize paths (two_kernel_max_frames 0 and 64), the batch form with and without fused."""
    w, h = 320, 180
    fb = w * h * 3 // 2
    batch = synth.nv12_batch(w, h, n, "D2", first_index=1000 + n)
    with mi_lumaeq.Context(0) as c:
        d_in = torch.from_numpy(batch.reshape(-1)).to("cuda:0")
        base = d_in.data_ptr()
        ins = [(base + k * fb, base + k * fb + w * h) for k in range(n)]
        for uv_mode in (UV_FILL128, UV_COPY):
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (0.0, 3, 5))):
                for k2 in ((0, 64) if op == "eq" else (8,)):
                    c.set_option("two_kernel_max_frames", k2)
                    want = torch.full_like(d_in, SENT)
                    got = torch.full_like(d_in, SENT)
                    ob = got.data_ptr()
                    outs = [(ob + k * fb, ob + k * fb + w * h) for k in range(n)]
                    if op == "eq":
                        c.equalize_hist_nv12_batch_dev(d_in, want, w, h, n, uv_mode, stream=stream())
                        c.equalize_hist_nv12_frames(ins, outs, w, h, uv_mode, stream=stream())
                    else:
                        c.clahe_nv12_batch_dev(d_in, want, w, h, n, uv_mode, *cfg, stream=stream())
                        c.clahe_nv12_frames(ins, outs, w, h, uv_mode, *cfg, stream=stream())
                    torch.cuda.synchronize()
                    assert torch.equal(got, want), (n, op, cfg, uv_mode, k2)
                    # and the batch form is right: spot-check the first and the last frame against the oracle
                    g = got.cpu().numpy().reshape(n, fb)
                    for k in {0, n - 1}:
                        y, uv = split(batch[k], w, h)
                        assert np.array_equal(g[k], np.concatenate([y_ref(y, op, cfg).reshape(-1), uv_ref(uv, uv_mode).reshape(-1)]))
        c.set_option("two_kernel_max_frames", 8)


def test_batch_sizes_on_surfaces():
    """130 separate surfaces (three chunks) in one call, both equalize paths."""
    w, h, n = 256, 144, 130
    frames, srcs, dsts = surfaces(w, h, n, 16, first=2000, pitch_align=64)
    with mi_lumaeq.Context(0) as c:
        for k2 in (0, 64):
            c.set_option("two_kernel_max_frames", k2)
            run(c, "eq", [s.planes() for s in srcs], [d.planes() for d in dsts], w, h, UV_COPY)
            check_surfaces(srcs, dsts, frames, w, h, "eq", UV_COPY, why=("k2", k2))
        run(c, "clahe", [s.planes() for s in srcs], [d.planes() for d in dsts], w, h, UV_FILL128, (3.0, 4, 4))
        check_surfaces(srcs, dsts, frames, w, h, "clahe", UV_FILL128, (3.0, 4, 4))


@pytest.mark.parametrize("w,h,pad", [(646, 362, 3), (1918, 1080, 9), (66, 34, 1)])
def test_unaligned_planes_and_in_place(w, h, pad):
    """Plane pointers offset by 1..15 bytes and pitches that are not multiples of 16; in place equals out of place."""
    n = 5
    pitch = w + pad
    frames = [synth.nv12_frame(w, h, DISTS[k], 3000 + k) for k in range(n)]
    srcs = [Surface(w, h, pitch, h + 2 * k, off=1 + (3 * k) % 15).fill(frames[k]) for k in range(n)]
    dsts = [Surface(w, h, pitch + 2, h + 4, off=15 - k) for k in range(n)]
    with mi_lumaeq.Context(0) as c:
        for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (2.0, 64, 2))):
            for uv_mode in (UV_FILL128, UV_COPY):
                for k2 in ((0, 8) if op == "eq" else (8,)):
                    c.set_option("two_kernel_max_frames", k2)
                    run(c, op, [s.planes() for s in srcs], [d.planes() for d in dsts], w, h, uv_mode, cfg)
                    check_surfaces(srcs, dsts, frames, w, h, op, uv_mode, cfg, why=("out of place", k2))
                    io = [Surface(w, h, pitch, h + 2 * k, off=1 + (3 * k) % 15).fill(frames[k]) for k in range(n)]
                    run(c, op, [s.planes() for s in io], None, w, h, uv_mode, cfg)
                    torch.cuda.synchronize()
                    for k in range(n):                        # in place: the same pixels as out of place, sentinels kept
                        want = io[k].expected(dsts[k].y.cpu().numpy(), dsts[k].uv.cpu().numpy())
                        assert np.array_equal(io[k].buf.cpu().numpy(), want), ("in place", op, cfg, uv_mode, k)
        c.set_option("two_kernel_max_frames", 8)


def test_full_size_4k():
    """Sixteen 4K frames of D1..D5 content on separate pitched surfaces (vertical stride 2176)."""
    w, h, n = 3840, 2160, 16
    frames, srcs, dsts = surfaces(w, h, n, 64, first=4000)
    ins, outs = [s.planes() for s in srcs], [d.planes() for d in dsts]
    with mi_lumaeq.Context(0) as c:
        run(c, "eq", ins, outs, w, h, UV_COPY)
        check_surfaces(srcs, dsts, frames, w, h, "eq", UV_COPY)
        run(c, "clahe", ins, outs, w, h, UV_FILL128, (2.0, 8, 8))
        check_surfaces(srcs, dsts, frames, w, h, "clahe", UV_FILL128, (2.0, 8, 8))


def test_argument_errors_write_nothing():
    w, h = 64, 32
    frames, srcs, dsts = surfaces(w, h, 2, 16, first=5000, pitch_align=128)
    s0, d0 = srcs[0], dsts[0]
    P = mi_lumaeq.Nv12FrameDev
    y_in, uv_in, y_out, uv_out = (s0.y.data_ptr(), s0.uv.data_ptr(), d0.y.data_ptr(), d0.uv.data_ptr())
    pitch = s0.pitch
    with mi_lumaeq.Context(0) as c:
        L, hc, st = c._L, c._h, stream()

        def eq(fr, n=None, ww=w, hh=h, p=(pitch, pitch, pitch, pitch), uv=UV_COPY):
            arr = (P * max(1, len(fr)))(*fr)
            return L.mi_equalize_hist_nv12_frames_dev(hc, arr if fr else None, len(fr) if n is None else n, ww, hh, *p, uv, st)

        def cl(fr, tx=8, ty=8, **kw):
            arr = (P * max(1, len(fr)))(*fr)
            p = kw.get("p", (pitch,) * 4)
            return L.mi_clahe_nv12_frames_dev(hc, arr, len(fr), w, h, *p, kw.get("uv", UV_COPY), 2.0, tx, ty, st)

        good = P(y_in, uv_in, y_out, uv_out)
        assert L.mi_equalize_hist_nv12_frames_dev(None, (P * 1)(good), 1, w, h, pitch, pitch, pitch, pitch, UV_COPY, st) == BAD_ARG
        assert eq([], n=1) == BAD_ARG                                  # null list, n > 0
        assert eq([good], n=-1) == BAD_ARG
        assert eq([good], ww=63) == BAD_ARG and eq([good], hh=31) == BAD_ARG
        for k in range(4):                                             # each pitch < W
            p = [pitch] * 4
            p[k] = w - 2
            assert eq([good], p=tuple(p)) == BAD_ARG, k
        assert eq([good, P(None, uv_in, y_out, uv_out)]) == BAD_ARG   # null Y planes, in any frame
        assert eq([P(y_in, uv_in, None, uv_out)]) == BAD_ARG
        assert eq([P(y_in, uv_in, y_out, None)]) == BAD_ARG            # null uv_out
        assert eq([P(y_in, None, y_out, uv_out)]) == BAD_ARG           # null uv_in with MI_UV_COPY ...
        assert eq([P(y_in, uv_in, y_in + 1, uv_out)]) == BAD_ARG       # partial overlaps of an output with an input plane
        assert eq([P(y_in, uv_in, y_out, uv_in + 16)]) == BAD_ARG
        assert eq([P(y_in, uv_in, y_out, y_in + pitch)]) == BAD_ARG    # uv_out over Y in
        assert eq([P(y_in, uv_in, uv_in, uv_out)]) == BAD_ARG          # y_out over UV in (copy)
        assert eq([P(y_in, uv_in, y_in, uv_out)], p=(pitch, pitch, pitch + 2, pitch)) == BAD_ARG   # "in place" at another pitch
        assert eq([good], uv=7) == BAD_ARG
        assert cl([good], tx=0) == BAD_ARG and cl([good], ty=-1) == BAD_ARG
        torch.cuda.synchronize()
        for s, d, f in zip(srcs, dsts, frames):
            y, uv = split(f, w, h)
            assert np.array_equal(s.buf.cpu().numpy(), s.expected(y, uv))
            assert np.array_equal(d.buf.cpu().numpy(), np.full(d.total, SENT, np.uint8)), "a refused call wrote"
        # MI_UV_FILL128 reads no chroma: a null uv_in is fine; zero sizes / no frames are MI_OK and write nothing
        assert eq([], n=0) == 0 and eq([good], ww=0) == 0 and eq([good], hh=0) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d0.buf.cpu().numpy(), np.full(d0.total, SENT, np.uint8))
        assert eq([P(y_in, None, y_out, uv_out)], uv=UV_FILL128) == 0
        check_surfaces(srcs[:1], dsts[:1], frames[:1], w, h, "eq", UV_FILL128)


def test_stream_graph_and_profiling():
    """A non-default torch stream; one torch.cuda.graph capture after an eager call, replayed on new pixels; with profiling on the
    launches land in the existing slots."""
    w, h, n = 1280, 720, 6
    frames, srcs, dsts = surfaces(w, h, n, 16, first=6000)
    ins, outs = [s.planes() for s in srcs], [d.planes() for d in dsts]
    with mi_lumaeq.Context(0) as c:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            run(c, "clahe", ins, outs, w, h, UV_COPY, (2.0, 8, 8), stream=side.cuda_stream)
        side.synchronize()
        check_surfaces(srcs, dsts, frames, w, h, "clahe", UV_COPY, why="side stream")

        run(c, "eq", ins, outs, w, h, UV_FILL128)                     # eager call of the captured shape sizes the scratch
        run(c, "clahe", ins, outs, w, h, UV_FILL128, (3.0, 4, 4))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run(c, "clahe", ins, outs, w, h, UV_FILL128, (3.0, 4, 4), stream=torch.cuda.current_stream().cuda_stream)
        fresh = [synth.nv12_frame(w, h, DISTS[(k + 2) % 5], 6100 + k) for k in range(n)]
        for s, f in zip(srcs, fresh):
            s.fill(f)
        for d in dsts:
            d.buf.fill_(SENT)
        g.replay()
        check_surfaces(srcs, dsts, fresh, w, h, "clahe", UV_FILL128, (3.0, 4, 4), why="graph replay")

        c.set_profiling(1)
        c.profile_read(reset=True)
        c.set_option("two_kernel_max_frames", 0)
        run(c, "eq", ins, outs, w, h, UV_COPY)
        run(c, "clahe", ins, outs, w, h, UV_COPY, (2.0, 8, 8))
        run(c, "clahe", ins, outs, w, h, UV_COPY, (2.0, 64, 2))
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
        c.set_profiling(0)
        c.set_option("two_kernel_max_frames", 8)
        assert len(prof) == 10
        for k, want in (("hist_partial_kernel", 1), ("equalize_lut_kernel", 1), ("lut_apply_kernel", 2), ("tile_hist_kernel", 2),
                        ("clahe_interp_kernel", 2)):
            assert prof[k]["launches"] == want, (k, prof[k])
        assert prof["equalize_fused_kernel"]["launches"] == 0
