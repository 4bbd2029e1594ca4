"""CLAHE on 16-bit 4:2:0 video frames (P010 / P012 / P016) on the GPU: the batched device form, the host form, the pipe, hipGraph
capture, argument errors and the stream demo.  Every comparison is bytes against a reference built here: oracle.clahe16 (OpenCV's
CLAHE on CV_16UC1, restated in C) on the Y view of each frame, plus the chroma rule applied in numpy (fill: every sample 0x8000;
copy: the input's chroma)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY, FMT_P010, OP_CLAHE, OP_EQUALIZE, OP_CHANNELS, PIPE_UV_HOST, PIPE_UV_DEVICE

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
CONFIGS = [(2.0, 8, 8), (3.0, 4, 4), (0.0, 3, 5)]


def letterboxed(w, h, frame_index):
    """P010 content with black bars (64 << 6) over the top and bottom eighth of the picture."""
    f = synth.p010_frame(w, h, "p010", frame_index)
    bar = max(2, h // 8)
    f[:bar] = 64 << 6
    f[h - bar:h] = 64 << 6
    return f


def batch(w, h, kinds, first=0):
    out = []
    for k, kind in enumerate(kinds):
        out.append(letterboxed(w, h, first + k) if kind == "bars" else synth.p010_frame(w, h, kind, first + k))
    return np.stack(out)


def luma_ref(frames, h, clip, tx, ty):
    return np.stack([oracle.clahe16(np.ascontiguousarray(f[:h]), clip, tx, ty) for f in frames])


def reference(frames, h, uv_mode, yref):
    out = frames.copy()
    out[:, :h] = yref
    if uv_mode == UV_FILL128:
        out[:, h:] = 0x8000
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda:0")


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_batch_variants(c, frames, w, h, clip, tx, ty, yref):
    """Both UV modes, out of place and in place; every output compared with the reference."""
    n = frames.shape[0]
    d_in = dev(frames)
    for uv in (UV_FILL128, UV_COPY):
        want = reference(frames, h, uv, yref)
        d_out = torch.full_like(d_in, 0xA5)
        c.clahe_p010_batch_dev(d_in, d_out, w, h, n, uv, clip, tx, ty, stream=stream())
        torch.cuda.synchronize()
        got = host16(d_out)
        assert np.array_equal(got, want), ("out of place", w, h, uv, clip, tx, ty,
                                           [k for k in range(n) if not np.array_equal(got[k], want[k])])
        d_io = d_in.clone()
        c.clahe_p010_batch_dev(d_io, d_io, w, h, n, uv, clip, tx, ty, stream=stream())
        torch.cuda.synchronize()
        got = host16(d_io)
        assert np.array_equal(got, want), ("in place", w, h, uv, clip, tx, ty,
                                           [k for k in range(n) if not np.array_equal(got[k], want[k])])
    assert np.array_equal(host16(d_in), frames), "the input of an out-of-place call was written"


@pytest.mark.parametrize("clip,tx,ty", CONFIGS)
def test_batch_4k_16_frames(clip, tx, ty):
    w, h = 3840, 2160
    frames = batch(w, h, ["p010"] * 11 + ["p012"] * 3 + ["p016", "bars"], first=100)
    yref = luma_ref(frames, h, clip, tx, ty)
    with mi_lumaeq.Context(0) as c:
        run_batch_variants(c, frames, w, h, clip, tx, ty, yref)


@pytest.mark.parametrize("clip,tx,ty", CONFIGS)
def test_batch_1080p(clip, tx, ty):
    w, h = 1920, 1080
    frames = batch(w, h, ["p010", "p012", "p016", "bars", "p010"], first=200)
    yref = luma_ref(frames, h, clip, tx, ty)
    with mi_lumaeq.Context(0) as c:
        run_batch_variants(c, frames, w, h, clip, tx, ty, yref)


@pytest.mark.parametrize("w,h", [(1918, 1078), (66, 34)])
@pytest.mark.parametrize("clip,tx,ty", [(2.0, 8, 8), (0.0, 3, 5)])
def test_batch_unaligned_geometry(w, h, clip, tx, ty):
    """Even sizes that need tile padding and put each frame's chroma (and every frame after the first) at an offset that is not
    16-byte aligned: the chroma kernel's unaligned head and tail, and the careful tile-histogram path."""
    assert (3 * w * h) % 16 and (2 * w * h) % 16
    frames = batch(w, h, ["p010", "p012", "bars"], first=300)
    yref = luma_ref(frames, h, clip, tx, ty)
    with mi_lumaeq.Context(0) as c:
        run_batch_variants(c, frames, w, h, clip, tx, ty, yref)


@pytest.mark.parametrize("w,h", [(1920, 1080), (1918, 1078)])
def test_luma_equals_u16_path(w, h):
    """The luma of a P010 call is, byte for byte, what mi_clahe_u16_batch_dev writes on the same Y planes (pitch 2W, frame stride 3WH)."""
    n = 3
    frames = batch(w, h, ["p012", "p010", "bars"], first=400)
    fstride = 3 * w * h
    with mi_lumaeq.Context(0) as c:
        d_in = dev(frames)
        d_p010 = torch.zeros_like(d_in)
        d_u16 = torch.zeros_like(d_in)
        c.clahe_p010_batch_dev(d_in, d_p010, w, h, n, UV_COPY, 2.0, 8, 8, stream=stream())
        c._chk(c._L.mi_clahe_u16_batch_dev(c._h, d_in.data_ptr(), 2 * w, fstride, d_u16.data_ptr(), 2 * w, fstride, w, h, n,
                                           2.0, 8, 8, stream()), "mi_clahe_u16_batch_dev")
        torch.cuda.synchronize()
        a, b = host16(d_p010), host16(d_u16)
        assert np.array_equal(a[:, :h], b[:, :h])
        assert np.array_equal(a[:, h:], frames[:, h:])


@pytest.mark.parametrize("w,h", [(1920, 1080), (66, 34)])
def test_host_form(w, h):
    """mi_clahe_p010 on an unpinned frame, on a frame registered with mi_host_register, and in place."""
    frame = synth.p010_frame(w, h, "p010", 500)
    yref = luma_ref(frame[None], h, 2.0, 8, 8)
    with mi_lumaeq.Context(0) as c:
        for uv in (UV_FILL128, UV_COPY):
            want = reference(frame[None], h, uv, yref)[0]
            got = c.clahe_p010(frame, w, h, uv, 2.0, 8, 8)
            assert np.array_equal(got, want), ("unpinned", uv)
            reg_in, reg_out = frame.copy(), np.zeros_like(frame)
            mi_lumaeq.host_register(reg_in)
            mi_lumaeq.host_register(reg_out)
            try:
                c.clahe_p010(reg_in, w, h, uv, 2.0, 8, 8, out=reg_out)
                assert np.array_equal(reg_out, want), ("registered", uv)
                c.clahe_p010(reg_in, w, h, uv, 2.0, 8, 8, out=reg_in)
                assert np.array_equal(reg_in, want), ("registered in place", uv)
            finally:
                mi_lumaeq.host_unregister(reg_in)
                mi_lumaeq.host_unregister(reg_out)
            io = frame.copy()
            c.clahe_p010(io, w, h, uv, 2.0, 8, 8, out=io)
            assert np.array_equal(io, want), ("in place", uv)


@pytest.mark.parametrize("uv_policy", [PIPE_UV_HOST, PIPE_UV_DEVICE])
@pytest.mark.parametrize("uv", [UV_FILL128, UV_COPY])
def test_pipe_p010(uv_policy, uv):
    w, h, n = 1280, 720, 7
    frames = batch(w, h, ["p010", "p012", "bars", "p016", "p010", "p010", "p012"], first=600)
    yref = luma_ref(frames, h, 3.0, 4, 4)
    want = reference(frames, h, uv, yref)
    outs = [np.zeros_like(frames[0]) for _ in range(n)]
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, op=OP_CLAHE, uv_mode=uv, clip_limit=3.0, tiles_x=4, tiles_y=4, depth=3, uv_policy=uv_policy,
                            format=FMT_P010) as pipe:
            assert pipe.frame_bytes == 3 * w * h
            done, k = [], 0
            while len(done) < n:
                while k < n and pipe.submit(frames[k], outs[k], 1000 + k):
                    k += 1
                tag, out = pipe.wait()
                done.append(tag)
                assert out is outs[tag - 1000]
            assert done == [1000 + i for i in range(n)], done
    for i in range(n):
        assert np.array_equal(outs[i], want[i]), (uv_policy, uv, i)


def test_pipe_p010_errors():
    with mi_lumaeq.Context(0) as c:
        for op in (OP_EQUALIZE, OP_CHANNELS):
            with pytest.raises(mi_lumaeq.MiError) as e:
                mi_lumaeq.Pipe(c, 64, 32, op=op, format=FMT_P010)
            assert e.value.status == UNSUPPORTED, op
        with pytest.raises(mi_lumaeq.MiError) as e:
            mi_lumaeq.Pipe(c, 65, 32, op=OP_CLAHE, format=FMT_P010)
        assert e.value.status == BAD_ARG
        with pytest.raises(mi_lumaeq.MiError) as e:
            mi_lumaeq.Pipe(c, 64, 32, op=OP_CLAHE, format=7)
        assert e.value.status == BAD_ARG
        # the context is still usable: a P010 pipe opens after the refusals
        with mi_lumaeq.Pipe(c, 64, 32, op=OP_CLAHE, format=FMT_P010) as pipe:
            f = synth.p010_frame(64, 32, "p010", 1)
            o = np.zeros_like(f)
            assert pipe.submit(f, o, 1)
            assert pipe.wait()[0] == 1
        assert np.array_equal(o, reference(f[None], 32, UV_FILL128, luma_ref(f[None], 32, 2.0, 8, 8))[0])


def test_hip_graph_capture_and_replay_p010():
    """The batched P010 form is captured after one eager call of the same shape and replayed on new data."""
    w, h, n = 1920, 1080, 4
    with mi_lumaeq.Context(0) as c:
        first = batch(w, h, ["p010"] * n, first=700)
        d_in = dev(first)
        d_out = torch.zeros_like(d_in)
        c.clahe_p010_batch_dev(d_in, d_out, w, h, n, UV_COPY, 2.0, 8, 8, stream=stream())    # warm-up: sizes the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.clahe_p010_batch_dev(d_in, d_out, w, h, n, UV_COPY, 2.0, 8, 8, stream=torch.cuda.current_stream().cuda_stream)
        for rep, kinds in enumerate((["p012"] * n, ["bars", "p010", "p016", "p012"])):
            frames = batch(w, h, kinds, first=800 + 10 * rep)
            d_in.copy_(dev(frames))
            d_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            want = reference(frames, h, UV_COPY, luma_ref(frames, h, 2.0, 8, 8))
            assert np.array_equal(host16(d_out), want), rep
        # eager calls on the same context keep working after replays
        c.clahe_p010_batch_dev(d_in, d_out, w, h, n, UV_FILL128, 2.0, 8, 8, stream=stream())
        torch.cuda.synchronize()
        frames = host16(d_in)
        assert np.array_equal(host16(d_out), reference(frames, h, UV_FILL128, luma_ref(frames, h, 2.0, 8, 8)))


def test_argument_errors():
    w, h = 64, 32
    frame = synth.p010_frame(w, h, "p010", 900)
    with mi_lumaeq.Context(0) as c:
        L, hc = c._L, c._h
        d = dev(np.concatenate([frame.reshape(-1), np.zeros(64, np.uint16)]))
        p = d.data_ptr()
        s = stream()

        def bd(ptr_in, ptr_out, ww, hh, n=1, uv=UV_COPY, tx=8, ty=8):
            return L.mi_clahe_p010_batch_dev(hc, ptr_in, ptr_out, ww, hh, n, uv, 2.0, tx, ty, s)

        def hf(a_in, a_out, ww, hh, uv=UV_COPY, tx=8, ty=8):
            return L.mi_clahe_p010(hc, a_in, a_out, ww, hh, uv, 2.0, tx, ty)
        buf = np.zeros(4096, np.uint16)
        hp = buf.ctypes.data
        for f in (bd, hf):
            ptr = p if f is bd else hp
            assert f(ptr, ptr, 63, 32) == BAD_ARG, f           # odd width
            assert f(ptr, ptr, 64, 31) == BAD_ARG, f           # odd height
            assert f(None, ptr, 64, 32) == BAD_ARG, f          # null input
            assert f(ptr, None, 64, 32) == BAD_ARG, f          # null output
            assert f(ptr + 1, ptr + 1, 64, 32) == BAD_ARG, f   # not 2-byte aligned
            assert f(ptr, ptr + 1, 64, 32) == BAD_ARG, f
            assert f(ptr, ptr, 64, 32, tx=0) == BAD_ARG, f     # tiles <= 0
            assert f(ptr, ptr, 64, 32, ty=-1) == BAD_ARG, f
            assert f(ptr, ptr, 64, 32, uv=2) == BAD_ARG, f     # no such UV mode
            assert f(None, None, 0, 32) == 0, f                # zero sizes: no-op
            assert f(None, None, 64, 0) == 0, f
            assert f(ptr, ptr, 65536, 16386) == UNSUPPORTED, f  # W*H beyond what the 16-bit path accepts (checked before any access)
        assert bd(None, None, 64, 32, n=0) == 0
        assert bd(p, p, 64, 32, n=-1) == BAD_ARG
        torch.cuda.synchronize()
        assert np.array_equal(host16(d)[: frame.size].reshape(frame.shape), frame), "a refused call wrote the frame"
        assert not buf.any(), "a refused host call wrote the frame"


def _demo():
    exe = ROOT / "opencv-opencl_amd" / "lib" / "nv12_stream"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT / "opencv-opencl_amd" / "cxx")], check=True)
    return exe


def test_stream_demo_p010_file_io(tmp_path):
    """nv12_stream --format p010 --op clahe: raw P010 files in and out, every output frame equals the reference, in order."""
    exe = _demo()
    w, h, n = 320, 180, 7
    frames = batch(w, h, ["p010", "p012", "bars", "p016", "p010", "p012", "p010"], first=1000)
    src = tmp_path / "in.p010"
    src.write_bytes(frames.tobytes())
    yref = luma_ref(frames, h, 3.0, 4, 4)
    for uv, args in (("copy", []), ("fill128", ["--uv-policy", "device", "--depth", "3"]), ("copy", ["--uv-policy", "device", "--no-pin"])):
        dst = tmp_path / f"out_{uv}.p010"
        r = subprocess.run([str(exe), "--format", "p010", "--op", "clahe", "--input", str(src), "--output", str(dst), "--width", str(w),
                            "--height", str(h), "--frames", str(n), "--workers", "2", "--uv", uv, "--clipLimit", "3.0", "--tile", "4"] + args,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.frombuffer(dst.read_bytes(), np.uint16).reshape(frames.shape)
        want = reference(frames, h, UV_COPY if uv == "copy" else UV_FILL128, yref)
        for k in range(n):
            assert np.array_equal(out[k], want[k]), (uv, args, k)


def test_stream_demo_p010_refuses_equalize():
    exe = _demo()
    for op in ("equalize", "channels"):
        r = subprocess.run([str(exe), "--format", "p010", "--op", op, "--width", "64", "--height", "32", "--frames", "2"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0, op
        assert "clahe" in r.stderr, r.stderr
