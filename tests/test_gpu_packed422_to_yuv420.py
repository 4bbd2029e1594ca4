"""Packed 4:2:2 frames in (YUY2 / UYVY), planar 4:2:0 frames out (I420 / YV12) on the GPU: mi_equalize_hist_packed422_to_yuv420_batch_dev
and mi_clahe_packed422_to_yuv420_batch_dev.  The expected Y plane is oracle.equalize_hist / oracle.clahe on the gathered luma; the
expected U and V planes are the even and the odd columns of the row-pair rounding mean (a + b + 1) >> 1 of the input chroma
(MI_UV_COPY), or 128 (MI_UV_FILL128).  Every output lives in sentinel-filled allocations with 64 guard bytes and the WHOLE allocation
is compared: every comparison in this file is exact bytes.  The shapes are the smallest at which the writer's walks repeat or change
path: ragged groups of 7 and of 1 macropixels, rows shorter than a group, two apply steps, apply bands without a row pair, a band
boundary through a row pair, the wide-grid kernel."""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
import test_gpu_packed422_to_nv12 as nv                 # helpers only: Batch, Nv12Out, the oracle's planes, the planar form's status
from mi_lumaeq import UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY
from mi_lumaeq.capi import Yuv420Planes, CHROMA_INTERLEAVED, CHROMA_PLANAR

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = nv.SENT
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]
WIDE = (2.0, 64, 2)                                      # tiles_x + 1 pairs do not fit the LDS table: the wide-grid kernel
align4 = nv.align4
stream = nv.stream


def up16(x):
    return (x + 15) & ~15


def expected_planes(frame, w, fmt, op, cfg, uv_mode, key=None):
    """(Y, U, V) as the header states them."""
    h = frame.shape[0]
    if uv_mode == UV_COPY:
        uv = nv.uv_mean(nv.chroma(frame, w, fmt))
        u, v = uv[:, 0::2], uv[:, 1::2]
    else:
        u = v = np.full((h // 2, w // 2), 128, np.uint8)
    return nv.y_ref(nv.luma(frame, w, fmt), op, cfg, key), u, v


class PlanarOut:
    """n planar 4:2:0 frames in sentinel-filled allocations with 64 guard bytes behind the last byte a frame may touch.
    kind: "one"  one allocation, Y then U then V, every plane at its own phase modulo 16;
          "yv12" the same with V's address below U's;
          "side" one allocation, Y then ONE chroma plane of pitch W whose rows hold a U row and a V row side by side;
          "own"  three allocations."""

    def __init__(self, w, h, n, kind="one", y_off=4, ye=4, ce=4, phases=(8, 4)):
        self.w, self.h, self.n, self.kind = w, h, n, kind
        self.y_pitch = align4(w) + ye
        self.c_pitch = w if kind == "side" else align4(w // 2) + ce
        assert self.y_pitch % 4 == 0 and self.c_pitch % 4 == 0
        ysz, csz = self.y_pitch * h, self.c_pitch * (h // 2)
        pa, pb = phases
        if kind == "own":
            self.fstride = max(ysz, csz) + 12
            sizes = [y_off + self.fstride * n + 64, pa + self.fstride * n + 64, pb + self.fstride * n + 64]
            self.at = {"y": (0, y_off), "u": (1, pa), "v": (2, pb)}
        elif kind == "side":
            c_at = up16(y_off + ysz) + pa
            self.fstride = up16(c_at + csz - y_off) + 4
            sizes = [y_off + self.fstride * n + 64]
            self.at = {"y": (0, y_off), "u": (0, c_at), "v": (0, c_at + w // 2)}
        else:
            a_at = up16(y_off + ysz) + pa
            b_at = up16(a_at + csz) + pb
            self.fstride = up16(b_at + csz - y_off) + 4
            sizes = [y_off + self.fstride * n + 64]
            first, second = ("u", "v") if kind == "one" else ("v", "u")
            self.at = {"y": (0, y_off), first: (0, a_at), second: (0, b_at)}
        assert self.fstride % 4 == 0
        self.bufs = [torch.full((s,), SENT, dtype=torch.uint8, device="cuda:0") for s in sizes]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)

    def ptr(self, name):
        bi, o = self.at[name]
        return self.bufs[bi].data_ptr() + o

    def planes(self, chroma=CHROMA_PLANAR, **kw):
        f = dict(y=self.ptr("y"), y_pitch=self.y_pitch, c0=self.ptr("u"), c1=self.ptr("v"), c_pitch=self.c_pitch,
                 frame_stride=self.fstride, chroma=chroma)
        f.update(kw)
        return Yuv420Planes(f["y"], f["y_pitch"], f["c0"], f["c1"], f["c_pitch"], f["frame_stride"], f["chroma"])

    def image(self, planes=None):
        """The allocations as they must read with `planes` = [(Y, U, V), ...] in them (None: untouched)."""
        imgs = [np.full(b.numel(), SENT, np.uint8) for b in self.bufs]
        if planes is not None:
            for k, (y, u, v) in enumerate(planes):
                for name, pitch, rows, cols, pl in (("y", self.y_pitch, self.h, self.w, y), ("u", self.c_pitch, self.h // 2, self.w // 2, u),
                                                    ("v", self.c_pitch, self.h // 2, self.w // 2, v)):
                    bi, o = self.at[name]
                    o += k * self.fstride
                    np.lib.stride_tricks.as_strided(imgs[bi][o:], shape=(rows, cols), strides=(pitch, 1))[:] = pl
        return imgs

    def clear(self):
        for b in self.bufs:
            b.fill_(SENT)

    def host(self):
        return [b.cpu().numpy() for b in self.bufs]

    def same(self, planes=None):
        return all(np.array_equal(g, w) for g, w in zip(self.host(), self.image(planes)))

    def plane(self, name, k):
        """Plane `name` of frame k as the device holds it, tight."""
        bi, o = self.at[name]
        pitch, rows, cols = (self.y_pitch, self.h, self.w) if name == "y" else (self.c_pitch, self.h // 2, self.w // 2)
        a = self.bufs[bi].cpu().numpy()
        return np.lib.stride_tricks.as_strided(a[o + k * self.fstride:], shape=(rows, cols), strides=(pitch, 1)).copy()


def run(c, op, cfg, src, planes, fmt, uv_mode, n=None, st=None):
    kw = dict(src.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if op == "eq":
        c.equalize_hist_packed422_to_yuv420_batch_dev(src.dev, planes, src.w, src.h, n, fmt, uv_mode, **kw)
    else:
        c.clahe_packed422_to_yuv420_batch_dev(src.dev, planes, src.w, src.h, n, fmt, uv_mode, *cfg, **kw)


def check_case(c, frames, w, h, fmt, uv_mode, op, cfg, dst, in_layout, key):
    """One call into `dst`, the whole of every allocation compared; the planar form must accept the size / grid pair."""
    assert nv.planar_status(c, w, h, len(frames), op, cfg) == 0, (w, h, op, cfg)
    src = nv.Batch(w, h, len(frames), in_layout).upload(frames)
    dst.clear()
    run(c, op, cfg, src, dst.planes(), fmt, uv_mode)
    torch.cuda.synchronize()
    want = dst.image([expected_planes(f, w, fmt, op, cfg, uv_mode, (key, k, fmt)) for k, f in enumerate(frames)])
    for bi, (got, wnt) in enumerate(zip(dst.host(), want)):
        assert np.array_equal(got, wnt), (w, h, fmt, uv_mode, op, cfg, dst.kind, bi, int((got != wnt).sum()), np.flatnonzero(got != wnt)[:8])
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


# ---- 1. 40 x 6, two frames: every phase of the Y base, a band boundary through a row pair, the wide-grid kernel, REFLECT_101 ------------
@pytest.mark.parametrize("y_off", [4, 8, 12])
def test_40x6_phases_and_bands(c, y_off):
    """Y bases 4, 8 and 12 past a 16-byte boundary, U and V at phases of their own.  CLAHE (2.0, 2, 2) has tile height 3: a band
    boundary cuts the row pair (2, 3).  (2.0, 64, 2) takes the wide-grid kernel.  (0.0, 3, 5) does not divide the frame."""
    w, h, n = 40, 6, 2
    for fmt in FMTS:
        frames = nv.make_frames(w, h, fmt, ["D1", "D3"], 300)
        for uv_mode in UVS:
            for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", WIDE), ("clahe", (0.0, 3, 5))):
                dst = PlanarOut(w, h, n, "one", y_off=y_off, phases=((y_off + 4) % 16, (y_off + 8) % 16))
                check_case(c, frames, w, h, fmt, uv_mode, op, cfg, dst, nv.LAYOUTS[y_off // 4 - 1], ("40x6", w, h))


# ---- 2. ragged groups, two apply steps, rows shorter than a group, bands without a pair --------------------------------------------------
@pytest.mark.parametrize("w,h", [(62, 200), (66, 200), (64, 200), (2, 2), (6, 2), (16386, 2)])
def test_group_tails_steps_and_bands(c, w, h):
    """62 x 200: a ragged group of 7 macropixels (dword + 2-byte + byte chroma tail).  66 x 200: a ragged group of 1 (a single byte),
    500 apply items.  64 x 200: 400 items, two steps.  2 x 2, 6 x 2: rows shorter than one group.  16386 x 2: G = 1025, five steps,
    apply bands without a row pair; pitches padded to multiples of 4."""
    grids = {2: [(2.0, 1, 1), (2.0, 64, 1)], 200: [(2.0, 4, 4), WIDE]}[h]
    for fmt in FMTS:
        frames = nv.make_frames(w, h, fmt, ["D2"], 400 + w)
        for uv_mode in UVS:
            for op, cfg in [("eq", None)] + [("clahe", g) for g in grids]:
                dst = PlanarOut(w, h, 1, "one", y_off=8, ye=0, ce=0, phases=(4, 12))
                check_case(c, frames, w, h, fmt, uv_mode, op, cfg, dst, nv.LAYOUTS[1], ("tails", w, h))


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["side", "yv12", "own"])
def test_layouts(c, kind):
    """U and V rows side by side in one pitched plane (c1 = c0 + W/2, c_pitch = W), YV12 order (V's address below U's), three
    separate allocations."""
    w, h, n = 64, 8, 2
    for fmt in FMTS:
        frames = nv.make_frames(w, h, fmt, ["D4", "D5"], 500)
        for uv_mode in UVS:
            for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", WIDE)):
                dst = PlanarOut(w, h, n, kind)
                if kind == "side":
                    assert dst.ptr("v") == dst.ptr("u") + w // 2 and dst.c_pitch == w
                if kind == "yv12":
                    assert dst.ptr("v") < dst.ptr("u")
                check_case(c, frames, w, h, fmt, uv_mode, op, cfg, dst, nv.LAYOUTS[0], ("layouts", w, h))


# ---- 4. identity with the NV12 form, both arithmetic modes ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(40, 6), (62, 200), (64, 200)])
def test_sibling_identity_and_fp_contract(c, w, h):
    """Y is the Y plane of mi_*_packed422_to_nv12_batch_dev on the same input, U / V its UV plane de-interleaved, in both
    clahe_fp_contract modes."""
    n = 2
    try:
        for fmt in FMTS:
            frames = nv.make_frames(w, h, fmt, ["D1", "D2"], 600 + w)
            src = nv.Batch(w, h, n, nv.LAYOUTS[2]).upload(frames)
            for contract in (0, 1):
                c.set_option("clahe_fp_contract", contract)
                for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", (3.0, 4, 3)), ("clahe", WIDE)):
                    ref = nv.Nv12Out(w, h, n, nv.OUT_LAYOUTS[0])
                    dst = PlanarOut(w, h, n, "one")
                    nv.run(c, op, cfg, src, ref, fmt, UV_COPY)
                    run(c, op, cfg, src, dst.planes(), fmt, UV_COPY)
                    torch.cuda.synchronize()
                    a = ref.host()[0]
                    planes = []
                    for k in range(n):
                        yo = ref.y_at[1] + k * ref.fstride
                        uo = ref.uv_at[1] + k * ref.fstride
                        y = a[yo: yo + ref.y_pitch * h].reshape(h, ref.y_pitch)[:, :w]
                        uv = a[uo: uo + ref.uv_pitch * (h // 2)].reshape(h // 2, ref.uv_pitch)[:, :w]
                        planes.append((y, uv[:, 0::2], uv[:, 1::2]))
                    assert dst.same(planes), (w, h, fmt, contract, op, cfg)
    finally:
        c.set_option("clahe_fp_contract", 0)


# ---- 5. interleaved output and launch accounting ----------------------------------------------------------------------------------------
def launches(c):
    prof = c.profile_read(reset=True)
    return {k: prof[k]["launches"] for k in mi_lumaeq.KERNEL_NAMES}


def test_interleaved_output_is_the_nv12_form():
    """MI_CHROMA_INTERLEAVED: the whole output allocation equals the NV12 form's and so do the launch counts; c1 is ignored."""
    w, h, n = 40, 6, 2
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for fmt in FMTS:
            frames = nv.make_frames(w, h, fmt, ["D1", "D5"], 700)
            src = nv.Batch(w, h, n, nv.LAYOUTS[0]).upload(frames)
            for uv_mode in UVS:
                for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", WIDE)):
                    ref, dst = nv.Nv12Out(w, h, n, nv.OUT_LAYOUTS[1]), nv.Nv12Out(w, h, n, nv.OUT_LAYOUTS[1])
                    launches(c)
                    nv.run(c, op, cfg, src, ref, fmt, uv_mode)
                    torch.cuda.synchronize()
                    want_l = launches(c)
                    planes = Yuv420Planes(dst.y_ptr, dst.y_pitch, dst.uv_ptr, None, dst.uv_pitch, dst.fstride, CHROMA_INTERLEAVED)
                    run(c, op, cfg, src, planes, fmt, uv_mode)
                    torch.cuda.synchronize()
                    assert launches(c) == want_l, (fmt, uv_mode, op, cfg)
                    assert sum(want_l.values()) > 0
                    for g, r in zip(dst.host(), ref.host()):
                        assert np.array_equal(g, r), (fmt, uv_mode, op, cfg)
                    assert dst.same([nv.expected_planes(f, w, fmt, op, cfg, uv_mode) for f in frames])
        c.set_profiling(0)


def test_launch_counts_equal_the_nv12_forms():
    """Planar calls make exactly the launches the NV12 form makes, slot by slot: no chroma launch, never the fused kernel."""
    w, h, n = 64, 48, 3
    frames = nv.make_frames(w, h, FMT_YUY2, ["D1", "D2", "D3"], 1000)
    src = nv.Batch(w, h, n, nv.LAYOUTS[0]).upload(frames)
    ref = nv.Nv12Out(w, h, n, nv.OUT_LAYOUTS[0])
    dst = PlanarOut(w, h, n, "one")
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for uv_mode in UVS:
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", WIDE)):
                launches(c)
                nv.run(c, op, cfg, src, ref, FMT_YUY2, uv_mode)
                torch.cuda.synchronize()
                want = launches(c)
                run(c, op, cfg, src, dst.planes(), FMT_YUY2, uv_mode)
                torch.cuda.synchronize()
                got = launches(c)
                assert got == want, (uv_mode, op, cfg, got, want)
                if op == "eq":
                    for k in mi_lumaeq.KERNEL_NAMES:
                        assert got[k] == (1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0), (uv_mode, k)
                assert dst.same([expected_planes(f, w, FMT_YUY2, op, cfg, uv_mode) for f in frames])
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    w, h, n = 40, 6, 2
    frames = nv.make_frames(w, h, FMT_YUY2, ["D1", "D2"], 800)
    src = nv.Batch(w, h, n, nv.LAYOUTS[0]).upload(frames)
    dst = PlanarOut(w, h, n, "one")
    L, hd = c._L, c._h
    ip, yp, up, vp = src.dev.data_ptr(), dst.ptr("y"), dst.ptr("u"), dst.ptr("v")
    base = dict(i=ip, ipitch=src.pitch, ifs=src.fstride, w=w, h=h, n=n, fmt=FMT_YUY2, uvm=UV_COPY)
    PLANE_KEYS = ("y", "y_pitch", "c0", "c1", "c_pitch", "frame_stride", "chroma")

    def args(kw):
        a = dict(base)
        a.update({k: v for k, v in kw.items() if k not in PLANE_KEYS})
        planes = dst.planes(**{k: v for k, v in kw.items() if k in PLANE_KEYS})
        return planes, (hd, a["i"], a["ipitch"], a["ifs"], ctypes.byref(planes), a["w"], a["h"], a["n"], a["fmt"], a["uvm"])

    def eq(**kw):
        keep, a = args(kw)
        return L.mi_equalize_hist_packed422_to_yuv420_batch_dev(*a, stream())

    def cl(tx=2, ty=2, **kw):
        keep, a = args(kw)
        return L.mi_clahe_packed422_to_yuv420_batch_dev(*a, 2.0, tx, ty, stream())
    bad = [dict(i=None), dict(y=None), dict(c0=None), dict(c1=None),                               # null pointers, a null c1 on a planar output
           dict(w=39), dict(h=5), dict(w=39, h=5), dict(w=0, h=5), dict(n=0, h=5), dict(w=39, h=0), dict(w=39, n=0),   # odd sizes, also next to a 0
           dict(w=-2), dict(h=-2), dict(h=-1), dict(n=-1),                                          # negative sizes
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),           # format, uv_mode
           dict(ipitch=2 * w - 4), dict(y_pitch=w - 4), dict(c_pitch=w // 2 - 4),                   # pitches below their rows
           dict(i=ip + 2), dict(y=yp + 2), dict(c0=up + 2), dict(c1=vp + 1), dict(ipitch=2 * w + 2), dict(y_pitch=w + 2),
           dict(c_pitch=w // 2 + 2), dict(ifs=src.fstride + 2), dict(frame_stride=dst.fstride + 2),  # not multiples of 4
           dict(chroma=2), dict(chroma=-1),                                                         # a chroma other than the two values
           dict(c1=up), dict(c0=yp), dict(c1=yp),                                                   # two equal output plane pointers
           dict(y=ip), dict(c0=ip), dict(c1=ip), dict(c1=ip + src.pitch + 4), dict(y=ip + src.pitch * (h - 1) + 2 * w - 4),   # an output meets its input's rows
           dict(c0=yp + 4), dict(c1=yp + dst.y_pitch * (h - 1) + w - 4)]                            # Y meets a chroma plane
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    assert L.mi_equalize_hist_packed422_to_yuv420_batch_dev(hd, ip, src.pitch, src.fstride, None, w, h, n, FMT_YUY2, UV_COPY, stream()) == BAD_ARG
    for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
        assert cl(tx, ty) == BAD_ARG
    # the documented consequence: a tight 36 x 4 planar frame has a chroma pitch of 18, not a multiple of 4
    tight = dict(w=36, h=4, n=1, y_pitch=36, c_pitch=18, c0=yp + 36 * 4, c1=yp + 36 * 4 + 18 * 2, frame_stride=36 * 4 * 3 // 2)
    assert eq(**tight) == BAD_ARG and cl(**tight) == BAD_ARG
    # a grid the planar form refuses: its status
    big = (2.0, 2048, 1024)
    assert nv.planar_status(c, w, h, n, "clahe", big) == UNSUPPORTED
    assert cl(big[1], big[2]) == UNSUPPORTED
    # zero sizes: MI_OK, nothing written
    for kw in (dict(w=0), dict(h=0), dict(n=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    torch.cuda.synchronize()
    assert dst.same(), "a refused or empty call wrote"
    assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
    # the same 36-wide frames with a padded chroma pitch are accepted, and the context still works
    f36 = [np.ascontiguousarray(f[:4, :72]) for f in frames]
    src36 = nv.Batch(36, 4, n, nv.LAYOUTS[0]).upload(f36)
    dst36 = PlanarOut(36, 4, n, "one", ye=0, ce=0)
    assert dst36.c_pitch == 20
    run(c, "eq", None, src36, dst36.planes(), FMT_YUY2, UV_COPY)
    torch.cuda.synchronize()
    assert dst36.same([expected_planes(f, 36, FMT_YUY2, "eq", None, UV_COPY) for f in f36])
    assert dst.same(), "a call on other buffers wrote"


def test_busy_while_a_pipe_has_frames_pending():
    from mi_lumaeq import synth
    w, h = 64, 48
    frame = synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = nv.Batch(w, h, 1).upload(nv.make_frames(w, h, FMT_YUY2, ["D1"], 1100))
    dst = PlanarOut(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            with pytest.raises(mi_lumaeq.MiError) as e:
                run(c, "eq", None, src, dst.planes(), FMT_YUY2, UV_COPY)
            assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same(), "a refused call wrote"


# ---- 7. hipGraph ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then capture on one stream and two replays on fresh inputs, as the NV12 form's test does."""
    w, h, n = 64, 48, 2
    fmt = FMT_UYVY
    frames = nv.make_frames(w, h, fmt, ["D1", "D2"], 900)
    src = nv.Batch(w, h, n, nv.LAYOUTS[1]).upload(frames)
    dst = PlanarOut(w, h, n, "one")
    planes = dst.planes()
    with mi_lumaeq.Context(0) as c:
        for op, cfg, uv_mode in (("eq", None, UV_COPY), ("clahe", (3.0, 4, 4), UV_COPY)):
            dst.clear()
            run(c, op, cfg, src, planes, fmt, uv_mode)                  # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert dst.same([expected_planes(f, w, fmt, op, cfg, uv_mode) for f in frames]), ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, cfg, src, planes, fmt, uv_mode, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                fresh = nv.make_frames(w, h, fmt, [nv.DISTS[(k + 2 + rep) % 5] for k in range(n)], 950 + 10 * rep)
                src.upload(fresh)
                dst.clear()
                g.replay()
                torch.cuda.synchronize()
                assert dst.same([expected_planes(f, w, fmt, op, cfg, uv_mode) for f in fresh]), ("graph replay", op, rep)
            src.upload(frames)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
