"""Packed 4:2:2 frames in (YUY2 / UYVY), NV12 frames out on the GPU: mi_equalize_hist_packed422_to_nv12_batch_dev and
mi_clahe_packed422_to_nv12_batch_dev.  The expected Y plane is oracle.equalize_hist / oracle.clahe on the gathered luma; the expected UV
plane is 128 (MI_UV_FILL128) or the rounding mean (a + b + 1) >> 1 of input chroma rows 2r and 2r+1 (MI_UV_COPY).  Every batch lives in
sentinel-filled allocations (padded pitches, gaps between planes and frames, bases 4 / 8 / 12 bytes past a 16-byte boundary) and the
WHOLE allocation is compared: every comparison in this file is exact bytes."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
DISTS = ["D1", "D2", "D3", "D4", "D5"]
CLAHE_CONFIGS = [(2.0, 8, 8), (3.0, 4, 4), (0.0, 3, 5), (2.0, 16, 16), (2.0, 64, 2)]      # the last takes the wide-grid fallback
OPS = [("eq", None)] + [("clahe", cfg) for cfg in CLAHE_CONFIGS]
# input, as the packed tests: (pitch - 2W, gap between frames, base offset from a 16-byte boundary)
LAYOUTS = [(4, 20, 4), (36, 0, 8), (0, 12, 12)]
# output: (y_pitch - align4(W), uv_pitch - align4(W), where the UV plane lies, gap, base offset); the two pitches always differ
OUT_LAYOUTS = [(4, 12, "behind", 0, 4), (36, 8, "gap", 24, 8), (0, 4, "own", 12, 12)]
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]


def stream():
    return torch.cuda.current_stream().cuda_stream


def align4(x):
    return (x + 3) & ~3


def luma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, fmt - 2:2 * w:2])


def chroma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, 3 - fmt:2 * w:2])


def uv_mean(c):
    """The header's chroma rule: UV row r is the per-byte rounding mean of chroma rows 2r and 2r+1."""
    a, b = c[0::2], c[1::2]
    return ((a.astype(np.uint16) + b + 1) >> 1).astype(np.uint8)


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


def expected_planes(frame, w, fmt, op, cfg, uv_mode, key=None):
    h = frame.shape[0]
    uv = uv_mean(chroma(frame, w, fmt)) if uv_mode == UV_COPY else np.full((h // 2, w), 128, np.uint8)
    return y_ref(luma(frame, w, fmt), op, cfg, key), uv


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
        a = np.full(self.total, SENT, np.uint8)
        if frames is not None:
            for k, f in enumerate(frames):
                o = self.off + k * self.fstride
                a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 2 * self.w] = f[:, : 2 * self.w]
        return a

    def upload(self, frames):
        self.buf.copy_(torch.from_numpy(self.image(frames)))
        return self

    def host(self):
        return self.buf.cpu().numpy()

    def kw(self):
        return {"in_pitch": self.pitch, "in_frame": self.fstride}


class Nv12Out:
    """n NV12 frames in sentinel-filled allocations: the Y plane of frame f at y0 + f * fstride (H rows at y_pitch), its UV plane at
    uv0 + f * fstride (H/2 rows at uv_pitch) -- directly behind the Y plane, behind a gap, or in an allocation of its own."""

    def __init__(self, w, h, n, layout=(0, 4, "behind", 0, 0)):
        ye, ue, where, gap, off = layout
        self.w, self.h, self.n = w, h, n
        self.y_pitch, self.uv_pitch = align4(w) + ye, align4(w) + ue
        ysz, usz = self.y_pitch * h, self.uv_pitch * (h // 2)
        if where == "own":
            self.fstride = max(ysz, usz) + gap
            sizes = [off + self.fstride * n + 64, 4 + self.fstride * n + 64]
            self.y_at, self.uv_at = (0, off), (1, 4)
        else:
            self.fstride = ysz + usz + 2 * gap
            sizes = [off + self.fstride * n + 64]
            self.y_at, self.uv_at = (0, off), (0, off + ysz + gap)
        assert self.fstride % 4 == 0
        self.bufs = [torch.full((s,), SENT, dtype=torch.uint8, device="cuda:0") for s in sizes]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)

    @property
    def y_ptr(self):
        return self.bufs[self.y_at[0]].data_ptr() + self.y_at[1]

    @property
    def uv_ptr(self):
        return self.bufs[self.uv_at[0]].data_ptr() + self.uv_at[1]

    def image(self, planes=None):
        """The allocations as they must read with `planes` = [(Y, UV), ...] in them (None: untouched)."""
        imgs = [np.full(b.numel(), SENT, np.uint8) for b in self.bufs]
        if planes is not None:
            for k, (y, uv) in enumerate(planes):
                for (bi, o), pitch, rows, pl in ((self.y_at, self.y_pitch, self.h, y), (self.uv_at, self.uv_pitch, self.h // 2, uv)):
                    o += k * self.fstride
                    imgs[bi][o: o + pitch * rows].reshape(rows, pitch)[:, : self.w] = pl
        return imgs

    def clear(self):
        for b in self.bufs:
            b.fill_(SENT)

    def host(self):
        return [b.cpu().numpy() for b in self.bufs]

    def same(self, planes=None):
        return all(np.array_equal(g, w) for g, w in zip(self.host(), self.image(planes)))

    def kw(self):
        return {"y_pitch": self.y_pitch, "uv_pitch": self.uv_pitch, "out_frame": self.fstride}


def run(c, op, cfg, src, dst, fmt, uv_mode, n=None, st=None):
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if op == "eq":
        c.equalize_hist_packed422_to_nv12_batch_dev(src.dev, dst.y_ptr, dst.uv_ptr, src.w, src.h, n, fmt, uv_mode, **kw)
    else:
        c.clahe_packed422_to_nv12_batch_dev(src.dev, dst.y_ptr, dst.uv_ptr, src.w, src.h, n, fmt, uv_mode, *cfg, **kw)


_planar_cache = {}


def planar_status(c, w, h, n, op, cfg):
    """What the planar form answers for this size / grid pair (0 = accepted)."""
    k = (w, h, n, op, cfg)
    if k not in _planar_cache:
        a = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        status = 0
        try:
            if op == "eq":
                c.equalize_hist_batch_dev(a, b, w, h, n, stream=stream())
            else:
                c.clahe_batch_dev(a, b, w, h, n, *cfg, stream=stream())
        except mi_lumaeq.MiError as e:
            status = e.status
        finally:
            torch.cuda.synchronize()
        _planar_cache[k] = status
    return _planar_cache[k]


def check_case(c, frames, w, h, fmt, uv_mode, op, cfg, li, key):
    n = len(frames)
    src = Batch(w, h, n, LAYOUTS[li]).upload(frames)
    dst = Nv12Out(w, h, n, OUT_LAYOUTS[li])
    status = planar_status(c, w, h, n, op, cfg)
    if status != 0:                                   # a size / grid pair the planar form refuses: the same status, nothing written
        with pytest.raises(mi_lumaeq.MiError) as e:
            run(c, op, cfg, src, dst, fmt, uv_mode)
        torch.cuda.synchronize()
        assert e.value.status == status, (w, h, op, cfg, e.value.status, status)
        assert dst.same(), "a refused call wrote"
        return
    run(c, op, cfg, src, dst, fmt, uv_mode)
    torch.cuda.synchronize()
    want = dst.image([expected_planes(f, w, fmt, op, cfg, uv_mode, (key, k, fmt)) for k, f in enumerate(frames)])
    for bi, (got, wnt) in enumerate(zip(dst.host(), want)):
        assert np.array_equal(got, wnt), (w, h, fmt, uv_mode, op, cfg, li, bi, int((got != wnt).sum()), np.flatnonzero(got != wnt)[:8])
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


def make_frames(w, h, fmt, dists, first):
    return [synth.packed422_frame(w, h, fmt, d, first + k) for k, d in enumerate(dists)]


# ---- 1. small sizes, full matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (62, 46), (2, 2), (4098, 4)])
def test_small_sizes_full_matrix(c, w, h):
    """Every format x uv_mode x op x layout on D1-D5.  62 x 46: W % 4 == 2 (a 2-byte row tail) and no tile grid divides it; 2 x 2: one
    macropixel, one row pair; 4098 x 4: rows of many groups plus a ragged one; (2.0, 64, 2) takes the wide-grid kernel."""
    for fmt in FMTS:
        frames = make_frames(w, h, fmt, DISTS, 100)
        for uv_mode in UVS:
            for op, cfg in OPS:
                for li in range(3):
                    check_case(c, frames, w, h, fmt, uv_mode, op, cfg, li, ("small", w, h))


# ---- 2. one large unaligned case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_large_unaligned(c, fmt):
    w, h = 1918, 1078
    frames = make_frames(w, h, fmt, DISTS[:2], 200)
    for i, (op, cfg) in enumerate(OPS):
        check_case(c, frames, w, h, fmt, UVS[(i + fmt) % 2], op, cfg, i % 3, ("large", w, h))


# ---- 3. identity with the existing forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_identity_with_existing_forms(c, n):
    """The Y plane is the planar form's output on the gathered plane and the luma of the packed form's output; with MI_UV_COPY the UV
    plane is the row-pair rounding mean of the packed form's output chroma.  Both CLAHE arithmetic modes."""
    w, h = 320, 90
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1312 + n)
    x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
    x[: n // 2 + 1, :, :] = (x[: n // 2 + 1, :, :] // 3) + 40                      # half of the frames low-contrast
    packed = torch.empty_like(x)
    nv12 = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")   # tight: UV directly behind Y, all defaults
    try:
        for fmt in FMTS:
            off = fmt - 2
            y = x[:, :, off::2].contiguous()
            yo = torch.empty_like(y)
            for contract in (0, 1):
                c.set_option("clahe_fp_contract", contract)
                for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (3.0, 5, 3))):
                    packed.fill_(SENT)
                    nv12.fill_(SENT)
                    if op == "eq":
                        c.equalize_hist_batch_dev(y, yo, w, h, n, stream=stream())
                        c.equalize_hist_packed422_batch_dev(x, packed, w, h, n, fmt, UV_COPY, stream=stream())
                        c.equalize_hist_packed422_to_nv12_batch_dev(x, nv12, None, w, h, n, fmt, UV_COPY, stream=stream())
                    else:
                        c.clahe_batch_dev(y, yo, w, h, n, *cfg, stream=stream())
                        c.clahe_packed422_batch_dev(x, packed, w, h, n, fmt, UV_COPY, *cfg, stream=stream())
                        c.clahe_packed422_to_nv12_batch_dev(x, nv12, None, w, h, n, fmt, UV_COPY, *cfg, stream=stream())
                    torch.cuda.synchronize()
                    why = (n, fmt, contract, op, cfg)
                    assert torch.equal(nv12[:, :h, :], yo), ("planar", why)
                    assert torch.equal(nv12[:, :h, :], packed[:, :, off::2]), ("packed luma", why)
                    ch = packed[:, :, 1 - off::2].to(torch.int16)
                    mean = ((ch[:, 0::2, :] + ch[:, 1::2, :] + 1) >> 1).to(torch.uint8)
                    assert torch.equal(nv12[:, h:, :], mean), ("packed chroma", why)
    finally:
        c.set_option("clahe_fp_contract", 0)


# ---- 4. chroma rounding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_chroma_rounding(c, fmt):
    """Row pairs (0, 1), (254, 255), (255, 255), (0, 255), (7, 8), (128, 128) in NEIGHBOURING chroma bytes (a carry or borrow between the
    bytes of a 4-byte-at-once mean would show), in both row orders, through full 16-column groups and a ragged one (W = 38)."""
    w, h = 38, 4
    pairs = [(0, 1), (254, 255), (255, 255), (0, 255), (7, 8), (128, 128)]
    mean = [1, 255, 255, 128, 8, 128]
    a = np.array([p[0] for p in pairs], np.uint8)[np.arange(w) % 6]
    b = np.array([p[1] for p in pairs], np.uint8)[np.arange(w) % 6]
    frame = synth.packed422_frame(w, h, fmt, "D2", 900)
    frame[:, 3 - fmt::2] = np.stack([a, b, b, a])
    want_uv = np.tile(np.array(mean, np.uint8)[np.arange(w) % 6], (h // 2, 1))
    assert np.array_equal(uv_mean(chroma(frame, w, fmt)), want_uv)
    for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 64, 2))):
        assert planar_status(c, w, h, 1, op, cfg) == 0, (op, cfg)       # LDS-table kernel (full and ragged groups), wide-grid kernel
        src = Batch(w, h, 1, LAYOUTS[0]).upload([frame])
        dst = Nv12Out(w, h, 1, OUT_LAYOUTS[0])
        run(c, op, cfg, src, dst, fmt, UV_COPY)
        torch.cuda.synchronize()
        assert dst.same([(y_ref(luma(frame, w, fmt), op, cfg), want_uv)]), (fmt, op, cfg)


# ---- 5. launch accounting --------------------------------------------------------------------------------------------------------
def test_launch_accounting():
    w, h, n = 64, 48, 3
    frames = make_frames(w, h, FMT_YUY2, DISTS[:n], 1000)
    src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
    dst = Nv12Out(w, h, n, OUT_LAYOUTS[0])
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for uv_mode in UVS:
            c.profile_read(reset=True)
            run(c, "eq", None, src, dst, FMT_YUY2, uv_mode)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            assert len(prof) == 10
            for k in mi_lumaeq.KERNEL_NAMES:
                want = 1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0
                assert prof[k]["launches"] == want, (uv_mode, k, prof[k])
            assert dst.same([expected_planes(f, w, FMT_YUY2, "eq", None, uv_mode) for f in frames])
        for cfg in ((2.0, 8, 8), (2.0, 64, 2)):
            assert planar_status(c, w, h, n, "clahe", cfg) == 0
            for uv_mode in UVS:
                c.profile_read(reset=True)
                run(c, "clahe", cfg, src, dst, FMT_YUY2, uv_mode)
                torch.cuda.synchronize()
                prof = c.profile_read(reset=True)
                for k in ("equalize_fused_kernel", "fused_finish_kernel", "color_kernel", "analyze_diff_kernel", "hist_partial_kernel",
                          "equalize_lut_kernel", "lut_apply_kernel"):
                    assert prof[k]["launches"] == 0, (cfg, uv_mode, k, prof[k])
                assert prof["tile_hist_kernel"]["launches"] == 1 and prof["clahe_interp_kernel"]["launches"] == 1, (cfg, uv_mode, prof)
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    w, h, n = 64, 48, 2
    frames = make_frames(w, h, FMT_YUY2, DISTS[:n], 700)
    src = Batch(w, h, n, LAYOUTS[0]).upload(frames)
    dst = Nv12Out(w, h, n, OUT_LAYOUTS[1])
    L, hd = c._L, c._h
    ip, yp, up = src.dev.data_ptr(), dst.y_ptr, dst.uv_ptr
    base = dict(i=ip, ipitch=src.pitch, ifs=src.fstride, y=yp, ypitch=dst.y_pitch, uv=up, uvpitch=dst.uv_pitch, ofs=dst.fstride,
                w=w, h=h, n=n, fmt=FMT_YUY2, uvm=UV_COPY)

    def args(kw):
        a = dict(base)
        a.update(kw)
        return (hd, a["i"], a["ipitch"], a["ifs"], a["y"], a["ypitch"], a["uv"], a["uvpitch"], a["ofs"], a["w"], a["h"], a["n"],
                a["fmt"], a["uvm"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_nv12_batch_dev(*args(kw), stream())

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_nv12_batch_dev(*args(kw), 2.0, tx, ty, stream())
    bad = [dict(i=None), dict(y=None), dict(uv=None),                                             # null frame pointers
           dict(w=63), dict(h=47), dict(w=63, h=47),                                              # odd width / height
           dict(w=-2), dict(h=-2), dict(h=-1), dict(n=-1),                                        # negative sizes
           dict(ipitch=2 * w - 4), dict(ypitch=w - 4), dict(uvpitch=w - 4),                       # pitches too small
           dict(i=ip + 2), dict(y=yp + 2), dict(uv=up + 1), dict(ipitch=2 * w + 2), dict(ypitch=w + 2), dict(uvpitch=w + 6),
           dict(ifs=src.fstride + 2), dict(ofs=dst.fstride + 2), dict(ofs=dst.fstride + 1),       # not multiples of 4
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),         # format, uv_mode
           dict(y=ip), dict(uv=ip)]                                                               # no in-place form
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert cl(tx, ty) == BAD_ARG
    # the documented consequence: a tight NV12 batch with W % 4 == 2 has a pitch that is not a multiple of 4
    assert eq(w=62, ypitch=62, uvpitch=62, ofs=62 * h * 3 // 2) == BAD_ARG
    assert cl(w=62, ypitch=62, uvpitch=62, ofs=62 * h * 3 // 2) == BAD_ARG
    # zero sizes: MI_OK, nothing written; an odd height is refused before a zero width or frame count is looked at
    for kw in (dict(w=0), dict(h=0), dict(n=0)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    for kw in (dict(w=0, h=47), dict(n=0, h=47)):
        assert eq(**kw) == BAD_ARG and cl(**kw) == BAD_ARG, kw
    torch.cuda.synchronize()
    assert dst.same(), "a refused or empty call wrote"
    assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
    # the same W % 4 == 2 frames with padded pitches are accepted (a destination of their own)
    src62 = Batch(62, h, n, LAYOUTS[0]).upload([f[:, :124] for f in frames])
    dst62 = Nv12Out(62, h, n, OUT_LAYOUTS[1])
    run(c, "eq", None, src62, dst62, FMT_YUY2, UV_COPY)
    torch.cuda.synchronize()
    assert dst62.same([expected_planes(np.ascontiguousarray(f[:, :124]), 62, FMT_YUY2, "eq", None, UV_COPY) for f in frames])
    assert dst.same(), "a call on other buffers wrote"
    # and the context still works
    run(c, "eq", None, src, dst, FMT_YUY2, UV_COPY)
    torch.cuda.synchronize()
    assert dst.same([expected_planes(f, w, FMT_YUY2, "eq", None, UV_COPY) for f in frames])


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Batch(w, h, 1).upload(make_frames(w, h, FMT_YUY2, ["D1"], 1100))
    dst = Nv12Out(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            with pytest.raises(mi_lumaeq.MiError) as e:
                run(c, "eq", None, src, dst, FMT_YUY2, UV_COPY)
            assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same(), "a refused call wrote"


# ---- 7. hipGraph -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then capture and two replays on fresh inputs (the way test_gpu_packed422.py does it for the packed
    form)."""
    w, h, n = 640, 360, 3
    fmt = FMT_UYVY
    frames = make_frames(w, h, fmt, DISTS[:n], 800)
    src = Batch(w, h, n, LAYOUTS[1]).upload(frames)
    dst = Nv12Out(w, h, n, OUT_LAYOUTS[1])
    with mi_lumaeq.Context(0) as c:
        for op, cfg, uv_mode in (("eq", None, UV_COPY), ("clahe", (3.0, 4, 4), UV_COPY), ("clahe", (2.0, 8, 8), UV_FILL128)):
            dst.clear()
            run(c, op, cfg, src, dst, fmt, uv_mode)                    # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert dst.same([expected_planes(f, w, fmt, op, cfg, uv_mode) for f in frames]), ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, cfg, src, dst, fmt, uv_mode, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                fresh = make_frames(w, h, fmt, [DISTS[(k + 2 + rep) % 5] for k in range(n)], 850 + 10 * rep)
                src.upload(fresh)
                dst.clear()
                g.replay()
                torch.cuda.synchronize()
                assert dst.same([expected_planes(f, w, fmt, op, cfg, uv_mode) for f in fresh]), ("graph replay", op, rep)
            src.upload(frames)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
