"""Interleaved BGR / RGB images in, pitched NV12 frames out on the GPU: mi_equalize_hist_bgr_to_nv12_batch_dev,
mi_clahe_bgr_to_nv12_batch_dev and their host forms.  Expected bytes are oracle.nv12_frame(oracle.bgr_to_nv12(img), W, H, uv_mode, op,
...), the image's last axis reversed first for MI_ORDER_RGB.  Pixels are full-range random bytes unless a test says otherwise (for such
images equalization changes about two thirds of a frame's bytes and swapping the channel order nearly all of them: an identity map or a
swapped order cannot pass).  The input and the two output planes live in sentinel-filled allocations with 64 guard bytes and the WHOLE
allocation is compared, input and output: every comparison in this file is exact.

How many workgroups bgr_to_nv12_hist_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_bgr_to_nv12 takes B = min(blocks_per_frame(W*H*9/4 bytes, H/2 rows, n, 2048),
ceil(items / 256)), and blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows --
whatever the CU count, which only lowers it.  So   B <= max(1, floor(W*H*9/4 / 16384)),  B <= H/2,
and the 256 lanes of a workgroup step through the frame by stride = 256 * B items: 16 x 2 pixel groups on the vector path (gx_n = W/16 per
row pair, the carried walk by += dby, gx += dgx with dby = stride / gx_n, dgx = stride % gx_n and a wrap when gx >= gx_n), 2 x 2 pixel
blocks on the byte path.  A shape with more items than 256 * min(both bounds) makes at least one lane take a second step."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import xfer, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, COLOR_BGR2YUV_I420

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
ORDERS = [ORDER_BGR, ORDER_RGB]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def rand_images(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


def expected(img, op, order, uv_mode):
    """The tight NV12 frame of W*H*3/2 bytes the call must produce for `img` (H x W x 3, in the order the call is told)."""
    kind, cfg = op
    h, w = img.shape[:2]
    bgr = img if order == ORDER_BGR else np.ascontiguousarray(img[:, :, ::-1])
    nv12 = oracle.bgr_to_nv12(bgr)
    return oracle.nv12_frame(nv12, w, h, uv_mode, 0) if kind == "eq" else oracle.nv12_frame(nv12, w, h, uv_mode, 1, *cfg)


class BgrIn:
    """n interleaved images in one sentinel-filled allocation: H rows of 3W bytes at `pitch`, frames `fstride` apart."""

    def __init__(self, w, h, n, pitch=None, frame_gap=0, off=0):
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = pitch or 3 * w
        self.fstride = self.pitch * h + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, images):
        a = np.full(self.total, SENT, np.uint8)
        for k, img in enumerate(images):
            o = self.off + k * self.fstride
            a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 3 * self.w] = img.reshape(self.h, 3 * self.w)
        return a

    def upload(self, images):
        self.buf.copy_(xfer.to_device(self.image(images)))
        return self

    def host(self):
        return xfer.to_host(self.buf)

    def kw(self):
        return {"in_pitch": self.pitch, "in_frame": self.fstride}


class Nv12Out:
    """n NV12 frames in one sentinel-filled allocation: the Y plane of frame f at off + f * fstride (H rows at y_pitch), its UV plane
    plane_gap bytes behind the Y rows (H/2 rows at uv_pitch), frame_gap bytes before the next frame."""

    def __init__(self, w, h, n, y_pitch=None, uv_pitch=None, plane_gap=0, frame_gap=0, off=0):
        self.w, self.h, self.n, self.off = w, h, n, off
        self.y_pitch, self.uv_pitch = y_pitch or w, uv_pitch or w
        self.uv_off = self.y_pitch * h + plane_gap
        self.fstride = self.uv_off + self.uv_pitch * (h // 2) + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def y_ptr(self):
        return self.buf.data_ptr() + self.off

    @property
    def uv_ptr(self):
        return self.y_ptr + self.uv_off

    def image(self, frames=None):
        a = np.full(self.total, SENT, np.uint8)
        w, h = self.w, self.h
        for k, f in enumerate(frames or []):
            o = self.off + k * self.fstride
            a[o: o + self.y_pitch * h].reshape(h, self.y_pitch)[:, :w] = f[: w * h].reshape(h, w)
            o += self.uv_off
            a[o: o + self.uv_pitch * (h // 2)].reshape(h // 2, self.uv_pitch)[:, :w] = f[w * h:].reshape(h // 2, w)
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def same(self, frames=None):
        got, want = xfer.to_host(self.buf), self.image(frames)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]

    def kw(self):
        return {"y_pitch": self.y_pitch, "uv_pitch": self.uv_pitch, "out_frame": self.fstride}


def run(c, op, src, dst, order, uv_mode, n=None, st=None):
    kind, cfg = op
    kw = dict(src.kw(), **dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_bgr_to_nv12_batch_dev(src.ptr, dst.y_ptr, dst.uv_ptr, src.w, src.h, n, order, uv_mode, **kw)
    else:
        c.clahe_bgr_to_nv12_batch_dev(src.ptr, dst.y_ptr, dst.uv_ptr, src.w, src.h, n, order, uv_mode, *cfg, **kw)


def check(c, images, op, order, uv_mode, src, dst):
    """One call on uploaded `images`: the whole output allocation is the oracle's image of it, the whole input allocation is what was
    uploaded."""
    src.upload(images)
    dst.clear()
    run(c, op, src, dst, order, uv_mode)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same([expected(img, op, order, uv_mode) for img in images])
    assert ok, (src.w, src.h, op, order, uv_mode, nbad, where)
    assert np.array_equal(src.host(), src.image(images)), "the input allocation was written"


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small batches leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def layout_terms(w, h, si, do):
    """The eight values the launcher ORs together for the vector path, relative to the (16-byte aligned) allocations, from the keyword
    arguments of BgrIn (si) and Nv12Out (do) alone."""
    ip = si.get("pitch") or 3 * w
    yp, up = do.get("y_pitch") or w, do.get("uv_pitch") or w
    uv_off = yp * h + do.get("plane_gap", 0)
    return {"in": si.get("off", 0), "in_pitch": ip, "in_frame": ip * h + si.get("frame_gap", 0), "y": do.get("off", 0), "y_pitch": yp,
            "uv": do.get("off", 0) + uv_off, "uv_pitch": up, "out_frame": uv_off + up * (h // 2) + do.get("frame_gap", 0)}


def misaligned(terms):
    return sorted(k for k, v in terms.items() if v % 16)


def build(w, h, n, si, do):
    """The two allocations of a layout; what layout_terms said about it holds for the real addresses."""
    src, dst = BgrIn(w, h, n, **si), Nv12Out(w, h, n, **do)
    real = {"in": src.ptr - src.buf.data_ptr(), "in_pitch": src.pitch, "in_frame": src.fstride, "y": dst.y_ptr - dst.buf.data_ptr(),
            "y_pitch": dst.y_pitch, "uv": dst.uv_ptr - dst.buf.data_ptr(), "uv_pitch": dst.uv_pitch, "out_frame": dst.fstride}
    assert real == layout_terms(w, h, si, do)
    return src, dst


# ---- 1. parity matrix ------------------------------------------------------------------------------------------------------------
ODD_66 = (dict(pitch=201, frame_gap=7, off=1), dict(y_pitch=67, uv_pitch=69, plane_gap=3, frame_gap=5, off=1))
PITCHED_64 = (dict(pitch=208, frame_gap=64, off=32), dict(y_pitch=80, uv_pitch=96, plane_gap=32, frame_gap=48, off=16))
PARITY = [
    # id, W, H, n, BgrIn layout, Nv12Out layout, vector path, the ops
    ("16x2", 16, 2, 1, {}, {}, True, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),                  # one vector group
    ("48x6", 48, 6, 2, {}, {}, True, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 5, 4))]),                  # gx_n = 3: the row walk wraps
    ("2x2", 2, 2, 1, {}, {}, False, [EQ]),                                                                   # one byte-path block
    ("66x34-odd", 66, 34, 2, *ODD_66, False, [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (3.0, 4, 3))]),          # nothing aligned: the byte path
    ("64x32-pitched", 64, 32, 2, *PITCHED_64, True, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 8, 8))]),   # padding, gaps, aligned
]


@pytest.mark.parametrize("name,w,h,n,si,do,vec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity_matrix(c, name, w, h, n, si, do, vec, ops):
    assert (w % 16 == 0 and not misaligned(layout_terms(w, h, si, do))) == vec
    src, dst = build(w, h, n, si, do)
    images = rand_images(w, h, n, 31)
    for op in ops:
        for order in ORDERS:
            for uv_mode in UV_MODES:
                check(c, images, op, order, uv_mode, src, dst)


# ---- 2. one alignment term at a time ---------------------------------------------------------------------------------------------
ONE_TERM = [
    # the broken term, BgrIn layout, Nv12Out layout (32 x 4: y_pitch * H and uv_pitch * H/2 stay multiples of 16 when a pitch moves by 8)
    ("in", dict(off=8), {}),
    ("in_pitch", dict(pitch=104), {}),
    ("in_frame", dict(frame_gap=8), {}),
    ("y", {}, dict(off=8, plane_gap=8, frame_gap=8)),
    ("y_pitch", {}, dict(y_pitch=40)),
    ("uv", {}, dict(plane_gap=8, frame_gap=8)),
    ("uv_pitch", {}, dict(uv_pitch=40)),
    ("out_frame", {}, dict(frame_gap=8)),
]


@pytest.mark.parametrize("term,si,do", ONE_TERM, ids=[t[0] for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, term, si, do):
    """Exactly one of the eight terms is no multiple of 16: the byte path, the same bytes, the same untouched guards."""
    w, h, n = 32, 4, 2
    assert misaligned(layout_terms(w, h, si, do)) == [term]
    src, dst = build(w, h, n, si, do)
    images = rand_images(w, h, n, 32)
    for op, order, uv_mode in ((EQ, ORDER_BGR, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, UV_FILL128)):
        check(c, images, op, order, uv_mode, src, dst)


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
PITCHED_112 = (dict(pitch=352, frame_gap=64, off=32), dict(y_pitch=128, uv_pitch=144, plane_gap=32, frame_gap=48, off=16))
LOOP_SHAPES = [
    # id, W, H, n, BgrIn layout, Nv12Out layout, vector path (see the module docstring for the bound on B)
    # bytes/16384 = 1.9: B = 1, stride 256; gx_n 6, groups 432, dby 42, dgx 4: the wrap fires whenever gx >= 2, the second step is partial
    ("96x144", 96, 144, 1, {}, {}, True),
    # bytes/16384 = 2.46: B <= 2, stride <= 512; gx_n 7, groups 560, dby 73, dgx 1; pitches, plane gap, frame gaps and bases multiples of 16
    ("112x160-pitched", 112, 160, 2, *PITCHED_112, True),
    # bytes/16384 = 4.5, H/2 = 4: B <= 4, stride <= 1024; gx_n 257, groups 1028, dby 3, dgx 253: four lanes take a second step, and wrap
    ("4112x8", 4112, 8, 1, {}, {}, True),
    # bytes/16384 = 4.5 but H/2 = 2 rows: B <= 2, stride <= 512; gx_n 512, groups 1024, dby 1, dgx 0: every lane steps straight down a row pair
    ("8192x4", 8192, 4, 1, {}, {}, True),
    # byte path, bytes/16384 = 0.3: B = 1; 33 x 17 = 561 blocks of 2 x 2 for 256 lanes: three steps, the last of 49 lanes
    ("66x34-odd", 66, 34, 2, *ODD_66, False),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,w,h,n,si,do,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, si, do, vec, order):
    """bgr_to_nv12_hist_kernel where a lane owns more than one group / block: with the histogram (equalizeHist, U and V computed) and
    without it (CLAHE 2 x 2, chroma filled)."""
    assert (w % 16 == 0 and not misaligned(layout_terms(w, h, si, do))) == vec
    bound = max(1, w * h * 9 // 4 // 16384)
    assert (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2), "the shape would not loop"
    src, dst = build(w, h, n, si, do)
    images = rand_images(w, h, n, 33)
    check(c, images, EQ, order, UV_COPY, src, dst)
    check(c, images, ("clahe", (2.0, 2, 2)), order, UV_FILL128, src, dst)


# ---- 4. histogram isolation ------------------------------------------------------------------------------------------------------
def test_histograms_do_not_leak_across_frames(c):
    """A constant colour (equalizeHist's single-bin shortcut: every pixel keeps its luma), noise and a horizontal ramp in one batch: each
    frame equals its own oracle result.  Then a two-colour checkerboard in one vector group."""
    w, h = 48, 6
    const = np.empty((h, w, 3), np.uint8)
    const[:] = (200, 31, 7)
    ramp = np.empty((h, w, 3), np.uint8)
    ramp[:] = (np.arange(w) * 255 // (w - 1)).astype(np.uint8)[None, :, None]
    ramp[:, :, 1] //= 2
    images = [const, rand_images(w, h, 1, 34)[0], ramp]
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        for order in ORDERS:
            check(c, images, op, order, UV_COPY, BgrIn(w, h, 3), Nv12Out(w, h, 3))
    w, h = 16, 2
    board = np.empty((h, w, 3), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    board[:] = np.where(((xx + yy) % 2 == 0)[:, :, None], np.array([250, 10, 90], np.uint8), np.array([5, 180, 220], np.uint8))
    for order in ORDERS:
        for uv_mode in UV_MODES:
            check(c, [board], EQ, order, uv_mode, BgrIn(w, h, 1), Nv12Out(w, h, 1))


# ---- 5. composition with the library's own pieces --------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_composition_with_the_librarys_own_pieces(c, op):
    """Y equals the planar op applied to the Y rows of mi_cvt_color_420_u8_batch_dev(BGR2YUV_I420); the de-interleaved U and V equal
    that call's U and V planes."""
    w, h, n = 64, 32, 3
    ysz = w * h
    d_bgr = xfer.to_device(np.stack(rand_images(w, h, n, 35)))
    d_i420 = torch.full((n, ysz * 3 // 2), SENT, dtype=torch.uint8, device="cuda:0")
    d_y = torch.full((n, ysz), SENT, dtype=torch.uint8, device="cuda:0")
    d_one = torch.full((n, ysz * 3 // 2), SENT, dtype=torch.uint8, device="cuda:0")
    c.cvt_color_420_batch_dev(d_bgr, d_i420, w, h, n, COLOR_BGR2YUV_I420, stream=stream())
    if op is EQ:
        c.equalize_hist_batch_dev(d_i420, d_y, w, h, n, src_frame=ysz * 3 // 2, stream=stream())
        c.equalize_hist_bgr_to_nv12_batch_dev(d_bgr, d_one, None, w, h, n, ORDER_BGR, UV_COPY, stream=stream())
    else:
        c.clahe_batch_dev(d_i420, d_y, w, h, n, *op[1], src_frame=ysz * 3 // 2, stream=stream())
        c.clahe_bgr_to_nv12_batch_dev(d_bgr, d_one, None, w, h, n, ORDER_BGR, UV_COPY, *op[1], stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(d_one[:, :ysz], d_y), op
    uv = d_one[:, ysz:].reshape(n, ysz // 4, 2)
    assert torch.equal(uv[:, :, 0], d_i420[:, ysz: ysz + ysz // 4]) and torch.equal(uv[:, :, 1], d_i420[:, ysz + ysz // 4:]), op


# ---- 6. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


FUSED_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass")


def test_launch_contract():
    """equalizeHist: one MI_K_COLOR, one MI_K_EQ_LUT, one MI_K_LUT_APPLY and no MI_K_HIST launch per call of n <= 256 frames -- at a
    batch size (n = 2) where the planar form would take hist_lut_kernel.  CLAHE: one MI_K_COLOR launch plus what mi_clahe_u8_batch_dev
    launches for the same plane in place."""
    w, h, n = 64, 32, 2
    images = rand_images(w, h, n, 36)
    src, dst = build(w, h, n, *PITCHED_64)
    with mi_lumaeq.Context(0) as c:
        before = {k: c.get_stat(k) for k in FUSED_STATS}
        c.set_profiling(1)
        c.profile_read(reset=True)
        check(c, images, EQ, ORDER_BGR, UV_COPY, src, dst)
        got = launches(c)
        want = {"color_kernel": 1, "equalize_lut_kernel": 1, "lut_apply_kernel": 1}
        assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, got
        for cfg in ((2.0, 4, 2), (2.0, 3, 5)):
            c.profile_read(reset=True)
            c.clahe_batch_dev(dst.y_ptr, dst.y_ptr, w, h, n, *cfg, src_step=dst.y_pitch, src_frame=dst.fstride, dst_step=dst.y_pitch,
                              dst_frame=dst.fstride, stream=stream())
            torch.cuda.synchronize()
            planar = launches(c)
            assert planar["color_kernel"] == 0 and sum(planar.values()) >= 2, planar
            c.profile_read(reset=True)
            check(c, images, ("clahe", cfg), ORDER_RGB, UV_FILL128, src, dst)
            got = launches(c)
            assert got == dict(planar, color_kernel=1), (cfg, got, planar)
        c.set_profiling(0)
        assert {k: c.get_stat(k) for k in FUSED_STATS} == before


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------
def frames_per_launch():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "bgr_nv12.inc.hpp").read_text()
    return int(re.search(r"constexpr\s+int\s+kBgrNv12FramesPerLaunch\s*=\s*(\d+)\s*;", src).group(1))


@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 1, 1))], ids=["eq", "clahe-1x1"])
def test_chunking(c, op):
    """One frame past the chunk: two launch sequences, the second of one frame; every frame distinct, every frame checked."""
    assert frames_per_launch() == 256
    w, h, n = 16, 2, 257
    check(c, rand_images(w, h, n, 37), op, ORDER_RGB, UV_COPY, BgrIn(w, h, n), Nv12Out(w, h, n))


# ---- 8. errors, zero sizes, busy -------------------------------------------------------------------------------------------------
def test_errors_and_zero_sizes_enqueue_nothing():
    w, h, n = 32, 16, 2
    images = rand_images(w, h, n, 38)
    src = BgrIn(w, h, n, pitch=112, frame_gap=16).upload(images)
    dst = Nv12Out(w, h, n, y_pitch=48, uv_pitch=48, frame_gap=16)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        base = dict(ctx=hd, i=src.ptr, ip=src.pitch, fi=src.fstride, y=dst.y_ptr, yp=dst.y_pitch, uv=dst.uv_ptr, up=dst.uv_pitch,
                    fo=dst.fstride, w=w, h=h, n=n, order=ORDER_BGR, uvm=UV_COPY)

        def args(kw):
            a = dict(base)
            a.update(kw)
            return (a["ctx"], a["i"], a["ip"], a["fi"], a["y"], a["yp"], a["uv"], a["up"], a["fo"], a["w"], a["h"], a["n"], a["order"],
                    a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_bgr_to_nv12_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_bgr_to_nv12_batch_dev(*args(kw), 2.0, tx, ty, stream())
        bad = [dict(ctx=None), dict(i=None), dict(y=None), dict(uv=None),                     # a null ctx or pointer
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, w=0), dict(h=15, n=0),      # odd sizes, also when another size is 0
               dict(w=-2), dict(h=-2), dict(n=-1),                                            # negative sizes
               dict(ip=3 * w - 1), dict(yp=w - 1), dict(up=w - 1),                            # a pitch below its row
               dict(order=2), dict(order=-1),                                                 # order other than the two
               dict(uvm=2), dict(uvm=-1),                                                     # a bad uv_mode
               dict(y=src.ptr), dict(uv=src.ptr), dict(uv=dst.y_ptr)]                         # no in-place form
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
        # zero sizes: MI_OK, nothing written
        for kw in (dict(w=0), dict(h=0), dict(n=0)):
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: their status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, yp=1 << 25, up=1 << 25)
        planar = L.mi_clahe_u8_batch_dev(hd, dst.y_ptr, 1 << 25, 1 << 26, dst.y_ptr, 1 << 25, 1 << 26, big["w"], 2, 1, 2.0, 2, 2, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, dst.y_ptr, dst.y_pitch, dst.fstride, dst.y_ptr, dst.y_pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024,
                                         stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(images)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        c.set_profiling(0)
        # and the context still works
        check(c, images, EQ, ORDER_RGB, UV_FILL128, src, dst)


def test_host_form_errors():
    w, h = 32, 16
    img = rand_images(w, h, 1, 39)[0]
    out = np.full(w * h * 3 // 2, SENT, np.uint8)
    ip, op = img.ctypes.data, out.ctypes.data
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        for a in ((None, ip, 3 * w, op, w, h, 0, 1), (hd, None, 3 * w, op, w, h, 0, 1), (hd, ip, 3 * w, None, w, h, 0, 1),
                  (hd, ip, 3 * w - 1, op, w, h, 0, 1), (hd, ip, 3 * w, op, w - 1, h, 0, 1), (hd, ip, 3 * w, op, w, h - 1, 0, 1),
                  (hd, ip, 3 * w, op, -2, h, 0, 1), (hd, ip, 3 * w, op, w, h, 2, 1), (hd, ip, 3 * w, op, w, h, 0, 2),
                  (hd, ip, 3 * w, ip, w, h, 0, 1), (hd, ip, 3 * w, op, w - 1, 0, 0, 1)):
            assert L.mi_equalize_hist_bgr_to_nv12(*a) == BAD_ARG, a
            assert L.mi_clahe_bgr_to_nv12(*a, 2.0, 2, 2) == BAD_ARG, a
        assert L.mi_clahe_bgr_to_nv12(hd, ip, 3 * w, op, w, h, 0, 1, 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_bgr_to_nv12(hd, ip, 3 * w, op, w, h, 0, 1, 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_bgr_to_nv12(hd, ip, 3 * w, op, 0, h, 0, 1) == 0
        assert (out == SENT).all() and c.get_stat("error_drains") == 0


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = BgrIn(w, h, 1).upload(rand_images(w, h, 1, 40))
    dst = Nv12Out(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, ORDER_BGR, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"


# ---- 9. hipGraph -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist and one CLAHE call captured on a single stream (one linear chain, no parallel
    branches) and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    cl = ("clahe", (2.0, 4, 2))
    src, dst_eq = build(w, h, n, *PITCHED_64)
    dst_cl = Nv12Out(w, h, n, **PITCHED_64[1])
    with mi_lumaeq.Context(0) as c:
        images = rand_images(w, h, n, 41)
        src.upload(images)
        for op, dst, uv_mode in ((EQ, dst_eq, UV_COPY), (cl, dst_cl, UV_FILL128)):        # the eager calls size the scratch
            dst.clear()
            run(c, op, src, dst, ORDER_BGR, uv_mode)
            torch.cuda.synchronize()
            assert dst.same([expected(img, op, ORDER_BGR, uv_mode) for img in images])[0], ("eager", op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            run(c, EQ, src, dst_eq, ORDER_BGR, UV_COPY, st=st)
            run(c, cl, src, dst_cl, ORDER_BGR, UV_FILL128, st=st)
        for rep in range(2):
            fresh = rand_images(w, h, n, 42 + rep)
            src.upload(fresh)
            dst_eq.clear()
            dst_cl.clear()
            g.replay()
            torch.cuda.synchronize()
            assert dst_eq.same([expected(img, EQ, ORDER_BGR, UV_COPY) for img in fresh])[0], ("graph replay", "eq", rep)
            assert dst_cl.same([expected(img, cl, ORDER_BGR, UV_FILL128) for img in fresh])[0], ("graph replay", "clahe", rep)
            assert np.array_equal(src.host(), src.image(fresh))


# ---- 10. host forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 6), (66, 34)])
def test_host_forms(w, h):
    """A view with padded rows at an odd address in, a tight frame out: both ops, both orders, both UV modes; the source is unchanged."""
    img = rand_images(w, h, 1, 43)[0]
    pitch = 3 * w + 23
    raw = np.full(h * pitch + 1, SENT, np.uint8)
    padded = raw[1:].reshape(h, pitch)
    view = padded[:, : 3 * w].reshape(h, w, 3)
    assert np.shares_memory(view, raw) and view.ctypes.data % 2 == 1
    view[:] = img
    raw0 = raw.copy()
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, ("clahe", (2.0, 3, 2))):
            for order in ORDERS:
                for uv_mode in UV_MODES:
                    want = expected(img, op, order, uv_mode)
                    if op is EQ:
                        got = c.equalize_hist_bgr_to_nv12(view, order, uv_mode)
                    else:
                        got = c.clahe_bgr_to_nv12(view, order, uv_mode, *op[1])
                    assert got.shape == (w * h * 3 // 2,) and np.array_equal(got, want), (op, order, uv_mode)
                    assert np.array_equal(raw, raw0), "the source was written"
        # a caller's own output buffer is filled and returned
        out = np.full(w * h * 3 // 2, SENT, np.uint8)
        assert c.equalize_hist_bgr_to_nv12(view, out=out) is out
        assert np.array_equal(out, expected(img, EQ, ORDER_BGR, UV_COPY))
        assert c.get_stat("error_drains") == 0
