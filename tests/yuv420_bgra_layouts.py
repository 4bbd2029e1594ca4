"""Layouts, expected bytes, the documented alignment rule and the seeded sweep for the tests of mi_*_yuv420_to_bgra*
(tests/test_gpu_yuv420_to_bgra.py, tests/test_gpu_yuv420_to_bgra_frames.py; the builder of the expected bytes, the restated rule and the
census of the sweep are backed without a GPU by tests/test_yuv420_to_bgra_abi.py and tests/test_yuv420_to_bgra_frames_abi.py).
The expected bytes take the oracle's existing path -- oracle.nv12_frame, then oracle.nv12_to_bgr, as expected_bgr of
tests/test_gpu_yuv420_to_bgr.py builds them, planar content interleaved for the oracle -- with channels 0 and 2 exchanged for
MI_ORDER_RGB and a fourth byte of 255 appended.  The images live in sentinel-filled (0x5A) allocations with 64 guard bytes, and the
WHOLE allocation is compared: every comparison is exact."""
import numpy as np

from test_gpu_yuv420 import SENT, EQ, Side, content, tight_frame  # noqa: F401  (re-exported)
from test_gpu_yuv420_to_bgr import SideBySide, expected_bgr  # noqa: F401  (re-exported)

ORDER_BGR, ORDER_RGB = 0, 1
# the six counters of the form: one count per call, one per batch or host call by its walk, the frames of list calls by theirs
COUNTERS = ("yuv420_bgra_onepass", "yuv420_bgra_twopass", "yuv420_bgra_vec", "yuv420_bgra_bytes",
            "yuv420_bgra_list_frames_vec", "yuv420_bgra_list_frames_bytes")
# the counters of the forms next door, which no new call may move
FOREIGN = ("nv12_bgr_onepass", "nv12_bgr_twopass", "yuv420_bgr_onepass", "yuv420_bgr_twopass", "yuv420_bgr_vec", "yuv420_bgr_bytes",
           "yuv420_bgr_list_frames_vec", "yuv420_bgr_list_frames_bytes")


def bgra_of(bgr, order, alpha=255, first=0, stride=4):
    """The H x W x 4 image of the H x W x 3 oracle image `bgr`: channels 0 and 2 exchanged for MI_ORDER_RGB, byte 3 = alpha.  `first`
    and `stride` exist for the builder's own test only: a channel offset other than 0 and a pixel stride other than 4 are the mistakes
    it must tell apart."""
    h, w = bgr.shape[:2]
    rows = np.full((h, 4 * w + 4), alpha, np.uint8)
    src = bgr if order == ORDER_BGR else bgr[:, :, ::-1]
    for ch in range(3):
        rows[:, first + ch: first + ch + stride * w: stride] = src[:, :, ch]
    return np.ascontiguousarray(rows[:, : 4 * w].reshape(h, w, 4))


def expected_bgra(w, h, n, seed, op, order, contract=False):
    """The images a call must produce for content(w, h, n, seed): the shared, read-only oracle images of expected_bgr, widened."""
    return [bgra_of(img, order) for img in expected_bgr(w, h, n, seed, op, contract)]


def with_alpha(img3):
    """an H x W x 3 image already in its final channel order -> H x W x 4 with A = 255"""
    return np.ascontiguousarray(np.concatenate([img3, np.full(img3.shape[:2] + (1,), 255, np.uint8)], axis=2))


class BgraOut:
    """n four-channel images in one sentinel-filled allocation: H rows of 4W bytes at `pitch`, frames `fstride` apart, the first
    `off` bytes into the allocation, 64 guard bytes behind the last."""

    def __init__(self, w, h, n, pitch=None, frame_gap=0, off=0):
        import torch
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = pitch or 4 * w
        self.fstride = self.pitch * h + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, images=None):
        a = np.full(self.total, SENT, np.uint8)
        for k, img in enumerate(images or []):
            o = self.off + k * self.fstride
            a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 4 * self.w] = img.reshape(self.h, 4 * self.w)
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def host(self):
        from mi_lumaeq import xfer
        return xfer.to_host(self.buf)

    def same(self, images=None):
        got, want = self.host(), self.image(images)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]

    def kw(self):
        return {"out_pitch": self.pitch, "out_frame": self.fstride}

    def terms(self):
        return {"d_out": self.off, "out_pitch": self.pitch, "out_frame_stride": self.fstride}


# ---- the documented alignment rule (include/mi_lumaeq.h), restated ----------------------------------------------------------------
def call_vec(w, planar, y, y_pitch, frame_stride, d_out, out_pitch, out_frame_stride, c0, c1, c_pitch):
    """Does a batch call walk 16 x 2 pixel groups?  W % 16 == 0; the six Y and image terms multiples of 16; the chroma terms multiples
    of 16 when interleaved (c1 is not looked at) and of 8 when planar."""
    six = all(t % 16 == 0 for t in (y, y_pitch, frame_stride, d_out, out_pitch, out_frame_stride))
    chroma = all(t % 8 == 0 for t in (c0, c1, c_pitch)) if planar else all(t % 16 == 0 for t in (c0, c_pitch))
    return w % 16 == 0 and six and chroma


def shape_vec(w, planar, y_pitch, c_pitch, out_pitch):
    """what the shape of a list call allows"""
    return w % 16 == 0 and y_pitch % 16 == 0 and out_pitch % 16 == 0 and c_pitch % (8 if planar else 16) == 0


def frame_vec(shape_ok, planar, y, c0, c1, out):
    """... and what a frame of it then decides by its own four addresses"""
    chroma = (c0 % 8 == 0 and c1 % 8 == 0) if planar else c0 % 16 == 0
    return bool(shape_ok) and y % 16 == 0 and out % 16 == 0 and chroma


def side_vec(w, src, dst):
    """call_vec on a Side / SideBySide and a BgraOut, relative to their 16-byte aligned allocations"""
    y, c0, c1 = src.offsets()
    planar = src.planar or isinstance(src, SideBySide)
    if isinstance(src, SideBySide):
        c1 = c0 + src.w // 2
    return call_vec(w, planar, y, src.y_pitch, src.fstride, dst.off, dst.pitch, dst.fstride, c0, c1 or 0, src.c_pitch)


def onepass_shape(w, h, tx, ty, max_pairs):
    """the one-pass shape: the tile grid divides the frame, tile width a multiple of 16, tiles_x + 1 pair tables in LDS"""
    return w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= max_pairs


# ---- the seeded sweep of the list form ---------------------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 7, 32


def draw_case(rng, kind):
    """W even in 2..96, H even in 2..40, 1..4 frames, a tile grid that fits the frame, a clip limit, the order, the layout (I420, YV12
    or interleaved), three pitches and per frame the offsets of (y, c0, c1, out) past a 16-byte boundary.  `aim` only steers the draw;
    classify() does not look at it."""
    aim = int(rng.integers(0, 4))                     # 0: vector one-pass, 1: vector, padded grid, 2: odd shape, 3: one frame broken
    n, order = int(rng.integers(1, 5)), int(rng.integers(0, 2))
    fmt = ("i420", "yv12", "nv12", "nv12")[int(rng.integers(0, 4))]
    clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
    tx, ty = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    if aim == 2:
        w, h = 2 * int(rng.integers(1, 49)), 2 * int(rng.integers(1, 21))
        tx, ty = min(tx, w // 2), min(ty, h // 2)
    else:
        w = 16 * tx * int(rng.integers(1, 6 // tx + 1))
        m = ty if ty % 2 == 0 else 2 * ty
        h = m * int(rng.integers(1, 40 // m + 1))
        if aim == 1:
            ty = next((t for t in range(ty + 1, ty + 4) if h % t and t <= h // 2), ty)   # REFLECT_101 padding
    crow = w if fmt == "nv12" else w // 2
    if aim == 2 and rng.random() < 0.6:
        yp, cp, op = w + int(rng.integers(0, 24)), crow + int(rng.integers(0, 24)), 4 * w + int(rng.integers(0, 24))
    else:
        yp = (w + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
        cp = (crow + 15) // 16 * 16 + 16 * int(rng.integers(0, 3)) if fmt == "nv12" else (crow + 7) // 8 * 8 + 8 * int(rng.integers(0, 3))
        op = 4 * w + 16 * int(rng.integers(0, 3))
    skews = []
    for k in range(n):
        s = [0, 0, 0, 0] if fmt == "nv12" else [0, 8 * int(rng.integers(0, 2)), 8 * int(rng.integers(0, 2)), 0]
        if aim == 3 and (k == n - 1 or rng.random() < 0.3):
            s[int(rng.integers(0, 4))] += int(rng.choice([1, 4, 8]))
        skews.append(tuple(s))
    return dict(kind=kind, w=w, h=h, n=n, tx=tx, ty=ty, clip=clip, order=order, fmt=fmt, y_pitch=yp, c_pitch=cp, out_pitch=op, skews=skews)


def classify(case, max_pairs):
    """The deltas of COUNTERS for a list call on `case` and its classes, from the header's words alone (clahe_fp_contract off):
    ((onepass, twopass, 0, 0, frames_vec, frames_bytes), {"vector" | "byte", "onepass" | "twopass", "planar" | "interleaved"})."""
    w, h, tx, ty, sk, n = case["w"], case["h"], case["tx"], case["ty"], case["skews"], case["n"]
    planar = case["fmt"] != "nv12"
    clahe = case["kind"] == "clahe"
    shape = shape_vec(w, planar, case["y_pitch"], case["c_pitch"], case["out_pitch"])
    addr = [frame_vec(shape, planar, *s) for s in sk]
    one = not clahe or (onepass_shape(w, h, tx, ty, max_pairs) and all(addr))
    if not one:                             # the decode reads the luma from aligned scratch planes: the caller's y address drops out
        addr = [frame_vec(shape, planar, 0, s[1], s[2], s[3]) for s in sk]
    nvec = sum(addr)
    classes = {"vector" if nvec == n else "byte", "onepass" if one else "twopass", "planar" if planar else "interleaved"}
    return (int(one), int(not one), 0, 0, nvec, n - nvec), classes


def refused_grid(case):
    """a tile grid with more tiles than pixels along an axis: kept out of the sweep's GPU runs"""
    return case["kind"] == "clahe" and (case["tx"] > case["w"] or case["ty"] > case["h"])


def sweep_cases(kind, seed=SWEEP_SEED):
    rng = np.random.default_rng([seed, 0 if kind == "eq" else 1])
    return [draw_case(rng, kind) for _ in range(SWEEP_CASES)]


def census(cases, max_pairs):
    out = dict.fromkeys(("vector", "byte", "onepass", "twopass", "planar", "interleaved", "refused"), 0)
    for k in cases:
        if refused_grid(k):
            out["refused"] += 1
            continue
        for name in classify(k, max_pairs)[1]:
            out[name] += 1
    return out
