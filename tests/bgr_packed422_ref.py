"""The reference, the layouts and the documented alignment rule for interleaved BGR / RGB in, packed 4:2:2 (YUY2 / UYVY) out
(mi_*_bgr_to_packed422*), built from oracle functions that exist: no new oracle code.

oracle.bgr_to_nv12 takes Y from every pixel and U, V from the top-left pixel of each 2 x 2 block.  On the image with every row doubled
(np.repeat(img, 2, axis=0)) Y row 2r is therefore the luma of image row r and UV row r is that row's left-pixel U V U V ...: the
header's definition of the packed frame's chroma (the 4:2:0 rule applied to every row on its own).  The luma is then mapped by
oracle.equalize_hist / oracle.clahe in the arithmetic mode of the call (oracle.set_fp_contract), the bytes interleaved by format, and
RGB order is the channel flip.  tests/test_bgr_to_packed422_abi.py backs the builder without a GPU against a NumPy restatement of
bt601_y / bt601_uv.

The input images and the output frames of the GPU tests live in sentinel-filled (0x5A) allocations with 64 guard bytes and the WHOLE
allocation is compared: every comparison is exact."""
import numpy as np

import oracle
from bgr_yuv420_layouts import SENT, BgrIn, rand_images  # noqa: F401  (the input side is the BGR -> 4:2:0 tests' own)

FMT_YUY2, FMT_UYVY = 2, 3
ORDER_BGR, ORDER_RGB = 0, 1
UV_FILL128, UV_COPY = 0, 1
COUNTERS = ("bgr_packed422_vec", "bgr_packed422_bytes")


def convert(img, order=ORDER_BGR):
    """H x W x 3 (in the order the call is told) -> (H x W unequalized luma, H x W chroma U V U V ... of the left pixel of each macropixel)."""
    h, w = img.shape[:2]
    assert w % 2 == 0
    bgr = img if order == ORDER_BGR else img[:, :, ::-1]
    nv12 = oracle.bgr_to_nv12(np.ascontiguousarray(np.repeat(bgr, 2, axis=0)))
    return np.ascontiguousarray(nv12[: 2 * h * w].reshape(2 * h, w)[0::2]), nv12[2 * h * w:].reshape(h, w).copy()


def mapped_luma(y, op, contract=False):
    """oracle.equalize_hist (("eq", None)) or oracle.clahe(*cfg) (("clahe", cfg)) on a luma plane, in the given arithmetic mode."""
    kind, cfg = op
    if kind == "eq":
        return oracle.equalize_hist(y)
    old = oracle.set_fp_contract(bool(contract))
    try:
        return oracle.clahe(y, *cfg)
    finally:
        oracle.set_fp_contract(old)


def pack(y, uv, fmt):
    """H x W luma and H x W chroma -> H x 2W packed frame: exactly Y0 U Y1 V (YUY2) or U Y0 V Y1 (UYVY)."""
    h, w = y.shape
    f = np.empty((h, 2 * w), np.uint8)
    f[:, fmt - 2::2] = y
    f[:, 3 - fmt::2] = uv
    return f


def expected(img, op, order, fmt, uv_mode, contract=False):
    """The tight H x 2W frame the call must produce for `img`; op None: the unequalized frame stage 1 leaves."""
    y, uv = convert(img, order)
    if uv_mode == UV_FILL128:
        uv = np.full_like(uv, 128)
    return pack(y if op is None else mapped_luma(y, op, contract), uv, fmt)


def formula(img, order=ORDER_BGR):
    """convert() restated in NumPy from the constants in the comment of oracle/color_oracle.c (OpenCV 4.4 ITUR_BT_601, shift 20), the
    chroma from the left pixel of every macropixel of every row."""
    b, g, r = (img[:, :, k if order == ORDER_BGR else 2 - k].astype(np.int64) for k in range(3))
    sat = lambda v: np.clip(v >> 20, 0, 255).astype(np.uint8)  # noqa: E731
    y = sat(269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20))
    bl, gl, rl = b[:, 0::2], g[:, 0::2], r[:, 0::2]
    uv = np.empty(y.shape, np.uint8)
    uv[:, 0::2] = sat(-155188 * rl - 305135 * gl + 460324 * bl + (1 << 19) + (128 << 20))
    uv[:, 1::2] = sat(460324 * rl - 385875 * gl - 74448 * bl + (1 << 19) + (128 << 20))
    return y, uv


class P422Out:
    """n packed frames in ONE sentinel-filled allocation: frame f at off + f * fstride, H rows of 2W bytes at `pitch`."""

    def __init__(self, w, h, n, pitch=None, frame_gap=0, off=0):
        import torch
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = pitch or 2 * w
        self.fstride = self.pitch * h + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def kw(self):
        return {"out_pitch": self.pitch, "out_frame": self.fstride}

    def image(self, frames=None):
        """The whole allocation with the tight H x 2W `frames` of expected() in place."""
        a = np.full(self.total, SENT, np.uint8)
        for k, f in enumerate(frames or []):
            o = self.off + k * self.fstride
            a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 2 * self.w] = f
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def host(self):
        from mi_lumaeq import xfer
        return xfer.to_host(self.buf)

    def same(self, frames=None):
        got, want = self.host(), self.image(frames)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]

    def terms(self):
        return {"out": self.off, "out_pitch": self.pitch, "out_frame": self.fstride}


def misaligned(w, src, dst):
    """The documented rule (include/mi_lumaeq.h), restated: the terms that keep a call off the 16-pixel groups, relative to the 16-byte
    aligned allocations: every one of the six a multiple of 16, and W % 16 == 0."""
    t = dict(src.terms(), **dst.terms())
    return sorted(k for k, v in t.items() if v % 16) + (["width"] if w % 16 else [])
