"""Layouts, expected bytes and the documented alignment rule for the tests of mi_*_bgra_to_yuv420* (tests/test_gpu_bgra_to_yuv420.py,
tests/test_gpu_bgra_to_yuv420_frames.py; the builder of the expected bytes is backed without a GPU by tests/test_bgra_to_yuv420_abi.py).
The expected bytes are the three-channel builder's (bgr_yuv420_layouts.expected) on the first three channels of the four-channel image:
the fourth byte takes no part.  The input images and the output planes live in sentinel-filled (0x5A) allocations with 64 guard bytes,
and the WHOLE allocation is compared: every comparison is exact."""
import numpy as np

from bgr_yuv420_layouts import SENT, ORDER_BGR, ORDER_RGB, Yuv420Out, as_fmt, deinterleave, expected  # noqa: F401  (re-exported)

COUNTERS = ("bgra_yuv420_vec", "bgra_yuv420_bytes")
LIST_COUNTERS = ("bgra_yuv420_list_frames_vec", "bgra_yuv420_list_frames_bytes")


def rand_images4(w, h, n, seed):
    """n full-range random H x W x 4 images: the fourth byte is random too, never constant."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]


def expected4(img, op, order, uv_mode):
    """The tight I420 frame of W*H*3/2 bytes the call must produce for the H x W x 4 `img`: the three-channel oracle on the image with
    its fourth byte removed."""
    return expected(np.ascontiguousarray(img[:, :, :3]), op, order, uv_mode)


def complement_x(images):
    """The same images with every fourth byte complemented: all colour bytes equal, every X byte different."""
    out = [img.copy() for img in images]
    for img in out:
        img[:, :, 3] ^= 0xFF
    return out


class BgraIn:
    """n four-channel images in one sentinel-filled allocation: H rows of 4W bytes at `pitch`, frames `fstride` apart."""

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

    def image(self, images):
        a = np.full(self.total, SENT, np.uint8)
        for k, img in enumerate(images):
            o = self.off + k * self.fstride
            a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 4 * self.w] = img.reshape(self.h, 4 * self.w)
        return a

    def upload(self, images):
        from mi_lumaeq import xfer
        self.buf.copy_(xfer.to_device(self.image(images)))
        return self

    def host(self):
        from mi_lumaeq import xfer
        return xfer.to_host(self.buf)

    def kw(self):
        return {"in_pitch": self.pitch, "in_frame": self.fstride}

    def terms(self):
        return {"in": self.off, "in_pitch": self.pitch, "in_frame": self.fstride}


class Nv12Out:
    """n NV12 frames in ONE sentinel-filled allocation.  Frame f starts at off + f * fstride with its Y plane (H rows of W bytes at
    y_pitch); uv_gap bytes lie before its UV plane (H/2 rows of W bytes at c_pitch); frame_gap bytes lie before the next frame."""
    planar = False

    def __init__(self, w, h, n, y_pitch=None, c_pitch=None, uv_gap=0, frame_gap=0, off=0):
        import torch
        self.w, self.h, self.n, self.off = w, h, n, off
        self.y_pitch = y_pitch or w
        self.c_pitch = c_pitch or w
        self.uv_off = self.y_pitch * h + uv_gap
        self.fstride = self.uv_off + self.c_pitch * (h // 2) + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def y_ptr(self):
        return self.buf.data_ptr() + self.off

    @property
    def uv_ptr(self):
        return self.y_ptr + self.uv_off

    def planes(self):
        import mi_lumaeq
        return mi_lumaeq.Yuv420Planes(self.y_ptr, self.y_pitch, self.uv_ptr, None, self.c_pitch, self.fstride, mi_lumaeq.CHROMA_INTERLEAVED)

    def image(self, frames=None):
        """The whole allocation with the tight I420 `frames` of expected4() in place, their chroma interleaved."""
        a = np.full(self.total, SENT, np.uint8)
        w, h = self.w, self.h
        ysz = w * h
        for k, f in enumerate(frames or []):
            nv12 = as_fmt(f, w, h, "nv12")
            o = self.off + k * self.fstride
            a[o: o + self.y_pitch * h].reshape(h, self.y_pitch)[:, :w] = nv12[:ysz].reshape(h, w)
            uv = nv12[ysz:].reshape(h // 2, w)
            for r in range(h // 2):
                s = o + self.uv_off + r * self.c_pitch
                a[s: s + w] = uv[r]
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def same(self, frames=None):
        from mi_lumaeq import xfer
        got, want = xfer.to_host(self.buf), self.image(frames)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]

    def terms(self):
        return {"y": self.off, "y_pitch": self.y_pitch, "c0": self.off + self.uv_off, "c_pitch": self.c_pitch, "frame_stride": self.fstride}


def is_planar(dst):
    return getattr(dst, "planar", True)


def misaligned(w, src, dst):
    """The documented rule (include/mi_lumaeq.h), restated: the terms that keep a call off the 16 x 2 pixel groups, relative to the
    16-byte aligned allocations.  Multiples of 16 for the image and Y terms; for the chroma terms multiples of 16 on an interleaved
    output (c0, c_pitch: one 16-byte UV store) and of 8 on a planar one (c0, c1, c_pitch: an 8-byte U and an 8-byte V store)."""
    t = dict(src.terms(), **dst.terms())
    cmod = 8 if is_planar(dst) else 16
    bad = sorted(k for k, v in t.items() if v % (cmod if k in ("c0", "c1", "c_pitch") else 16))
    return bad + (["width"] if w % 16 else [])
