"""Layouts, expected bytes and the documented alignment rule for the tests of mi_*_bgr_to_yuv420* (tests/test_gpu_bgr_to_yuv420.py; the
builder of the expected bytes is backed without a GPU by tests/test_bgr_to_yuv420_abi.py).  The input images and the three output planes
live in sentinel-filled (0x5A) allocations with 64 guard bytes, and the WHOLE allocation is compared: every comparison is exact."""
import numpy as np

import oracle

SENT = 0x5A
ORDER_BGR, ORDER_RGB = 0, 1
COUNTERS = ("bgr_yuv420_vec", "bgr_yuv420_bytes")


def rand_images(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


def deinterleave(nv12, w, h):
    """A tight NV12 frame as a tight I420 frame: Y, then the U bytes, then the V bytes."""
    ysz = w * h
    uv = nv12[ysz:]
    return np.concatenate([nv12[:ysz], uv[0::2], uv[1::2]])


def expected(img, op, order, uv_mode):
    """The tight I420 frame of W*H*3/2 bytes the call must produce for `img` (H x W x 3, in the order the call is told): Y is
    oracle.nv12_frame(oracle.bgr_to_nv12(bgr), ...)[:W*H], U and V that frame's chroma de-interleaved."""
    kind, cfg = op
    h, w = img.shape[:2]
    bgr = img if order == ORDER_BGR else np.ascontiguousarray(img[:, :, ::-1])
    nv12 = oracle.bgr_to_nv12(bgr)
    out = oracle.nv12_frame(nv12, w, h, uv_mode, 0) if kind == "eq" else oracle.nv12_frame(nv12, w, h, uv_mode, 1, *cfg)
    return deinterleave(out, w, h)


def as_fmt(i420, w, h, fmt):
    """The tight I420 frame of expected() laid out as a tight "i420", "yv12" or "nv12" frame."""
    ysz, csz = w * h, w * h // 4
    y, u, v = i420[:ysz], i420[ysz: ysz + csz], i420[ysz + csz:]
    if fmt == "i420":
        return i420
    if fmt == "yv12":
        return np.concatenate([y, v, u])
    return np.concatenate([y, np.stack([u, v], axis=1).reshape(-1)])


class BgrIn:
    """n interleaved images in one sentinel-filled allocation: H rows of 3W bytes at `pitch`, frames `fstride` apart."""

    def __init__(self, w, h, n, pitch=None, frame_gap=0, off=0):
        import torch
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


class Yuv420Out:
    """n planar 4:2:0 frames in ONE sentinel-filled allocation.  Frame f starts at off + f * fstride with its Y plane (H rows of W bytes
    at y_pitch); u_gap bytes lie before its U plane and v_gap bytes before its V plane (each H/2 rows of W/2 bytes at c_pitch), which
    follow the Y rows in the order U, V -- or V, U with v_first (YV12); frame_gap bytes lie before the next frame.  side_by_side: ONE
    pitched chroma plane of H/2 rows at c_pitch >= W holds the U rows and, W/2 bytes further, the V rows (c1 = c0 + W/2; u_gap lies
    before it, v_gap is not used)."""

    def __init__(self, w, h, n, y_pitch=None, c_pitch=None, u_gap=0, v_gap=0, frame_gap=0, off=0, v_first=False, side_by_side=False):
        import torch
        self.w, self.h, self.n, self.off = w, h, n, off
        self.y_pitch = y_pitch or w
        self.c_pitch = c_pitch or (w if side_by_side else w // 2)
        plane = self.c_pitch * (h // 2)
        end_y = self.y_pitch * h
        if side_by_side:
            first = end_y + u_gap
            self.u_off, self.v_off = (first + w // 2, first) if v_first else (first, first + w // 2)
            end = first + plane
        elif v_first:
            self.v_off = end_y + v_gap
            self.u_off = self.v_off + plane + u_gap
            end = self.u_off + plane
        else:
            self.u_off = end_y + u_gap
            self.v_off = self.u_off + plane + v_gap
            end = self.v_off + plane
        self.fstride = end + frame_gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def y_ptr(self):
        return self.buf.data_ptr() + self.off

    @property
    def u_ptr(self):
        return self.y_ptr + self.u_off

    @property
    def v_ptr(self):
        return self.y_ptr + self.v_off

    def planes(self):
        import mi_lumaeq
        return mi_lumaeq.Yuv420Planes(self.y_ptr, self.y_pitch, self.u_ptr, self.v_ptr, self.c_pitch, self.fstride, mi_lumaeq.CHROMA_PLANAR)

    def image(self, frames=None):
        """The whole allocation with the tight I420 `frames` of expected() in place."""
        a = np.full(self.total, SENT, np.uint8)
        w, h = self.w, self.h
        ysz, csz, rows = w * h, w * h // 4, h // 2
        for k, f in enumerate(frames or []):
            o = self.off + k * self.fstride
            a[o: o + self.y_pitch * h].reshape(h, self.y_pitch)[:, :w] = f[:ysz].reshape(h, w)
            for po, plane in ((self.u_off, f[ysz: ysz + csz]), (self.v_off, f[ysz + csz:])):
                p = plane.reshape(rows, w // 2)
                for r in range(rows):
                    s = o + po + r * self.c_pitch
                    a[s: s + w // 2] = p[r]
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def same(self, frames=None):
        from mi_lumaeq import xfer
        got, want = xfer.to_host(self.buf), self.image(frames)
        return np.array_equal(got, want), int((got != want).sum()), np.flatnonzero(got != want)[:8]

    def terms(self):
        return {"y": self.off, "y_pitch": self.y_pitch, "c0": self.off + self.u_off, "c1": self.off + self.v_off, "c_pitch": self.c_pitch,
                "frame_stride": self.fstride}


def misaligned(w, src, dst):
    """The documented rule (include/mi_lumaeq.h), restated: the terms that keep a PLANAR call off the 16 x 2 pixel groups, relative to
    the 16-byte aligned allocations.  Multiples of 16 for the image and Y terms, of 8 for the chroma terms."""
    t = dict(src.terms(), **dst.terms())
    bad = sorted(k for k, v in t.items() if v % (8 if k in ("c0", "c1", "c_pitch") else 16))
    return bad + (["width"] if w % 16 else [])
