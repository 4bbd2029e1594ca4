"""The reference, the layouts and the documented alignment rule for 4:2:0 (NV12 / I420 / YV12) in, packed 4:2:2 (YUY2 / UYVY) out
(mi_*_yuv420_to_packed422*), built from pieces that exist: no new oracle code.

The frame a call must produce is bgr_packed422_ref.pack(mapped_luma(Y), np.repeat(UV row, 2, axis=0), fmt): the luma mapped by
oracle.equalize_hist / oracle.clahe in the arithmetic mode of the call, and input chroma row r, as an NV12 row U0 V0 U1 V1 ..., under both
output rows 2r and 2r+1 (MI_UV_COPY) or 128 (MI_UV_FILL128).  Content is test_gpu_yuv420.content (full-range random planes, U and V drawn
independently), the input side is test_gpu_yuv420.Side and the output side bgr_packed422_ref.P422Out: sentinel-filled (0x5A)
allocations with 64 guard bytes of which the WHOLE is compared: every comparison is exact.  tests/test_yuv420_to_packed422_abi.py backs
the builder without a GPU."""
import numpy as np

from bgr_packed422_ref import FMT_YUY2, FMT_UYVY, UV_COPY, UV_FILL128, SENT, P422Out, mapped_luma, pack  # noqa: F401
from test_gpu_yuv420 import Side, content  # noqa: F401

PASS_COUNTERS = ("yuv420_packed422_onepass", "yuv420_packed422_twopass")
WALK_COUNTERS = ("yuv420_packed422_vec", "yuv420_packed422_bytes")
COUNTERS = PASS_COUNTERS + WALK_COUNTERS
SRC_FMTS = ("nv12", "i420", "yv12")
_ref = {}


def uv_rows(u, v):
    """H/2 x W/2 U and V planes -> the H/2 x W interleaved rows U0 V0 U1 V1 ... an NV12 frame holds."""
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


def expected_frame(planes, op, fmt, uv_mode, contract=False):
    """The tight H x 2W frame the call must produce for one (Y, U, V) of content(); op None: the luma unmapped.  The mapped luma of a
    frame is computed once and shared (it is the expensive part and does not depend on the format or the UV mode)."""
    y, u, v = planes
    if op is None:
        yy = y
    else:
        key = (y.shape, y.tobytes(), op, bool(contract))
        if key not in _ref:
            _ref[key] = mapped_luma(np.ascontiguousarray(y), op, contract)
        yy = _ref[key]
    uv = np.repeat(uv_rows(u, v), 2, axis=0)
    return pack(yy, uv if uv_mode == UV_COPY else np.full_like(uv, 128), fmt)


def expected(w, h, n, seed, op, fmt, uv_mode, contract=False):
    return [expected_frame(p, op, fmt, uv_mode, contract) for p in content(w, h, n, seed)]


def chroma_back_to_nv12(frame, fmt):
    """mi_*_packed422_to_nv12's chroma rule restated in NumPy: UV row r of the NV12 frame is the rounded-up mean of the chroma bytes of
    packed rows 2r and 2r+1."""
    c = frame[:, 3 - fmt::2].astype(np.uint16)
    return ((c[0::2] + c[1::2] + 1) >> 1).astype(np.uint8)


def misaligned(src, dst, uv_mode=UV_COPY):
    """The documented rule (include/mi_lumaeq.h), restated: the terms that keep a call off the 16 x 2 pixel groups, relative to the
    16-byte aligned allocations.  The Y and output terms are multiples of 16; under MI_UV_COPY the chroma terms are multiples of 16
    (interleaved) or of 8 (planar); W % 16 == 0."""
    yo, c0, c1 = src.offsets()
    t = {"y": yo % 16, "y_pitch": src.y_pitch % 16, "frame_stride": src.fstride % 16}
    t.update({k: v % 16 for k, v in dst.terms().items()})
    if uv_mode == UV_COPY:
        m = 8 if src.planar else 16
        t.update({"c0": c0 % m, "c_pitch": src.c_pitch % m})
        if src.planar:
            t["c1"] = c1 % m
    return sorted(k for k, v in t.items() if v) + (["width"] if src.w % 16 else [])


def onepass_clahe(src, dst, cfg, uv_mode=UV_COPY, contract=False):
    """The header's rule for the one-pass CLAHE, restated: the tile grid divides the frame, the tile width is a multiple of 16,
    clahe_fp_contract is off and every alignment term but the width holds (the width follows from the tile width)."""
    _, tx, ty = cfg
    w, h = src.w, src.h
    return (not contract and w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= 15 and
            [t for t in misaligned(src, dst, uv_mode) if t != "width"] == [])
