"""The reference, the layouts and the documented alignment rule for four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 (YUY2 / UYVY)
out (mi_*_bgra_to_packed422*): no new oracle code.  The expected bytes are the three-channel builder's (bgr_packed422_ref.expected) on
the image with its fourth byte removed; the input side is the BGRA -> 4:2:0 tests' own (BgraIn, rand_images4: full-range random bytes,
the fourth byte included), the output side the BGR -> packed 4:2:2 tests' own (P422Out).  tests/test_bgra_to_packed422_abi.py backs the
builder without a GPU.

The input images and the output frames of the GPU tests live in sentinel-filled (0x5A) allocations with 64 guard bytes and the WHOLE
allocation is compared: every comparison is exact."""
import numpy as np

import bgr_packed422_ref as ref3
from bgr_packed422_ref import (FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB, UV_FILL128, UV_COPY, P422Out, convert, mapped_luma,  # noqa: F401
                               pack, formula)
from bgra_yuv420_layouts import SENT, BgraIn, rand_images4  # noqa: F401

COUNTERS = ("bgra_packed422_vec", "bgra_packed422_bytes")
LIST_COUNTERS = ("bgra_packed422_list_frames_vec", "bgra_packed422_list_frames_bytes")
# no call of this form may move one of these
SIBLING_COUNTERS = ("bgr_packed422_vec", "bgr_packed422_bytes", "bgr_packed422_list_frames_vec", "bgr_packed422_list_frames_bytes")


def first3(img):
    """The H x W x 4 image with its fourth byte removed, contiguous."""
    assert img.ndim == 3 and img.shape[2] == 4
    return np.ascontiguousarray(img[:, :, :3])


def expected(img, op, order, fmt, uv_mode, contract=False):
    """The tight H x 2W frame the call must produce for the H x W x 4 `img`: the three-channel reference on its first three channels."""
    return ref3.expected(first3(img), op, order, fmt, uv_mode, contract)


def with_x(images, x):
    """The same images with every fourth byte set to `x` (an int), or to fresh random bytes (x = "random"): all colour bytes equal."""
    out = [img.copy() for img in images]
    rng = np.random.default_rng(977)
    for img in out:
        img[:, :, 3] = rng.integers(0, 256, img.shape[:2], dtype=np.uint8) if x == "random" else x
    return out


def misaligned(w, src, dst):
    """The documented rule (include/mi_lumaeq.h), restated: the terms that keep a call off the 16-pixel groups, relative to the 16-byte
    aligned allocations: every one of the six a multiple of 16, and W % 16 == 0."""
    t = dict(src.terms(), **dst.terms())
    return sorted(k for k, v in t.items() if v % 16) + (["width"] if w % 16 else [])


def frame_vec(w, in_pitch, out_pitch, in_addr, out_addr):
    """The list form's rule, restated: the shape allows the groups (W % 16 == 0, both pitches multiples of 16) and the frame's own two
    addresses are multiples of 16."""
    return w % 16 == 0 and in_pitch % 16 == 0 and out_pitch % 16 == 0 and in_addr % 16 == 0 and out_addr % 16 == 0
