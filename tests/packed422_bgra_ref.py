"""Expected bytes, the documented store-path rule, the shapes and the layouts for the tests of mi_*_packed422_to_bgra*
(tests/test_gpu_packed422_to_bgra.py, tests/test_gpu_packed422_to_bgra_frames.py; backed without a GPU by
tests/test_packed422_to_bgra_abi.py, tests/test_packed422_to_bgra_frames_abi.py and tests/test_packed422_to_bgra_shapes.py).

The expected image is packed422_bgr_ref.expected(...) -- the oracle's luma in the call's arithmetic mode, every row decoded with its OWN
chroma, the channels already in the call's order -- with a fourth channel of 255 appended.  No new oracle code.  Images live in
sentinel-filled (0x5A) allocations with guard bytes and the WHOLE allocation is compared: every comparison is exact.  This module needs
no GPU to import; the two layout classes import torch when they are built."""
import numpy as np

import packed422_bgr_ref as bgr_ref
from packed422_bgr_ref import (FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB, luma, chroma, mapped_luma,  # noqa: F401  (re-exported)
                               alternating_chroma_frame)

SENT = 0x5A
GUARD = 64
EQ = ("eq", None)
# the four counters of the form: batch and host CALLS by the store path of their launch, FRAMES of list calls by theirs
COUNTERS = ("packed422_bgra_wide", "packed422_bgra_bytes", "packed422_bgra_list_frames_wide", "packed422_bgra_list_frames_bytes")
# the counters of the forms next door, which no call of this form may move
FOREIGN = ("packed422_bgr_list_frames_wide", "packed422_bgr_list_frames_bytes", "yuv420_bgra_onepass", "yuv420_bgra_twopass",
           "yuv420_bgra_vec", "yuv420_bgra_bytes", "yuv420_bgra_list_frames_vec", "yuv420_bgra_list_frames_bytes")


def with_alpha(img3):
    """an H x W x 3 image already in its final channel order -> H x W x 4 with A = 255"""
    return np.ascontiguousarray(np.concatenate([img3, np.full(img3.shape[:2] + (1,), 255, np.uint8)], axis=2))


def expected(frame, w, fmt, order, op, cfg=None, contract=False, y_mapped=None):
    """The CV_8UC4 image of one packed frame: the three-channel reference, widened."""
    return with_alpha(bgr_ref.expected(frame, w, fmt, order, op, cfg, contract, y_mapped))


def random_frame(w, h, fmt, seed):
    """Independent random Y, U and V: H rows of 2W bytes."""
    return np.random.default_rng(seed).integers(0, 256, (h, 2 * w), dtype=np.uint8)


def frame_wide(out, out_pitch, out_frame=0):
    """The header's rule: a frame is wide when its image address is a multiple of 4 and so are out_pitch and, for a batch,
    out_frame_stride (a list passes 0)."""
    return (out | out_pitch | out_frame) % 4 == 0


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
# parity matrix: 2 x 1 one macropixel (ragged nd = 1, a band of one row); 16 x 1 one full group; 18 x 3 a full group, then nd = 1;
# 30 x 5 a full group, then nd = 7; 40 x 6 two full groups and a ragged one of 8 columns (nd = 4); 66 x 34 four full groups, nd = 1
PARITY_SHAPES = [(2, 1), (16, 1), (18, 3), (30, 5), (40, 6), (66, 34)]
# equalizeHist; CLAHE whose grid divides every width above (or pads); a grid that pads (REFLECT_101); 65 pairs: the global kernel
CL22, CL54, CL642 = ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 5, 4)), ("clahe", (2.0, 64, 2))
PARITY_OPS = [EQ, CL22, CL54, CL642]
LDS_OPS = (CL22, CL54)
OPTIONS = [(1, 0), (0, 0), (1, 1), (0, 1)]           # (clahe_float_tables, clahe_fp_contract): the four <FT, FMA> rungs
OUT_LAYOUTS = ["aligned16", "aligned4", "odd", "tight"]
K_MAX_PAIRS = 63                                      # kMaxPairsLds (kernels/clahe.hip.h); tests/clahe_u8_rungs.py reads it from there

# walks past their first step: (id, W, H, n, op).  The apply kernel keeps lut_apply422_bgr_body's walk:
# packed422_geometry_cases.walk("lut_apply422_bgr", W, H) gives (items of the smallest band, G, step 256, bound on B)
LOOP_SHAPES = [
    # 2WH / 16384 = 3.1: up to three bands of 128 / 129 / 129 rows; G = 5, drow 51, dgrp 1: 640 / 645 / 645 items, three steps each, and
    # the group wraps into the next row; two frames
    ("66x386x2", 66, 386, 2, EQ),
    # one row of 32772 bytes: B may be 2, and then band 0 has no rows; G = 1025 > 256: drow 0, dgrp 256, a lane walks along the row,
    # five steps, the last of one item
    ("16386x1", 16386, 1, 1, EQ),
    # CLAHE 2 x 2 on 64 x 200: 4 column groups, 64 phases, many bands and sub-bands of full groups.  (A sub-band holds rows_per_band /
    # subs rows, about 8 once the chip wants more workgroups than there are bands: fewer than the 64 phases, so every lane has at most
    # ONE row here and takes the one-row loop -- tests/test_packed422_to_bgra_shapes.py does the arithmetic.  The shape below is the
    # one whose lanes own several rows.)
    ("64x200-cl22", 64, 200, 1, CL22),
    # 31 dwords: the fourth group of every row is ragged (nd = 7) over all 200 rows
    ("62x200-cl22", 62, 200, 1, CL22),
    # 65 column groups in one segment, 256 / 65 = 3 phases; sub-bands of 8 or 9 rows: a lane owns two or three rows of its sub-band, so
    # the two-rows-in-flight loop runs, and for the lanes with three rows its one-row tail behind it
    ("1040x44-cl22", 1040, 44, 1, CL22),
]


def out_layout(w, name):
    """(pitch, gap between frames, base offset) of an image allocation.  aligned16: base, pitch and frame stride multiples of 16;
    aligned4: multiples of 4 and the pitch no multiple of 16; odd: an odd base with pitch 4W + 1; tight: pitch 4W, no gap."""
    if name == "aligned16":
        return (4 * w + 15) // 16 * 16 + 16, 32, 0
    if name == "aligned4":
        pitch = 4 * w + 4
        return (pitch + 4 if pitch % 16 == 0 else pitch), 8, 4
    if name == "odd":
        return 4 * w + 1, 3, 5
    return 4 * w, 0, 0


class Batch:
    """n packed frames in one sentinel-filled allocation: rows of 2W bytes at `pitch`, frames `fstride` apart, first frame `off` in."""

    def __init__(self, w, h, n, layout=(0, 0, 0)):
        import torch
        extra, gap, off = layout
        self.w, self.h, self.n, self.off = w, h, n, off
        self.pitch = 2 * w + extra
        self.fstride = self.pitch * h + gap
        self.total = off + self.fstride * n + GUARD
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def image(self, frames=None):
        a = np.full(self.total, SENT, np.uint8)
        if frames is not None:
            for k, f in enumerate(frames):
                o = self.off + k * self.fstride
                a[o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : 2 * self.w] = f[:, : 2 * self.w]
        return a

    def upload(self, frames):
        import torch
        self.buf.copy_(torch.from_numpy(self.image(frames)))
        return self

    def host(self):
        return self.buf.cpu().numpy()

    def kw(self):
        return {"in_pitch": self.pitch, "in_frame": self.fstride}


class BgraOut:
    """n four-channel images in one sentinel-filled allocation: rows of 4W bytes at `pitch`, images `fstride` apart, the first `off`
    bytes in, GUARD bytes behind the last."""

    def __init__(self, w, h, n, layout="aligned16", pitch=None, fstride=None, off=None):
        import torch
        self.w, self.h, self.n = w, h, n
        p, gap, o = out_layout(w, layout)
        self.pitch = p if pitch is None else pitch
        self.off = o if off is None else off
        self.fstride = self.pitch * h + gap if fstride is None else fstride
        assert self.pitch >= 4 * w and (n == 1 or self.fstride >= self.pitch * (h - 1) + 4 * w)
        self.total = self.off + self.fstride * (n - 1) + self.pitch * h + GUARD
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    @property
    def wide(self):
        return frame_wide(self.ptr, self.pitch, self.fstride)

    def image(self, images=None):
        a = np.full(self.total, SENT, np.uint8)
        if images is not None:
            for k, im in enumerate(images):
                o = self.off + k * self.fstride
                rows = np.lib.stride_tricks.as_strided(a[o:], shape=(self.h, 4 * self.w), strides=(self.pitch, 1))
                rows[:] = im.reshape(self.h, 4 * self.w)
        return a

    def clear(self):
        self.buf.fill_(SENT)

    def host(self):
        return self.buf.cpu().numpy()

    def same(self, images=None):
        return np.array_equal(self.host(), self.image(images))

    def kw(self):
        return {"out_pitch": self.pitch, "out_frame": self.fstride}
