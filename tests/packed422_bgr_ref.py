"""The reference for packed 4:2:2 in (YUY2 / UYVY), interleaved BGR / RGB out, built from oracle functions that exist: no new oracle code.

oracle.nv12_to_bgr decodes row y with chroma row y // 2.  A packed frame of height H, whose every row carries its own chroma, therefore
decodes exactly like an NV12 frame of height 2H whose Y rows 2r and 2r + 1 both hold (mapped) luma row r and whose UV row r holds packed
row r's chroma as U V U V ...: the even rows of that image are the answer.  RGB order is the channel flip.  The mapped luma is
oracle.equalize_hist / oracle.clahe on the gathered luma, in the arithmetic mode of the call (oracle.set_fp_contract)."""
import numpy as np

import oracle

FMT_YUY2, FMT_UYVY = 2, 3
ORDER_BGR, ORDER_RGB = 0, 1


def luma(frame, w, fmt):
    """The W luma bytes of every row: byte offset 0 (YUY2) or 1 (UYVY) of each 2-byte pixel."""
    return np.ascontiguousarray(frame[:, fmt - 2:2 * w:2])


def chroma(frame, w, fmt):
    """The W chroma bytes of every row, U V U V ... for exactly Y0 U Y1 V (YUY2) and U Y0 V Y1 (UYVY)."""
    return np.ascontiguousarray(frame[:, 3 - fmt:2 * w:2])


def decode(y, uv, order=ORDER_BGR):
    """H x W luma and H x W chroma (U V U V ... per row, one pair per macropixel) -> H x W x 3, through oracle.nv12_to_bgr on the
    row-doubled NV12 frame."""
    h, w = y.shape
    assert uv.shape == (h, w) and w % 2 == 0
    nv12 = np.concatenate([np.repeat(y, 2, axis=0).reshape(-1), np.ascontiguousarray(uv).reshape(-1)])
    bgr = oracle.nv12_to_bgr(nv12, w, 2 * h)[0::2]
    return np.ascontiguousarray(bgr if order == ORDER_BGR else bgr[:, :, ::-1])


def mapped_luma(y, op, cfg=None, contract=False):
    """oracle.equalize_hist (op "eq") or oracle.clahe(*cfg) (op "clahe") on a luma plane, in the given arithmetic mode."""
    if op == "eq":
        return oracle.equalize_hist(y)
    old = oracle.set_fp_contract(bool(contract))
    try:
        return oracle.clahe(y, *cfg)
    finally:
        oracle.set_fp_contract(old)


def expected(frame, w, fmt, order, op, cfg=None, contract=False, y_mapped=None):
    """The image of one packed frame (H rows of at least 2W bytes); y_mapped: the mapped luma when the caller has it cached."""
    if y_mapped is None:
        y_mapped = mapped_luma(luma(frame, w, fmt), op, cfg, contract)
    return decode(y_mapped, chroma(frame, w, fmt), order)


def decode_formula(y, uv, order=ORDER_BGR):
    """The decode restated in NumPy from the constants in the comment of oracle/color_oracle.c (OpenCV 4.4 ITUR_BT_601, shift 20)."""
    yy = np.maximum(0, y.astype(np.int64) - 16) * 1220542
    u = np.repeat(uv[:, 0::2].astype(np.int64) - 128, 2, axis=1)
    v = np.repeat(uv[:, 1::2].astype(np.int64) - 128, 2, axis=1)
    r = (yy + (1 << 19) + 1673527 * v) >> 20
    g = (yy + (1 << 19) - 852492 * v - 409993 * u) >> 20
    b = (yy + (1 << 19) + 2116026 * u) >> 20
    ch = (b, g, r) if order == ORDER_BGR else (r, g, b)
    return np.stack([np.clip(c, 0, 255).astype(np.uint8) for c in ch], axis=2)


def alternating_chroma_frame(w, h, fmt, seed=0):
    """A frame that tells 4:2:2 from 4:2:0: even rows carry strong chroma, odd rows chroma 128, the luma is random."""
    rng = np.random.default_rng(seed)
    f = np.empty((h, 2 * w), np.uint8)
    f[:, fmt - 2::2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    c = np.full((h, w), 128, np.uint8)
    c[0::2, 0::2] = 30 + (np.arange(w // 2, dtype=np.int64) * 7 % 40).astype(np.uint8)       # U far below 128
    c[0::2, 1::2] = 220 - (np.arange(w // 2, dtype=np.int64) * 5 % 30).astype(np.uint8)      # V far above 128
    f[:, 3 - fmt::2] = c
    return f
