"""Packed 4:2:2 in, BGR / RGB out (mi_*_packed422_to_bgr*) at the ABI level, without a GPU: the header declares the four entry points
with their parameter lists and says that the chroma order matters here, the binding lists the symbols and has the four Context methods,
both libraries export them, a null context is refused without touching the caller's buffers -- and the reference the GPU tests use
(tests/packed422_bgr_ref.py) is checked against a NumPy restatement of the decode, against known answers, and for telling 4:2:2 from
4:2:0."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import packed422_bgr_ref as ref
from packed422_bgr_ref import FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1

DEV = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride, "
       "int width, int height, int n_frames, int format, int order")
HOST = "mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step, int width, int height, int format, int order"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_packed422_to_bgr_batch_dev": DEV + ", void* stream",
    "mi_clahe_packed422_to_bgr_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_packed422_to_bgr": HOST,
    "mi_clahe_packed422_to_bgr": HOST + CLAHE,
}
NAMES = list(PARAMS)


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    assert _norm(m.group(1)) == _norm(PARAMS[name])


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3), ("MI_ORDER_BGR", 0), ("MI_ORDER_RGB", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert not re.search(r"\bMI_FMT_\w+\s*=\s*4\b", txt), "no new format value"


def test_header_states_the_contract():
    """What a caller cannot guess: the chroma order matters here (and YVYU is not served), odd heights, no output alignment rule."""
    m = re.search(r"/\*\s*mi_\*_packed422_to_bgr\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> BGR forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("CHROMA ORDER MATTERS", "exactly Y0 U Y1 V", "exactly U Y0 V Y1", "YVYU", "does not hold", "odd heights are legal",
                   "No alignment is required of d_out", "W % 4 == 2", "slower, the same bytes out", "never written", "MI_ERR_BUSY",
                   "no uv_mode parameter", "d_out == d_in", "shift 20"):
        assert needle in txt, needle


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_bgr_batch_dev", "clahe_packed422_to_bgr_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        for kw in ("in_pitch", "in_frame", "out_pitch", "out_frame", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
        assert params["fmt"].default == FMT_YUY2 and params["order"].default == ORDER_BGR
    for m in ("equalize_hist_packed422_to_bgr", "clahe_packed422_to_bgr"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert params["out"].default is None and params["fmt"].default == FMT_YUY2 and params["order"].default == ORDER_BGR


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (h, 2 * w), dtype=np.uint8)
    dst = np.full(3 * w * h, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    dev = (None, src.ctypes.data, 2 * w, 2 * w * h, dst.ctypes.data, 3 * w, 3 * w * h, w, h, 1, FMT_YUY2, ORDER_BGR)
    host = (None, src.ctypes.data, 2 * w, dst.ctypes.data, 3 * w, w, h, FMT_YUY2, ORDER_BGR)
    assert built_lib.mi_equalize_hist_packed422_to_bgr_batch_dev(*dev, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_bgr_batch_dev(*dev, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_equalize_hist_packed422_to_bgr(*host) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_bgr(*host, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


# ---- the reference helper ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FMT_YUY2, FMT_UYVY])
@pytest.mark.parametrize("order", [ORDER_BGR, ORDER_RGB])
@pytest.mark.parametrize("w,h", [(2, 1), (2, 3), (18, 5), (64, 4), (50, 13)])
def test_doubled_row_reference_equals_the_formula(w, h, fmt, order):
    """The helper's route through oracle.nv12_to_bgr on a row-doubled NV12 frame gives what the decode formula, restated from the
    constants in the comment of oracle/color_oracle.c, gives on random frames -- W = 2 and odd heights included."""
    rng = np.random.default_rng(1000 * w + 10 * h + fmt)
    frame = rng.integers(0, 256, (h, 2 * w + 6), dtype=np.uint8)          # padded rows: only 2W bytes of a row count
    y, uv = ref.luma(frame, w, fmt), ref.chroma(frame, w, fmt)
    assert y.shape == uv.shape == (h, w)
    off = fmt - 2
    assert np.array_equal(y, frame[:, off:2 * w:2]) and np.array_equal(uv[:, 0::2], frame[:, 1 - off:2 * w:4])      # U before V
    assert np.array_equal(uv[:, 1::2], frame[:, 3 - off:2 * w:4])
    got = ref.decode(y, uv, order)
    assert got.shape == (h, w, 3) and got.flags.c_contiguous
    assert np.array_equal(got, ref.decode_formula(y, uv, order))
    assert np.array_equal(ref.decode(y, uv, ORDER_RGB), ref.decode(y, uv, ORDER_BGR)[:, :, ::-1])


def test_known_answers():
    def px(y, u, v):
        return tuple(int(c) for c in ref.decode(np.array([[y, y]], np.uint8), np.array([[u, v]], np.uint8))[0, 0])
    assert px(16, 128, 128) == (0, 0, 0)
    assert px(235, 128, 128) == (255, 255, 255)
    # one saturating case per channel, both ways: (B, G, R)
    assert px(235, 255, 128)[0] == 255 and px(16, 0, 128)[0] == 0            # B follows U
    assert px(235, 128, 255)[2] == 255 and px(16, 128, 0)[2] == 0            # R follows V
    assert px(235, 0, 0)[1] == 255 and px(16, 255, 255)[1] == 0              # G falls with U and V
    # unsaturated: Y = 128, U = 100, V = 160 by the formula
    yy = (128 - 16) * 1220542
    want = ((yy + (1 << 19) + 2116026 * -28) >> 20, (yy + (1 << 19) - 852492 * 32 - 409993 * -28) >> 20, (yy + (1 << 19) + 1673527 * 32) >> 20)
    assert px(128, 100, 160) == want and all(0 < c < 255 for c in want)
    # the two pixels of a macropixel share its chroma, the next macropixel has its own
    img = ref.decode(np.array([[100, 100, 100, 100]], np.uint8), np.array([[60, 200, 200, 60]], np.uint8))
    assert np.array_equal(img[0, 0], img[0, 1]) and np.array_equal(img[0, 2], img[0, 3]) and not np.array_equal(img[0, 1], img[0, 2])


@pytest.mark.parametrize("fmt", [FMT_YUY2, FMT_UYVY])
def test_reference_tells_422_from_420(fmt):
    """Even rows with strong chroma, odd rows with chroma 128: decoding every row with its own chroma differs from decoding both rows
    of a pair with their rounding mean (what packed -> NV12 -> BGR gives), on the even rows and on the odd rows."""
    w, h = 18, 6
    frame = ref.alternating_chroma_frame(w, h, fmt, 7)
    y, uv = ref.luma(frame, w, fmt), ref.chroma(frame, w, fmt)
    assert (uv[1::2] == 128).all() and (np.abs(uv[0::2].astype(int) - 128) >= 50).all()
    mean = ((uv[0::2].astype(np.uint16) + uv[1::2] + 1) >> 1).astype(np.uint8)
    own, shared = ref.decode(y, uv), ref.decode(y, np.repeat(mean, 2, axis=0))
    assert not np.array_equal(own[0::2], shared[0::2]) and not np.array_equal(own[1::2], shared[1::2])
    # and the odd rows, whose chroma is neutral, come out grey: B == G == R up to the rounding of the three constants
    assert np.abs(own[1::2].astype(int) - own[1::2, :, 1:2].astype(int)).max() <= 1
    assert np.array_equal(ref.expected(frame, w, fmt, ORDER_BGR, "eq"), ref.decode(ref.mapped_luma(y, "eq"), uv))
