"""Packed 4:2:2 frames (YUY2 / UYVY) at the ABI level, without a GPU: the header declares the four entry points with their parameter
lists and the two format values, the binding lists them, both libraries export them, no struct grew (minor version 3, MI_K_COUNT
10), every entry point refuses a null context without touching the buffers it was given, and synth.packed422_frame interleaves
synth.y_plane with the hashed chroma."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import synth

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1
NAMES = ["mi_equalize_hist_packed422_batch_dev", "mi_clahe_packed422_batch_dev", "mi_equalize_hist_packed422", "mi_clahe_packed422"]

BATCH = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, void* d_out, size_t out_pitch, "
         "size_t out_frame_stride, int width, int height, int n_frames, int format, mi_uv_mode uv_mode")
HOST = ("mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_pitch, int width, int height, int format, "
        "mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_packed422_batch_dev": BATCH + ", void* stream",
    "mi_clahe_packed422_batch_dev": BATCH + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
    "mi_equalize_hist_packed422": HOST,
    "mi_clahe_packed422": HOST + ", double clip_limit, int tiles_x, int tiles_y",
}


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    assert _norm(m.group(1)) == _norm(PARAMS[name])


def test_header_enum_and_sizes():
    txt = _header()
    for name, v in (("MI_FMT_NV12", 0), ("MI_FMT_P010", 1), ("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert (mi_lumaeq.FMT_YUY2, mi_lumaeq.FMT_UYVY) == (2, 3)
    assert len(mi_lumaeq.KERNEL_NAMES) == 10


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422", "clahe_packed422", "equalize_hist_packed422_batch_dev", "clahe_packed422_batch_dev"):
        assert callable(getattr(mi_lumaeq.Context, m)), m


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    src = synth.packed422_frame(w, h, 2, "D1", 3)
    dst = np.full((h, 2 * w), 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    a = (None, src.ctypes.data, 2 * w, 2 * w * h, dst.ctypes.data, 2 * w, 2 * w * h, w, h, 1, 2, 1)
    assert built_lib.mi_equalize_hist_packed422_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 2 * w, dst.ctypes.data, 2 * w, w, h, 3, 0)
    assert built_lib.mi_equalize_hist_packed422(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("dist", synth.DISTS)
def test_synth_frame_interleaves_y_plane_and_chroma(fmt, dist):
    w, h = 62, 7
    f = synth.packed422_frame(w, h, fmt, dist, 5)
    assert f.shape == (h, 2 * w) and f.dtype == np.uint8 and f.flags.c_contiguous
    off = fmt - 2
    assert np.array_equal(f[:, off::2], synth.y_plane(w, h, dist, 5))
    chroma = synth.random_bytes(w * h, synth.frame_seed(5) ^ 0xA5A5).reshape(h, w)
    assert np.array_equal(f[:, 1 - off::2], chroma)
    assert len(np.unique(chroma)) > 16, "the chroma must be checkable: not a constant"
    with pytest.raises(ValueError):
        synth.packed422_frame(w, h, 7)
