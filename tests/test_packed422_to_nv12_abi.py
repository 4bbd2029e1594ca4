"""Packed 4:2:2 in, NV12 out (mi_*_packed422_to_nv12_batch_dev) at the ABI level, without a GPU: the header declares both entry points
with their parameter lists, no struct or enum grew (minor version 3, MI_K_COUNT 10), the binding lists both symbols and has the two
Context methods, both libraries export them, and a null context is refused without touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import synth

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1
NAMES = ["mi_equalize_hist_packed422_to_nv12_batch_dev", "mi_clahe_packed422_to_nv12_batch_dev"]

COMMON = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, "
          "void* d_y_out, size_t y_pitch, void* d_uv_out, size_t uv_pitch, size_t out_frame_stride, "
          "int width, int height, int n_frames, int format, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_packed422_to_nv12_batch_dev": COMMON + ", void* stream",
    "mi_clahe_packed422_to_nv12_batch_dev": COMMON + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
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


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_NV12", 0), ("MI_FMT_P010", 1), ("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert not re.search(r"\bMI_FMT_\w+\s*=\s*4\b", txt), "no new format value"


def test_header_states_the_contract():
    """The parts of the contract a caller cannot guess: the chroma rule and that it is the header's own, the refused tight pitch."""
    m = re.search(r"/\*\s*mi_\*_packed422_to_nv12_batch_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> NV12 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("(a + b + 1) >> 1", "no outside pin", "W % 4 == 2", "MI_ERR_BUSY", "never written", "height` is even"):
        assert needle in txt, needle


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_nv12_batch_dev", "clahe_packed422_to_nv12_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        for kw in ("in_pitch", "in_frame", "y_pitch", "uv_pitch", "out_frame", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    src = synth.packed422_frame(w, h, 2, "D1", 3)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    a = (None, src.ctypes.data, 2 * w, 2 * w * h, dst.ctypes.data, w, dst.ctypes.data + w * h, w, w * h * 3 // 2, w, h, 1, 2, 1)
    assert built_lib.mi_equalize_hist_packed422_to_nv12_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_nv12_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)
