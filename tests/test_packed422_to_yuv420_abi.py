"""Packed 4:2:2 in, planar 4:2:0 (or NV12) out (mi_*_packed422_to_yuv420*) at the ABI level, without a GPU: the header declares the six
entry points with their parameter lists, no struct or enum grew (minor version 3, MI_K_COUNT 10), the binding lists the symbols and has
the six Context methods, both libraries export them, a null context is refused without touching the caller's buffers, and the header
comment states the parts of the contract a caller cannot guess."""
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

BATCH = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, const mi_yuv420_planes* out, "
         "int width, int height, int n_frames, int format, mi_uv_mode uv_mode")
HOST = ("mi_ctx* ctx, const uint8_t* in, size_t in_pitch, const mi_yuv420_planes* out, "
        "int width, int height, int format, mi_uv_mode uv_mode")
LIST = ("mi_ctx* ctx, const mi_packed422_yuv420_frame_dev* frames, int n_frames, "
        "int width, int height, size_t in_pitch, size_t y_pitch, size_t c_pitch, int out_chroma, int format, mi_uv_mode uv_mode")
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_packed422_to_yuv420_batch_dev": BATCH + ", void* stream",
    "mi_clahe_packed422_to_yuv420_batch_dev": BATCH + CLAHE + ", void* stream",
    "mi_equalize_hist_packed422_to_yuv420": HOST,
    "mi_clahe_packed422_to_yuv420": HOST + CLAHE,
    "mi_equalize_hist_packed422_to_yuv420_frames_dev": LIST + ", void* stream",
    "mi_clahe_packed422_to_yuv420_frames_dev": LIST + CLAHE + ", void* stream",
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


def test_list_entry_is_the_existing_four_address_struct():
    assert re.search(r"typedef\s+mi_bgr_yuv420_frame_dev\s+mi_packed422_yuv420_frame_dev\s*;", _header())
    assert ctypes.sizeof(mi_lumaeq.capi.BgrYuv420FrameDev) == 32


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_NV12", 0), ("MI_FMT_P010", 1), ("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert not re.search(r"\bMI_FMT_\w+\s*=\s*4\b", txt), "no new format value"
    assert ctypes.sizeof(mi_lumaeq.capi.Yuv420Planes) == 56


def test_header_states_the_contract():
    """The chroma rule and that it is the header's own, the refused tight chroma pitch, the input that is never written."""
    m = re.search(r"/\*\s*mi_\*_packed422_to_yuv420\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> 4:2:0 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("(a + b + 1) >> 1", "no outside pin", "W % 8 != 0", "never written", "MI_ERR_BUSY", "c0 is always U"):
        assert needle in txt, needle


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_yuv420_batch_dev", "clahe_packed422_to_yuv420_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        for kw in ("in_pitch", "in_frame", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
    for m in ("equalize_hist_packed422_to_yuv420_frames_dev", "clahe_packed422_to_yuv420_frames_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        assert inspect.signature(f).parameters["stream"].default == 0, m
    for m in ("equalize_hist_packed422_to_yuv420", "clahe_packed422_to_yuv420"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert params["dst_fmt"].default == "i420" and params["out"].default is None and params["planes"].default is None, m


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
    planes = mi_lumaeq.capi.Yuv420Planes.i420(dst.ctypes.data, w, h)
    entry = mi_lumaeq.capi.BgrYuv420FrameDev(src.ctypes.data, planes.y, planes.c0, planes.c1)
    L, P = built_lib, ctypes.byref(planes)
    cl = (ctypes.c_double(2.0), 2, 2)
    assert L.mi_equalize_hist_packed422_to_yuv420_batch_dev(None, src.ctypes.data, 2 * w, 2 * w * h, P, w, h, 1, 2, 1, None) == MI_ERR_BAD_ARG
    assert L.mi_clahe_packed422_to_yuv420_batch_dev(None, src.ctypes.data, 2 * w, 2 * w * h, P, w, h, 1, 2, 1, *cl, None) == MI_ERR_BAD_ARG
    assert L.mi_equalize_hist_packed422_to_yuv420(None, src.ctypes.data, 2 * w, P, w, h, 2, 1) == MI_ERR_BAD_ARG
    assert L.mi_clahe_packed422_to_yuv420(None, src.ctypes.data, 2 * w, P, w, h, 2, 1, *cl) == MI_ERR_BAD_ARG
    E = ctypes.byref(entry)
    assert L.mi_equalize_hist_packed422_to_yuv420_frames_dev(None, E, 1, w, h, 2 * w, w, w // 2, 1, 2, 1, None) == MI_ERR_BAD_ARG
    assert L.mi_clahe_packed422_to_yuv420_frames_dev(None, E, 1, w, h, 2 * w, w, w // 2, 1, 2, 1, *cl, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)
