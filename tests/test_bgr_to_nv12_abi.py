"""Interleaved BGR / RGB in, NV12 out (mi_*_bgr_to_nv12*) at the ABI level, without a GPU: the header declares the four entry points with
their parameter lists, no struct or profiling enum grew (MI_K_COUNT 10), the header comment states the contract a caller cannot guess, the
binding lists the symbols and has the four Context methods with their keyword defaults, both libraries export them, the C++ helpers exist,
and a call without a context fails loudly without touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1
DEV = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, void* d_y_out, size_t y_pitch, void* d_uv_out, "
       "size_t uv_pitch, size_t out_frame_stride, int width, int height, int n_frames, int order, mi_uv_mode uv_mode")
HOST = "mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* nv12_out, int width, int height, int order, mi_uv_mode uv_mode"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_bgr_to_nv12_batch_dev": DEV + ", void* stream",
    "mi_clahe_bgr_to_nv12_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_bgr_to_nv12": HOST,
    "mi_clahe_bgr_to_nv12": HOST + CLAHE,
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


def test_declared_after_the_nv12_to_bgr_block_and_no_slot_added():
    txt = _header()
    assert txt.index("mi_clahe_nv12_to_bgr_frames_dev") < txt.index("mi_equalize_hist_bgr_to_nv12_batch_dev") < txt.index("mi_host_register")
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10


def test_header_states_the_contract():
    """What a caller cannot guess: the OpenCV sequence the bytes equal, where the chroma comes from, what is written, the two stages and
    their slots, the byte count, the error rules."""
    m = re.search(r"/\*\s*mi_\*_bgr_to_nv12\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGR -> NV12 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("COLOR_BGR2YUV_I420", "COLOR_RGB2YUV_I420", "top-left", "never written", "W bytes of each output row", "MI_K_COLOR",
                   "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST", "6.5", "7.5", "256 frames", "clahe_fp_contract", "REFLECT_101",
                   "MI_ERR_BUSY", "d_y_out == d_in, d_uv_out == d_in or d_y_out == d_uv_out", "even when another size is 0",
                   "a bad uv_mode", "mi_cvt_color_420_u8", "Nothing is enqueued unless all checks pass"):
        assert needle in txt, needle


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgr_to_nv12_batch_dev", "clahe_bgr_to_nv12_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:7] == ["self", "d_in", "d_y_out", "d_uv_out", "width", "height", "n_frames"], m
        for kw in ("in_pitch", "in_frame", "y_pitch", "uv_pitch", "out_frame"):
            assert kw in params and params[kw].default is None, (m, kw)
        assert params["stream"].default == 0
        assert params["order"].default == mi_lumaeq.ORDER_BGR and params["uv_mode"].default == mi_lumaeq.UV_COPY
    for m in ("equalize_hist_bgr_to_nv12", "clahe_bgr_to_nv12"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:2] == ["self", "img"], m
        assert params["order"].default == mi_lumaeq.ORDER_BGR and params["uv_mode"].default == mi_lumaeq.UV_COPY
        assert params["out"].default is None
    for m in ("clahe_bgr_to_nv12_batch_dev", "clahe_bgr_to_nv12"):
        params = inspect.signature(getattr(mi_lumaeq.Context, m)).parameters
        assert (params["clip_limit"].default, params["tiles_x"].default, params["tiles_y"].default) == (2.0, 8, 8), m


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_cxx_helpers_are_declared():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistBGRToNV12", "mi_equalize_hist_bgr_to_nv12"), ("claheBGRToNV12", "mi_clahe_bgr_to_nv12")):
        assert re.search(r"inline\s+void\s+" + fn + r"\s*\(", txt), fn
        assert re.search(r"\b" + abi + r"\s*\(", txt), abi
    assert txt.index("equalizeHistNV12ToBGR") < txt.index("equalizeHistBGRToNV12")


def test_new_sources_are_registered():
    csrc = ROOT / "opencv-opencl_amd" / "csrc"
    assert (csrc / "kernels" / "bgr_nv12.hip.h").exists() and (csrc / "host" / "bgr_nv12.inc.hpp").exists()
    assert '#include "kernels/bgr_nv12.hip.h"' in (csrc / "lumaeq_kernels.hip.h").read_text()
    assert '#include "host/bgr_nv12.inc.hpp"' in (csrc / "mi_lumaeq.hip").read_text()


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    a = (None, src.ctypes.data, 3 * w, 3 * w * h, dst.ctypes.data, w, dst.ctypes.data + w * h, w, w * h * 3 // 2, w, h, 1, 0, 1)
    assert built_lib.mi_equalize_hist_bgr_to_nv12_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_nv12_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 3 * w, dst.ctypes.data, w, h, 0, 1)
    assert built_lib.mi_equalize_hist_bgr_to_nv12(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_nv12(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)
