"""Interleaved BGR / RGB in, NV12 out on a list of pitched device frames (mi_*_bgr_to_nv12_frames_dev) at the ABI level, without a GPU:
the header declares the two entry points with their parameter lists and the list entry struct behind the batch block, no struct or enum
grew (MI_K_COUNT 10), the new comment block states the parts of the contract a caller cannot guess while the batch form's block is left
alone, the binding lists the symbols and has the methods with their keyword defaults, both libraries export the symbols, the host file
is part of the translation unit, and a null context is refused without touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_bgr_nv12_frame_dev* frames, int n_frames, int width, int height, "
        "size_t in_pitch, size_t y_pitch, size_t uv_pitch, int order, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_bgr_to_nv12_frames_dev": LIST + ", void* stream",
    "mi_clahe_bgr_to_nv12_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
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


def test_header_declares_the_list_entry():
    m = re.search(r"typedef\s+struct\s+mi_bgr_nv12_frame_dev\s*\{(.*?)\}\s*mi_bgr_nv12_frame_dev\s*;", _header(), re.S)
    assert m, "mi_bgr_nv12_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* in; void* y; void* uv;"
    f = mi_lumaeq.BgrNv12FrameDev
    assert [n.rstrip("_") for n, _ in f._fields_] == ["in", "y", "uv"]
    assert ctypes.sizeof(f) == 24
    assert mi_lumaeq.BgrNv12FrameDev is mi_lumaeq.capi.BgrNv12FrameDev and "BgrNv12FrameDev" in mi_lumaeq.__all__


def test_declared_behind_the_batch_block_and_nothing_grew():
    txt = _header()
    at = [txt.index(s) for s in ("mi_clahe_bgr_to_nv12(", "mi_bgr_nv12_frame_dev", "mi_equalize_hist_bgr_to_nv12_frames_dev",
                                 "mi_clahe_bgr_to_nv12_frames_dev", "mi_host_register")]
    assert at == sorted(at), "the list form is declared after the mi_*_bgr_to_nv12* block and before mi_host_register"
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert sorted(set(re.findall(r"\bMI_FMT_\w+", txt))) == ["MI_FMT_NV12", "MI_FMT_P010", "MI_FMT_UYVY", "MI_FMT_YUY2"], "no new format"
    assert sorted(set(re.findall(r"\bMI_ORDER_\w+", txt))) == ["MI_ORDER_BGR", "MI_ORDER_RGB"], "no new order"


def test_header_states_the_contract():
    """A comment block of its own; the batch form's block is left as it was."""
    m = re.search(r"/\*\s*mi_\*_bgr_to_nv12_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGR -> NV12 list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("read only during the call", "share width, height, order, uv_mode and the three pitches", "each has its own addresses",
                   "exactly what mi_*_bgr_to_nv12_batch_dev writes", "only the W bytes of each output row are written", "never written",
                   "none is required of any address or pitch", "per-frame alignment", "chunk of 64 frames", "MI_K_COLOR", "MI_K_EQ_LUT",
                   "MI_K_LUT_APPLY", "no MI_K_HIST", "mi_clahe_nv12_frames_dev", "same profiling slots", "hold the unequalized luma",
                   "no in-place form", "its own Y or UV plane", "its Y plane those of its own UV plane", "several entries", "not checked",
                   "a null `frames` with n_frames > 0", "a null in / y / uv in any entry", "refused even when another size is 0",
                   "a bad uv_mode", "MI_ERR_UNSUPPORTED", "MI_OK, nothing written", "Nothing is enqueued unless every frame passes",
                   "MI_ERR_BUSY", "holds the addresses it was captured with", "clahe_fp_contract", "REFLECT_101"):
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_bgr_to_nv12\*.*?\*/", HEADER.read_text(), re.S)
    assert batch and "frames_dev" not in batch.group(0) and "256 frames" in batch.group(0), "the batch form's comment was not extended"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgr_to_nv12_frames", "clahe_bgr_to_nv12_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:8] == ["self", "ins", "ys", "uvs", "width", "height", "order", "uv_mode"], m
        assert params["order"].default == mi_lumaeq.ORDER_BGR and params["uv_mode"].default == mi_lumaeq.UV_COPY
        for kw in ("in_pitch", "y_pitch", "uv_pitch"):
            assert kw in params and params[kw].default is None, (m, kw)
        assert params["stream"].default == 0
    assert list(inspect.signature(mi_lumaeq.Context.equalize_hist_bgr_to_nv12_frames).parameters)[8:] == \
        ["in_pitch", "y_pitch", "uv_pitch", "stream"]
    p = inspect.signature(mi_lumaeq.Context.clahe_bgr_to_nv12_frames).parameters
    assert list(p)[8:] == ["clip_limit", "tiles_x", "tiles_y", "in_pitch", "y_pitch", "uv_pitch", "stream"]
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_host_file_is_included_behind_the_batch_form():
    assert (CSRC / "host" / "bgr_nv12_frames.inc.hpp").exists()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/bgr_nv12.inc.hpp"') < tu.index('#include "host/bgr_nv12_frames.inc.hpp"')
    kernels = (CSRC / "kernels" / "bgr_nv12.hip.h").read_text()
    for name in ("bgr_to_nv12_hist_frames_kernel", "StridedBgrNv12", "TableBgrNv12", "BgrNv12List"):
        assert name in kernels, name
    assert re.search(r"static_assert\(sizeof\(BgrNv12Frame\)\s*==\s*24\b", kernels)
    host = (CSRC / "host" / "bgr_nv12.inc.hpp").read_text()
    assert re.search(r"constexpr\s+int\s+kBgrNv12FramesPerLaunch\s*=\s*256\s*;", host), "the batch form keeps its chunk of 256 frames"


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    entry = mi_lumaeq.BgrNv12FrameDev(src.ctypes.data, dst.ctypes.data, dst.ctypes.data + w * h)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, 3 * w, w, w, 0, 1)
    assert built_lib.mi_equalize_hist_bgr_to_nv12_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_nv12_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
