"""NV12 in, interleaved BGR / RGB out on a list of pitched device frames (mi_*_nv12_to_bgr_frames_dev) at the ABI level, without a GPU:
the header declares the two entry points with their parameter lists and the list entry struct, no struct or enum grew (minor version 3,
MI_K_COUNT 10, no new MI_FMT_* or MI_ORDER_*), the new comment block states the parts of the contract a caller cannot guess while the
batch form's block is left alone, the binding lists the symbols and has the methods with their keyword defaults, both libraries export
the symbols, and a null context is refused without touching the caller's buffers."""
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

LIST = ("mi_ctx* ctx, const mi_nv12_bgr_frame_dev* frames, int n_frames, "
        "int width, int height, size_t y_pitch, size_t uv_pitch, size_t out_pitch, int order")
PARAMS = {
    "mi_equalize_hist_nv12_to_bgr_frames_dev": LIST + ", void* stream",
    "mi_clahe_nv12_to_bgr_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
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
    m = re.search(r"typedef\s+struct\s+mi_nv12_bgr_frame_dev\s*\{(.*?)\}\s*mi_nv12_bgr_frame_dev\s*;", _header(), re.S)
    assert m, "mi_nv12_bgr_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* y; const void* uv; void* out;"
    f = mi_lumaeq.Nv12BgrFrameDev
    assert [n for n, _ in f._fields_] == ["y", "uv", "out"]
    assert ctypes.sizeof(f) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert mi_lumaeq.Nv12BgrFrameDev is mi_lumaeq.capi.Nv12BgrFrameDev and "Nv12BgrFrameDev" in mi_lumaeq.__all__


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_NV12", 0), ("MI_FMT_P010", 1), ("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3), ("MI_ORDER_BGR", 0), ("MI_ORDER_RGB", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert sorted(set(re.findall(r"\bMI_FMT_\w+", txt))) == ["MI_FMT_NV12", "MI_FMT_P010", "MI_FMT_UYVY", "MI_FMT_YUY2"], "no new format"
    assert sorted(set(re.findall(r"\bMI_ORDER_\w+", txt))) == ["MI_ORDER_BGR", "MI_ORDER_RGB"], "no new order"


def test_header_states_the_contract():
    """A comment block of its own; the batch form's block is left as it was."""
    m = re.search(r"/\*\s*mi_\*_nv12_to_bgr_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the NV12 -> BGR list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("no in-place form", "read only during the call", "per-frame alignment", "Nothing is enqueued unless every frame passes",
                   "MI_ERR_BUSY", "nv12_bgr_onepass", "nv12_bgr_twopass", "never written", "not checked", "REFLECT_101",
                   "clahe_fp_contract", "a null `frames` with n_frames > 0", "refused even when another size is 0",
                   "MI_OK, nothing written", "holds the addresses it was captured with", "same profiling slots"):
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_nv12_to_bgr\*:.*?\*/", HEADER.read_text(), re.S)
    assert batch and "frames_dev" not in batch.group(0), "the batch form's comment was not extended"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_nv12_to_bgr_frames", "clahe_nv12_to_bgr_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[1:7] == ["ys", "uvs", "outs", "width", "height", "order"], m
        assert params["order"].default == mi_lumaeq.ORDER_BGR
        for kw in ("y_pitch", "uv_pitch", "out_pitch"):
            assert kw in params and params[kw].default is None, (m, kw)
        assert params["stream"].default == 0
    p = inspect.signature(mi_lumaeq.Context.clahe_nv12_to_bgr_frames).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    src = np.arange(w * h * 3 // 2, dtype=np.uint8)
    dst = np.full(w * h * 3, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    entry = mi_lumaeq.Nv12BgrFrameDev(src.ctypes.data, src.ctypes.data + w * h, dst.ctypes.data)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, w, w, 3 * w, 0)
    assert built_lib.mi_equalize_hist_nv12_to_bgr_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_nv12_to_bgr_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
