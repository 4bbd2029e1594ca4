"""Packed 4:2:2 in, NV12 out on frames given one by one -- the device list form (mi_*_packed422_to_nv12_frames_dev) and the host-pointer
form (mi_*_packed422_to_nv12) -- at the ABI level, without a GPU: the header declares the four entry points with their parameter lists
and the list entry struct, no struct or enum grew (minor version 3, MI_K_COUNT 10, no new MI_FMT_*), the header comment states the
parts of the contract a caller cannot guess, the binding lists the symbols and has the methods, both libraries export the symbols,
and a null context is refused without touching the caller's buffers."""
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

LIST = ("mi_ctx* ctx, const mi_packed422_nv12_frame_dev* frames, int n_frames, "
        "int width, int height, size_t in_pitch, size_t y_pitch, size_t uv_pitch, int format, mi_uv_mode uv_mode")
HOST = ("mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* y_out, size_t y_pitch, uint8_t* uv_out, size_t uv_pitch, "
        "int width, int height, int format, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_packed422_to_nv12_frames_dev": LIST + ", void* stream",
    "mi_clahe_packed422_to_nv12_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
    "mi_equalize_hist_packed422_to_nv12": HOST,
    "mi_clahe_packed422_to_nv12": HOST + ", double clip_limit, int tiles_x, int tiles_y",
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
    m = re.search(r"typedef\s+struct\s+mi_packed422_nv12_frame_dev\s*\{(.*?)\}\s*mi_packed422_nv12_frame_dev\s*;", _header(), re.S)
    assert m, "mi_packed422_nv12_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* in; void* y_out; void* uv_out;"
    f = mi_lumaeq.Packed422Nv12FrameDev
    assert [n for n, _ in f._fields_] == ["in_", "y_out", "uv_out"]
    assert ctypes.sizeof(f) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert mi_lumaeq.Packed422Nv12FrameDev is mi_lumaeq.capi.Packed422Nv12FrameDev and "Packed422Nv12FrameDev" in mi_lumaeq.__all__


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_NV12", 0), ("MI_FMT_P010", 1), ("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert not re.search(r"\bMI_FMT_\w+\s*=\s*4\b", txt), "no new format value"


def test_header_states_the_contract():
    """A comment block of its own (the batch form's is left as it was): no in-place form, multiples of 4, the per-frame alignment,
    the tight W % 4 == 2 pitch refused by the device form and accepted by the host form."""
    m = re.search(r"/\*\s*mi_\*_packed422_to_nv12_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> NV12 list and host forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("no in-place form", "multiple of 4", "its own alignment modulo 16", "W % 4 == 2", "MI_ERR_BUSY", "never written",
                   "(a + b + 1) >> 1", "not checked", "read only during the call", "Nothing is enqueued unless every frame passes",
                   "mi_equalize_hist_packed422_to_nv12 / mi_clahe_packed422_to_nv12", "ANY address", "no copy on in / y_out / uv_out"):
        assert needle in txt, needle
    dev, host = txt.split("mi_equalize_hist_packed422_to_nv12 / mi_clahe_packed422_to_nv12", 1)
    assert re.search(r"W % 4 == 2 is not a multiple of 4 and is refused", dev), "the device form refuses the tight pitch"
    assert re.search(r"W % 4 == 2 is accepted", host), "the host form accepts it"
    batch = re.search(r"/\*\s*mi_\*_packed422_to_nv12_batch_dev.*?\*/", HEADER.read_text(), re.S)
    assert batch and "frames_dev" not in batch.group(0), "the batch form's comment was not extended"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_nv12_frames", "clahe_packed422_to_nv12_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[1:8] == ["inputs", "y_outputs", "uv_outputs", "width", "height", "fmt", "uv_mode"], m
        for kw in ("in_pitch", "y_pitch", "uv_pitch", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
    for m in ("equalize_hist_packed422_to_nv12", "clahe_packed422_to_nv12"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        assert list(inspect.signature(f).parameters)[1:3] == ["frame", "width"], m


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
    entry = mi_lumaeq.Packed422Nv12FrameDev(src.ctypes.data, dst.ctypes.data, dst.ctypes.data + w * h)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, 2 * w, w, w, 2, 1)
    assert built_lib.mi_equalize_hist_packed422_to_nv12_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_nv12_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 2 * w, dst.ctypes.data, w, dst.ctypes.data + w * h, w, w, h, 2, 1)
    assert built_lib.mi_equalize_hist_packed422_to_nv12(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_nv12(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
