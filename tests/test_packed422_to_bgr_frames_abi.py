"""Packed 4:2:2 in, BGR / RGB out on a list of device frames (mi_*_packed422_to_bgr_frames_dev) at the ABI level, without a GPU: the
header declares both entry points with their parameter lists and the 16-byte list entry, no struct or enum grew (minor version 3,
MI_K_COUNT 10, no new MI_FMT_*), the header comment states the parts of the contract a caller cannot guess and names the two
statistics, the binding lists the symbols and has the methods with matching signatures, both libraries export the symbols, and a null
context is refused without touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import synth, FMT_YUY2, ORDER_BGR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_packed422_bgr_frame_dev* frames, int n_frames, "
        "int width, int height, size_t in_pitch, size_t out_pitch, int format, int order")
PARAMS = {
    "mi_equalize_hist_packed422_to_bgr_frames_dev": LIST + ", void* stream",
    "mi_clahe_packed422_to_bgr_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)
STATS = ("packed422_bgr_list_frames_wide", "packed422_bgr_list_frames_bytes")


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
    m = re.search(r"typedef\s+struct\s+mi_packed422_bgr_frame_dev\s*\{(.*?)\}\s*mi_packed422_bgr_frame_dev\s*;", _header(), re.S)
    assert m, "mi_packed422_bgr_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* in; void* out;"
    f = mi_lumaeq.Packed422BgrFrameDev
    assert [n for n, _ in f._fields_] == ["in_", "out"]
    assert ctypes.sizeof(ctypes.c_void_p) == 8 and ctypes.sizeof(f) == 16
    assert mi_lumaeq.Packed422BgrFrameDev is mi_lumaeq.capi.Packed422BgrFrameDev and "Packed422BgrFrameDev" in mi_lumaeq.__all__


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3), ("MI_ORDER_BGR", 0), ("MI_ORDER_RGB", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert not re.search(r"\bMI_FMT_\w+\s*=\s*4\b", txt), "no new format value"


def test_header_states_the_contract():
    """A comment block of its own: the bytes are the batch form's, one pass, the input rules, no output alignment rule, the per-frame
    store path and the two statistics that count it, the overlap rule, nothing enqueued unless every frame passes."""
    m = re.search(r"/\*\s*mi_\*_packed422_to_bgr_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> BGR list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("read only during the call", "exactly what mi_*_packed422_to_bgr_batch_dev writes", "exactly Y0 U Y1 V",
                   "exactly U Y0 V Y1", "clahe_fp_contract", "clahe_float_tables", "one pass", "no scratch Y plane",
                   "in_pitch is a multiple of 4", "every `in` is a multiple of 4", "NO alignment rule", "W % 4 == 2",
                   "slower, the same bytes out", "never written", "no in-place form", "not checked", "MI_ERR_BUSY",
                   "Nothing is enqueued unless every frame passes") + STATS:
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_packed422_to_bgr\*.*?\*/", HEADER.read_text(), re.S)
    assert batch and "no frame-list form" not in _norm(batch.group(0).replace("\n *", " ")), "the batch form's comment still denies the list form"


def test_statistics_are_named_where_they_are_served():
    capi = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "capi.inc.hpp").read_text()
    ctx = (ROOT / "opencv-opencl_amd" / "csrc" / "host" / "context.inc.hpp").read_text()
    for s in STATS:
        assert '!strcmp(name, "%s")' % s in capi, s
    assert re.search(r"packed422_bgr_list_frames_wide\s*=\s*0\s*,\s*packed422_bgr_list_frames_bytes\s*=\s*0\s*;", ctx)


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_bgr_frames", "clahe_packed422_to_bgr_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[1:7] == ["inputs", "outs", "width", "height", "fmt", "order"], m
        assert params["fmt"].default == FMT_YUY2 and params["order"].default == ORDER_BGR
        for kw in ("in_pitch", "out_pitch", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
    p = inspect.signature(mi_lumaeq.Context.clahe_packed422_to_bgr_frames).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    src = synth.packed422_frame(w, h, FMT_YUY2, "D1", 3)
    dst = np.full(3 * w * h, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    entry = mi_lumaeq.Packed422BgrFrameDev(src.ctypes.data, dst.ctypes.data)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, 2 * w, 3 * w, FMT_YUY2, ORDER_BGR)
    assert built_lib.mi_equalize_hist_packed422_to_bgr_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_bgr_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
