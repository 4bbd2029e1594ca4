"""Packed 4:2:2 frame lists (mi_*_packed422_frames_dev) at the ABI level, without a GPU: the header declares both entry points with
their parameter lists and the mi_packed422_frame_dev struct, the binding lists the symbols, the methods and a 16-byte struct, both
libraries export the symbols, no struct grew (minor version 3, MI_K_COUNT 10), and a null context is refused by both entry points
without touching the buffers the list names."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1
SHAPE = ("mi_ctx* ctx, const mi_packed422_frame_dev* frames, int n_frames, int width, int height, size_t in_pitch, size_t out_pitch, "
         "int format, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_packed422_frames_dev": SHAPE + ", void* stream",
    "mi_clahe_packed422_frames_dev": SHAPE + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
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


def test_header_declares_the_struct_and_no_struct_grew():
    txt = _header()
    m = re.search(r"typedef\s+struct\s+mi_packed422_frame_dev\s*\{(.*?)\}\s*mi_packed422_frame_dev\s*;", txt, re.S)
    assert m, "mi_packed422_frame_dev is not declared"
    assert [_norm(f) for f in m.group(1).split(";") if f.strip()] == ["const void* in", "void* out"]
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "symbols were added, no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "the new launches are charged to the existing profiling slots"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10


def test_binding_lists_symbols_methods_and_struct():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_frames", "clahe_packed422_frames"):
        assert callable(getattr(mi_lumaeq.Context, m)), m
    S = capi.Packed422FrameDev
    assert ctypes.sizeof(S) == 16
    assert [f[0] for f in S._fields_] == ["in_", "out"] and (S.in_.offset, S.out.offset) == (0, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    """A null context is refused before any HIP call: host stand-ins for the device frames stay as they are, and so does the list."""
    w, h = 8, 4
    src = np.arange(2 * w * h, dtype=np.uint8).reshape(h, 2 * w)
    dst = np.full((2, h, 2 * w), 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    frames = (capi.Packed422FrameDev * 2)(capi.Packed422FrameDev(src.ctypes.data, dst[0].ctypes.data),
                                          capi.Packed422FrameDev(src.ctypes.data, dst[1].ctypes.data))
    before = bytes(frames)
    a = (None, frames, 2, w, h, 2 * w, 2 * w, 2, 1)
    assert built_lib.mi_equalize_hist_packed422_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_frames_dev(*a, 2.0, 2, 2, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_equalize_hist_packed422_frames_dev(None, None, 0, 0, 0, 0, 0, 2, 0, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_frames_dev(None, None, 0, 0, 0, 0, 0, 3, 0, 2.0, 8, 8, None) == MI_ERR_BAD_ARG
    assert bytes(frames) == before and np.array_equal(src, s0) and np.array_equal(dst, d0)
