"""Planar / interleaved 4:2:0 frames on a list of separately allocated, pitched device planes (mi_*_yuv420_frames_dev) at the ABI level,
without a GPU: the header declares the two entry points with their parameter lists and the list entry struct behind the mi_*_yuv420
block, no struct or enum grew (MI_K_COUNT 10, minor version 3), the new comment block states the parts of the contract a caller cannot
guess while the batch form's block is left alone, the binding lists the symbols and has the methods with their keyword defaults, both
libraries export the symbols, the host file is part of the translation unit, the kernel file has the two policies and the shared
per-frame predicate, and a null context is refused without touching the caller's buffers."""
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

LIST = ("mi_ctx* ctx, const mi_yuv420_frame_dev* frames, int n_frames, int width, int height, "
        "size_t y_in_pitch, size_t c_in_pitch, int in_chroma, size_t y_out_pitch, size_t c_out_pitch, int out_chroma, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_yuv420_frames_dev": LIST + ", void* stream",
    "mi_clahe_yuv420_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)
FIELDS = ["y_in", "c0_in", "c1_in", "y_out", "c0_out", "c1_out"]


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
    m = re.search(r"typedef\s+struct\s+mi_yuv420_frame_dev\s*\{(.*?)\}\s*mi_yuv420_frame_dev\s*;", _header(), re.S)
    assert m, "mi_yuv420_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* y_in; const void* c0_in; const void* c1_in; void* y_out; void* c0_out; void* c1_out;"
    f = mi_lumaeq.Yuv420FrameDev
    assert [n for n, _ in f._fields_] == FIELDS
    assert all(t is ctypes.c_void_p for _, t in f._fields_)
    assert ctypes.sizeof(f) == 48
    assert mi_lumaeq.Yuv420FrameDev is mi_lumaeq.capi.Yuv420FrameDev and "Yuv420FrameDev" in mi_lumaeq.__all__


def test_declared_behind_the_yuv420_block_and_nothing_grew():
    txt = _header()
    at = [txt.index(s) for s in ("mi_clahe_yuv420(", "mi_yuv420_frame_dev", "mi_equalize_hist_yuv420_frames_dev",
                                 "mi_clahe_yuv420_frames_dev", "mi_host_register")]
    assert at == sorted(at), "the list form is declared after the mi_*_yuv420 block and before mi_host_register"
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert sorted(set(re.findall(r"\bMI_CHROMA_\w+", txt))) == ["MI_CHROMA_INTERLEAVED", "MI_CHROMA_PLANAR"], "no new layout"
    assert sorted(set(re.findall(r"\bMI_FMT_\w+", txt))) == ["MI_FMT_NV12", "MI_FMT_P010", "MI_FMT_UYVY", "MI_FMT_YUY2"], "no new format"
    assert ctypes.sizeof(mi_lumaeq.Yuv420Planes) == 56, "mi_yuv420_planes did not grow"


def test_header_states_the_contract():
    """A comment block of its own; the batch form's block is left as it was."""
    m = re.search(r"/\*\s*mi_\*_yuv420_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the 4:2:0 list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("read only during the call", "each has its own addresses", "no per-frame pitches", "c0 is always the U plane",
                   "exchanges the two addresses", "ignored and may be NULL", "in_chroma must still be one of the two values",
                   "mi_*_yuv420_batch_dev writes for that frame alone with n_frames = 1", "clahe_fp_contract", "REFLECT_101",
                   "not the pitch padding", "none is required of any address or pitch", "per-frame alignment", "W % 32 == 0",
                   "without the frame-stride term", "its neighbours stay vectorised", "In place, per frame", "moves nothing",
                   "mix in-place and out-of-place frames", "chunk of 64 frames", "never the fused equalizeHist kernel", "MI_K_LUT_APPLY",
                   "every frame copies all of its chroma in place", "same profiling slots", "yuv420_list_frames_vec",
                   "yuv420_list_frames_bytes", "FRAMES (not calls)", "not touched by list calls", "pointer equality, not address ranges",
                   "c1 = c0 + W/2, c_pitch = W", "several entries", "not checked", "a null `frames` with n_frames > 0",
                   "refused even when another size is 0", "a bad uv_mode", "tiles <= 0", "MI_ERR_UNSUPPORTED", "MI_OK, nothing written",
                   "Nothing is enqueued unless every frame passes", "MI_ERR_BUSY", "holds the addresses it was captured with"):
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_yuv420\*.*?\*/", HEADER.read_text(), re.S)
    assert batch and "frames_dev" not in batch.group(0) and "256 frames" in batch.group(0), "the batch form's comment was not extended"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    head = ["self", "frames", "width", "height", "y_in_pitch", "c_in_pitch", "in_chroma", "y_out_pitch", "c_out_pitch", "out_chroma",
            "uv_mode"]
    for m in ("equalize_hist_yuv420_frames_dev", "clahe_yuv420_frames_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:11] == head, m
        assert params["uv_mode"].default == mi_lumaeq.UV_COPY and params["stream"].default == 0
        batch = inspect.signature(getattr(mi_lumaeq.Context, m.replace("_frames_dev", "_batch_dev"))).parameters
        for kw in ("uv_mode", "stream", "clip_limit", "tiles_x", "tiles_y"):
            assert (kw in params) == (kw in batch) and (kw not in params or params[kw].default == batch[kw].default), (m, kw)
    assert list(inspect.signature(mi_lumaeq.Context.equalize_hist_yuv420_frames_dev).parameters)[11:] == ["stream"]
    p = inspect.signature(mi_lumaeq.Context.clahe_yuv420_frames_dev).parameters
    assert list(p)[11:] == ["clip_limit", "tiles_x", "tiles_y", "stream"]
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_host_file_is_included_behind_the_batch_form():
    assert (CSRC / "host" / "yuv420_frames.inc.hpp").exists()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/yuv420.inc.hpp"') < tu.index('#include "host/yuv420_frames.inc.hpp"')
    kernels = (CSRC / "kernels" / "yuv420.hip.h").read_text()
    for name in ("yuv420_chroma_frames_kernel", "yuv420_chroma_kernel", "StridedYuv420", "TableYuv420", "Yuv420List", "yuv420_frame_vec"):
        assert name in kernels, name
    assert re.search(r"static_assert\(sizeof\(Yuv420Frame\)\s*==\s*32\b", kernels), "four addresses an entry: the Y planes are not in it"
    assert re.search(r"__host__\s+__device__[^;{]*\byuv420_frame_vec\s*\(", kernels), "one predicate for the host's count and the kernel's branch"
    host = (CSRC / "host" / "yuv420_frames.inc.hpp").read_text()
    assert "yuv420_frame_vec(" in host and "kFramesPerLaunch" in host
    batch = (CSRC / "host" / "yuv420.inc.hpp").read_text()
    assert re.search(r"constexpr\s+int\s+kYuv420FramesPerLaunch\s*=\s*256\s*;", batch), "the batch form keeps its chunk of 256 frames"


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    s, d, ysz, csz = src.ctypes.data, dst.ctypes.data, w * h, w * h // 4
    entry = mi_lumaeq.Yuv420FrameDev(s, s + ysz, s + ysz + csz, d, d + ysz, None)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, w, w // 2, 1, w, w, 0, 1)
    assert built_lib.mi_equalize_hist_yuv420_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_yuv420_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
