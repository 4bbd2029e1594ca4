"""4:2:0 frames described by mi_yuv420_planes in, interleaved BGR / RGB out (mi_*_yuv420_to_bgr*) at the ABI level, without a GPU: the header
declares the four entry points with their parameter lists, no profiling slot was added (MI_K_COUNT 10), the header comment states the
contract, the binding lists the symbols and has the four Context methods with their defaults, both libraries export them, the C++
helpers exist and compile, and a call without a context or a device fails loudly without touching the caller's buffers."""
import ctypes
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import Yuv420Planes

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1
DEV = ("mi_ctx* ctx, const mi_yuv420_planes* in, void* d_out, size_t out_pitch, size_t out_frame_stride, "
       "int width, int height, int n_frames, int order")
HOST = "mi_ctx* ctx, const mi_yuv420_planes* in, uint8_t* out, size_t out_step, int width, int height, int order"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_yuv420_to_bgr_batch_dev": DEV + ", void* stream",
    "mi_clahe_yuv420_to_bgr_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_yuv420_to_bgr": HOST,
    "mi_clahe_yuv420_to_bgr": HOST + CLAHE,
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


def test_no_profiling_slot_was_added():
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", _header())
    assert len(mi_lumaeq.KERNEL_NAMES) == 10


def test_header_states_the_contract():
    """What a caller cannot guess: the two compositions the bytes equal, the interleaved routing, the multiples-of-8 rule, the counters,
    the error rules."""
    m = re.search(r"/\*\s*mi_\*_yuv420_to_bgr\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the 4:2:0 -> BGR forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("mi_clahe_nv12_to_bgr_batch_dev", "mi_equalize_hist_nv12_to_bgr_batch_dev",       # the NV12 form on interleaved U, V
                   "mi_*_yuv420_batch_dev", "MI_UV_COPY", "mi_cvt_color_420_u8_batch_dev", "MI_COLOR_YUV2BGR_NV12",   # the two calls
                   "COLOR_YUV2BGR_I420", "MI_CHROMA_INTERLEAVED", "d_uv = in->c0", "uv_pitch = in->c_pitch", "in->c1 ignored",
                   "nv12_bgr_onepass", "nv12_bgr_twopass",
                   "in->c0, in->c1 and in->c_pitch are multiples of 8", "W % 16 == 0", "one 8-byte U load, one 8-byte V load",
                   "yuv420_bgr_onepass", "yuv420_bgr_twopass", "yuv420_bgr_vec", "yuv420_bgr_bytes",
                   "REFLECT_101", "clahe_fp_contract", "never written", "3*W bytes of each output row", "MI_ERR_BUSY",
                   "even when another size is 0", "Nothing is enqueued unless", "no in-place form",
                   "d_out equal to any input plane pointer", "a null in->c1 on a PLANAR input", "MI_ERR_UNSUPPORTED"):
        assert needle in txt, needle


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_yuv420_to_bgr_batch_dev", "clahe_yuv420_to_bgr_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:6] == ["self", "src", "d_out", "width", "height", "n_frames"], m
        for kw in ("out_pitch", "out_frame", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
        assert params["order"].default == mi_lumaeq.ORDER_BGR
    cl = inspect.signature(mi_lumaeq.Context.clahe_yuv420_to_bgr_batch_dev).parameters
    assert (cl["clip_limit"].default, cl["tiles_x"].default, cl["tiles_y"].default) == (2.0, 8, 8)
    for m in ("equalize_hist_yuv420_to_bgr", "clahe_yuv420_to_bgr"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:5] == ["self", "frame", "width", "height", "src_fmt"], m
        assert params["order"].default == mi_lumaeq.ORDER_BGR and params["out"].default is None
    cl = inspect.signature(mi_lumaeq.Context.clahe_yuv420_to_bgr).parameters
    assert (cl["clip_limit"].default, cl["tiles_x"].default, cl["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_cxx_helpers_are_declared():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistYUV420ToBGR", "mi_equalize_hist_yuv420_to_bgr"), ("claheYUV420ToBGR", "mi_clahe_yuv420_to_bgr")):
        m = re.search(r"inline\s+void\s+" + fn + r"\s*\((.*?)\)\s*\{", txt, re.S)
        assert m, fn
        sig = _norm(m.group(1))
        assert sig.startswith("const YUV420View& in, unsigned char* out, size_t outStep, int width, int height"), sig
        assert sig.endswith("ChannelOrder order = ORDER_BGR"), sig
        assert re.search(r"\b" + abi + r"\s*\(", txt), abi


def test_cxx_helpers_compile(tmp_path):
    """A three-line translation unit that calls both helpers, against the header alone."""
    gxx = shutil.which("g++")
    assert gxx, "no g++ to check mi_cv.hpp with"
    tu = tmp_path / "yuv420_to_bgr_tu.cpp"
    tu.write_text('#include "mi_cv.hpp"\n'
                  "void f(unsigned char* p, unsigned char* o) { const micv::YUV420View v = micv::YUV420View::i420(p, 16, 4);\n"
                  "  micv::equalizeHistYUV420ToBGR(v, o, 48, 16, 4); micv::claheYUV420ToBGR(v, o, 48, 16, 4, 2.0, micv::Size(2, 2), micv::ORDER_RGB); }\n")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", str(ROOT / "opencv-opencl_amd" / "cxx"),
                        "-I", str(ROOT / "include"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _buffers(w, h):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    dst = np.full(w * h * 3, 0x5A, np.uint8)
    return src, dst


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    src, dst = _buffers(w, h)
    s0, d0 = src.copy(), dst.copy()
    for fmt in (Yuv420Planes.i420, Yuv420Planes.yv12, Yuv420Planes.nv12):
        p = ctypes.byref(fmt(src.ctypes.data, w, h))
        a = (None, p, dst.ctypes.data, 3 * w, 3 * w * h, w, h, 1, 0)
        assert built_lib.mi_equalize_hist_yuv420_to_bgr_batch_dev(*a, None) == MI_ERR_BAD_ARG
        assert built_lib.mi_clahe_yuv420_to_bgr_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
        b = (None, p, dst.ctypes.data, 3 * w, w, h, 0)
        assert built_lib.mi_equalize_hist_yuv420_to_bgr(*b) == MI_ERR_BAD_ARG
        assert built_lib.mi_clahe_yuv420_to_bgr(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


def test_no_device_fails_loudly(built_lib):
    """Without a HIP device there is no context to call with: creation fails with MI_ERR_NO_DEVICE, nothing computes on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_yuv420_to_bgr.py")
    with pytest.raises(mi_lumaeq.MiError) as e:
        mi_lumaeq.Context(0)
    assert e.value.status == 5
