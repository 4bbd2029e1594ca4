"""Planar / interleaved 4:2:0 frames (mi_*_yuv420*) at the ABI level, without a GPU: the header declares the four entry points with
their parameter lists, the plane descriptor with its members and the two chroma layouts, behind the BGR -> NV12 list form and before
mi_host_register; no struct, version or enum of the existing ABI grew; the descriptor's layout from the C compiler is the binding's;
the comment block of the new form states the contract; the binding lists the symbols and has the methods with their defaults; both
libraries export the symbols; the C++ helpers and the new sources exist; a null context is refused without touching a buffer."""
import ctypes
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1
SIDES = "mi_ctx* ctx, const mi_yuv420_planes* in, const mi_yuv420_planes* out, int width, int height"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_yuv420_batch_dev": SIDES + ", int n_frames, mi_uv_mode uv_mode, void* stream",
    "mi_clahe_yuv420_batch_dev": SIDES + ", int n_frames, mi_uv_mode uv_mode" + CLAHE + ", void* stream",
    "mi_equalize_hist_yuv420": SIDES + ", mi_uv_mode uv_mode",
    "mi_clahe_yuv420": SIDES + ", mi_uv_mode uv_mode" + CLAHE,
}
NAMES = list(PARAMS)
FIELDS = ["y", "y_pitch", "c0", "c1", "c_pitch", "frame_stride", "chroma"]


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    assert _norm(m.group(1)) == _norm(PARAMS[name])


def test_header_declares_the_descriptor_and_the_layouts():
    txt = _header()
    m = re.search(r"typedef\s+struct\s+mi_yuv420_planes\s*\{(.*?)\}\s*mi_yuv420_planes\s*;", txt, re.S)
    assert m, "mi_yuv420_planes is not declared"
    decls = [_norm(d) for d in m.group(1).split(";") if d.strip()]
    assert decls == ["void* y", "size_t y_pitch", "void* c0", "void* c1", "size_t c_pitch", "size_t frame_stride", "int chroma"], decls
    assert re.search(r"enum\s*\{\s*MI_CHROMA_INTERLEAVED\s*=\s*0\s*,\s*MI_CHROMA_PLANAR\s*=\s*1\s*\}\s*;", txt)
    assert (mi_lumaeq.CHROMA_INTERLEAVED, mi_lumaeq.CHROMA_PLANAR) == (0, 1)
    S = mi_lumaeq.Yuv420Planes
    assert S is capi.Yuv420Planes and "Yuv420Planes" in mi_lumaeq.__all__
    assert "CHROMA_INTERLEAVED" in mi_lumaeq.__all__ and "CHROMA_PLANAR" in mi_lumaeq.__all__
    assert [n for n, _ in S._fields_] == FIELDS
    assert ctypes.sizeof(S) == 56


LAYOUT = ('int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mi_yuv420_planes), '
          + ", ".join(f"offsetof(mi_yuv420_planes, {f})" for f in FIELDS) + "); return 0; }\n")


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++11")])
def test_descriptor_layout_matches_c_compiler(tmp_path, lang, std):
    compiler = shutil.which("cc" if lang == "c" else "c++") or shutil.which("gcc" if lang == "c" else "g++")
    if compiler is None:
        pytest.fail(f"no {lang} compiler on PATH")
    src = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi_lumaeq.h"\n' + LAYOUT)
    exe = tmp_path / "probe.bin"
    subprocess.run([compiler, f"-std={std}", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    S = capi.Yuv420Planes
    assert got[0] == ctypes.sizeof(S) == 56
    assert got[1:] == [getattr(S, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48]


def test_declared_behind_the_list_form_and_nothing_grew():
    txt = _header()
    at = [txt.index(s) for s in ("mi_clahe_bgr_to_nv12(", "mi_bgr_nv12_frame_dev", "mi_equalize_hist_bgr_to_nv12_frames_dev",
                                 "mi_clahe_bgr_to_nv12_frames_dev", "MI_CHROMA_INTERLEAVED", "mi_yuv420_planes",
                                 "mi_equalize_hist_yuv420_batch_dev", "mi_clahe_yuv420_batch_dev", "mi_equalize_hist_yuv420(",
                                 "mi_clahe_yuv420(", "mi_host_register")]
    assert at == sorted(at), "the yuv420 block lies between the BGR -> NV12 list form and mi_host_register"
    full = HEADER.read_text()
    assert full.index("mi_clahe_yuv420(") < full.index("optional: pin caller-owned host buffers")
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", full), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert sorted(set(re.findall(r"\bMI_FMT_\w+", txt))) == ["MI_FMT_NV12", "MI_FMT_P010", "MI_FMT_UYVY", "MI_FMT_YUY2"], "no new format"
    assert sorted(set(re.findall(r"\bMI_ORDER_\w+", txt))) == ["MI_ORDER_BGR", "MI_ORDER_RGB"], "no new order"
    m = re.search(r"typedef\s+struct\s+mi_pipe_config\s*\{(.*?)\}\s*mi_pipe_config\s*;", txt, re.S)
    assert m and _norm(m.group(1)).endswith("int format;"), "mi_pipe_config keeps `format` as its last member"


def test_header_states_the_contract():
    """A comment block of its own; the neighbouring blocks are left as they were."""
    m = re.search(r"/\*\s*mi_\*_yuv420\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the yuv420 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("I420 / YV12", "NV12", "c0 is always the U (Cb) plane and c1 the V (Cr) plane", "SECOND chroma plane", "NV21 is not supported",
                   "read only during the call", "never written, except where a plane is processed in place",
                   "byte for byte what mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev write", "fused equalizeHist kernel included",
                   "clahe_fp_contract", "two_kernel_max_frames", "REFLECT_101",
                   "uv[r][2i] = U[r][i], uv[r][2i+1] = V[r][i]", "the inverse", "a row copy",
                   "every chroma byte of the output is 128", "are not read and may be NULL",
                   "only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each output row are written", "not the pitch padding",
                   "gaps between planes", "gaps between frames", "Width and height are even",
                   "No alignment is required of any pointer, pitch or stride",
                   "W % 32 == 0 and all chroma pointers, both c_pitch and both frame_stride are multiples of 16", "the same bytes out",
                   "A same-layout move and a fill have no rule", "EXACTLY the same plane on both sides",
                   "the same address, the same pitch, the same frame_stride", "the same layout",
                   "In-place chroma with MI_UV_COPY moves nothing", "writes 128", "ONE launch of its own per chunk of 256 frames",
                   "MI_K_LUT_APPLY", "yuv420_chroma_vec", "yuv420_chroma_bytes", "counts in neither", "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph",
                   "HOST pointers", "frame_stride is ignored", "mi_*_packed422_to_nv12", "pinned", "tight at the kernels' own pitches",
                   "no copy on the caller's memory is in flight", "mi_cvt_color_420_u8", "MI_ERR_UNSUPPORTED",
                   "a null ctx, `in` or `out`", "a null y", "a null out->c0", "a null out->c1 on a PLANAR output",
                   "a null input chroma pointer that MI_UV_COPY needs", "a `chroma` other than the two values", "a bad uv_mode",
                   "a negative size", "refused even when another size is 0", "y_pitch < W", "a c_pitch below its row", "tiles <= 0",
                   "two output plane pointers of the call that are equal", "other than that exact in-place case",
                   "Any other overlap: undefined, not checked", "MI_OK, nothing written", "Nothing is enqueued unless all checks pass"):
        assert needle in txt, needle
    lst = re.search(r"/\*\s*mi_\*_bgr_to_nv12_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert lst and "yuv420" not in lst.group(0), "the list form's comment was not extended"
    pin = re.search(r"/\*\s*---- optional: pin caller-owned host buffers.*?\*/", HEADER.read_text(), re.S)
    assert pin and "yuv420" not in pin.group(0)


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_yuv420_batch_dev", "clahe_yuv420_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        p = inspect.signature(f).parameters
        assert list(p)[:7] == ["self", "src", "dst", "width", "height", "n_frames", "uv_mode"], m
        assert p["uv_mode"].default == mi_lumaeq.UV_COPY and p["stream"].default == 0
    assert list(inspect.signature(mi_lumaeq.Context.equalize_hist_yuv420_batch_dev).parameters)[7:] == ["stream"]
    p = inspect.signature(mi_lumaeq.Context.clahe_yuv420_batch_dev).parameters
    assert list(p)[7:] == ["clip_limit", "tiles_x", "tiles_y", "stream"]
    for m in ("equalize_hist_yuv420", "clahe_yuv420"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        p = inspect.signature(f).parameters
        assert list(p)[:7] == ["self", "frame", "width", "height", "src_fmt", "dst_fmt", "uv_mode"], m
        assert p["uv_mode"].default == mi_lumaeq.UV_COPY and p["out"].default is None
    for m in ("clahe_yuv420_batch_dev", "clahe_yuv420"):
        p = inspect.signature(getattr(mi_lumaeq.Context, m)).parameters
        assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8), m


def test_tight_frame_makers():
    """nv12 / i420 / yv12 of the binding: YV12 is I420 with the two chroma addresses exchanged, c0 always the U plane."""
    w, h, b = 6, 4, 4096
    P = mi_lumaeq.Yuv420Planes
    n, i, y = P.nv12(b, w, h), P.i420(b, w, h), P.yv12(b, w, h)
    assert (n.y, n.y_pitch, n.c0, n.c1, n.c_pitch, n.frame_stride, n.chroma) == (b, 6, b + 24, None, 6, 36, 0)
    assert (i.y, i.y_pitch, i.c0, i.c1, i.c_pitch, i.frame_stride, i.chroma) == (b, 6, b + 24, b + 30, 3, 36, 1)
    assert (y.y, y.y_pitch, y.c0, y.c1, y.c_pitch, y.frame_stride, y.chroma) == (b, 6, b + 30, b + 24, 3, 36, 1)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_cxx_helpers_are_declared():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    assert re.search(r"struct\s+YUV420View\s*\{", txt)
    for maker in ("nv12", "i420", "yv12"):
        assert re.search(r"static\s+YUV420View\s+" + maker + r"\s*\(\s*unsigned char\*\s*\w+,\s*int\s+\w+,\s*int\s+\w+\)", txt), maker
    for fn, abi in (("equalizeHistYUV420", "mi_equalize_hist_yuv420"), ("claheYUV420", "mi_clahe_yuv420")):
        assert re.search(r"inline\s+void\s+" + fn + r"\s*\(\s*const YUV420View&\s*in,\s*const YUV420View&\s*out,\s*int width,\s*int height,"
                         r"\s*int uvMode", txt), fn
        assert re.search(r"\b" + abi + r"\s*\(", txt), abi
    assert txt.index("claheBGRToNV12") < txt.index("YUV420View") < txt.index("equalizeHistYUV420") < txt.index("claheYUV420")


def test_new_sources_are_registered():
    assert (CSRC / "kernels" / "yuv420.hip.h").exists() and (CSRC / "host" / "yuv420.inc.hpp").exists()
    assert '#include "kernels/yuv420.hip.h"' in (CSRC / "lumaeq_kernels.hip.h").read_text()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/bgr_nv12_frames.inc.hpp"') < tu.index('#include "host/yuv420.inc.hpp"')
    kernels = (CSRC / "kernels" / "yuv420.hip.h").read_text()
    for name in ("yuv420_chroma_kernel", "__builtin_amdgcn_perm", "uv_rows(", "uv_flat("):
        assert name in kernels, name
    assert "__shared__" not in kernels, "the chroma kernel uses no LDS"
    host = (CSRC / "host" / "yuv420.inc.hpp").read_text()
    assert re.search(r"constexpr\s+int\s+kYuv420FramesPerLaunch\s*=\s*256\s*;", host)
    assert "MI_K_LUT_APPLY, yuv420_chroma_kernel" in host
    assert "equalize_dev(c, s, y, nullptr)" in host and re.search(r"clahe_dev\(c, s, y, [^)]*nullptr\)", host), "the luma is the planar forms' own"


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    rng = np.random.default_rng(19)
    src = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    a, b = mi_lumaeq.Yuv420Planes.i420(src.ctypes.data, w, h), mi_lumaeq.Yuv420Planes.nv12(dst.ctypes.data, w, h)
    a0, b0 = bytes(a), bytes(b)
    args = (None, ctypes.byref(a), ctypes.byref(b), w, h)
    assert built_lib.mi_equalize_hist_yuv420_batch_dev(*args, 1, 1, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_yuv420_batch_dev(*args, 1, 1, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_equalize_hist_yuv420(*args, 1) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_yuv420(*args, 1, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(a) == a0 and bytes(b) == b0
