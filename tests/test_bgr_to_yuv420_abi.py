"""Interleaved BGR / RGB in, 4:2:0 frames described by mi_yuv420_planes out (mi_*_bgr_to_yuv420*) at the ABI level, without a GPU: the
header declares the four entry points with their parameter lists behind the 4:2:0 -> BGR list form, no struct, profiling enum or version
grew, the header comment states the contract a caller cannot guess, the binding lists the symbols and has the four Context methods with
their keyword defaults, both libraries export them, the C++ helpers exist, the two new sources are included where they belong, a call
without a context fails loudly without touching the caller's buffers -- and the builder of the expected bytes of the GPU tests
(tests/bgr_yuv420_layouts.py) is the oracle's own I420 conversion."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import oracle
from bgr_yuv420_layouts import as_fmt, deinterleave, expected, rand_images

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1
DEV = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, const mi_yuv420_planes* out, int width, int height, "
       "int n_frames, int order, mi_uv_mode uv_mode")
HOST = "mi_ctx* ctx, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out, int width, int height, int order, mi_uv_mode uv_mode"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_bgr_to_yuv420_batch_dev": DEV + ", void* stream",
    "mi_clahe_bgr_to_yuv420_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_bgr_to_yuv420": HOST,
    "mi_clahe_bgr_to_yuv420": HOST + CLAHE,
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


def test_declared_behind_the_yuv420_to_bgr_list_form_and_nothing_grew():
    txt = _header()
    assert txt.index("mi_clahe_yuv420_to_bgr_frames_dev") < txt.index("mi_equalize_hist_bgr_to_yuv420_batch_dev") < txt.index("mi_host_register")
    for name in NAMES:
        assert txt.index("mi_clahe_yuv420_to_bgr_frames_dev") < txt.index(name) < txt.index("mi_host_register"), name
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", txt), "no struct grew: the minor version stays 3"
    assert ctypes.sizeof(mi_lumaeq.Yuv420Planes) == 56


def test_header_states_the_contract():
    """What a caller cannot guess: the OpenCV sequence the bytes equal, where the chroma comes from and goes, what is written, the two
    stages and their slots, the byte counts, the alignment rule, the counters, the interleaved delegation, the error rules."""
    m = re.search(r"/\*\s*mi_\*_bgr_to_yuv420\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGR -> 4:2:0 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("COLOR_BGR2YUV_I420", "COLOR_RGB2YUV_I420", "cv::equalizeHist", "clahe->apply", "top-left",
                   "U plane going to out->c0 and the V plane to out->c1", "every chroma byte 128", "c0 is always U and c1 always V",
                   "never written", "Only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each output row are written",
                   "not the pitch padding", "MI_K_COLOR", "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST", "mi_clahe_u8_batch_dev",
                   "IN PLACE in out->y", "two_kernel_max_frames", "6.5", "7.5", "256 frames", "holds the unequalized luma",
                   "W % 16 == 0", "out->c0, out->c1 and out->c_pitch are multiples of 8", "one 8-byte U store and one 8-byte V store",
                   "2 x 2 pixel blocks with byte accesses", '"bgr_yuv420_vec"', '"bgr_yuv420_bytes"', "moves exactly one of them",
                   "moves neither", "out->chroma == MI_CHROMA_INTERLEAVED: the call IS the NV12 form's", "d_uv_out = out->c0",
                   "out->c1 ignored", "none of the counters below moves", "clahe_fp_contract", "REFLECT_101", "MI_STREAM_CTX", "MI_ERR_BUSY",
                   "hipGraph", "HOST pointers", "frame_stride is ignored", "Synchronous", "16-byte aligned offset",
                   "no copy on the caller's memory is in flight", "mi_cvt_color_420_u8_batch_dev(MI_COLOR_BGR2YUV_I420)",
                   "a null ctx, d_in or `out`", "a null out->y or out->c0", "a null out->c1 on a PLANAR output",
                   "a `chroma` other than the two values", "an `order` other than the two", "a bad uv_mode", "a negative size",
                   "even when another size is 0", "in_pitch < 3*W", "y_pitch < W", "a c_pitch below its row", "tiles <= 0",
                   "two output plane pointers of the call that are equal", "an output plane pointer equal to d_in",
                   "c1 = c0 + W/2, c_pitch = W", "MI_ERR_UNSUPPORTED", "Nothing is enqueued unless every check passes"):
        assert needle in txt, needle


def test_stat_names_are_documented_next_to_their_siblings():
    txt = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc = txt[: txt.index("mi_status mi_ctx_get_stat(")]
    assert doc.index('"yuv420_bgr_vec"') < doc.index('"bgr_yuv420_vec" / "bgr_yuv420_bytes"')
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    assert re.search(r"uint64_t\s+bgr_yuv420_vec\s*=\s*0\s*,\s*bgr_yuv420_bytes\s*=\s*0\s*;", ctx)
    assert ctx.index("yuv420_bgr_vec = 0, yuv420_bgr_bytes = 0") < ctx.index("bgr_yuv420_vec = 0")


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgr_to_yuv420_batch_dev", "clahe_bgr_to_yuv420_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:6] == ["self", "d_in", "dst", "width", "height", "n_frames"], m
        for kw in ("in_pitch", "in_frame"):
            assert kw in params and params[kw].default is None, (m, kw)
        assert params["stream"].default == 0
        assert params["order"].default == mi_lumaeq.ORDER_BGR and params["uv_mode"].default == mi_lumaeq.UV_COPY
    for m in ("equalize_hist_bgr_to_yuv420", "clahe_bgr_to_yuv420"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:3] == ["self", "img", "dst_fmt"], m
        assert params["dst_fmt"].default == "i420"
        assert params["order"].default == mi_lumaeq.ORDER_BGR and params["uv_mode"].default == mi_lumaeq.UV_COPY
        assert params["out"].default is None
    for m in ("clahe_bgr_to_yuv420_batch_dev", "clahe_bgr_to_yuv420"):
        params = inspect.signature(getattr(mi_lumaeq.Context, m)).parameters
        assert (params["clip_limit"].default, params["tiles_x"].default, params["tiles_y"].default) == (2.0, 8, 8), m


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_cxx_helpers_are_declared():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistBGRToYUV420", "mi_equalize_hist_bgr_to_yuv420"), ("claheBGRToYUV420", "mi_clahe_bgr_to_yuv420")):
        m = re.search(r"inline\s+void\s+" + fn + r"\s*\((.*?)\)\s*\{", txt, re.S)
        assert m, fn
        sig = _norm(m.group(1))
        assert sig.startswith("const unsigned char* in, size_t inStep, const YUV420View& out, int width, int height"), sig
        assert "ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY" in sig, sig
        assert re.search(r"\b" + abi + r"\s*\(", txt), abi
    assert "double clipLimit, Size tiles" in _norm(re.search(r"inline\s+void\s+claheBGRToYUV420\s*\((.*?)\)\s*\{", txt, re.S).group(1))
    assert txt.index("claheYUV420ToBGR") < txt.index("equalizeHistBGRToYUV420") < txt.index("claheBGRToYUV420")


def test_new_sources_are_registered():
    assert (CSRC / "kernels" / "bgr_yuv420.hip.h").exists() and (CSRC / "host" / "bgr_yuv420.inc.hpp").exists()
    k = (CSRC / "lumaeq_kernels.hip.h").read_text()
    assert 0 <= k.index('#include "kernels/bgr_nv12.hip.h"') < k.index('#include "kernels/bgr_yuv420.hip.h"')
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/yuv420_bgr_frames.inc.hpp"') < tu.index('#include "host/bgr_yuv420.inc.hpp"')
    kern = (CSRC / "kernels" / "bgr_yuv420.hip.h").read_text()
    assert re.search(r"template\s*<int ORDER, int UVMODE, bool HIST>\s*__global__[^;{]*\bbgr_to_yuv420_hist_kernel\s*\(", kern)
    job = re.search(r"struct\s+BgrYuv420Job\s*\{(.*?)\};", kern, re.S).group(1)
    job = re.sub(r"//[^\n]*", "", job)
    for field in ("in", "y", "u", "v", "in_step", "y_step", "c_step", "in_frame", "out_frame", "width", "height", "vec"):
        assert re.search(r"\b" + field + r"\s*[,;]", job), field
    host = (CSRC / "host" / "bgr_yuv420.inc.hpp").read_text()
    for fn in ("check_bgr_nv12", "equalize_bgr_nv12_dev", "clahe_bgr_nv12_dev", "equalize_bgr_yuv420_dev", "clahe_bgr_yuv420_dev",
               "launch_apply", "clahe_dev", "stage_in", "StreamDrain"):
        assert re.search(r"\b" + fn + r"\b", host), fn


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 4
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    planes = mi_lumaeq.Yuv420Planes.i420(dst.ctypes.data, w, h)
    a = (None, src.ctypes.data, 3 * w, 3 * w * h, ctypes.byref(planes), w, h, 1, 0, 1)
    assert built_lib.mi_equalize_hist_bgr_to_yuv420_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_yuv420_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 3 * w, ctypes.byref(planes), w, h, 0, 1)
    assert built_lib.mi_equalize_hist_bgr_to_yuv420(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_yuv420(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


@pytest.mark.parametrize("w,h", [(2, 2), (16, 2), (48, 6), (66, 34), (64, 32)])
def test_expected_bytes_builder_is_the_oracles_i420(w, h):
    """oracle.bgr_to_i420 -- cv::cvtColor(COLOR_BGR2YUV_I420) itself -- equals oracle.bgr_to_nv12 plane by plane: Y identical,
    U = uv[0::2], V = uv[1::2].  So the GPU tests' expected frame (the NV12 oracle's, de-interleaved) is the I420 sequence of the
    header; and full-range random pixels leave an identity map no chance."""
    img = rand_images(w, h, 1, 50 + w)[0]
    i420 = oracle.bgr_to_i420(img).reshape(-1)
    nv12 = oracle.bgr_to_nv12(img)
    ysz = w * h
    uv = nv12[ysz:]
    assert np.array_equal(i420[:ysz], nv12[:ysz])
    assert np.array_equal(i420[ysz: ysz + ysz // 4], uv[0::2]) and np.array_equal(i420[ysz + ysz // 4:], uv[1::2])
    assert np.array_equal(deinterleave(nv12, w, h), i420)
    # the builder itself: equalized Y, the conversion's U and V (or 128), for both orders
    for order in (0, 1):
        bgr = img if order == 0 else np.ascontiguousarray(img[:, :, ::-1])
        conv = oracle.bgr_to_i420(bgr).reshape(-1)
        got = expected(img, ("eq", None), order, 1)
        assert np.array_equal(got[:ysz], oracle.equalize_hist(conv[:ysz].reshape(h, w)).reshape(-1))
        assert np.array_equal(got[ysz:], conv[ysz:])
        assert (expected(img, ("clahe", (2.0, 2, 1)), order, 0)[ysz:] == 128).all()
    for fmt in ("i420", "yv12", "nv12"):
        f = as_fmt(i420, w, h, fmt)
        assert f.size == i420.size and np.array_equal(f[:ysz], i420[:ysz])
    assert np.array_equal(as_fmt(i420, w, h, "nv12"), nv12)
    if (w, h) in ((64, 32), (66, 34)):
        changed = (expected(img, ("eq", None), 0, 1)[:ysz] != i420[:ysz]).mean()
        assert changed > 0.9, changed
