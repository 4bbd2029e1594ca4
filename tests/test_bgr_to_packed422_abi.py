"""Interleaved BGR / RGB in, packed 4:2:2 frames (YUY2 / UYVY) out (mi_*_bgr_to_packed422*) at the ABI level, without a GPU: the header
declares the four entry points with their parameter lists behind the BGR -> 4:2:0 list form, no struct, profiling enum or version grew,
the header comment states the contract a caller cannot guess, the binding lists the symbols and has the four Context methods with their
keyword defaults, both libraries export them, the C++ helpers exist, the two new sources are included where they belong, a call without
a context fails loudly without touching the caller's buffers -- and the builder of the expected bytes of the GPU tests
(tests/bgr_packed422_ref.py) equals a NumPy restatement of bt601_y / bt601_uv on the left pixel of every macropixel."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from bgr_packed422_ref import (FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, convert, expected, formula, pack,
                               rand_images)

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1
DEV = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride, "
       "int width, int height, int n_frames, int order, int format, mi_uv_mode uv_mode")
HOST = ("mi_ctx* ctx, const uint8_t* in, size_t in_step, uint8_t* out, size_t out_pitch, int width, int height, int order, int format, "
        "mi_uv_mode uv_mode")
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_bgr_to_packed422_batch_dev": DEV + ", void* stream",
    "mi_clahe_bgr_to_packed422_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_bgr_to_packed422": HOST,
    "mi_clahe_bgr_to_packed422": HOST + CLAHE,
}
NAMES = list(PARAMS)
SHAPES = [(2, 1), (16, 1), (6, 3), (48, 5), (64, 32), (66, 35)]


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    assert _norm(m.group(1)) == _norm(PARAMS[name])


def test_declared_behind_the_bgr_to_yuv420_list_form_and_nothing_grew():
    txt = _header()
    for name in NAMES:
        assert txt.index("mi_clahe_bgr_to_yuv420_frames_dev") < txt.index(name + "(") < txt.index("mi_host_register"), name
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", txt), "no struct grew: the minor version stays 3"
    assert re.findall(r"\bMI_FMT_(\w+)\s*=\s*(\d+)", txt) == [("NV12", "0"), ("P010", "1"), ("YUY2", "2"), ("UYVY", "3")], "no new MI_FMT_* value"
    assert (mi_lumaeq.FMT_YUY2, mi_lumaeq.FMT_UYVY) == (2, 3)


def test_header_states_the_contract():
    """What a caller cannot guess: where luma and chroma come from, that the chroma rule is the library's own, the byte order of the two
    formats, what is written, the alignment rule, the two stages and their slots, the byte counts, the counters, the error rules."""
    m = re.search(r"/\*\s*mi_\*_bgr_to_packed422\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGR -> packed 4:2:2 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("bt601_y(b, g, r) for every pixel", "COLOR_BGR2YUV_I420", "COLOR_RGB2YUV_I420", "mi_cvt_color_420_u8", "cv::equalizeHist",
                   "clahe->apply", "mi_equalize_hist_u8_batch_dev / mi_clahe_u8_batch_dev", "clahe_fp_contract", "REFLECT_101",
                   "bt601_uv of the LEFT pixel (2k, y)", "without averaging", "applied to every row on its own", "every chroma byte 128",
                   "the chroma arithmetic is skipped", "the library's own definition", "consistent with its decode",
                   "mi_*_packed422_to_bgr* reads back the same U and V for both pixels", "No claim is made about COLOR_BGR2YUV_YUY2",
                   "later than the 4.4", "exactly Y0 U Y1 V", "exactly U Y0 V Y1", "MI_ORDER_RGB reads R, G, B",
                   "Width is even", "odd heights are legal", "in_pitch >= 3*W", "at any address", "The input is never written",
                   "out_pitch >= 2*W", "multiples of 4", "Only the 2*W bytes of each output row are written", "not the pitch padding",
                   "not the gaps between frames", "W % 16 == 0", "are all multiples of 16", "three 16-byte loads, two 16-byte stores",
                   "six byte loads and one aligned dword store", "the same bytes out", "256 frames", "MI_K_COLOR", "MI_K_EQ_LUT",
                   "MI_K_LUT_APPLY", "no MI_K_HIST", "IN PLACE on the output frame", "whatever uv_mode is", "mi_clahe_packed422_batch_dev",
                   "every shape in one pass", "two_kernel_max_frames", "3 + 2 + 2 + 2 = 9", "5 + 2 + 4 = 11", "holds the unequalized luma",
                   '"bgr_packed422_vec"', '"bgr_packed422_bytes"', "moves exactly one of them", "moves neither", "MI_STREAM_CTX",
                   "MI_ERR_BUSY", "hipGraph", "Synchronous", "any out_pitch >= 2*W", "tight and 16-byte aligned",
                   "no copy on the caller's memory is in flight", "no in-place form", "d_out == d_in is MI_ERR_BAD_ARG",
                   "any other overlap of input and output is undefined", "a null ctx, d_in or d_out", "an odd width",
                   "even when another size is 0", "a negative size", "in_pitch < 3*W", "out_pitch < 2*W", "an `order` other than the two",
                   "a `format` other than the two", "a bad uv_mode", "tiles <= 0", "MI_OK, nothing written", "MI_ERR_UNSUPPORTED",
                   "Nothing is enqueued unless every check passes", "mi_*_bgr_to_packed422_frames_dev"):
        assert needle in txt, needle


def test_stat_names_are_documented_next_to_their_siblings():
    txt = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc = txt[: txt.index("mi_status mi_ctx_get_stat(")]
    assert doc.index('"bgr_yuv420_vec" / "bgr_yuv420_bytes"') < doc.index('"bgr_packed422_vec" / "bgr_packed422_bytes"')
    body = txt[txt.index("mi_status mi_ctx_get_stat("):]
    for k in ("bgr_packed422_vec", "bgr_packed422_bytes"):
        assert re.search(r'strcmp\(name, "' + k + r'"\)\) \{ \*out = c->' + k + ";", body), k
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    assert re.search(r"uint64_t\s+bgr_packed422_vec\s*=\s*0\s*,\s*bgr_packed422_bytes\s*=\s*0\s*;", ctx)
    assert ctx.index("bgr_yuv420_vec = 0, bgr_yuv420_bytes = 0") < ctx.index("bgr_packed422_vec = 0")


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgr_to_packed422_batch_dev", "clahe_bgr_to_packed422_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:6] == ["self", "d_in", "d_out", "width", "height", "n_frames"], m
        for kw in ("in_pitch", "in_frame", "out_pitch", "out_frame"):
            assert kw in params and params[kw].default is None, (m, kw)
        assert params["stream"].default == 0
        assert (params["order"].default, params["fmt"].default, params["uv_mode"].default) == (mi_lumaeq.ORDER_BGR, mi_lumaeq.FMT_YUY2,
                                                                                               mi_lumaeq.UV_COPY)
    for m in ("equalize_hist_bgr_to_packed422", "clahe_bgr_to_packed422"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:2] == ["self", "img"], m
        assert (params["order"].default, params["fmt"].default, params["uv_mode"].default) == (mi_lumaeq.ORDER_BGR, mi_lumaeq.FMT_YUY2,
                                                                                               mi_lumaeq.UV_COPY)
        assert params["out"].default is None
    for m in ("clahe_bgr_to_packed422_batch_dev", "clahe_bgr_to_packed422"):
        params = inspect.signature(getattr(mi_lumaeq.Context, m)).parameters
        assert (params["clip_limit"].default, params["tiles_x"].default, params["tiles_y"].default) == (2.0, 8, 8), m


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_cxx_helpers_are_declared():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistBGRToPacked422", "mi_equalize_hist_bgr_to_packed422"), ("claheBGRToPacked422", "mi_clahe_bgr_to_packed422")):
        m = re.search(r"inline\s+void\s+" + fn + r"\s*\((.*?)\)\s*\{", txt, re.S)
        assert m, fn
        sig = _norm(m.group(1))
        assert sig.startswith("const unsigned char* in, size_t inStep, unsigned char* out, size_t outPitch, int width, int height"), sig
        assert "PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY" in sig, sig
        assert re.search(r"\b" + abi + r"\s*\(", txt), abi
    assert "double clipLimit, Size tiles" in _norm(re.search(r"inline\s+void\s+claheBGRToPacked422\s*\((.*?)\)\s*\{", txt, re.S).group(1))
    assert txt.index("claheBGRToYUV420") < txt.index("equalizeHistBGRToPacked422") < txt.index("claheBGRToPacked422")


def test_new_sources_are_registered():
    assert (CSRC / "kernels" / "bgr_packed422.hip.h").exists() and (CSRC / "host" / "bgr_packed422.inc.hpp").exists()
    k = (CSRC / "lumaeq_kernels.hip.h").read_text()
    assert 0 <= k.index('#include "kernels/bgr_yuv420.hip.h"') < k.index('#include "kernels/bgr_packed422.hip.h"')
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/bgr_yuv420_frames.inc.hpp"') < tu.index('#include "host/bgr_packed422.inc.hpp"')
    kern = (CSRC / "kernels" / "bgr_packed422.hip.h").read_text()
    assert re.search(r"template\s*<int ORDER, int OFF, int UVMODE, bool HIST>\s*__global__[^;{]*\bbgr_to_packed422_hist_kernel\s*\("
                     r"BgrPacked422Job j, uint32_t\* __restrict__ partial\)", kern)
    job = re.search(r"struct\s+BgrPacked422Job\s*\{(.*?)\};", kern, re.S).group(1)
    job = re.sub(r"//[^\n]*", "", job)
    for field in ("in", "out", "in_step", "out_step", "in_frame", "out_frame", "width", "height", "vec"):
        assert re.search(r"\b" + field + r"\s*[,;]", job), field
    for fn in ("load_bgr16", "lds_inc", "kCopies", "bt601_y", "bt601_uv"):
        assert re.search(r"\b" + fn + r"\b", kern), fn
    host = (CSRC / "host" / "bgr_packed422.inc.hpp").read_text()
    for fn in ("PackedOut", "clahe422_dev", "launch_pair", "equalize_lut_kernel", "kBgrNv12FramesPerLaunch", "MI_K_COLOR", "stage_in",
               "stage_out", "StreamDrain", "bgr_packed422_vec", "bgr_packed422_bytes"):
        assert re.search(r"\b" + fn + r"\b", host), fn
    assert "MI_K_HIST" not in re.sub(r"//[^\n]*", "", host), "stage 1 counts: the form has no MI_K_HIST launch"
    # the three-channel pixel form of the templates in that file: 3 bytes a pixel, the byte basis (3 + 2) / 2 a pixel, its own kernels
    for piece in ("struct BgrTo422", "static constexpr int kPx = 3;", "static long long grid_bytes(long long px) { return px * 5 / 2; }",
                  "bgr_to_packed422_hist_kernel<ORDER, OFF, UVMODE, HIST>", "bgr_to_packed422_hist_frames_kernel<ORDER, OFF, UVMODE, HIST>",
                  "bgr_packed422_entry<BgrTo422>"):
        assert piece in host, piece
    for other in ("packed422_bgra", "bgra422", "bgra_packed422", "bgra_to_packed422"):
        assert other not in host.lower(), "the three-channel file does not know the four-channel form"
    assert (ROOT / "tools" / "bgr_to_packed422_ab.py").exists()


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    dst = np.full(w * h * 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    a = (None, src.ctypes.data, 3 * w, 3 * w * h, dst.ctypes.data, 2 * w, 2 * w * h, w, h, 1, 0, FMT_YUY2, 1)
    assert built_lib.mi_equalize_hist_bgr_to_packed422_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_packed422_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 3 * w, dst.ctypes.data, 2 * w, w, h, 0, FMT_UYVY, 1)
    assert built_lib.mi_equalize_hist_bgr_to_packed422(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_packed422(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


@pytest.mark.parametrize("w,h", SHAPES)
def test_reference_builder_is_the_left_pixel_rule(w, h):
    """convert() -- oracle.bgr_to_nv12 on the row-doubled image -- equals bt601_y of every pixel and bt601_uv of the left pixel of every
    macropixel of every row, restated in NumPy, for both orders; expected() interleaves exactly Y0 U Y1 V / U Y0 V Y1; and on full-range
    random pixels neither an identity map nor a 4:2:0 chroma can pass."""
    img = rand_images(w, h, 1, 60 + w)[0]
    for order in (ORDER_BGR, ORDER_RGB):
        y, uv = convert(img, order)
        fy, fuv = formula(img, order)
        assert y.shape == uv.shape == (h, w)
        assert np.array_equal(y, fy) and np.array_equal(uv, fuv), (w, h, order)
        for fmt in (FMT_YUY2, FMT_UYVY):
            raw = expected(img, None, order, fmt, UV_COPY)
            assert raw.shape == (h, 2 * w) and np.array_equal(raw, pack(fy, fuv, fmt))
            mp = raw.reshape(h, w // 2, 4)
            yi, ui, vi = ((0, 2), 1, 3) if fmt == FMT_YUY2 else ((1, 3), 0, 2)
            assert np.array_equal(mp[:, :, yi[0]], fy[:, 0::2]) and np.array_equal(mp[:, :, yi[1]], fy[:, 1::2])
            assert np.array_equal(mp[:, :, ui], fuv[:, 0::2]) and np.array_equal(mp[:, :, vi], fuv[:, 1::2])
            eq = expected(img, ("eq", None), order, fmt, UV_COPY)
            assert np.array_equal(eq[:, 3 - fmt::2], fuv), "the chroma is the conversion's"
            fill = expected(img, ("clahe", (2.0, 2, 1)), order, fmt, UV_FILL128)
            assert (fill[:, 3 - fmt::2] == 128).all()
    if (w, h) in ((64, 32), (66, 35)):
        y, uv = convert(img)
        eq = expected(img, ("eq", None), ORDER_BGR, FMT_YUY2, UV_COPY)
        assert (eq[:, 0::2] != y).mean() > 0.9, "equalization changes the luma"
        cl = expected(img, ("clahe", (2.0, 4, 3)), ORDER_BGR, FMT_YUY2, UV_COPY)
        assert (cl[:, 0::2] != y).mean() > 0.9, "CLAHE changes the luma"
        assert (uv[1::2] != uv[0:-1:2][: uv[1::2].shape[0]]).mean() > 0.9, "odd-row chroma differs from the row above"
