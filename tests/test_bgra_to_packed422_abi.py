"""Four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 frames (YUY2 / UYVY) out (mi_*_bgra_to_packed422*) at the ABI level, without a
GPU: the header declares the four batch / host entry points with the three-channel form's parameter lists, no struct, profiling enum or
version grew, the header comment states the contract a caller cannot guess, the sibling's "Not built" line no longer lists BGRA input,
the binding lists the symbols and has the four Context methods with the sibling's argument order, both libraries export them, the C++
helpers exist, the new sources are included where they belong, a call without a context fails loudly without touching the caller's
buffers -- and the builder of the expected bytes of the GPU tests (tests/bgra_packed422_ref.py) equals the NumPy `formula` of
bgr_packed422_ref on the first three channels, and tells the mistakes a four-byte reader can make from the right bytes."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import bgr_packed422_ref as ref3
from bgra_packed422_ref import (COUNTERS, LIST_COUNTERS, FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, expected, first3,
                                formula, pack, rand_images4, with_x)

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
    "mi_equalize_hist_bgra_to_packed422_batch_dev": DEV + ", void* stream",
    "mi_clahe_bgra_to_packed422_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_bgra_to_packed422": HOST,
    "mi_clahe_bgra_to_packed422": HOST + CLAHE,
}
NAMES = list(PARAMS)
SHAPES = [(2, 1), (16, 1), (6, 3), (48, 5), (64, 32), (66, 35)]


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


def _params(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    return _norm(m.group(1))


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point_with_the_siblings_parameters(name):
    assert _params(name) == _norm(PARAMS[name])
    assert _params(name) == _params(name.replace("bgra_to_packed422", "bgr_to_packed422")), "the three-channel form's signature"


def test_nothing_grew():
    txt = _header()
    for name in NAMES:
        assert txt.index("mi_clahe_bgr_to_packed422_frames_dev(") < txt.index(name + "(") < txt.index("mi_host_register"), name
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", txt), "no struct grew: the minor version stays 3"
    assert re.findall(r"\bMI_FMT_(\w+)\s*=\s*(\d+)", txt) == [("NV12", "0"), ("P010", "1"), ("YUY2", "2"), ("UYVY", "3")], "no new MI_FMT_* value"
    assert txt.count("typedef struct mi_bgr_packed422_frame_dev") == 1 and "mi_bgra_packed422_frame_dev" not in txt


def test_header_states_the_contract():
    m = re.search(r"/\*\s*mi_\*_bgra_to_packed422\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGRA -> packed 4:2:2 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("CV_8UC4", "byte for byte what mi_*_bgr_to_packed422* writes for the image with its fourth byte removed",
                   "bt601_y(b, g, r) of every pixel", "cv::equalizeHist", "CLAHE::apply", "clahe_fp_contract", "REFLECT_101",
                   "bt601_uv of the LEFT pixel (2k, y)", "without averaging", "every chroma byte 128", "exactly Y0 U Y1 V",
                   "exactly U Y0 V Y1", "MI_ORDER_BGR reads B, G, R, X", "R, G, B, X", "read with its pixel and takes part in nothing",
                   "in_pitch >= 4*W", "at any address", "The input is never written", "out_pitch >= 2*W", "multiples of 4",
                   "Only the 2*W bytes of each output row are written", "Width is even", "odd heights are legal",
                   "Every CLAHE shape runs in one pass", "W % 16 == 0", "are all multiples of 16", "four 16-byte loads",
                   "two 16-byte stores", "8*mx + {0,1,2} and 8*mx + 4 + {0,1,2}", "one aligned dword store", "the same bytes out",
                   "256 frames", "MI_K_COLOR", "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST", "IN PLACE on the output frame",
                   "mi_clahe_packed422_batch_dev", "two_kernel_max_frames", "4 + 2 + 2 + 2 = 10", "6 + 2 + 4 = 12",
                   "holds the unequalized luma", "moves exactly one of them", "moves neither",
                   "No call of this form moves a bgr_packed422* counter", "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph", "Synchronous",
                   "staged in like mi_*_bgra_to_yuv420's", "comes back like mi_*_bgr_to_packed422's", "0x7fffffff / 4",
                   "no copy on the caller's memory is in flight", "d_out == d_in is MI_ERR_BAD_ARG", "an odd width",
                   "even when another size is 0", "a negative size", "in_pitch < 4*W", "out_pitch < 2*W", "a bad uv_mode", "tiles <= 0",
                   "MI_OK, nothing written", "MI_ERR_UNSUPPORTED", "Nothing is enqueued unless every check passes",
                   "mi_*_bgra_to_packed422_frames_dev", "YVYU / VYUY", "chroma averaging", "a use for the alpha byte", "P010 / 16-bit") \
            + tuple('"%s"' % k for k in COUNTERS):
        assert needle in txt, needle
    sib = re.search(r"/\*\s*mi_\*_bgr_to_packed422\*.*?\*/", HEADER.read_text(), re.S)
    stxt = _norm(sib.group(0).replace("\n *", " "))
    tail = stxt[stxt.index("Not built:"):]
    assert "BGRA" not in tail and "YVYU / VYUY" in tail and "chroma averaging" in tail, "the sibling still lists BGRA input as not built"
    assert "mi_*_bgra_to_packed422*" in stxt, "the sibling's comment points to the new block"


def test_stat_names_are_served_and_documented():
    txt = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc = txt[: txt.index("mi_status mi_ctx_get_stat(")]
    body = txt[txt.index("mi_status mi_ctx_get_stat("):]
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    assert '"bgra_packed422_vec" / "bgra_packed422_bytes"' in doc
    assert '"bgra_packed422_list_frames_vec" / "bgra_packed422_list_frames_bytes"' in doc
    for k in COUNTERS + LIST_COUNTERS:
        assert re.search(r'strcmp\(name, "' + k + r'"\)\) \{ \*out = c->' + k + ";", body), k
        assert re.search(r"\b" + k + r"\s*=\s*0\b", ctx), k


def test_binding_has_the_siblings_argument_order():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgra_to_packed422_batch_dev", "clahe_bgra_to_packed422_batch_dev", "equalize_hist_bgra_to_packed422",
              "clahe_bgra_to_packed422"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        sib = getattr(mi_lumaeq.Context, m.replace("bgra_to_packed422", "bgr_to_packed422"))
        p, q = inspect.signature(f).parameters, inspect.signature(sib).parameters
        assert list(p) == list(q), m
        assert [v.default for v in p.values()] == [v.default for v in q.values()], m
    p = inspect.signature(mi_lumaeq.Context.equalize_hist_bgra_to_packed422_batch_dev).parameters
    assert list(p)[:6] == ["self", "d_in", "d_out", "width", "height", "n_frames"]
    assert (p["order"].default, p["fmt"].default, p["uv_mode"].default) == (mi_lumaeq.ORDER_BGR, mi_lumaeq.FMT_YUY2, mi_lumaeq.UV_COPY)


def test_binding_refuses_three_channel_host_images():
    """The host wrappers take H x W x 4 arrays only; the refusal needs no context."""
    c = mi_lumaeq.Context.__new__(mi_lumaeq.Context)
    for bad in (np.zeros((4, 8, 3), np.uint8), np.zeros((4, 32), np.uint8), np.zeros((4, 8, 4), np.uint16)):
        with pytest.raises(mi_lumaeq.MiError):
            c._bgra_packed422_host(bad, None, "t")
    with pytest.raises(mi_lumaeq.MiError):
        c._bgra_packed422_host(np.zeros((4, 8, 4), np.uint8), np.zeros((3, 16), np.uint8), "t")           # one row short
    img, h, w, step, out = c._bgra_packed422_host(np.zeros((4, 8, 4), np.uint8), None, "t")
    assert (h, w, step, out.shape) == (4, 8, 32, (4, 16))
    padded = np.lib.stride_tricks.as_strided(np.zeros((4, 40), np.uint8), (4, 8, 4), (40, 4, 1))
    assert c._bgra_packed422_host(padded, None, "t")[3] == 40


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s
            assert getattr(L, s).argtypes == getattr(L, s.replace("bgra_to_packed422", "bgr_to_packed422")).argtypes, s


def test_cxx_helpers_are_declared():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistBGRAToPacked422", "mi_equalize_hist_bgra_to_packed422"), ("claheBGRAToPacked422", "mi_clahe_bgra_to_packed422")):
        m = re.search(r"inline\s+void\s+" + fn + r"\s*\((.*?)\)\s*\{(.*?)\n\}", txt, re.S)
        assert m, fn
        sig = _norm(m.group(1))
        assert sig.startswith("const unsigned char* in, size_t inStep, unsigned char* out, size_t outPitch, int width, int height"), sig
        assert "PackedFormat format = FMT_YUY2, ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY" in sig, sig
        assert re.search(r"\b" + abi + r"\s*\(\s*c\s*,\s*in\s*,\s*inStep\s*,", m.group(2)), (fn, "forwards to", abi)
    assert "double clipLimit, Size tiles" in _norm(re.search(r"inline\s+void\s+claheBGRAToPacked422\s*\((.*?)\)\s*\{", txt, re.S).group(1))
    assert txt.index("claheBGRToPacked422") < txt.index("equalizeHistBGRAToPacked422") < txt.index("claheBGRAToPacked422")


def test_new_sources_are_registered():
    assert (CSRC / "kernels" / "bgra_packed422.hip.h").exists() and (CSRC / "host" / "bgra_packed422.inc.hpp").exists()
    k = (CSRC / "lumaeq_kernels.hip.h").read_text()
    for before in ("bgr_packed422", "bgra_yuv420", "packed422"):
        assert 0 <= k.index('#include "kernels/%s.hip.h"' % before) < k.index('#include "kernels/bgra_packed422.hip.h"'), before
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    for before in ("bgr_packed422_frames", "bgra_yuv420", "packed422"):
        assert 0 <= tu.index('#include "host/%s.inc.hpp"' % before) < tu.index('#include "host/bgra_packed422.inc.hpp"'), before
    assert tu.index('#include "host/bgra_packed422.inc.hpp"') < tu.index('#include "host/bgra_packed422_frames.inc.hpp"') \
        < tu.index('#include "host/pipe.inc.hpp"')
    kern = (CSRC / "kernels" / "bgra_packed422.hip.h").read_text()
    for entry in ("bgra_to_packed422_hist_kernel", "bgra_to_packed422_hist_frames_kernel"):
        assert re.search(r"template\s*<int ORDER, int OFF, int UVMODE, bool HIST>\s*__global__[^;{]*\b" + entry + r"\s*\(", kern), entry
    assert re.search(r"template\s*<int ORDER, int OFF, int UVMODE, bool HIST, class Frames>[^;{]*\bvoid\s+bgra_to_packed422_hist_body\s*\(", kern)
    assert len(re.findall(r"\bvoid\s+bgra_to_packed422_hist_body\s*\(", kern)) == 1, "one body for both address policies"
    code = re.sub(r"//[^\n]*", "", kern)
    for name in ("StridedBgraPacked422", "TableBgraPacked422", "Packed422List", "bgra_px<ORDER>", "bt601_y", "bt601_uv", "lds_inc",
                 "lds_hist_bin", "kCopies", "put_y<OFF>", "kUShift", "kVShift", "kFill", "u32x4"):
        assert name in code, name
    assert not re.search(r"\b(269484|528482|102760|460324)\b", kern), "the BT.601 arithmetic is reused, not restated"
    assert "load_bgr16" not in code, "every dword is one pixel: no unpacking across dwords"
    assert "struct Packed422List" not in code and "struct Packed422Frame" not in code, "Packed422List is used as it is"
    assert "asm" not in code and "__builtin_nontemporal" not in code, "plain loads and stores, no inline assembly"
    assert re.search(r"static_assert\(sizeof\(BgraPacked422Job\)\s*\+\s*sizeof\(Packed422List\)\s*\+\s*sizeof\(uint32_t\*\)\s*\+\s*256\s*<=\s*4096", kern)
    assert re.search(r"__host__\s+__device__[^;{]*\bbgra_packed422_frame_vec\s*\(", kern), "one rule for the kernel and the host's counters"
    # the four-channel file holds the pixel form and the extern "C" functions; the one implementation, a template on the form, is
    # bgr_packed422.inc.hpp's
    host = (CSRC / "host" / "bgra_packed422.inc.hpp").read_text()
    hcode = re.sub(r"//[^\n]*", "", host)
    for fn in ("struct BgraTo422", "using Job = BgraPacked422Job;", "bgra_to_packed422_hist_kernel<ORDER, OFF, UVMODE, HIST>",
               "bgra_to_packed422_hist_frames_kernel<ORDER, OFF, UVMODE, HIST>", "bgra_packed422_frame_vec(shape_vec, in, out)",
               "bgra_packed422_vec", "bgra_packed422_bytes", "bgr_packed422_entry<BgraTo422>"):
        assert fn in hcode, fn
    assert not re.search(r"\bmi_status\s+(?!mi_)\w+\s*\(", hcode), "nothing but the form and the extern \"C\" functions"
    generic = re.sub(r"//[^\n]*", "", (CSRC / "host" / "bgr_packed422.inc.hpp").read_text())
    for fn in ("check_bgr_packed422", "launch_bgr_to_packed422", "bgr_packed422_in_place", "PackedOut", "clahe422_dev", "launch_pair",
               "equalize_lut_kernel", "kBgrNv12FramesPerLaunch", "MI_K_COLOR", "check_yuv420_limits", "stage_in", "stage_out", "StreamDrain"):
        assert re.search(r"\b" + fn + r"\b", generic), fn
    assert len(re.findall(r"template <class F(?:, int OFF)?>\s*mi_status (check_bgr_packed422|launch_bgr_to_packed422|equalize_bgr_packed422_dev|"
                          r"clahe_bgr_packed422_dev|bgr_packed422_dev|bgr_packed422_host|bgr_packed422_entry)\(", generic)) == 7, \
        "each written once, for every form"
    assert "MI_K_HIST" not in generic and "hist_lut_kernel" not in generic
    assert "F::template kernel<O, FMT, U, true>" in generic and "F::template frames_kernel<O, FMT, U, true>" in generic
    assert "MI_K_HIST" not in hcode and "hist_lut_kernel" not in hcode, "stage 1 counts: the form has no MI_K_HIST launch"
    assert not re.search(r"\bbgr_packed422_(vec|bytes|list_frames_vec|list_frames_bytes)\b", hcode), "no three-channel counter is moved"
    assert not re.search(r"\bbgr_to_packed422_hist(_frames)?_kernel\b", hcode), "stage 1 is this form's own kernel"
    # the form's constants (bytes per pixel 4, byte basis px * 3: half of 4 + 2 bytes per pixel) and the one expression using each
    assert "static constexpr int kPx = 4;" in hcode
    assert re.search(r"static long long grid_bytes\(long long px\) \{ return px \* 3; \}", hcode), "the grid's byte basis"
    assert re.search(r"blocks_per_frame\(c, F::grid_bytes\(px\), a\.height, nf, 2048\)", generic)
    assert re.search(r"in_pitch < F::kPx \* \(size_t\)a\.width", generic) and re.search(r"0x7fffffffLL / F::kPx", generic)
    assert 'kInPitch = "in_pitch < 4 * width"' in hcode and "fail(c, MI_ERR_BAD_ARG, F::kInPitch)" in generic
    assert (ROOT / "tools" / "bgra_to_packed422_ab.py").exists()


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 4, dtype=np.uint8)
    dst = np.full(w * h * 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    a = (None, src.ctypes.data, 4 * w, 4 * w * h, dst.ctypes.data, 2 * w, 2 * w * h, w, h, 1, 0, FMT_YUY2, 1)
    assert built_lib.mi_equalize_hist_bgra_to_packed422_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgra_to_packed422_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 4 * w, dst.ctypes.data, 2 * w, w, h, 0, FMT_UYVY, 1)
    assert built_lib.mi_equalize_hist_bgra_to_packed422(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgra_to_packed422(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


@pytest.mark.parametrize("w,h", SHAPES)
def test_expected_bytes_are_the_formula_on_the_first_three_channels(w, h):
    """expected() on an H x W x 4 image is the NumPy restatement of bt601_y / bt601_uv (bgr_packed422_ref.formula) on its first three
    channels, interleaved exactly Y0 U Y1 V / U Y0 V Y1, for both orders; the fourth byte -- 0x00, 0xFF or random -- changes nothing."""
    img = rand_images4(w, h, 1, 70 + w)[0]
    for order in (ORDER_BGR, ORDER_RGB):
        fy, fuv = formula(first3(img), order)
        for fmt in (FMT_YUY2, FMT_UYVY):
            raw = expected(img, None, order, fmt, UV_COPY)
            assert raw.shape == (h, 2 * w) and np.array_equal(raw, pack(fy, fuv, fmt)), (order, fmt)
            assert np.array_equal(raw, ref3.expected(first3(img), None, order, fmt, UV_COPY))
            eq = expected(img, ("eq", None), order, fmt, UV_COPY)
            assert np.array_equal(eq[:, 3 - fmt::2], fuv), "the chroma is the conversion's"
            assert np.array_equal(eq, ref3.expected(first3(img), ("eq", None), order, fmt, UV_COPY))
            fill = expected(img, ("clahe", (2.0, 2, 1)), order, fmt, UV_FILL128)
            assert (fill[:, 3 - fmt::2] == 128).all()
            for x in (0x00, 0xFF, "random"):
                assert np.array_equal(expected(with_x([img], x)[0], ("eq", None), order, fmt, UV_COPY), eq), x


@pytest.mark.parametrize("w,h", [(16, 4), (6, 3), (66, 35)])
def test_expected_bytes_tell_a_four_byte_readers_mistakes(w, h):
    """The right bytes differ between the two orders, from the frame of a kernel with a wrong channel offset (every pixel read one byte
    late: G, R, X as colour), from one that steps 3 bytes a pixel along the 4-byte rows, and from one that reads the fourth byte as a
    channel (B, G, X): none of these can pass the GPU tests.  Already the unequalized frames differ."""
    img = rand_images4(w, h, 1, 80 + w)[0]
    rows = img.reshape(h, 4 * w)
    late = np.ascontiguousarray(img[:, :, 1:4])                                      # G, R, X read as B, G, R
    stride3 = np.ascontiguousarray(rows[:, : 3 * w].reshape(h, w, 3))                # pixel x read at byte 3x of its 4W-byte row
    x_as_r = np.ascontiguousarray(img[:, :, [0, 1, 3]])                              # the fourth byte read as the third channel
    x_as_b = np.ascontiguousarray(img[:, :, [3, 1, 2]])                              # ... as the first
    for op in (None, ("eq", None)):
        for fmt in (FMT_YUY2, FMT_UYVY):
            want = expected(img, op, ORDER_BGR, fmt, UV_COPY)
            assert not np.array_equal(want, expected(img, op, ORDER_RGB, fmt, UV_COPY)), "the two orders"
            for name, wrong in (("offset", late), ("stride", stride3), ("x as r", x_as_r), ("x as b", x_as_b)):
                assert not np.array_equal(want, ref3.expected(wrong, op, ORDER_BGR, fmt, UV_COPY)), (name, op, fmt)
            assert not np.array_equal(want, expected(img, op, ORDER_BGR, 5 - fmt, UV_COPY)), "the two formats"
    # the luma alone tells a wrong red / blue byte; the chroma alone tells it too
    y, uv = formula(first3(img))
    for wrong in (late, x_as_r, x_as_b):
        wy, wuv = formula(wrong)
        assert not np.array_equal(y, wy) and not np.array_equal(uv, wuv)
