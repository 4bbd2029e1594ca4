"""Four-channel BGRA / RGBA (CV_8UC4) in, 4:2:0 frames described by mi_yuv420_planes out (mi_*_bgra_to_yuv420*) at the ABI level, without
a GPU: the header declares the four batch and host entry points with their parameter lists behind mi_clahe_yuv420_to_packed422_frames_dev
and before mi_host_register, no struct, profiling enum or version grew, the header comment states the contract a caller cannot guess,
the statistics stand next to their siblings, the binding lists the symbols and has the four Context methods with their keyword defaults,
both libraries export them, the C++ helpers exist and forward, the new sources are included where they belong, a call without a context
fails loudly without touching the caller's buffers -- and the builder of the expected bytes of the GPU tests
(tests/bgra_yuv420_layouts.py) is the oracle's I420 conversion of the first three channels and tells a wrong channel offset or a wrong
pixel stride apart."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import oracle
from bgra_yuv420_layouts import expected, expected4, rand_images4

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1
DEV = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, const mi_yuv420_planes* out, int width, int height, "
       "int n_frames, int order, mi_uv_mode uv_mode")
HOST = "mi_ctx* ctx, const uint8_t* in, size_t in_step, const mi_yuv420_planes* out, int width, int height, int order, mi_uv_mode uv_mode"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_bgra_to_yuv420_batch_dev": DEV + ", void* stream",
    "mi_clahe_bgra_to_yuv420_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_bgra_to_yuv420": HOST,
    "mi_clahe_bgra_to_yuv420": HOST + CLAHE,
}
NAMES = list(PARAMS)
SIBLING = {n: n.replace("_bgra_", "_bgr_") for n in NAMES}


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


def _decl(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    return _norm(m.group(1))


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point(name):
    assert _decl(name) == _norm(PARAMS[name])
    assert _decl(name) == _decl(SIBLING[name]), "the parameter list of the three-channel sibling"


def test_declared_in_their_window_and_nothing_grew():
    txt = _header()
    for name in NAMES:
        assert txt.index("mi_clahe_yuv420_to_packed422_frames_dev") < txt.index(name) < txt.index("mi_host_register"), name
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert ctypes.sizeof(mi_lumaeq.Yuv420Planes) == 56
    assert sorted(set(re.findall(r"\bMI_ORDER_\w+", txt))) == ["MI_ORDER_BGR", "MI_ORDER_RGB"], "no new order"
    assert sorted(set(re.findall(r"\bMI_CHROMA_\w+", txt))) == ["MI_CHROMA_INTERLEAVED", "MI_CHROMA_PLANAR"], "no new chroma layout"
    assert not re.search(r"\bmi_bgra_\w*frame_dev\b", txt), "the list entry is the existing mi_bgr_yuv420_frame_dev"


def test_header_states_the_contract():
    """What a caller cannot guess: the OpenCV codes the bytes equal, that X takes no part, where the chroma comes from and goes, what is
    written, the two stages and their slots, the byte counts, the alignment rule of both chroma layouts, that an interleaved output is
    not handed on, the counters, the host form's limit, the error rules."""
    m = re.search(r"/\*\s*mi_\*_bgra_to_yuv420\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGRA -> 4:2:0 forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("CV_8UC4", "COLOR_BGRA2YUV_I420", "COLOR_RGBA2YUV_I420", "cv::equalizeHist", "clahe->apply", "top-left",
                   "takes no part in any output byte", "for the image with X removed", "B, G, R, X per pixel", "R, G, B, X",
                   "U plane going to out->c0 and the V plane to out->c1", "every chroma byte 128", "c0 is always U and c1 always V",
                   "never written", "in_pitch >= 4*W",
                   "Only the W bytes (Y, interleaved UV) or W/2 bytes (planar U, V) of each output row are written", "not the pitch padding",
                   "Both chroma layouts are this form's own kernels", "MI_CHROMA_INTERLEAVED output is not handed to another form",
                   "MI_K_COLOR", "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST", "mi_clahe_u8_batch_dev", "IN PLACE in out->y",
                   "two_kernel_max_frames", "4 + 1.5 + 1 + 1 = 7.5", "5.5 + 3 = 8.5", "256 frames", "holds the unequalized luma",
                   "none is required of any pointer, pitch or stride", "W % 16 == 0", "multiples of 16 for interleaved chroma",
                   "one 16-byte UV store", "of 8 for planar chroma", "one 8-byte U store and one 8-byte V store",
                   "eight 16-byte loads", "2 x 2 pixel blocks with byte accesses", '"bgra_yuv420_vec"', '"bgra_yuv420_bytes"',
                   "moves exactly one of them", "moves neither", "clahe_fp_contract", "REFLECT_101", "MI_STREAM_CTX", "MI_ERR_BUSY",
                   "hipGraph", "HOST pointers", "frame_stride is ignored", "Synchronous", "a row of 4*W bytes", "16-byte aligned offset",
                   "no copy on the caller's memory is in flight", "W*H > 0x7fffffff / 4: MI_ERR_UNSUPPORTED",
                   "a null ctx, d_in or `out`", "a null out->y or out->c0", "a null out->c1 on a PLANAR output",
                   "a `chroma` other than the two values", "an `order` other than the two", "a bad uv_mode", "a negative size",
                   "even when another size is 0", "in_pitch < 4*W", "y_pitch < W", "a c_pitch below its row", "tiles <= 0",
                   "two output plane pointers of the call that are equal", "an output plane pointer equal to d_in",
                   "c1 = c0 + W/2, c_pitch = W", "pointers and pitches are not looked at then", "MI_ERR_UNSUPPORTED",
                   "Nothing is enqueued unless every check passes"):
        assert needle in txt, needle


def test_stat_names_stand_next_to_their_siblings():
    txt = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc = txt[: txt.index("mi_status mi_ctx_get_stat(")]
    assert doc.index('"bgr_yuv420_list_frames_vec" / "bgr_yuv420_list_frames_bytes"') < doc.index('"bgra_yuv420_vec" / "bgra_yuv420_bytes"') \
        < doc.index('"bgra_yuv420_list_frames_vec" / "bgra_yuv420_list_frames_bytes"')
    body = txt[txt.index("mi_status mi_ctx_get_stat("):]
    at = [body.index(s) for s in ('"bgr_yuv420_list_frames_bytes"', '"bgra_yuv420_vec"', '"bgra_yuv420_bytes"',
                                  '"bgra_yuv420_list_frames_vec"', '"bgra_yuv420_list_frames_bytes"', '"unknown stat"')]
    assert at == sorted(at)
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    assert re.search(r"uint64_t\s+bgra_yuv420_vec\s*=\s*0\s*,\s*bgra_yuv420_bytes\s*=\s*0\s*;", ctx)
    assert re.search(r"bgra_yuv420_list_frames_vec\s*=\s*0\s*,\s*bgra_yuv420_list_frames_bytes\s*=\s*0\s*;", ctx)
    assert ctx.index("bgr_yuv420_list_frames_vec = 0") < ctx.index("bgra_yuv420_vec = 0") < ctx.index("bgra_yuv420_list_frames_vec = 0")


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    pairs = [("equalize_hist_bgra_to_yuv420_batch_dev", "equalize_hist_bgr_to_yuv420_batch_dev"),
             ("clahe_bgra_to_yuv420_batch_dev", "clahe_bgr_to_yuv420_batch_dev"),
             ("equalize_hist_bgra_to_yuv420", "equalize_hist_bgr_to_yuv420"), ("clahe_bgra_to_yuv420", "clahe_bgr_to_yuv420")]
    for m, sib in pairs:
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        p, q = inspect.signature(f).parameters, inspect.signature(getattr(mi_lumaeq.Context, sib)).parameters
        assert list(p) == list(q), (m, "the parameter names of the three-channel sibling")
        assert [p[k].default for k in p] == [q[k].default for k in q], (m, "and its keyword defaults")
    p = inspect.signature(mi_lumaeq.Context.equalize_hist_bgra_to_yuv420_batch_dev).parameters
    assert list(p)[:6] == ["self", "d_in", "dst", "width", "height", "n_frames"]
    assert p["in_pitch"].default is None and p["in_frame"].default is None and p["stream"].default == 0
    assert p["order"].default == mi_lumaeq.ORDER_BGR and p["uv_mode"].default == mi_lumaeq.UV_COPY
    p = inspect.signature(mi_lumaeq.Context.clahe_bgra_to_yuv420).parameters
    assert list(p)[:3] == ["self", "img", "dst_fmt"] and p["dst_fmt"].default == "i420" and p["out"].default is None
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_cxx_helpers_are_declared_and_forward():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistBGRAToYUV420", "mi_equalize_hist_bgra_to_yuv420"), ("claheBGRAToYUV420", "mi_clahe_bgra_to_yuv420")):
        m = re.search(r"inline\s+void\s+" + fn + r"\s*\((.*?)\)\s*\{(.*?)\n\}", txt, re.S)
        assert m, fn
        sig = _norm(m.group(1))
        assert sig.startswith("const unsigned char* in, size_t inStep, const YUV420View& out, int width, int height"), sig
        assert "ChannelOrder order = ORDER_BGR, UVMode uv = UV_COPY" in sig, sig
        assert re.search(r"\b" + abi + r"\s*\(\s*c\s*,\s*in\s*,\s*inStep\s*,", m.group(2)), (fn, "forwards to", abi)
    assert "double clipLimit, Size tiles" in _norm(re.search(r"inline\s+void\s+claheBGRAToYUV420\s*\((.*?)\)\s*\{", txt, re.S).group(1))
    assert txt.index("claheBGRToYUV420") < txt.index("equalizeHistBGRAToYUV420") < txt.index("claheBGRAToYUV420") \
        < txt.index("equalizeHistBGRToPacked422")


def test_new_sources_are_registered():
    assert (CSRC / "kernels" / "bgra_yuv420.hip.h").exists() and (CSRC / "host" / "bgra_yuv420.inc.hpp").exists()
    k = (CSRC / "lumaeq_kernels.hip.h").read_text()
    assert 0 <= k.index('#include "kernels/bgr_yuv420.hip.h"') < k.index('#include "kernels/bgra_yuv420.hip.h"')
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/yuv420_packed422_frames.inc.hpp"') < tu.index('#include "host/bgra_yuv420.inc.hpp"') \
        < tu.index('#include "host/bgra_yuv420_frames.inc.hpp"') < tu.index('#include "host/pipe.inc.hpp"')
    kern = (CSRC / "kernels" / "bgra_yuv420.hip.h").read_text()
    for entry in ("bgra_to_yuv420_hist_kernel", "bgra_to_yuv420_hist_frames_kernel"):
        assert re.search(r"template\s*<int ORDER, int CHROMA, int UVMODE, bool HIST>\s*__global__[^;{]*\b" + entry + r"\s*\(", kern), entry
    assert len(re.findall(r"\bvoid\s+bgra_to_yuv420_hist_body\s*\(", kern)) == 1, "one body for both layouts and both address policies"
    for name in ("StridedBgraYuv420", "TableBgraYuv420", "bt601_y", "bt601_uv", "lds_inc", "lds_hist_bin", "kCopies", "kFramesPerLaunch"):
        assert re.search(r"\b" + name + r"\b", kern), name
    assert not re.search(r"\b(269484|528482|102760|460324)\b", kern), "the BT.601 arithmetic is reused, not restated"
    assert "load_bgr16" not in re.sub(r"//[^\n]*", "", kern), "every dword is one pixel: no unpacking across dwords"
    assert re.search(r"static_assert\(sizeof\(BgraYuv420Frame\)\s*==\s*32\b", kern)
    assert re.search(r"static_assert\(sizeof\(BgraYuv420Job\)\s*\+\s*sizeof\(BgraYuv420List\)[^;]*<=\s*4096", kern)
    assert re.search(r"__host__\s+__device__[^;{]*\bbgra_yuv420_frame_vec\s*\(", kern), "one rule for the kernel and the host's counters"
    host = (CSRC / "host" / "bgra_yuv420.inc.hpp").read_text()
    for fn in ("check_bgra_yuv420", "launch_bgra_to_yuv420", "equalize_bgra_yuv420_dev", "clahe_bgra_yuv420_dev", "check_yuv420_limits",
               "launch_apply", "clahe_dev", "stage_in", "PlaneOut", "StreamDrain", "equalize_lut_kernel"):
        assert re.search(r"\b" + fn + r"\b", host), fn
    code = re.sub(r"//[^\n]*", "", host)
    for other in ("check_bgr_nv12", "equalize_bgr_nv12_dev", "clahe_bgr_nv12_dev", "bgr_to_nv12_hist_kernel", "bgr_to_yuv420_hist_kernel"):
        assert other not in code, (other, "an interleaved output is not handed to another form")
    assert re.search(r"px \* 11 / 4", code), "the grid's byte basis: half of 4 + 1.5 bytes per pixel"


@pytest.mark.parametrize("chroma", [mi_lumaeq.CHROMA_PLANAR, mi_lumaeq.CHROMA_INTERLEAVED])
def test_null_context_is_bad_arg_and_touches_nothing(built_lib, chroma):
    w, h = 8, 4
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 4, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    mk = mi_lumaeq.Yuv420Planes.i420 if chroma == mi_lumaeq.CHROMA_PLANAR else mi_lumaeq.Yuv420Planes.nv12
    planes = mk(dst.ctypes.data, w, h)
    a = (None, src.ctypes.data, 4 * w, 4 * w * h, ctypes.byref(planes), w, h, 1, 0, 1)
    assert built_lib.mi_equalize_hist_bgra_to_yuv420_batch_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgra_to_yuv420_batch_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    b = (None, src.ctypes.data, 4 * w, ctypes.byref(planes), w, h, 0, 1)
    assert built_lib.mi_equalize_hist_bgra_to_yuv420(*b) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgra_to_yuv420(*b, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


@pytest.mark.parametrize("w,h", [(16, 4), (6, 4)])
def test_expected_bytes_builder_discriminates(w, h):
    """expected4 is oracle.bgr_to_i420 -- cv::cvtColor(COLOR_BGR2YUV_I420) -- plane by plane on the first three channels, with Y equalized;
    it differs between the two orders, from the frame of a kernel that reads every pixel one byte late (G, R, X as colour) and from the
    frame of a kernel that steps 3 bytes a pixel along the 4-byte rows: neither mistake can pass the GPU tests."""
    img = rand_images4(w, h, 1, 60 + w)[0]
    ysz, csz = w * h, w * h // 4
    for order in (0, 1):
        bgr = np.ascontiguousarray(img[:, :, :3] if order == 0 else img[:, :, 2::-1])
        conv = oracle.bgr_to_i420(bgr).reshape(-1)
        got = expected4(img, ("eq", None), order, 1)
        assert got.shape == (ysz * 3 // 2,)
        assert np.array_equal(got[:ysz], oracle.equalize_hist(conv[:ysz].reshape(h, w)).reshape(-1))
        assert np.array_equal(got[ysz: ysz + csz], conv[ysz: ysz + csz]) and np.array_equal(got[ysz + csz:], conv[ysz + csz:])
        assert (expected4(img, ("clahe", (2.0, 2, 1)), order, 0)[ysz:] == 128).all()
        cl = expected4(img, ("clahe", (2.0, 2, 1)), order, 1)
        assert np.array_equal(cl[:ysz], oracle.clahe(conv[:ysz].reshape(h, w), 2.0, 2, 1).reshape(-1)) and np.array_equal(cl[ysz:], conv[ysz:])
    want = expected4(img, ("eq", None), 0, 1)
    assert not np.array_equal(want, expected4(img, ("eq", None), 1, 1)), "the two orders"
    late = np.ascontiguousarray(img[:, :, 1:4])                                      # G, R, X read as B, G, R
    assert not np.array_equal(want, expected(late, ("eq", None), 0, 1)), "a pixel read one byte late"
    rows = img.reshape(h, 4 * w)
    stride3 = np.ascontiguousarray(rows[:, : 3 * w].reshape(h, w, 3))                # pixel x read at byte 3x of its 4W-byte row
    assert not np.array_equal(want, expected(stride3, ("eq", None), 0, 1)), "a 3-byte pixel stride on 4-byte rows"
    for wrong in (late, stride3):                                                    # and already the unequalized planes differ
        assert not np.array_equal(oracle.bgr_to_i420(np.ascontiguousarray(img[:, :, :3])), oracle.bgr_to_i420(wrong))
