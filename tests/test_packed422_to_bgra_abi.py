"""Packed 4:2:2 in, BGRA / RGBA out (mi_*_packed422_to_bgra*: batch and host forms) at the ABI level, without a GPU: the header
declares the four entry points with the parameter lists of their three-channel siblings and states the contract and every error case,
no struct, enum or profiling slot grew, the binding lists the symbols and has the four Context methods, both libraries export them, the
new sources are registered and carry their static_asserts, the four counter names are served by mi_ctx_get_stat, a null context is
refused without touching the caller's buffers -- and the builder of the expected bytes (tests/packed422_bgra_ref.py) and its restated
store-path rule are checked on their own."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import packed422_bgr_ref as bgr_ref
import packed422_bgra_ref as ref
from packed422_bgra_ref import FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1

DEV = ("mi_ctx* ctx, const void* d_in, size_t in_pitch, size_t in_frame_stride, void* d_out, size_t out_pitch, size_t out_frame_stride, "
       "int width, int height, int n_frames, int format, int order")
HOST = "mi_ctx* ctx, const uint8_t* in, size_t in_pitch, uint8_t* out, size_t out_step, int width, int height, int format, int order"
CLAHE = ", double clip_limit, int tiles_x, int tiles_y"
PARAMS = {
    "mi_equalize_hist_packed422_to_bgra_batch_dev": DEV + ", void* stream",
    "mi_clahe_packed422_to_bgra_batch_dev": DEV + CLAHE + ", void* stream",
    "mi_equalize_hist_packed422_to_bgra": HOST,
    "mi_clahe_packed422_to_bgra": HOST + CLAHE,
}
NAMES = list(PARAMS)
SIBLING = {n: n.replace("_to_bgra", "_to_bgr") for n in NAMES}


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


def test_nothing_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3), ("MI_ORDER_BGR", 0), ("MI_ORDER_RGB", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert not re.search(r"\bMI_FMT_\w+\s*=\s*4\b", txt), "no new format value"
    assert not re.search(r"\bmi_packed422_bgra\w*frame_dev\b", txt), "the list entry is the existing mi_packed422_bgr_frame_dev"


def test_header_states_the_contract_and_names_each_error_case():
    m = re.search(r"/\*\s*mi_\*_packed422_to_bgra\*.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> BGRA forms"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("COLOR_YUV2BGRA_YUY2", "_UYVY", "COLOR_YUV2RGBA_", "extractChannel", "insertChannel",
                   "byte for byte what mi_*_packed422_to_bgr* writes", "the fourth byte is 255", "its own chroma",
                   "exactly Y0 U Y1 V", "exactly U Y0 V Y1", "YVYU", "multiples of 4", "odd heights are legal", "never written",
                   "out_pitch >= 4*W", "No alignment is required", "an odd address and an odd pitch are legal",
                   "not the pitch padding, not the gap between frames",
                   "WIDE when its image address is a multiple of 4", "out_frame_stride", "four 16-byte stores", "no pixel straddles a dword",
                   "dword stores", "slower, the same bytes out",
                   "one pass", "no scratch Y plane", "no two-pass fallback", "REFLECT_101", "clahe_fp_contract", "clahe_float_tables",
                   "too wide for the LDS pair table",
                   "Never the fused equalizeHist kernel", "existing profiling slots", "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph capture",
                   "packed422_bgra_wide", "packed422_bgra_bytes", "No existing counter moves",
                   # the error cases
                   "a null ctx or frame pointer", "an odd width", "negative size", "in_pitch < 2*W or out_pitch < 4*W",
                   "not a multiple of 4", "a `format` or an `order` other than the two", "tiles <= 0", "d_out == d_in",
                   "the rows of the image meet the rows of the input", "W*H > 0x7fffffff / 4: MI_ERR_UNSUPPORTED",
                   "more than 65535 tiles", "a height above 65535 with tiles_x > 62", "MI_ERR_UNSUPPORTED",
                   "width, height or n_frames of 0: MI_OK, nothing written", "Nothing is enqueued unless all checks pass"):
        assert needle in txt, needle
    other = re.search(r"/\*\s*mi_\*_bgra_to_yuv420\*.*?\*/", HEADER.read_text(), re.S)
    assert other and "Not built: packed 4:2:2 in, BGRA out" not in _norm(other.group(0).replace("\n *", " "))


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_bgra_batch_dev", "clahe_packed422_to_bgra_batch_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params) == list(inspect.signature(getattr(mi_lumaeq.Context, m.replace("_to_bgra", "_to_bgr"))).parameters), m
        for kw in ("in_pitch", "in_frame", "out_pitch", "out_frame", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
        assert params["fmt"].default == FMT_YUY2 and params["order"].default == ORDER_BGR
    for m in ("equalize_hist_packed422_to_bgra", "clahe_packed422_to_bgra"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params) == list(inspect.signature(getattr(mi_lumaeq.Context, m.replace("_to_bgra", "_to_bgr"))).parameters), m
        assert params["out"].default is None and params["fmt"].default == FMT_YUY2 and params["order"].default == ORDER_BGR
    p = inspect.signature(mi_lumaeq.Context.clahe_packed422_to_bgra).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s
            assert getattr(L, s).argtypes == getattr(L, SIBLING[s]).argtypes, s


def test_cxx_helpers_are_declared_and_forward():
    txt = (ROOT / "opencv-opencl_amd" / "cxx" / "mi_cv.hpp").read_text()
    for fn, abi in (("equalizeHistPacked422ToBGRA", "mi_equalize_hist_packed422_to_bgra"), ("clahePacked422ToBGRA", "mi_clahe_packed422_to_bgra")):
        m = re.search(r"inline\s+void\s+" + fn + r"\s*\((.*?)\)\s*\{(.*?)\n\}", txt, re.S)
        assert m, fn
        assert "PackedFormat format = FMT_YUY2" in m.group(1) and "ChannelOrder order = ORDER_BGR" in m.group(1)
        assert abi + "(c, in, inPitch, out, outStep, width, height, (int)format, (int)order" in m.group(2), fn
    assert txt.index("claheYUV420ToBGRA") < txt.index("equalizeHistPacked422ToBGRA") < txt.index("clahePacked422ToBGRA")


def test_new_sources_are_registered_and_assert_their_sizes():
    k = (CSRC / "lumaeq_kernels.hip.h").read_text()
    assert 0 <= k.index('#include "kernels/yuv420_bgra.hip.h"') < k.index('#include "kernels/packed422_bgra.hip.h"')
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert tu.index('"host/packed422_bgr_frames.inc.hpp"') < tu.index('"host/packed422_bgra.inc.hpp"') \
        < tu.index('"host/packed422_bgra_frames.inc.hpp"') < tu.index('"host/pipe.inc.hpp"')
    kern = (CSRC / "kernels" / "packed422_bgra.hip.h").read_text()
    # the LUT-apply and the interpolation body are the three-channel file's, templates on the block and a store policy; this file
    # brings the policy, wraps them, and keeps the wide-grid fallback written out
    for name in ("lut_apply422_bgr_body<OFF, Store422Bgra<ORDER>>", "clahe_interp422_bgr_body<FT, FMA, OFF, Store422Bgra<ORDER>>",
                 "clahe_interp422_bgra_global_body", "Packed422Bgra", "Strided422Bgra", "Table422Bgra", "Packed422List", "Store422Bgra",
                 "chroma422", "bt601_uv_terms", "bt601_px_bgr", "bgra_dword", "clahe_px"):
        assert name in kern, name
    shared = (CSRC / "kernels" / "packed422_bgr.hip.h").read_text()
    for name in ("lut_apply422_bgr_body(const Block& p, const Frames& fr,", "clahe_interp422_bgr_body(const Block& p, const Frames& fr,",
                 "S::group(", "S::kGroupBytes", "S::kPxBytes", "gather422", "chroma422", "load422_tail", "lut_vec", "interp_stage",
                 "clahe_vec16_f32", "clahe_vec16", "clahe_px"):
        assert name in shared, name
    assert not re.search(r"\b(1673527|852492|409993|2116026|1220542)\b", kern), "the BT.601 arithmetic is reused, not restated"
    code = re.sub(r"//[^\n]*", "", kern)
    assert "decode422_16" not in code and "store422_px" not in code, "every pixel is one dword: none of the 48-byte packing"
    assert re.search(r"__host__\s+__device__[^;{]*\bpacked422_bgra_frame_wide\s*\(", kern), "one rule for the kernel and the host's counters"
    assert re.search(r"\bpacked422_bgra_frame_wide\s*\([^)]*\)\s*\{\s*return packed422_image_wide\(out, out_step, out_frame\);", kern), \
        "... which is the one rule of both image forms"
    assert re.search(r"__host__\s+__device__[^;{]*\bpacked422_image_wide\s*\(", shared)
    assert re.search(r"static_assert\(sizeof\(Packed422Bgra\)\s*==\s*sizeof\(Packed422Bgr\)", kern)
    assert re.search(r"static_assert\(sizeof\(Packed422List\)\s*\+\s*sizeof\(Packed422Bgra\)[^;]*<=\s*4096", kern)
    # the sizes those asserts add up, restated: 128 entries of two pointers, the block of six 8-byte and three 4-byte fields
    p422 = (CSRC / "kernels" / "packed422.hip.h").read_text()
    per_launch = int(re.search(r"#define\s+MI_PACKED422_FRAMES_PER_LAUNCH\s+(\d+)", p422).group(1))
    assert per_launch == 128 and per_launch * 16 == 2048
    block = 6 * 8 + 3 * 4 + 4                                       # padded to a multiple of 8
    assert block == 64 and 2048 + block + 256 + 256 < 4096           # ClaheGeom and the scalars are far below 256 bytes
    # the host side: the four-channel file holds the pixel form, the three-channel file the one implementation it instantiates
    host = (CSRC / "host" / "packed422_bgra.inc.hpp").read_text()
    hcode = re.sub(r"//[^\n]*", "", host)
    for fn in ("struct Bgra422Image", "static constexpr int kPx = 4;", "using Block = Packed422Bgra;", "check_packed422_bgr<Bgra422Image>",
               "packed422_bgr_call<Bgra422Image>", "check_packed422_bgr_host<Bgra422Image>", "packed422_bgr_host<Bgra422Image>",
               "lut_apply422_bgra_frames_kernel<OFF, ORDER>, lut_apply422_bgra_kernel<OFF, ORDER>",
               "clahe_interp422_bgra_global_frames_kernel<OFF, ORDER>, clahe_interp422_bgra_global_kernel<OFF, ORDER>",
               "clahe_interp422_bgra_frames_kernel<FT, FMA, OFF, ORDER>, clahe_interp422_bgra_kernel<FT, FMA, OFF, ORDER>"):
        assert fn in hcode, fn
    assert not re.search(r"\bmi_status\s+(?!mi_)\w+\s*\(", hcode), "nothing but the form and the extern \"C\" functions"
    generic = re.sub(r"//[^\n]*", "", (CSRC / "host" / "packed422_bgr.inc.hpp").read_text())
    for fn in ("check_packed422_bgr", "packed422_bgr_batch", "BgrOut", "packed422_dev<BgrOut<F, 1>>", "packed422_dev<BgrOut<F, 0>>",
               "check_packed422_bgr_host", "stage_in", "stage_out", "packed422_image_wide", "0x7fffffffLL / F::kPx",
               "a.out_pitch < F::kPx * (size_t)a.in.width", "Span(h.out, h.out_pitch, F::kPx * w, rows)", "out_row = F::kPx * w",
               "F::count_call(c, packed422_image_wide(a.out, (long long)a.out_pitch, (long long)a.out_frame));"):
        assert fn in generic, fn
    assert len(re.findall(r"template <class F>\s*mi_status (check_packed422_bgr|packed422_bgr_dev|packed422_bgr_call|check_packed422_bgr_host|"
                          r"packed422_bgr_host)\(", generic)) == 5, "each written once, for every form"
    frames = re.sub(r"//[^\n]*", "", (CSRC / "host" / "packed422_bgra_frames.inc.hpp").read_text())
    assert "check_packed422_bgr_frames<Bgra422Image>" in frames and "packed422_bgr_frames_dev<Bgra422Image>" in frames
    assert not re.search(r"\bmi_status\s+(?!mi_)\w+\s*\(", frames), "nothing but the extern \"C\" functions"
    gframes = re.sub(r"//[^\n]*", "", (CSRC / "host" / "packed422_bgr_frames.inc.hpp").read_text())
    assert "f0 += kPacked422FramesPerLaunch" in gframes and "n_wide += packed422_image_wide(f.out, (long long)sh.out_pitch, 0);" in gframes
    assert "F::count_list(c, n_frames, n_wide);" in gframes and "Span(f.out, s.out_pitch, F::kPx * w, rows)" in gframes


def test_the_shared_stage_sequence_is_untouched():
    """packed422.inc.hpp names no writer but its own two; the three-channel kernels and host files do not know the new form."""
    for rel in ("host/packed422.inc.hpp", "host/packed422_bgr.inc.hpp", "host/packed422_bgr_frames.inc.hpp", "kernels/packed422_bgr.hip.h",
                "kernels/yuv420_bgra.hip.h"):
        assert "bgra422" not in (CSRC / rel).read_text().lower() and "packed422_bgra" not in (CSRC / rel).read_text(), rel


def test_counter_names_are_served():
    capi = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc, body = capi[: capi.index("mi_status mi_ctx_get_stat(")], capi[capi.index("mi_status mi_ctx_get_stat("):]
    for s in ref.COUNTERS:
        assert '"%s"' % s in doc, s
        assert re.search(r'!strcmp\(name, "%s"\)\) \{ \*out = c->%s; return MI_OK; \}' % (s, s), body), s
    at = [body.index('"%s"' % s) for s in ("packed422_bgr_list_frames_bytes",) + ref.COUNTERS + ("bgr_packed422_vec",)]
    assert at == sorted(at)
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    for a, b in zip(ref.COUNTERS[0::2], ref.COUNTERS[1::2]):
        assert re.search(r"unsigned long long %s\s*=\s*0\s*,\s*%s\s*=\s*0\s*;" % (a, b), ctx), (a, b)
    assert set(ref.COUNTERS).isdisjoint(ref.FOREIGN)


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (h, 2 * w), dtype=np.uint8)
    dst = np.full(4 * w * h, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    dev = (None, src.ctypes.data, 2 * w, 2 * w * h, dst.ctypes.data, 4 * w, 4 * w * h, w, h, 1, FMT_YUY2, ORDER_BGR)
    host = (None, src.ctypes.data, 2 * w, dst.ctypes.data, 4 * w, w, h, FMT_YUY2, ORDER_BGR)
    assert built_lib.mi_equalize_hist_packed422_to_bgra_batch_dev(*dev, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_bgra_batch_dev(*dev, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_equalize_hist_packed422_to_bgra(*host) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_bgra(*host, ctypes.c_double(2.0), 2, 2) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0)


# ---- the reference helper ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FMT_YUY2, FMT_UYVY])
@pytest.mark.parametrize("order", [ORDER_BGR, ORDER_RGB])
def test_expected_bytes_builder(fmt, order):
    """The three-channel reference in bytes 0..2 (already in the call's channel order), 255 in byte 3; the RGB image is the BGR image
    with channels 0 and 2 exchanged; the alternating-chroma frame tells a shared chroma row from a row's own."""
    w, h = 18, 5
    frame = ref.random_frame(w, h, fmt, 9)
    for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2))):
        img = ref.expected(frame, w, fmt, order, op, cfg)
        assert img.shape == (h, w, 4) and img.dtype == np.uint8 and img.flags.c_contiguous
        assert np.array_equal(img[..., :3], bgr_ref.expected(frame, w, fmt, order, op, cfg)) and (img[..., 3] == 255).all()
        other = ref.expected(frame, w, fmt, 1 - order, op, cfg)
        assert np.array_equal(img[..., 2::-1], other[..., :3]) and not np.array_equal(img, other)
    y, uv = ref.luma(frame, w, fmt), ref.chroma(frame, w, fmt)
    assert np.array_equal(ref.expected(frame, w, fmt, order, "eq")[..., :3], bgr_ref.decode_formula(ref.mapped_luma(y, "eq"), uv, order))
    alt = ref.alternating_chroma_frame(w, 6, fmt, 7)
    ya, ua = ref.luma(alt, w, fmt), ref.chroma(alt, w, fmt)
    mean = ((ua[0::2].astype(np.uint16) + ua[1::2] + 1) >> 1).astype(np.uint8)
    own = ref.expected(alt, w, fmt, order, "eq")[..., :3]
    shared = bgr_ref.decode(ref.mapped_luma(ya, "eq"), np.repeat(mean, 2, axis=0), order)
    assert not np.array_equal(own[0::2], shared[0::2]) and not np.array_equal(own[1::2], shared[1::2])


def test_restated_rule_agrees_with_a_hand_written_table():
    base = 0x7000_0000
    assert ref.frame_wide(base, 128, 512) and ref.frame_wide(base + 4, 132, 516) and ref.frame_wide(base + 12, 128)
    for bad in ((base + 1, 128, 512), (base + 2, 128, 512), (base, 129, 512), (base, 130, 512), (base, 128, 513), (base, 128, 514),
                (base + 3, 131, 515)):
        assert not ref.frame_wide(*bad), bad
    for name, wide in (("aligned16", True), ("aligned4", True), ("odd", False), ("tight", True)):
        for w in (2, 16, 18, 30, 40, 66):
            pitch, gap, off = ref.out_layout(w, name)
            assert pitch >= 4 * w and ref.frame_wide(base + off, pitch, pitch * 5 + gap) == wide, (name, w)
            if name == "aligned16":
                assert pitch % 16 == 0 and (pitch * 5 + gap) % 16 == 0 and off == 0
            if name == "aligned4":
                assert pitch % 16 != 0
            if name == "odd":
                assert pitch == 4 * w + 1 and off % 2 == 1
