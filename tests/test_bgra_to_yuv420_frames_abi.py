"""Four-channel BGRA / RGBA (CV_8UC4) in, planar 4:2:0 (I420 / YV12) or NV12 out on a list of pitched device frames
(mi_*_bgra_to_yuv420_frames_dev) at the ABI level, without a GPU: the header declares the two entry points with the parameter lists of
their three-channel siblings, on the existing list entry mi_bgr_yuv420_frame_dev, behind the mi_*_bgra_to_yuv420 host forms and before
mi_host_register; no struct or enum grew (minor version 3, MI_K_COUNT 10); the comment block of its own states the parts of the
contract a caller cannot guess; the binding lists the symbols and has the methods with their keyword defaults; both libraries export
the symbols; the host file is part of the translation unit behind the batch form's; the two statistics stand behind their siblings;
and a null context is refused without touching the caller's buffers."""
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

LIST = ("mi_ctx* ctx, const mi_bgr_yuv420_frame_dev* frames, int n_frames, int width, int height, "
        "size_t in_pitch, size_t y_pitch, size_t c_pitch, int chroma, int order, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_bgra_to_yuv420_frames_dev": LIST + ", void* stream",
    "mi_clahe_bgra_to_yuv420_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)


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
    assert _decl(name) == _decl(name.replace("_bgra_", "_bgr_")), "the parameter list of the three-channel sibling"


def test_declared_behind_the_host_forms_and_nothing_grew():
    txt = _header()
    at = [txt.index(s) for s in ("mi_clahe_yuv420_to_packed422_frames_dev", "mi_clahe_bgra_to_yuv420(",
                                 "mi_equalize_hist_bgra_to_yuv420_frames_dev", "mi_clahe_bgra_to_yuv420_frames_dev", "mi_host_register")]
    assert at == sorted(at), "the list form is declared after the mi_*_bgra_to_yuv420 host forms and before mi_host_register"
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert len(re.findall(r"typedef\s+struct\s+mi_bgr_yuv420_frame_dev\b", txt)) == 1
    assert not re.search(r"typedef\s+struct\s+mi_bgra_\w+", txt), "the list entry is the existing mi_bgr_yuv420_frame_dev {in, y, c0, c1}"
    assert ctypes.sizeof(mi_lumaeq.BgrYuv420FrameDev) == 32 and ctypes.sizeof(mi_lumaeq.Yuv420Planes) == 56


def test_header_states_the_contract():
    """A comment block of its own, behind the host forms' declarations; the batch form's block does not speak of the list form."""
    raw = HEADER.read_text()
    m = re.search(r"/\*\s*mi_\*_bgra_to_yuv420_frames_dev.*?\*/", raw, re.S)
    assert m, "no header comment for the BGRA -> 4:2:0 list form"
    assert m.start() > raw.index("mi_status mi_clahe_bgra_to_yuv420("), "the block stands behind the host forms' declarations"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in (
            # bytes
            "CV_8UC4", "mi_bgr_yuv420_frame_dev {in, y, c0, c1}", "read only during the call", "each has its own addresses",
            "There are no per-frame pitches", "H rows of 4*W bytes at in_pitch >= 4*W", "B, G, R, X per pixel", "X takes no part",
            "byte for byte what mi_*_bgra_to_yuv420_batch_dev writes for that frame alone at the same pitches",
            "COLOR_BGRA2YUV_I420", "only the W bytes of each Y and interleaved UV row and the W/2 bytes of each planar U and V row are written",
            "not the pitch padding", "not the gaps", "The images are never written", "c0 is always U and c1 always V",
            "a YV12 caller exchanges the two", "clahe_fp_contract", "REFLECT_101",
            # interleaved lists stay here
            "c1 is ignored and may be NULL", "not handed to another form",
            "one pair of entry points and one set of counters serves both layouts",
            # alignment
            "none is required of any address or pitch", "The shape decides what is allowed", "W % 16 == 0",
            "in_pitch and y_pitch are multiples of 16 and c_pitch is a multiple of 16 (interleaved) or 8 (planar)",
            "Each frame then decides by its own addresses",
            "its in and y are multiples of 16 and its c0 is a multiple of 16 (interleaved) or its c0 and c1 are multiples of 8 (planar)",
            "2 x 2 pixel blocks with byte accesses", "its neighbours stay vectorised",
            # stages
            "per chunk of 64 frames", "not the batch form's 256", "MI_K_COLOR", "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST",
            "never the fused equalizeHist kernel nor the single-launch histogram + LUT kernel", "mi_clahe_nv12_frames_dev",
            "IN PLACE", "same profiling slots", "holds the unequalized luma",
            # counters
            '"bgra_yuv420_list_frames_vec"', '"bgra_yuv420_list_frames_bytes"', "count the FRAMES", "n_frames in total per call",
            '"bgra_yuv420_vec" / "bgra_yuv420_bytes" are not touched by list calls',
            "A call that returns an error or has nothing to do moves none",
            # overlap
            "no in-place form", "(4*W bytes each)", "meet the rows of a plane of its own frame",
            "its Y plane meet the rows of a chroma plane of its own", "compared as address ranges", "on a PLANAR list when c0 == c1",
            "c1 = c0 + W/2, c_pitch = W", "may appear in several entries", "not checked",
            # errors
            "a null ctx", "a null `frames` with n_frames > 0", "a null in, y or c0 in any entry", "a null c1 in any entry on a PLANAR list",
            "a `chroma` other than the two", "an `order` other than the two", "a bad uv_mode", "a negative size",
            "refused even when another size is 0", "in_pitch < 4*W", "y_pitch < W", "W interleaved, W/2 planar", "tiles <= 0",
            "MI_ERR_UNSUPPORTED", "MI_OK, nothing written", "n_frames == 0 with a null list is MI_OK",
            "Nothing is enqueued unless every frame passes", "a bad last entry leaves the first frames' outputs untouched",
            # streams and capture
            "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph", "holds the addresses it was captured with"):
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_bgra_to_yuv420\*.*?\*/", raw, re.S)
    assert batch and "frames_dev" not in batch.group(0) and "256 frames" in batch.group(0), "the batch form's block is about the batch form"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgra_to_yuv420_frames_dev", "clahe_bgra_to_yuv420_frames_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        p, q = inspect.signature(f).parameters, inspect.signature(getattr(mi_lumaeq.Context, m.replace("_bgra_", "_bgr_"))).parameters
        assert list(p) == list(q) and [p[k].default for k in p] == [q[k].default for k in q], (m, "the sibling's signature and defaults")
        assert list(p)[:10] == ["self", "frames", "width", "height", "in_pitch", "y_pitch", "c_pitch", "chroma", "order", "uv_mode"], m
        assert all(p[k].default is inspect.Parameter.empty for k in list(p)[1:8]), m
        assert p["order"].default == mi_lumaeq.ORDER_BGR and p["uv_mode"].default == mi_lumaeq.UV_COPY and p["stream"].default == 0
    assert list(inspect.signature(mi_lumaeq.Context.equalize_hist_bgra_to_yuv420_frames_dev).parameters)[10:] == ["stream"]
    p = inspect.signature(mi_lumaeq.Context.clahe_bgra_to_yuv420_frames_dev).parameters
    assert list(p)[10:] == ["clip_limit", "tiles_x", "tiles_y", "stream"]
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_host_file_is_included_behind_the_batch_form():
    assert (CSRC / "host" / "bgra_yuv420_frames.inc.hpp").exists()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/bgra_yuv420.inc.hpp"') < tu.index('#include "host/bgra_yuv420_frames.inc.hpp"') \
        < tu.index('#include "host/pipe.inc.hpp"')
    host = (CSRC / "host" / "bgra_yuv420_frames.inc.hpp").read_text()
    for fn in ("check_bgra_yuv420", "launch_bgra_to_yuv420", "launch_apply", "clahe_dev", "bgra_yuv420_frame_vec", "kFramesPerLaunch", "Span",
               "FrameList", "BgraYuv420List", "mi_bgr_yuv420_frame_dev"):
        assert re.search(r"\b" + fn + r"\b", host), fn
    code = re.sub(r"//[^\n]*", "", host)
    assert "kBgraYuv420FramesPerLaunch" not in code and "kBgrNv12FramesPerLaunch" not in code, "the list form's chunk is kFramesPerLaunch"
    for other in ("check_bgr_nv12_frames", "bgr_nv12_frames_dev", "bgr_yuv420_frames_dev"):
        assert other not in code, (other, "an interleaved list is not handed to another form")
    assert re.search(r"Span\s+si\(f\.in,\s*s\.in_pitch,\s*4 \* w,\s*rows\)", code), "the image's row range is 4*W bytes"
    batch = (CSRC / "host" / "bgra_yuv420.inc.hpp").read_text()
    assert re.search(r"launch_bgra_to_yuv420\([^)]*const BgraYuv420List\*\s*fl\s*=\s*nullptr\)", batch, re.S)


def test_stat_names_stand_behind_their_siblings():
    txt = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc = txt[: txt.index("mi_status mi_ctx_get_stat(")]
    assert doc.index('"bgra_yuv420_vec" / "bgra_yuv420_bytes"') < doc.index('"bgra_yuv420_list_frames_vec" / "bgra_yuv420_list_frames_bytes"')
    body = txt[txt.index("mi_status mi_ctx_get_stat("):]
    assert body.index('"bgra_yuv420_bytes"') < body.index('"bgra_yuv420_list_frames_vec"') < body.index('"bgra_yuv420_list_frames_bytes"') \
        < body.index('"unknown stat"')
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    assert re.search(r"bgra_yuv420_list_frames_vec\s*=\s*0\s*,\s*bgra_yuv420_list_frames_bytes\s*=\s*0\s*;", ctx)
    assert ctx.index("bgra_yuv420_vec = 0, bgra_yuv420_bytes = 0") < ctx.index("bgra_yuv420_list_frames_vec = 0")


@pytest.mark.parametrize("chroma", [mi_lumaeq.CHROMA_PLANAR, mi_lumaeq.CHROMA_INTERLEAVED])
def test_null_context_is_bad_arg_and_touches_nothing(built_lib, chroma):
    w, h = 8, 4
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, w * h * 4, dtype=np.uint8)
    dst = np.full(w * h * 3 // 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    y = dst.ctypes.data
    entry = mi_lumaeq.BgrYuv420FrameDev(src.ctypes.data, y, y + w * h, y + w * h + w * h // 4)
    e0 = bytes(entry)
    cp = w // 2 if chroma == mi_lumaeq.CHROMA_PLANAR else w
    a = (None, ctypes.byref(entry), 1, w, h, 4 * w, w, cp, chroma, 0, 1)
    assert built_lib.mi_equalize_hist_bgra_to_yuv420_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgra_to_yuv420_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
