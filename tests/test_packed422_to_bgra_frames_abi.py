"""Packed 4:2:2 in, BGRA / RGBA out on a list of device frames (mi_*_packed422_to_bgra_frames_dev) at the ABI level, without a GPU: the
header declares both entry points with the parameter lists of their three-channel siblings, the list entry is the existing 16-byte
mi_packed422_bgr_frame_dev (no struct was added), the header comment states the parts of the contract a caller cannot guess, names the
two statistics and every error case, the binding lists the symbols and has the methods with matching signatures, both libraries export
the symbols, and a null context is refused without touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import packed422_bgra_ref as ref
from mi_lumaeq import FMT_YUY2, ORDER_BGR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_packed422_bgr_frame_dev* frames, int n_frames, "
        "int width, int height, size_t in_pitch, size_t out_pitch, int format, int order")
PARAMS = {
    "mi_equalize_hist_packed422_to_bgra_frames_dev": LIST + ", void* stream",
    "mi_clahe_packed422_to_bgra_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)
SIBLING = {n: n.replace("_to_bgra", "_to_bgr") for n in NAMES}
STATS = ref.COUNTERS[2:]


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


def test_the_list_entry_is_the_existing_one():
    txt = _header()
    assert len(re.findall(r"typedef\s+struct\s+mi_packed422_bgr_frame_dev\b", txt)) == 1
    assert not re.search(r"\bmi_packed422_bgra\w*frame_dev\b", txt), "no struct was added"
    f = mi_lumaeq.Packed422BgrFrameDev
    assert ctypes.sizeof(f) == 16 and [n for n, _ in f._fields_] == ["in_", "out"]
    assert not hasattr(mi_lumaeq.capi, "Packed422BgraFrameDev")
    assert txt.index("mi_clahe_packed422_to_bgr_frames_dev") < txt.index(NAMES[0]) < txt.index(NAMES[1]) < txt.index("mi_equalize_hist_bgr_to_nv12")


def test_header_states_the_contract_and_names_each_error_case():
    m = re.search(r"/\*\s*mi_\*_packed422_to_bgra_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the packed -> BGRA list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("existing mi_packed422_bgr_frame_dev {in, out}", "read only during the call",
                   "exactly what mi_*_packed422_to_bgra_batch_dev writes for that frame alone", "A = 255",
                   "clahe_fp_contract", "clahe_float_tables", "REFLECT_101", "too wide for the LDS pair table", "one pass",
                   "no scratch Y plane", "no two-pass fallback",
                   "in_pitch is a multiple of 4", "every `in` is a multiple of 4", "The same input may appear in several entries",
                   "never written", "NO alignment rule", "odd addresses included", "out_pitch >= 4*W", "not the pitch padding",
                   "PER FRAME", "its neighbours stay wide", "slower, the same bytes out", "n_frames in total per call",
                   'list calls do not touch "packed422_bgra_wide"', "no existing counter moves",
                   "per chunk of 128 frames", "Never the fused equalizeHist kernel", "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph capture",
                   # the error cases
                   "a null ctx", "a null `frames` with n_frames > 0", "a null in / out in any entry", "an `in` that is not a multiple of 4",
                   "an odd width", "a negative size", "in_pitch < 2*W or not a multiple of 4", "out_pitch < 4*W",
                   "a `format` or an `order` other than the two", "tiles <= 0", "no in-place form",
                   "meet the rows of its own input", "not checked", "more than 65535 tiles", "a height above 65535 with tiles_x > 62",
                   "MI_ERR_UNSUPPORTED", "width, height or n_frames of 0: MI_OK, nothing written",
                   "Nothing is enqueued unless every frame passes", "a bad last entry leaves the first frames' images untouched") + STATS:
        assert needle in txt, needle


def test_statistics_are_named_where_they_are_served():
    capi = (CSRC / "host" / "capi.inc.hpp").read_text()
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    for s in STATS:
        assert '!strcmp(name, "%s")' % s in capi, s
    assert re.search(r"packed422_bgra_list_frames_wide\s*=\s*0\s*,\s*packed422_bgra_list_frames_bytes\s*=\s*0\s*;", ctx)
    # the four-channel pixel form (packed422_bgra.inc.hpp) counts; the one chunk loop (packed422_bgr_frames.inc.hpp) calls it once
    form = (CSRC / "host" / "packed422_bgra.inc.hpp").read_text()
    assert "c->packed422_bgra_list_frames_wide += n_wide;" in form
    assert "c->packed422_bgra_list_frames_bytes += (unsigned long long)n_frames - n_wide;" in form
    loop = (CSRC / "host" / "packed422_bgr_frames.inc.hpp").read_text()
    assert loop.count("F::count_list(c, n_frames, n_wide);") == 1
    frames = (CSRC / "host" / "packed422_bgra_frames.inc.hpp").read_text()
    assert "packed422_bgr_frames_dev<Bgra422Image>" in frames
    for txt in (frames, form):
        assert "packed422_bgr_list_frames" not in re.sub(r"//[^\n]*", "", txt), "the three-channel form's counters are not this form's"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_packed422_to_bgra_frames", "clahe_packed422_to_bgra_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params) == list(inspect.signature(getattr(mi_lumaeq.Context, m.replace("_to_bgra", "_to_bgr"))).parameters), m
        assert list(params)[1:7] == ["inputs", "outs", "width", "height", "fmt", "order"], m
        assert params["fmt"].default == FMT_YUY2 and params["order"].default == ORDER_BGR
        for kw in ("in_pitch", "out_pitch", "stream"):
            assert kw in params and params[kw].default in (None, 0), (m, kw)
    p = inspect.signature(mi_lumaeq.Context.clahe_packed422_to_bgra_frames).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_binding_defaults_to_a_row_of_four_bytes_a_pixel():
    """Raw addresses and no pitches: 2 * width in, 4 * width out (the three-channel helper keeps its 3 * width)."""
    from mi_lumaeq.capi import _packed422_bgr_list
    arr, n, ip, op = _packed422_bgr_list([64, 128], [4096, 8192], 10, None, None, "t", px=4)
    assert (n, ip, op) == (2, 20, 40) and (arr[1].in_, arr[1].out) == (128, 8192)
    assert _packed422_bgr_list([64], [4096], 10, None, None, "t")[3] == 30
    with pytest.raises(mi_lumaeq.MiError):
        _packed422_bgr_list([64, 128], [4096], 10, None, None, "t", px=4)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s
            assert getattr(L, s).argtypes == getattr(L, SIBLING[s]).argtypes, s


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    src = np.random.default_rng(3).integers(0, 256, (h, 2 * w), dtype=np.uint8)
    dst = np.full(4 * w * h, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    entry = mi_lumaeq.Packed422BgrFrameDev(src.ctypes.data, dst.ctypes.data)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, 2 * w, 4 * w, FMT_YUY2, ORDER_BGR)
    assert built_lib.mi_equalize_hist_packed422_to_bgra_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_packed422_to_bgra_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
