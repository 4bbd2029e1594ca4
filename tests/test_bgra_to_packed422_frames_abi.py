"""Four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 (YUY2 / UYVY) out on a list of device frames
(mi_*_bgra_to_packed422_frames_dev) at the ABI level, without a GPU: the header declares both entry points with the three-channel list
form's parameter lists on the existing mi_bgr_packed422_frame_dev entry, no struct or enum grew, a header comment of its own states the
contract and names the two statistics, the binding lists the symbols and has the methods with the sibling's argument order and derives
the four-byte pitches, both libraries export the symbols, the new source is included behind the batch form's, the kernel file has the
list entry, the by-value table and the bound on its arguments, and a null context is refused without touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import FMT_YUY2, ORDER_BGR, UV_COPY
from bgra_packed422_ref import LIST_COUNTERS, frame_vec

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_bgr_packed422_frame_dev* frames, int n_frames, "
        "int width, int height, size_t in_pitch, size_t out_pitch, int order, int format, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_bgra_to_packed422_frames_dev": LIST + ", void* stream",
    "mi_clahe_bgra_to_packed422_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)


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
    assert _params(name) == _params(name.replace("bgra_to_packed422", "bgr_to_packed422")), "the three-channel list form's signature"


def test_declared_behind_the_batch_form_and_nothing_grew():
    txt = _header()
    for name in NAMES:
        assert txt.index("mi_clahe_bgra_to_packed422(") < txt.index(name + "(") < txt.index("mi_host_register"), name
    assert txt.count("typedef struct mi_bgr_packed422_frame_dev") == 1, "the list entry is the existing one"
    assert "bgra_packed422_frame_dev" not in txt, "no new list entry type"
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert ctypes.sizeof(mi_lumaeq.BgrPacked422FrameDev) == 16


def test_header_states_the_contract():
    m = re.search(r"/\*\s*mi_\*_bgra_to_packed422_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGRA -> packed 4:2:2 list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("read only during the call", "existing mi_bgr_packed422_frame_dev", "No new struct, enum or version",
                   "exactly what mi_*_bgra_to_packed422_batch_dev writes", "share width, height, the pair of pitches",
                   "order, format and uv_mode", "no per-frame pitches", "in_pitch >= 4*W", "at any address", "X takes no part",
                   "never written", "out_pitch >= 2*W", "every `out` and out_pitch are multiples of 4",
                   "Only the 2*W bytes of each output row are written", "W % 16 == 0 and in_pitch and out_pitch are multiples of 16",
                   "its own `in` and `out` are both multiples of 16", "four 16-byte loads, two 16-byte stores",
                   "one aligned dword store", "slower, the same bytes out", "the kernel decides by and the host counts by",
                   "per chunk of 128 frames", "not the batch form's 256", "MI_K_COLOR", "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST",
                   "IN PLACE", "mi_clahe_packed422_frames_dev", "two_kernel_max_frames", "by n_frames in total",
                   'does not touch "bgra_packed422_vec" / "bgra_packed422_bytes"', "nor any bgr_packed422* counter", "no in-place form",
                   "meet the rows of its own output frame", "The same image may appear in several entries", "not checked",
                   "a null `frames` with n_frames > 0", "MI_ERR_UNSUPPORTED", "n_frames == 0 with a null list is MI_OK",
                   "Nothing is enqueued unless every frame passes", "a bad last entry leaves the earlier frames' outputs untouched",
                   "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph") + LIST_COUNTERS:
        assert needle in txt, needle
    # the chunk the comment names is the capacity of stage 2's table
    k = (CSRC / "kernels" / "packed422.hip.h").read_text()
    assert int(re.search(r"#define\s+MI_PACKED422_FRAMES_PER_LAUNCH\s+(\d+)", k).group(1)) == 128


def test_binding_has_the_siblings_argument_order():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgra_to_packed422_frames", "clahe_bgra_to_packed422_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        sib = getattr(mi_lumaeq.Context, m.replace("bgra_to_packed422", "bgr_to_packed422"))
        p, q = inspect.signature(f).parameters, inspect.signature(sib).parameters
        assert list(p) == list(q), m
        assert [v.default for v in p.values()] == [v.default for v in q.values()], m
        assert list(p)[:8] == ["self", "ins", "outs", "width", "height", "order", "fmt", "uv_mode"], m


def test_binding_derives_the_four_byte_pitches():
    """Raw addresses: the tight pitches of four-byte pixels; a given pitch wins; unequal list lengths are refused; the three-channel
    default of the shared helper is unchanged."""
    arr, n, ip, op = mi_lumaeq.capi._bgr_packed422_list([4096, 8192], [12288, 16384], 10, None, None, "t", ch=4)
    assert (n, ip, op) == (2, 40, 20) and (arr[1].in_, arr[1].out) == (8192, 16384)
    assert mi_lumaeq.capi._bgr_packed422_list([4096], [8192], 10, 48, 32, "t", ch=4)[2:] == (48, 32)
    assert mi_lumaeq.capi._bgr_packed422_list([4096], [8192], 10, None, None, "t")[2:] == (30, 20)
    with pytest.raises(mi_lumaeq.MiError):
        mi_lumaeq.capi._bgr_packed422_list([4096], [], 10, None, None, "t", ch=4)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s
            assert getattr(L, s).argtypes == getattr(L, s.replace("bgra_to_packed422", "bgr_to_packed422")).argtypes, s


def test_new_sources_are_registered():
    assert (CSRC / "host" / "bgra_packed422_frames.inc.hpp").exists()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/bgra_packed422.inc.hpp"') < tu.index('#include "host/bgra_packed422_frames.inc.hpp"')
    assert tu.index('#include "host/bgr_packed422_frames.inc.hpp"') < tu.index('#include "host/bgra_packed422_frames.inc.hpp"')
    kern = (CSRC / "kernels" / "bgra_packed422.hip.h").read_text()
    assert re.search(r"template\s*<int ORDER, int OFF, int UVMODE, bool HIST>\s*__global__[^;{]*\bbgra_to_packed422_hist_frames_kernel\s*\("
                     r"BgraPacked422Job j, Packed422List l, uint32_t\* __restrict__ partial\)", kern), "the table travels by value"
    assert re.search(r"__host__ __device__[^;{]*\bbgra_packed422_frame_vec\s*\(", kern)
    assert re.search(r"static_assert\(sizeof\(BgraPacked422Job\) \+ sizeof\(Packed422List\) \+ sizeof\(uint32_t\*\) \+ 256 <= 4096", kern)
    # this file: the extern "C" functions on the four-channel form; the form: bgra_packed422.inc.hpp; the one check, chunk loop and
    # entry, templates on the form: bgr_packed422_frames.inc.hpp
    host = (CSRC / "host" / "bgra_packed422_frames.inc.hpp").read_text()
    code = re.sub(r"//[^\n]*", "", host)
    assert code.count("bgr_packed422_frames_entry<BgraTo422>(") == 2 and "mi_bgr_packed422_frame_dev" in code
    assert not re.search(r"\bmi_status\s+(?!mi_)\w+\s*\(", code), "nothing but the extern \"C\" functions"
    form = re.sub(r"//[^\n]*", "", (CSRC / "host" / "bgra_packed422.inc.hpp").read_text())
    for fn in ("bgra_packed422_frame_vec", "bgra_packed422_list_frames_vec", "bgra_packed422_list_frames_bytes"):
        assert re.search(r"\b" + fn + r"\b", form), fn
    assert re.search(r"count_list\(mi_ctx\* c, int n_frames, unsigned long long n_vec\)\s*\{\s*c->bgra_packed422_list_frames_vec \+= n_vec;\s*"
                     r"c->bgra_packed422_list_frames_bytes \+= \(unsigned long long\)n_frames - n_vec;\s*\}", form)
    generic_text = (CSRC / "host" / "bgr_packed422_frames.inc.hpp").read_text()
    for fn in ("check_bgr_packed422", "launch_bgr_to_packed422", "kPacked422FramesPerLaunch", "Packed422List", "PackedOut", "clahe422_dev",
               "launch_pair", "equalize_lut_kernel", "MI_K_COLOR", "Span", "meets", "mi_bgr_packed422_frame_dev"):
        assert re.search(r"\b" + fn + r"\b", generic_text), fn
    generic = re.sub(r"//[^\n]*", "", generic_text)
    assert "n_vec += F::frame_vec(shape_vec, io.f[k].in, io.f[k].out);" in generic and generic.count("F::count_list(c, n_frames, n_vec);") == 1
    for txt in (code, generic):
        assert "MI_K_HIST" not in txt and "hist_lut_kernel" not in txt, "stage 1 counts: the form has no MI_K_HIST launch"
        assert not re.search(r"\bbgra_packed422_(vec|bytes)\b", txt), "list calls do not touch the per-call counters"
        assert "count_call" not in txt, "list calls do not touch the per-call counters"
    for txt in (code, form):
        assert not re.search(r"\bbgr_packed422_(vec|bytes|list_frames_vec|list_frames_bytes)\b", txt), "no three-channel counter is moved"
    assert 'kPx = 4;' in form
    assert re.search(r"Span\(f\.in, s\.in_pitch, F::kPx \* w, rows\)\.meets\(Span\(f\.out, s\.out_pitch, 2 \* w, rows\)\)", generic)


def test_the_restated_rule():
    """bgra_packed422_ref.frame_vec, the rule the GPU tests predict the counters by: every one of the five terms at a time."""
    assert frame_vec(32, 128, 64, 4096, 8192)
    for kw in (dict(w=24), dict(ip=136), dict(op=72), dict(i=4096 + 8), dict(o=8192 + 4)):
        a = dict(w=32, ip=128, op=64, i=4096, o=8192)
        a.update(kw)
        assert not frame_vec(a["w"], a["ip"], a["op"], a["i"], a["o"]), kw


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 4, dtype=np.uint8)
    dst = np.full(w * h * 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    entry = mi_lumaeq.BgrPacked422FrameDev(src.ctypes.data, dst.ctypes.data)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, 4 * w, 2 * w, ORDER_BGR, FMT_YUY2, UV_COPY)
    assert built_lib.mi_equalize_hist_bgra_to_packed422_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgra_to_packed422_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
