"""Interleaved BGR / RGB in, packed 4:2:2 (YUY2 / UYVY) out on a list of device frames (mi_*_bgr_to_packed422_frames_dev) at the ABI
level, without a GPU: the header declares both entry points with their parameter lists and the 16-byte list entry behind the batch
form, no struct or enum grew (minor version 3, MI_K_COUNT 10, no new MI_FMT_*), a header comment of its own states the parts of the
contract a caller cannot guess and names the two statistics, the batch form's comment no longer denies the list form, the binding lists
the symbols and has the methods with matching signatures and defaults, both libraries export the symbols, the new source is included
behind the batch form's, the kernel file has the list entry and the bound on its arguments, and a null context is refused without
touching the caller's buffers."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
from mi_lumaeq import FMT_YUY2, ORDER_BGR, UV_COPY

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_bgr_packed422_frame_dev* frames, int n_frames, "
        "int width, int height, size_t in_pitch, size_t out_pitch, int order, int format, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_bgr_to_packed422_frames_dev": LIST + ", void* stream",
    "mi_clahe_bgr_to_packed422_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)
STATS = ("bgr_packed422_list_frames_vec", "bgr_packed422_list_frames_bytes")


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _norm(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_entry_point(name):
    m = re.search(r"\bmi_status\s+" + name + r"\s*\((.*?)\)\s*;", _header(), re.S)
    assert m, f"{name} is not declared in mi_lumaeq.h"
    assert _norm(m.group(1)) == _norm(PARAMS[name])


def test_declared_behind_the_batch_form():
    txt = _header()
    for name in NAMES:
        assert txt.index("mi_clahe_bgr_to_packed422(") < txt.index(name + "(") < txt.index("mi_host_register"), name


def test_header_declares_the_list_entry():
    m = re.search(r"typedef\s+struct\s+mi_bgr_packed422_frame_dev\s*\{(.*?)\}\s*mi_bgr_packed422_frame_dev\s*;", _header(), re.S)
    assert m, "mi_bgr_packed422_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* in; void* out;"
    f = mi_lumaeq.BgrPacked422FrameDev
    assert [n for n, _ in f._fields_] == ["in_", "out"]
    assert ctypes.sizeof(ctypes.c_void_p) == 8 and ctypes.sizeof(f) == 16
    assert mi_lumaeq.BgrPacked422FrameDev is mi_lumaeq.capi.BgrPacked422FrameDev and "BgrPacked422FrameDev" in mi_lumaeq.__all__


def test_no_struct_or_enum_grew():
    """The list entry is the one new type; nothing that exists grew."""
    txt = _header()
    assert txt.count("typedef struct mi_bgr_packed422_frame_dev") == 1
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert re.findall(r"\bMI_FMT_(\w+)\s*=\s*(\d+)", txt) == [("NV12", "0"), ("P010", "1"), ("YUY2", "2"), ("UYVY", "3")], "no new MI_FMT_* value"
    for name, v in (("MI_ORDER_BGR", 0), ("MI_ORDER_RGB", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name


def test_header_states_the_contract():
    """A comment block of its own: the bytes are the batch form's, the list is read during the call only, one shape a call, the input
    and output rules, the per-frame walk and the two statistics that count it, the chunking, the overlap rule, nothing enqueued unless
    every frame passes, the empty call, the stream rules."""
    m = re.search(r"/\*\s*mi_\*_bgr_to_packed422_frames_dev.*?\*/", HEADER.read_text(), re.S)
    assert m, "no header comment for the BGR -> packed 4:2:2 list form"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("read only during the call", "exactly what mi_*_bgr_to_packed422_batch_dev writes", "exactly Y0 U Y1 V",
                   "exactly U Y0 V Y1", "clahe_fp_contract", "share width, height, the pair of pitches", "order, format and uv_mode",
                   "no per-frame pitches", "in_pitch >= 3*W", "at any address", "never written", "out_pitch >= 2*W",
                   "every `out` and out_pitch are multiples of 4", "Only the 2*W bytes of each output row are written",
                   "W % 16 == 0 and in_pitch and out_pitch are multiples of 16", "its own `in` and `out` are both multiples of 16",
                   "six byte loads and one aligned dword store", "slower, the same bytes out", "per chunk of 128 frames",
                   "not the batch form's 256", "MI_K_COLOR", "MI_K_EQ_LUT", "MI_K_LUT_APPLY", "no MI_K_HIST", "IN PLACE",
                   "mi_clahe_packed422_frames_dev", "two_kernel_max_frames", "by n_frames in total",
                   'does not touch "bgr_packed422_vec" / "bgr_packed422_bytes"', "no in-place form", "meet the rows of its own output frame",
                   "The same image may appear in several entries", "not checked", "a null `frames` with n_frames > 0",
                   "MI_ERR_UNSUPPORTED", "n_frames == 0 with a null list is MI_OK", "Nothing is enqueued unless every frame passes",
                   "a bad last entry leaves the earlier frames' outputs untouched", "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph") + STATS:
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_bgr_to_packed422\*.*?\*/", HEADER.read_text(), re.S)
    assert batch, "the batch form's comment is gone"
    btxt = _norm(batch.group(0).replace("\n *", " "))
    assert "Not built: the frame-list form" not in btxt, "the batch form's comment still denies the list form"
    assert "mi_*_bgr_to_packed422_frames_dev" in btxt and "256 frames" in btxt
    # the chunk the comment names is the capacity of stage 2's table
    k = (CSRC / "kernels" / "packed422.hip.h").read_text()
    assert int(re.search(r"#define\s+MI_PACKED422_FRAMES_PER_LAUNCH\s+(\d+)", k).group(1)) == 128


def test_statistics_are_named_where_they_are_served():
    capi = (CSRC / "host" / "capi.inc.hpp").read_text()
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    doc = capi[: capi.index("mi_status mi_ctx_get_stat(")]
    assert doc.index('"bgr_packed422_vec" / "bgr_packed422_bytes"') < doc.index('"bgr_packed422_list_frames_vec" / "bgr_packed422_list_frames_bytes"')
    for s in STATS:
        assert '!strcmp(name, "%s")) { *out = c->%s;' % (s, s) in capi, s
    assert re.search(r"bgr_packed422_list_frames_vec\s*=\s*0\s*,\s*bgr_packed422_list_frames_bytes\s*=\s*0\s*;", ctx)
    assert ctx.index("bgr_packed422_vec = 0") < ctx.index("bgr_packed422_list_frames_vec = 0")


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_bgr_to_packed422_frames", "clahe_bgr_to_packed422_frames"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[:8] == ["self", "ins", "outs", "width", "height", "order", "fmt", "uv_mode"], m
        assert (params["order"].default, params["fmt"].default, params["uv_mode"].default) == (ORDER_BGR, FMT_YUY2, UV_COPY)
        assert params["in_pitch"].default is None and params["out_pitch"].default is None and params["stream"].default == 0
    p = inspect.signature(mi_lumaeq.Context.clahe_bgr_to_packed422_frames).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)
    assert callable(mi_lumaeq.capi._bgr_packed422_list)


def test_binding_derives_the_pitches():
    """Raw addresses: the tight pitches; a given pitch wins; unequal list lengths are refused."""
    arr, n, ip, op = mi_lumaeq.capi._bgr_packed422_list([4096, 8192], [12288, 16384], 10, None, None, "t")
    assert (n, ip, op) == (2, 30, 20) and (arr[1].in_, arr[1].out) == (8192, 16384)
    assert mi_lumaeq.capi._bgr_packed422_list([4096], [8192], 10, 48, 32, "t")[2:] == (48, 32)
    assert mi_lumaeq.capi._bgr_packed422_list([], [], 10, None, None, "t")[1] == 0
    with pytest.raises(mi_lumaeq.MiError):
        mi_lumaeq.capi._bgr_packed422_list([4096], [], 10, None, None, "t")


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


def test_new_sources_are_registered():
    assert (CSRC / "host" / "bgr_packed422_frames.inc.hpp").exists()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    assert 0 <= tu.index('#include "host/bgr_packed422.inc.hpp"') < tu.index('#include "host/bgr_packed422_frames.inc.hpp"')
    kern = (CSRC / "kernels" / "bgr_packed422.hip.h").read_text()
    assert re.search(r"template\s*<int ORDER, int OFF, int UVMODE, bool HIST>\s*__global__[^;{]*\bbgr_to_packed422_hist_frames_kernel\s*\("
                     r"BgrPacked422Job j, Packed422List l, uint32_t\* __restrict__ partial\)", kern)
    # the batch entry keeps its head and its parameter list (its text and ISA are the parent's)
    assert re.search(r"template\s*<int ORDER, int OFF, int UVMODE, bool HIST>\s*__global__[^;{]*\bbgr_to_packed422_hist_kernel\s*\("
                     r"BgrPacked422Job j, uint32_t\* __restrict__ partial\)", kern)
    # one rule for the walk of a frame, shared by the kernel and the host's count
    assert re.search(r"__host__ __device__[^;{]*\bbgr_packed422_frame_vec\s*\(", kern)
    assert len(re.findall(r"\bbgr_packed422_frame_vec\s*\(", kern)) == 2
    assert re.search(r"static_assert\(sizeof\(BgrPacked422Job\) \+ sizeof\(Packed422List\) \+ sizeof\(uint32_t\*\) \+ 256 <= 4096", kern)
    assert "asm" not in re.sub(r"//[^\n]*", "", kern), "no inline assembly"
    host = (CSRC / "host" / "bgr_packed422_frames.inc.hpp").read_text()
    for fn in ("check_bgr_packed422", "launch_bgr_to_packed422", "kPacked422FramesPerLaunch", "Packed422List", "PackedOut", "clahe422_dev",
               "launch_pair", "equalize_lut_kernel", "MI_K_COLOR", "Span"):
        assert re.search(r"\b" + fn + r"\b", host), fn
    # the walk rule and the counters are the pixel form's (bgr_packed422.inc.hpp); the one chunk loop asks the form
    form = re.sub(r"//[^\n]*", "", (CSRC / "host" / "bgr_packed422.inc.hpp").read_text())
    for fn in ("bgr_packed422_frame_vec", "bgr_packed422_list_frames_vec", "bgr_packed422_list_frames_bytes"):
        assert re.search(r"\b" + fn + r"\b", form), fn
    assert "n_vec += F::frame_vec(shape_vec, io.f[k].in, io.f[k].out);" in host and host.count("F::count_list(c, n_frames, n_vec);") == 1
    assert host.count("bgr_packed422_frames_entry<BgrTo422>(") == 2
    for other in ("packed422_bgra", "bgra422", "bgra_packed422", "bgra_to_packed422"):
        assert other not in host.lower(), "the three-channel file does not know the four-channel form"
    code = re.sub(r"//[^\n]*", "", host)
    assert "MI_K_HIST" not in code and "hist_lut_kernel" not in code, "stage 1 counts: the form has no MI_K_HIST launch"
    assert "The frame-list form (mi_*_bgr_to_packed422_frames_dev) is not built" not in (CSRC / "host" / "bgr_packed422.inc.hpp").read_text()


def test_null_context_is_bad_arg_and_touches_nothing(built_lib):
    w, h = 8, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, w * h * 3, dtype=np.uint8)
    dst = np.full(w * h * 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    entry = mi_lumaeq.BgrPacked422FrameDev(src.ctypes.data, dst.ctypes.data)
    e0 = bytes(entry)
    a = (None, ctypes.byref(entry), 1, w, h, 3 * w, 2 * w, ORDER_BGR, FMT_YUY2, UV_COPY)
    assert built_lib.mi_equalize_hist_bgr_to_packed422_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_bgr_to_packed422_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0
