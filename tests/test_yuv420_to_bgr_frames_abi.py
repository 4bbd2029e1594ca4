"""Planar 4:2:0 (I420 / YV12) or NV12 in, interleaved BGR / RGB out on a list of pitched device frames
(mi_*_yuv420_to_bgr_frames_dev) at the ABI level, without a GPU: the header declares the two entry points with their parameter lists and
the list entry struct, no struct or enum grew (minor version 3, MI_K_COUNT 10, no new MI_FMT_* or MI_ORDER_*), the new comment block
states the parts of the contract a caller cannot guess while the batch form's block is left alone, the binding lists the symbols and has
the methods with their keyword defaults, both libraries export the symbols, a null context is refused without touching the caller's
buffers, and the seeded cases of the GPU sweep hold enough of every class (the documented rule restated in
tests/yuv420_bgr_frames_cases.py)."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import yuv420_bgr_frames_cases as cases

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_yuv420_bgr_frame_dev* frames, int n_frames, "
        "int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int order")
PARAMS = {
    "mi_equalize_hist_yuv420_to_bgr_frames_dev": LIST + ", void* stream",
    "mi_clahe_yuv420_to_bgr_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
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


def test_header_declares_the_list_entry():
    m = re.search(r"typedef\s+struct\s+mi_yuv420_bgr_frame_dev\s*\{(.*?)\}\s*mi_yuv420_bgr_frame_dev\s*;", _header(), re.S)
    assert m, "mi_yuv420_bgr_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* y; const void* c0; const void* c1; void* out;"
    f = mi_lumaeq.Yuv420BgrFrameDev
    assert [n for n, _ in f._fields_] == ["y", "c0", "c1", "out"]
    assert ctypes.sizeof(f) == 32 == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert mi_lumaeq.Yuv420BgrFrameDev is mi_lumaeq.capi.Yuv420BgrFrameDev and "Yuv420BgrFrameDev" in mi_lumaeq.__all__


def test_no_struct_or_enum_grew():
    txt = _header()
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    for name, v in (("MI_FMT_NV12", 0), ("MI_FMT_P010", 1), ("MI_FMT_YUY2", 2), ("MI_FMT_UYVY", 3), ("MI_ORDER_BGR", 0), ("MI_ORDER_RGB", 1),
                    ("MI_CHROMA_INTERLEAVED", 0), ("MI_CHROMA_PLANAR", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), txt), name
    assert sorted(set(re.findall(r"\bMI_FMT_\w+", txt))) == ["MI_FMT_NV12", "MI_FMT_P010", "MI_FMT_UYVY", "MI_FMT_YUY2"], "no new format"
    assert sorted(set(re.findall(r"\bMI_ORDER_\w+", txt))) == ["MI_ORDER_BGR", "MI_ORDER_RGB"], "no new order"
    assert sorted(set(re.findall(r"\bMI_CHROMA_\w+", txt))) == ["MI_CHROMA_INTERLEAVED", "MI_CHROMA_PLANAR"], "no new chroma layout"
    m = re.search(r"typedef\s+struct\s+mi_yuv420_planes\s*\{(.*?)\}\s*mi_yuv420_planes\s*;", txt, re.S)
    assert m and ctypes.sizeof(mi_lumaeq.Yuv420Planes) == 56, "mi_yuv420_planes did not grow"


def test_header_states_the_contract():
    """A comment block of its own, behind the batch form's declarations; the batch form's block is left as it was."""
    raw = HEADER.read_text()
    m = re.search(r"/\*\s*mi_\*_yuv420_to_bgr_frames_dev.*?\*/", raw, re.S)
    assert m, "no header comment for the 4:2:0 -> BGR list form"
    assert m.start() > raw.index("mi_status mi_clahe_yuv420_to_bgr("), "the block stands behind the batch form's declarations"
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("no in-place form", "read only during the call", "per-frame alignment", "Nothing is enqueued unless every frame passes",
                   "MI_ERR_BUSY", "yuv420_bgr_onepass", "yuv420_bgr_twopass", "yuv420_bgr_list_frames_vec", "yuv420_bgr_list_frames_bytes",
                   "are not touched by list calls", "never written", "not checked", "REFLECT_101", "clahe_fp_contract",
                   "a null `frames` with n_frames > 0", "refused even when another size is 0", "MI_OK, nothing written",
                   "holds the addresses it was captured with", "same profiling slots", "c0 is always U and c1 always V",
                   "a YV12 caller exchanges the two", "MI_CHROMA_INTERLEAVED", "mi_*_nv12_to_bgr_frames_dev", "c1 is ignored and may be NULL",
                   "nv12_bgr_onepass", "c_pitch is a multiple of 8", "c0 and c1 multiples of 8", "c1 = c0 + W/2", "a null c1 in any entry",
                   "byte for byte what mi_*_yuv420_to_bgr_batch_dev writes for that frame alone", "per chunk of 64 frames",
                   "compared as address ranges", "may appear in several entries", "MI_ERR_UNSUPPORTED", "a `chroma` other than the two",
                   "W interleaved, W/2 planar", "out_pitch < 3*W", "tiles <= 0"):
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_yuv420_to_bgr\*:.*?\*/", raw, re.S)
    assert batch and "frames_dev" not in batch.group(0), "the batch form's comment was not extended"


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_yuv420_to_bgr_frames_dev", "clahe_yuv420_to_bgr_frames_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[1:7] == ["frames", "width", "height", "y_pitch", "c_pitch", "chroma"], m
        assert all(params[p].default is inspect.Parameter.empty for p in list(params)[1:7]), m
        assert params["order"].default == mi_lumaeq.ORDER_BGR
        assert params["out_pitch"].default is None
        assert params["stream"].default == 0
    p = inspect.signature(mi_lumaeq.Context.clahe_yuv420_to_bgr_frames_dev).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


@pytest.mark.parametrize("chroma", [mi_lumaeq.CHROMA_PLANAR, mi_lumaeq.CHROMA_INTERLEAVED])
def test_null_context_is_bad_arg_and_touches_nothing(built_lib, chroma):
    w, h = 8, 4
    src = np.arange(w * h * 3 // 2, dtype=np.uint8)
    dst = np.full(w * h * 3, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    y = src.ctypes.data
    entry = mi_lumaeq.Yuv420BgrFrameDev(y, y + w * h, y + w * h + w * h // 4, dst.ctypes.data)
    e0 = bytes(entry)
    cp = w // 2 if chroma == mi_lumaeq.CHROMA_PLANAR else w
    a = (None, ctypes.byref(entry), 1, w, h, w, cp, chroma, 3 * w, 0)
    assert built_lib.mi_equalize_hist_yuv420_to_bgr_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_yuv420_to_bgr_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0


def max_pairs_lds_f32():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "clahe.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kMaxPairsLdsF32\s*=\s*(\d+)\s*;", src).group(1))


def test_the_sweep_holds_every_class():
    """The GPU sweep's seeded cases, classified by the documented rule restated in yuv420_bgr_frames_cases.classify: at least 6 cases in
    each of the four classes, within the sizes the sweep promises, both orders, all three layouts, both ops."""
    K = max_pairs_lds_f32()
    sweep = cases.sweep_cases()
    count = cases.class_counts(sweep, K)
    assert len(sweep) == 32 and set(count) == set(cases.CLASSES) and sum(count.values()) == 32
    assert min(count.values()) >= 6, count
    for k in sweep:
        assert k["w"] % 2 == 0 and k["h"] % 2 == 0 and 2 <= k["w"] <= 128 and 2 <= k["h"] <= 48 and 1 <= k["n"] <= 4, k
        assert len(k["skews"]) == k["n"]
        name, d = cases.classify(k, K)
        assert len(d) == len(cases.COUNTERS) and d[4] == d[5] == 0, "list calls never touch yuv420_bgr_vec / yuv420_bgr_bytes"
        if name == "interleaved":
            assert d[:6] == (0,) * 6 and d[6] + d[7] == 1, "an INTERLEAVED list moves the NV12 form's counters only"
        else:
            assert d[0] + d[1] == 1 and d[2] + d[3] == k["n"] and d[6:] == (0, 0), (name, d)
            assert (name == "byte-frames") == (d[3] > 0)
            assert name != "vector-onepass" or d[0] == 1
            assert name != "vector-twopass" or d[1] == 1
    assert {k["order"] for k in sweep} == {0, 1} and {k["fmt"] for k in sweep} == {"i420", "yv12", "nv12"}
    assert {k["kind"] for k in sweep} == {"eq", "clahe"}
    planar = [(k, cases.classify(k, K)) for k in sweep if k["fmt"] != "nv12"]
    assert any(k["kind"] == "clahe" and d[0] for k, (_, d) in planar), "a one-pass CLAHE case"
    assert any(0 < d[2] < k["n"] for k, (_, d) in planar), "a call whose frames take both walks"


def test_the_rule_on_hand_made_cases():
    """classify() on the cases of tests/test_gpu_yuv420_to_bgr_frames.py's alignment tests, so that the restated rule is itself pinned."""
    K = max_pairs_lds_f32()
    base = dict(kind="eq", w=32, h=16, n=3, tx=2, ty=2, clip=2.0, order=0, fmt="i420", y_pitch=48, c_pitch=24, out_pitch=112,
                skews=[(0, 0, 0, 0)] * 3)
    assert cases.classify(base, K) == ("vector-onepass", (1, 0, 3, 0, 0, 0, 0, 0))
    assert cases.classify(dict(base, kind="clahe"), K) == ("vector-onepass", (1, 0, 3, 0, 0, 0, 0, 0))
    for bad in ((1, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 8)):
        sk = [(0, 0, 0, 0), bad, (0, 0, 0, 0)]
        assert cases.classify(dict(base, skews=sk), K) == ("byte-frames", (1, 0, 2, 1, 0, 0, 0, 0))
        # two-pass: the decode reads Y from aligned scratch, so a broken y address alone leaves every frame on the vector walk
        want = ("vector-twopass", (0, 1, 3, 0, 0, 0, 0, 0)) if bad[0] else ("byte-frames", (0, 1, 2, 1, 0, 0, 0, 0))
        assert cases.classify(dict(base, kind="clahe", skews=sk), K) == want
    assert cases.classify(dict(base, kind="clahe", skews=[(0, 8, 8, 0)] * 3), K) == ("vector-onepass", (1, 0, 3, 0, 0, 0, 0, 0))
    assert cases.classify(dict(base, c_pitch=20), K) == ("byte-frames", (1, 0, 0, 3, 0, 0, 0, 0))
    assert cases.classify(dict(base, kind="clahe", y_pitch=40), K) == ("byte-frames", (0, 1, 0, 3, 0, 0, 0, 0))
    assert cases.classify(dict(base, kind="clahe", fmt="nv12", c_pitch=48), K) == ("interleaved", (0, 0, 0, 0, 0, 0, 1, 0))
    assert cases.classify(dict(base, kind="clahe", fmt="nv12", c_pitch=40), K) == ("interleaved", (0, 0, 0, 0, 0, 0, 0, 1))
