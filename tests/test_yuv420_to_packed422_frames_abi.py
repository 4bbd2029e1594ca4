"""4:2:0 (NV12 / I420 / YV12) in, packed 4:2:2 (YUY2 / UYVY) out on a list of pitched device frames
(mi_*_yuv420_to_packed422_frames_dev) at the ABI level, without a GPU: the header declares the two entry points with their parameter
lists and the list entry struct, no struct or enum grew (minor version 3, MI_K_COUNT 10, the four MI_FMT_*), the new comment block
stands behind the batch form's declarations and states the parts of the contract a caller cannot guess while the batch form's block is
left alone, the binding lists the symbols and has the struct and the methods with their keyword defaults, both libraries export the
symbols, a null context is refused without touching the caller's buffers, the new sources are registered where they belong with the
kernel signatures the design names and no inline assembly, the two new statistics are declared, returned and documented, and the seeded
cases of the GPU sweep hold enough of every class (the documented rule restated in tests/yuv420_packed422_frames_cases.py)."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import mi_lumaeq
import yuv420_packed422_frames_cases as cases

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
MI_ERR_BAD_ARG = 1

LIST = ("mi_ctx* ctx, const mi_yuv420_packed422_frame_dev* frames, int n_frames, "
        "int width, int height, size_t y_pitch, size_t c_pitch, int chroma, size_t out_pitch, int format, mi_uv_mode uv_mode")
PARAMS = {
    "mi_equalize_hist_yuv420_to_packed422_frames_dev": LIST + ", void* stream",
    "mi_clahe_yuv420_to_packed422_frames_dev": LIST + ", double clip_limit, int tiles_x, int tiles_y, void* stream",
}
NAMES = list(PARAMS)
STATS = ("yuv420_packed422_list_frames_vec", "yuv420_packed422_list_frames_bytes")


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
    m = re.search(r"typedef\s+struct\s+mi_yuv420_packed422_frame_dev\s*\{(.*?)\}\s*mi_yuv420_packed422_frame_dev\s*;", _header(), re.S)
    assert m, "mi_yuv420_packed422_frame_dev is not declared"
    assert _norm(m.group(1)) == "const void* y; const void* c0; const void* c1; void* out;"
    f = mi_lumaeq.Yuv420Packed422FrameDev
    assert [n for n, _ in f._fields_] == ["y", "c0", "c1", "out"]
    assert ctypes.sizeof(f) == 32 == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert mi_lumaeq.Yuv420Packed422FrameDev is mi_lumaeq.capi.Yuv420Packed422FrameDev and "Yuv420Packed422FrameDev" in mi_lumaeq.__all__


def test_declared_behind_the_batch_form_and_nothing_grew():
    txt = _header()
    for name in NAMES:
        assert txt.index("mi_clahe_yuv420_to_packed422(") < txt.index(name + "(") < txt.index("mi_host_register"), name
    assert txt.index("mi_clahe_yuv420_to_packed422(") < txt.index("typedef struct mi_yuv420_packed422_frame_dev") < txt.index(NAMES[0] + "(")
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", HEADER.read_text()), "no struct grew: the minor version stays 3"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "no profiling slot was added"
    assert len(mi_lumaeq.KERNEL_NAMES) == 10
    assert re.findall(r"\bMI_FMT_(\w+)\s*=\s*(\d+)", txt) == [("NV12", "0"), ("P010", "1"), ("YUY2", "2"), ("UYVY", "3")], "no new MI_FMT_* value"
    assert sorted(set(re.findall(r"\bMI_CHROMA_\w+", txt))) == ["MI_CHROMA_INTERLEAVED", "MI_CHROMA_PLANAR"], "no new chroma layout"
    assert ctypes.sizeof(mi_lumaeq.Yuv420Planes) == 56, "mi_yuv420_planes did not grow"


def test_header_states_the_contract():
    """A comment block of its own, behind the batch form's declarations; the batch form's block is left as it was."""
    raw = HEADER.read_text()
    m = re.search(r"/\*\s*mi_\*_yuv420_to_packed422_frames_dev:.*?\*/", raw, re.S)
    assert m, "no header comment for the 4:2:0 -> packed 4:2:2 list form"
    assert m.start() > raw.index("mi_status mi_clahe_yuv420_to_packed422("), "the block stands behind the batch form's declarations"
    assert m.end() < raw.index("typedef struct mi_yuv420_packed422_frame_dev")
    txt = _norm(m.group(0).replace("\n *", " "))
    for needle in ("read only during the call", "both even", "There are no per-frame pitches", "MI_CHROMA_INTERLEAVED", "MI_CHROMA_PLANAR",
                   "c1 is ignored and may be NULL", "c0 is always U and c1 always V", "a YV12 caller exchanges the two",
                   "is not handed to another form", "one set of counters serves both layouts",
                   "byte for byte what mi_*_yuv420_to_packed422_batch_dev writes for that frame alone", "exactly Y0 U Y1 V",
                   "exactly U Y0 V Y1", "output rows 2r and 2r+1", "every chroma byte is 128", "clahe_fp_contract", "REFLECT_101",
                   "only the 2*W bytes of each output row are written", "never written",
                   "c0, c1 and c_pitch are not read and decide nothing", "not the walk, not the overlap check, not an error",
                   "may be NULL", "multiples of 4", "per-frame alignment", "W % 16 == 0", "y_pitch and out_pitch are multiples of 16",
                   "c_pitch is a multiple of 16 (interleaved) or 8 (planar)", "its y and out are multiples of 16",
                   "its c0 is a multiple of 16 (interleaved) or its c0 and c1 are multiples of 8 (planar)",
                   "while its neighbours stay vectorised", "the same bytes out", "per chunk of 64 frames", "one MI_K_HIST",
                   "one MI_K_EQ_LUT", "MI_K_LUT_APPLY", "never the fused equalizeHist kernel", "two_kernel_max_frames",
                   "MI_K_CLAHE_INTERP", "one-pass shape", "every frame of the call satisfies the address rule", "scratch Y planes",
                   "one MI_K_COLOR launch", "the frame's y drops out of its rule", "same profiling slots",
                   '"yuv420_packed422_onepass" / "yuv420_packed422_twopass"',
                   '"yuv420_packed422_list_frames_vec" / "yuv420_packed422_list_frames_bytes"', "n_frames in total per call",
                   '"yuv420_packed422_vec" / "yuv420_packed422_bytes" are not touched by list calls', "moves none", "no in-place form",
                   "compared as address ranges", "c1 = c0 + W/2", "may appear in several entries", "not checked",
                   "a null `frames` with n_frames > 0", "a null y or out in any entry", "under MI_UV_COPY a null c0",
                   "an `out` in any entry or an out_pitch that is not a multiple of 4", "a `format` other than the two",
                   "a `chroma` other than the two", "a bad uv_mode", "a negative size", "refused even when another size is 0", "y_pitch < W",
                   "W interleaved, W/2 planar", "out_pitch < 2*W", "tiles <= 0", "MI_ERR_UNSUPPORTED", "MI_OK, nothing written",
                   "n_frames == 0 with a null list is MI_OK", "Nothing is enqueued unless every frame passes",
                   "a bad last entry leaves the earlier frames' outputs untouched", "MI_STREAM_CTX", "MI_ERR_BUSY", "hipGraph",
                   "holds the addresses it was captured with"):
        assert needle in txt, needle
    batch = re.search(r"/\*\s*mi_\*_yuv420_to_packed422\*:.*?\*/", raw, re.S)
    assert batch and "frames_dev" not in batch.group(0), "the batch form's comment was not extended"
    assert "Not built: a frame-list form" in _norm(batch.group(0).replace("\n *", " "))


def test_binding_lists_the_symbols():
    for s in NAMES:
        assert s in mi_lumaeq.DECLARED_SYMBOLS, s
    for m in ("equalize_hist_yuv420_to_packed422_frames_dev", "clahe_yuv420_to_packed422_frames_dev"):
        f = getattr(mi_lumaeq.Context, m, None)
        assert callable(f), m
        params = inspect.signature(f).parameters
        assert list(params)[1:7] == ["frames", "width", "height", "y_pitch", "c_pitch", "chroma"], m
        assert all(params[p].default is inspect.Parameter.empty for p in list(params)[1:7]), m
        assert (params["fmt"].default, params["uv_mode"].default) == (mi_lumaeq.FMT_YUY2, mi_lumaeq.UV_COPY)
        assert params["out_pitch"].default is None
        assert params["stream"].default == 0
    p = inspect.signature(mi_lumaeq.Context.clahe_yuv420_to_packed422_frames_dev).parameters
    assert (p["clip_limit"].default, p["tiles_x"].default, p["tiles_y"].default) == (2.0, 8, 8)


def test_both_libraries_export_them(built_lib):
    for L in (built_lib, mi_lumaeq.test_lib()):
        for s in NAMES:
            assert hasattr(L, s), f"{s} is not exported"
            assert len(getattr(L, s).argtypes) == len(PARAMS[s].split(",")), s


@pytest.mark.parametrize("chroma", [mi_lumaeq.CHROMA_PLANAR, mi_lumaeq.CHROMA_INTERLEAVED])
@pytest.mark.parametrize("uv_mode", [mi_lumaeq.UV_COPY, mi_lumaeq.UV_FILL128])
def test_null_context_is_bad_arg_and_touches_nothing(built_lib, chroma, uv_mode):
    w, h = 8, 4
    src = np.arange(w * h * 3 // 2, dtype=np.uint8)
    dst = np.full(w * h * 2, 0x5A, np.uint8)
    s0, d0 = src.copy(), dst.copy()
    y = src.ctypes.data
    entry = mi_lumaeq.Yuv420Packed422FrameDev(y, y + w * h, y + w * h + w * h // 4, dst.ctypes.data)
    e0 = bytes(entry)
    cp = w // 2 if chroma == mi_lumaeq.CHROMA_PLANAR else w
    a = (None, ctypes.byref(entry), 1, w, h, w, cp, chroma, 2 * w, mi_lumaeq.FMT_YUY2, uv_mode)
    assert built_lib.mi_equalize_hist_yuv420_to_packed422_frames_dev(*a, None) == MI_ERR_BAD_ARG
    assert built_lib.mi_clahe_yuv420_to_packed422_frames_dev(*a, ctypes.c_double(2.0), 2, 2, None) == MI_ERR_BAD_ARG
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and bytes(entry) == e0


def test_new_sources_are_registered():
    assert (CSRC / "host" / "yuv420_packed422_frames.inc.hpp").exists()
    tu = (CSRC / "mi_lumaeq.hip").read_text()
    a, b = tu.index('#include "host/yuv420_packed422.inc.hpp"'), tu.index('#include "host/yuv420_packed422_frames.inc.hpp"')
    assert a < b and tu[a:b].count("#include") == 1, "directly behind yuv420_packed422.inc.hpp"
    kern = (CSRC / "kernels" / "yuv420_packed422.hip.h").read_text()
    assert re.search(r"template\s*<int OFF, bool PLANAR, bool LUT>\s*__global__[^;{]*\byuv420_to_packed422_frames_kernel\s*\("
                     r"Yuv420P422List l, Yuv420P422Job j, const uint8_t\* __restrict__ luts\)", kern)
    assert re.search(r"template\s*<int OFF, bool PLANAR>\s*__global__[^;{]*\byuv420_packed422_clahe_interp_frames_kernel\s*\("
                     r"Yuv420P422List l, Yuv420P422Job j, ClaheGeom g,\s*const uint8_t\* __restrict__ luts, int subs, int groups\)", kern)
    # the batch kernels keep their signatures
    assert re.search(r"\byuv420_to_packed422_kernel\s*\(Yuv420P422Job j, const uint8_t\* __restrict__ luts\)", kern)
    assert re.search(r"\byuv420_packed422_clahe_interp_kernel\s*\(Yuv420P422Job j, ClaheGeom g,", kern)
    assert kern.count("a change there is made here too") >= 2, "the copies say so"
    assert re.search(r"struct\s+Yuv420P422List\s*\{\s*Yuv420P422Frame\s+f\[kFramesPerLaunch\];\s*\};", kern)
    assert re.search(r"static_assert\(sizeof\(Yuv420P422Frame\) == 32", kern)
    assert len(re.findall(r"static_assert\(sizeof\(Yuv420P422List\) \+ sizeof\(Yuv420P422Job\)[^;]*<= 4096", kern)) == 2
    assert re.search(r"__host__ __device__ __forceinline__ bool yuv420_packed422_frame_vec\(", kern), "one rule for the kernel and the host"
    assert "asm" not in re.sub(r"//[^\n]*", "", kern), "no inline assembly"
    host = (CSRC / "host" / "yuv420_packed422_frames.inc.hpp").read_text()
    for fn in ("Yuv420P422FramesShape", "check_yuv420_packed422_frames", "check_yuv420_packed422", "Span", "kFramesPerLaunch", "FrameList",
               "Yuv420P422List", "launch_hist_partials", "equalize_lut_kernel", "launch_tile_luts", "nv12_bgr_onepass_shape", "clahe_dev",
               "d_planes", "launch_yuv420_to_packed422", "launch_yuv420_packed422_interp", "yuv420_packed422_frame_vec",
               "yuv420_packed422_onepass", "yuv420_packed422_twopass") + STATS:
        assert re.search(r"\b" + fn + r"\b", host), fn
    for src in (host, (CSRC / "host" / "yuv420_packed422.inc.hpp").read_text()):
        code = re.sub(r"//[^\n]*", "", src)
        assert "hist_lut_kernel" not in code and "fused" not in code, "never the fused kernel, never hist_lut_kernel"
    assert not re.search(r"\byuv420_packed422_(vec|bytes)\b", re.sub(r"//[^\n]*", "", host)), "list calls do not touch the batch form's walk counters"
    assert "--list" in (ROOT / "tools" / "yuv420_to_packed422_ab.py").read_text()
    assert "yuv420_to_packed422_frames" in (ROOT / "tools" / "stress_random.py").read_text()


def test_stat_names_are_declared_returned_and_documented():
    txt = (CSRC / "host" / "capi.inc.hpp").read_text()
    doc = txt[: txt.index("mi_status mi_ctx_get_stat(")]
    assert doc.index('"yuv420_packed422_vec" / "yuv420_packed422_bytes"') < doc.index('"' + STATS[0] + '" / "' + STATS[1] + '"')
    body = txt[txt.index("mi_status mi_ctx_get_stat("):]
    for k in STATS:
        assert re.search(r'strcmp\(name, "' + k + r'"\)\) \{ \*out = c->' + k + ";", body), k
        assert body.index('"yuv420_packed422_bytes"') < body.index('"' + k + '"')
    ctx = (CSRC / "host" / "context.inc.hpp").read_text()
    assert re.search(STATS[0] + r"\s*=\s*0\s*,\s*" + STATS[1] + r"\s*=\s*0\s*;", ctx)
    assert ctx.index("yuv420_packed422_vec = 0") < ctx.index(STATS[0] + " = 0")
    for doc_file in ("DESIGN.md", "INTEGRATION.md"):
        d = (ROOT / doc_file).read_text().replace("`", "")
        for k in STATS:
            assert '"' + k + '"' in d, (doc_file, k)
    assert "mi_*_yuv420_to_packed422_frames_dev" in (ROOT / "README.md").read_text().replace("`", "")


def max_pairs_lds_f32():
    src = (CSRC / "kernels" / "clahe.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kMaxPairsLdsF32\s*=\s*(\d+)\s*;", src).group(1))


def test_the_sweep_holds_every_class():
    """The GPU sweep's seeded cases, classified by the documented rule restated in yuv420_packed422_frames_cases.classify: at least 4
    cases in each of the four classes (a condition on the inputs, met by the choice of the seed), within the sizes the sweep promises,
    both formats, all three layouts, both ops."""
    K = max_pairs_lds_f32()
    sweep = cases.sweep_cases()
    count = cases.class_counts(sweep, K)
    assert len(sweep) == 32 and set(count) == set(cases.CLASSES) and sum(count.values()) == 32
    assert min(count.values()) >= 4, count
    for k in sweep:
        assert k["w"] % 2 == 0 and k["h"] % 2 == 0 and 2 <= k["w"] <= 128 and 2 <= k["h"] <= 48 and 1 <= k["n"] <= 4, k
        assert len(k["skews"]) == k["n"] and all(s[3] % 4 == 0 for s in k["skews"]) and k["out_pitch"] % 4 == 0, k
        assert k["y_pitch"] >= k["w"] and k["out_pitch"] >= 2 * k["w"] and k["c_pitch"] >= (k["w"] if k["src"] == "nv12" else k["w"] // 2)
        name, d = cases.classify(k, K)
        assert len(d) == len(cases.COUNTERS) and d[4] == d[5] == 0, "list calls never touch yuv420_packed422_vec / yuv420_packed422_bytes"
        assert d[0] + d[1] == 1 and d[2] + d[3] == k["n"], (name, d)
        assert (name == "fill128") == (k["uv_mode"] == cases.UV_FILL128)
        assert name != "byte-frames" or d[3] > 0
        assert name != "vector-onepass" or (d[0] == 1 and d[3] == 0)
        assert name != "vector-twopass" or (d[1] == 1 and d[3] == 0)
    assert {k["fmt"] for k in sweep} == {cases.FMT_YUY2, cases.FMT_UYVY} and {k["src"] for k in sweep} == {"nv12", "i420", "yv12"}
    assert {k["kind"] for k in sweep} == {"eq", "clahe"}
    every = [(k, cases.classify(k, K)) for k in sweep]
    assert any(k["kind"] == "clahe" and name == "vector-onepass" for k, (name, _) in every), "a one-pass CLAHE case"
    assert any(0 < d[2] < k["n"] for k, (_, d) in every), "a call whose frames take both walks"
    assert any(name == "byte-frames" and k["src"] == "nv12" for k, (name, _) in every)
    assert any(name == "byte-frames" and k["src"] != "nv12" for k, (name, _) in every)


def test_the_rule_on_hand_made_cases():
    """classify() on the cases of tests/test_gpu_yuv420_to_packed422_frames.py's alignment tests, so that the restated rule is itself
    pinned."""
    K = max_pairs_lds_f32()
    base = dict(kind="eq", w=32, h=4, n=3, tx=2, ty=1, clip=2.0, fmt=cases.FMT_YUY2, uv_mode=cases.UV_COPY, src="i420", y_pitch=48,
                c_pitch=24, out_pitch=80, skews=[(0, 0, 0, 0)] * 3)
    nv12 = dict(base, src="nv12", c_pitch=48)
    for b in (base, nv12):
        assert cases.classify(b, K) == ("vector-onepass", (1, 0, 3, 0, 0, 0))
        assert cases.classify(dict(b, kind="clahe"), K) == ("vector-onepass", (1, 0, 3, 0, 0, 0))
    broken = [(base, (1, 0, 0, 0), True), (base, (0, 0, 0, 4), True), (nv12, (0, 8, 0, 0), True), (base, (0, 8, 8, 0), False),
              (base, (0, 0, 4, 0), True), (base, (0, 4, 0, 0), True), (nv12, (1, 0, 0, 0), True)]
    for b, bad, breaks in broken:
        sk = [(0, 0, 0, 0), bad, (0, 0, 0, 0)]
        if not breaks:
            assert cases.classify(dict(b, skews=sk), K) == ("vector-onepass", (1, 0, 3, 0, 0, 0))
            assert cases.classify(dict(b, kind="clahe", skews=sk), K) == ("vector-onepass", (1, 0, 3, 0, 0, 0))
            continue
        assert cases.classify(dict(b, skews=sk), K) == ("byte-frames", (1, 0, 2, 1, 0, 0))
        # two-pass: the pack reads Y from aligned scratch, so a broken y address alone leaves every frame on the vector walk
        want = ("vector-twopass", (0, 1, 3, 0, 0, 0)) if bad[0] else ("byte-frames", (0, 1, 2, 1, 0, 0))
        assert cases.classify(dict(b, kind="clahe", skews=sk), K) == want
        # MI_UV_FILL128: the chroma addresses decide nothing
        fill = cases.classify(dict(b, uv_mode=cases.UV_FILL128, skews=sk), K)
        assert fill == ("fill128", (1, 0, 2, 1, 0, 0) if bad[0] or bad[3] else (1, 0, 3, 0, 0, 0))
    assert cases.classify(dict(base, c_pitch=20), K) == ("byte-frames", (1, 0, 0, 3, 0, 0))
    assert cases.classify(dict(base, c_pitch=20, uv_mode=cases.UV_FILL128), K) == ("fill128", (1, 0, 3, 0, 0, 0))
    assert cases.classify(dict(nv12, c_pitch=40), K) == ("byte-frames", (1, 0, 0, 3, 0, 0))
    assert cases.classify(dict(base, kind="clahe", y_pitch=40), K) == ("byte-frames", (0, 1, 0, 3, 0, 0))
    assert cases.classify(dict(base, kind="clahe", tx=1, ty=3), K) == ("vector-twopass", (0, 1, 3, 0, 0, 0))
