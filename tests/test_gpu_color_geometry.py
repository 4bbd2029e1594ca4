"""The colour-domain kernels (kernels/color.hip.h, kernels/color_clahe.hip.h, host/color.inc.hpp) at the shapes where their loops and
slices repeat: tile histograms past their first step and second item, uneven row slices, column segments and idle phases of the one-pass
BGR CLAHE and its hand-over to the planes, grid-stride loops of the fused equalizeHist, the carried (by, gx) walk of the NV12 form with
its wrap, one workgroup a frame for the stand-alone conversions, and more rows than the grid has.  test_gpu_parity.py and
test_gpu_strided_batch_forms.py cover layouts and arithmetic at sizes where every lane runs every loop body at most once.

tests/color_geometry_cases.py holds the cases and says, property by property, which case reaches it; tests/test_color_geometry_shapes.py
proves on the CPU that they do for every CU count from 64 to 1024, which is why the context fixture asserts that the device lies in that
range.  Every comparison is exact: full-range random bytes, a different content in every frame, whole sentinel-filled allocations with
guard bytes (tests/strided_layouts.py) against the oracle -- the output, and the input as well (in place it is the output).  The CLAHE
and equalizeHist groups also prove which path ran, from the launch counts of one profiled call."""
import functools

import numpy as np
import pytest
import torch

import color_geometry_cases as g
import mi_lumaeq
import oracle
import strided_layouts as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert g.CU_MIN <= cu <= g.CU_MAX, f"the case tables are proven for {g.CU_MIN}..{g.CU_MAX} CUs, this device has {cu}"
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def empty_cache():
    """The many-frame batches leave nothing cached in torch's allocator for the modules that run after this one."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def launches(c):
    prof = c.profile_read(reset=True)
    return {k: prof[k]["launches"] for k in mi_lumaeq.KERNEL_NAMES}


def check(src, dst, frames, want, call, why, c=None):
    """Upload `frames` into src (dst, when it is another Side, stays sentinel), run call(src, dst) and compare both allocations whole.
    With a context: the call is profiled, and its launch counts per kernel kind are returned."""
    src.upload(frames)
    if dst is not src:
        dst.upload(None)
    for s in (src, dst):
        assert s.buf.data_ptr() % 16 == 0, "the layouts count on a 16-byte aligned allocation"
    counts = None
    if c is not None:
        c.set_profiling(True)
        launches(c)
    try:
        call(src, dst)
        torch.cuda.synchronize()
        if c is not None:
            counts = launches(c)
    finally:
        if c is not None:
            c.set_profiling(False)
    if dst is src:
        L.assert_sides(src, src.image(want), why)
    else:
        L.assert_sides([src, dst], [src.image(frames), dst.image(want)], why)
    return counts


def bgr_side(w, h, n, off=0, pitch=None, stride=None, name=""):
    pitch = 3 * w if pitch is None else pitch
    return L.Side(h, 3 * w, pitch, off, n, h * pitch if stride is None else stride, name)


def strides(src, dst):
    return dict(src_step=src.pitch, src_frame=src.frame_stride, dst_step=dst.pitch, dst_frame=dst.frame_stride)


def only(**kinds):
    """Launch counts with every kind not named at zero."""
    return {k: kinds.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}


def onepass_counts(tile_lut):
    return only(tile_hist_kernel=1, tile_lut_kernel=1 if tile_lut else 0, clahe_interp_kernel=1)


def assert_path(counts, path, tile_lut, why):
    if path == "onepass":
        assert counts == onepass_counts(tile_lut), (why, counts)
    else:
        assert counts["color_kernel"] == 2, (why, counts)


# ---- a. bgr_tile_hist_kernel<512>: items, steps and slices -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clahe_case(w, h, n, clip, tx, ty, seed):
    frames = rand((n, h, w, 3), seed)
    return frames, tuple(oracle.bgr_luma_op(f, mi_lumaeq.OP_CLAHE, clip, tx, ty) for f in frames)


def clahe_call(c, w, h, n, clip, tx, ty):
    return lambda s, d: c.bgr_luma_op_batch_dev(s.ptr, d.ptr, w, h, n, mi_lumaeq.OP_CLAHE, clip, tx, ty, **strides(s, d))


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("case", g.TILE_HIST_SHAPES, ids=[k["id"] for k in g.TILE_HIST_SHAPES])
def test_tile_hist_steps_and_slices(c, case, inplace):
    """One-pass CLAHE where a tile-histogram workgroup has more than 512 items, a second loop step, more slots than lanes, or uneven
    row slices (see the table for each shape); the launch counts prove the one-pass kernels ran, with tile_lut_kernel iff S > 1."""
    w, h, tx, ty, n = case["w"], case["h"], case["tx"], case["ty"], g.A_N
    plan = g.onepass_plan(cu_count(), w, h, tx, ty, n)
    assert {k: plan[k] for k in ("S", "slices", "segs", "phases", "subs")} == {k: case["reach"][k] for k in ("S", "slices", "segs", "phases", "subs")}
    frames, want = clahe_case(w, h, n, g.A_CLIP, tx, ty, 11)
    src = bgr_side(w, h, n, name="src")
    dst = src if inplace else bgr_side(w, h, n, name="dst")
    counts = check(src, dst, frames, want, clahe_call(c, w, h, n, g.A_CLIP, tx, ty), (case["id"], inplace), c)
    assert_path(counts, "onepass", plan["tile_lut"], case["id"])


@pytest.mark.parametrize("case", g.TILE_HIST_SHAPES, ids=[k["id"] for k in g.TILE_HIST_SHAPES])
def test_tile_hist_shapes_through_planes(c, case):
    """The cross-check: the same shapes with bgr_fused off go through the Y / U / V planes (two color_kernel launches) to the same bytes."""
    w, h, tx, ty, n = case["w"], case["h"], case["tx"], case["ty"], g.A_N
    frames, want = clahe_case(w, h, n, g.A_CLIP, tx, ty, 11)
    src, dst = bgr_side(w, h, n, name="src"), bgr_side(w, h, n, name="dst")
    try:
        c.set_option("bgr_fused", 0)
        counts = check(src, dst, frames, want, clahe_call(c, w, h, n, g.A_CLIP, tx, ty), (case["id"], "planes"), c)
    finally:
        c.set_option("bgr_fused", 1)
    assert_path(counts, "planes", None, case["id"])


# ---- b. bgr_clahe_interp_kernel: bands, phases and the hand-over to planes -------------------------------------------------------
@pytest.mark.parametrize("case", g.INTERP_CASES, ids=[k["id"] for k in g.INTERP_CASES])
def test_interp_bands_phases_and_planes(c, case):
    """Odd band edges with an idle lane, the largest pair table, and each reason for which bgr_luma_dev leaves the one-pass kernels:
    the pair table, tile_w % 16, REFLECT_101 padding, alignment, clahe_fp_contract.  The launch counts say which path ran."""
    w, h, tx, ty, clip = case["w"], case["h"], case["tx"], case["ty"], case["clip"]
    n, off, contract = case.get("n", g.B_N), case.get("off", 0), case.get("contract", False)
    aligned = off % 16 == 0 and (3 * w) % 16 == 0 and (3 * w * h) % 16 == 0
    assert g.shape_ok(w, h, tx, ty, contract, aligned) == case["why"]
    tile_lut = g.onepass_plan(cu_count(), w, h, tx, ty, n)["tile_lut"] if case["path"] == "onepass" else None
    if "reach" in case:
        assert tile_lut == case["reach"].get("tile_lut", False)
    src = bgr_side(w, h, n, off=off, name="src")
    dst = src if case.get("inplace") else bgr_side(w, h, n, off=off, name="dst")
    prev = oracle.set_fp_contract(contract)
    try:
        c.set_option("clahe_fp_contract", 1 if contract else 0)
        if contract:
            frames = rand((n, h, w, 3), 21)
            want = tuple(oracle.bgr_luma_op(f, mi_lumaeq.OP_CLAHE, clip, tx, ty) for f in frames)
        else:
            frames, want = clahe_case(w, h, n, clip, tx, ty, 21)
        counts = check(src, dst, frames, want, clahe_call(c, w, h, n, clip, tx, ty), case["id"], c)
    finally:
        c.set_option("clahe_fp_contract", 0)
        oracle.set_fp_contract(prev)
    assert_path(counts, case["path"], tile_lut, case["id"])


# ---- c. fused BGR equalizeHist ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def equalize_case(w, h, n):
    frames = rand((n, h, w, 3), 31)
    return frames, tuple(oracle.bgr_luma_op(f, mi_lumaeq.OP_EQUALIZE) for f in frames)


@pytest.mark.parametrize("fused", [1, 0], ids=["bgr_fused", "planes"])
@pytest.mark.parametrize("case", g.EQUALIZE_CASES, ids=[k["id"] for k in g.EQUALIZE_CASES])
def test_fused_equalize_loops(c, case, fused):
    """bgr_luma_hist_kernel / bgr_luma_apply_kernel where some lanes take a second group, with a ragged tail, with a workgroup that
    counts nothing, and on the byte body; tight pitch, so a frame is one row of W * H pixels.  bgr_fused 1: two color-kind launches
    and one equalize_lut_kernel, no hist_partial_kernel.  bgr_fused 0: the same bytes through the planes."""
    w, h, n, off = case["w"], case["h"], g.C_N, case["off"]
    assert g.equalize_reach(cu_count(), case, n) == case["reach"]
    stride = (3 * w * h + 15) // 16 * 16 + 16
    frames, want = equalize_case(w, h, n)
    src, dst = bgr_side(w, h, n, off=off, stride=stride, name="src"), bgr_side(w, h, n, off=off, stride=stride, name="dst")
    try:
        c.set_option("bgr_fused", fused)
        counts = check(src, dst, frames, want,
                       lambda s, d: c.bgr_luma_op_batch_dev(s.ptr, d.ptr, w, h, n, mi_lumaeq.OP_EQUALIZE, **strides(s, d)), (case["id"], fused), c)
    finally:
        c.set_option("bgr_fused", 1)
    if fused:
        assert counts == only(color_kernel=2, equalize_lut_kernel=1), (case["id"], counts)
    else:
        assert counts["color_kernel"] == 2 and counts != only(color_kernel=2, equalize_lut_kernel=1), (case["id"], counts)


# ---- d. nv12_bgr_equalize_batch_dev ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", g.NV12_CASES, ids=[k["id"] for k in g.NV12_CASES])
def test_nv12_bgr_equalize_walks(c, case):
    """The carried (by, gx) walk of nv12_bgr_hist_kernel / nv12_bgr_apply_kernel with a second step and its wrap, and the 2 x 2 block
    body over several steps; in place, and on two different frame strides."""
    w, h, n, off = case["w"], case["h"], case["n"], case["off"]
    assert g.nv12_reach(cu_count(), case) == case["reach"]
    rows, frame = h * 3 // 2, w * h * 3 // 2
    frames = rand((n, rows, w), 41)
    want = tuple(oracle.nv12_bgr_equalize(f, w, h).reshape(rows, w) for f in frames)
    src = L.Side(rows, w, w, off, n, frame + case["extra"][0], "in")
    dst = src if case["extra"][1] is None else L.Side(rows, w, w, off, n, frame + case["extra"][1], "out")
    check(src, dst, frames, want,
          lambda s, d: c.nv12_bgr_equalize_batch_dev(s.ptr, d.ptr, w, h, n, in_frame=s.frame_stride, out_frame=d.frame_stride), case["id"])


# ---- e. many small frames: one workgroup a frame ---------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV_I420, mi_lumaeq.COLOR_YUV2BGR_NV12], ids=["BGR2YUV_I420", "YUV2BGR_NV12"])
@pytest.mark.parametrize("case", g.CVT420_MANY, ids=[k["id"] for k in g.CVT420_MANY])
def test_many_frames_cvt420(c, case, code):
    """8 * cu_count frames: cvt420_kernel gets one workgroup a frame, whose lanes step through the frame more than once -- the vector
    body with the carried walk and its wrap (96 x 96), the byte body in three steps (66 x 34)."""
    w, h = case["w"], case["h"]
    n = g.FRAMES_PER_CU * cu_count()
    assert g.cvt420_reach(cu_count(), case) == case["reach"]
    enc = code == mi_lumaeq.COLOR_BGR2YUV_I420
    rows = h * 3 // 2
    c3, pl = bgr_side(w, h, n, name="c3"), L.Side(rows, w, w, 0, n, rows * w, "planar")
    if enc:
        frames = rand((n, h, w, 3), 51)
        want = [oracle.bgr_to_i420(f) for f in frames]
    else:
        frames = rand((n, rows, w), 52)
        want = [oracle.nv12_to_bgr(f, w, h) for f in frames]
    src, dst = (c3, pl) if enc else (pl, c3)
    check(src, dst, frames, want, lambda s, d: c.cvt_color_420_batch_dev(s.ptr, d.ptr, w, h, n, code, **strides(s, d)), (case["id"], code))


@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV, mi_lumaeq.COLOR_YUV2BGR], ids=["BGR2YUV", "YUV2BGR"])
def test_many_frames_color(c, code):
    """8 * cu_count tight frames of 67 x 63: 12663 bytes, 7 modulo 16, so frames 0, 16, 32, ... take color_kernel's vector body (263
    groups on 256 lanes, a 13-pixel tail) and all others its byte body in 17 steps, one workgroup a frame."""
    w, h = g.COLOR_MANY["w"], g.COLOR_MANY["h"]
    n = g.FRAMES_PER_CU * cu_count()
    assert g.color_many_reach(cu_count()) == g.COLOR_MANY["reach"]
    frames = rand((n, h, w, 3), 61)
    fn = oracle.bgr2yuv if code == mi_lumaeq.COLOR_BGR2YUV else oracle.yuv2bgr
    want = fn(frames.reshape(n * h, w, 3)).reshape(n, h, w, 3)                   # a per-pixel map: one call for the whole batch
    assert np.array_equal(want[17], fn(frames[17]))
    src, dst = bgr_side(w, h, n, name="src"), bgr_side(w, h, n, name="dst")
    check(src, dst, frames, want, lambda s, d: c.cvt_color_batch_dev(s.ptr, d.ptr, w, h, n, code, **strides(s, d)), code)


# ---- f. more rows than the grid has ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [mi_lumaeq.COLOR_BGR2YUV, mi_lumaeq.COLOR_YUV2BGR], ids=["BGR2YUV", "YUV2BGR"])
def test_row_loop_second_step(c, code):
    """16 x 65540 at a pitch of 64 on both sides: row-wise addressing with 65535 grid rows, so rows 65535..65539 come from the second
    step of color_kernel's row loop."""
    k = g.COLOR_ROWS
    w, h, n, pitch = k["w"], k["h"], k["n"], k["pitch"]
    assert g.color_rows_reach(cu_count()) == k["reach"]
    frames = rand((n, h, w, 3), 71)
    fn = oracle.bgr2yuv if code == mi_lumaeq.COLOR_BGR2YUV else oracle.yuv2bgr
    want = [fn(f) for f in frames]
    src, dst = bgr_side(w, h, n, pitch=pitch, name="src"), bgr_side(w, h, n, pitch=pitch, name="dst")
    check(src, dst, frames, want, lambda s, d: c.cvt_color_batch_dev(s.ptr, d.ptr, w, h, n, code, **strides(s, d)), code)
