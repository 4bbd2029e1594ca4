"""NV12 in, BGR / RGB out at the shapes where the kernels of kernels/nv12_bgr.hip.h repeat themselves: grid-stride loops past their first
step, CLAHE bands that start on an odd row, column segments, the largest pair table and the hand-over to the two-pass fallback, one
alignment term broken at a time, and a seeded random sweep.  test_gpu_nv12_to_bgr.py covers layouts, guards, errors, chunking and graphs
at sizes where every lane runs every loop body at most once; its helpers are used here unchanged.  Every comparison is exact: the whole
sentinel-filled output allocation against oracle.nv12_to_bgr(oracle.nv12_frame(...)), the whole input allocation against what was
uploaded, and the (nv12_bgr_onepass, nv12_bgr_twopass) counter delta of every call.  Y, U and V are full-range random bytes.

How many workgroups nv12_to_bgr_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of group 1 are chosen
by it.  launch_nv12_to_bgr takes B = min(blocks_per_frame(W*H*9/4 bytes, H/2 rows, n, 2048), ceil(items / 256)), and blocks_per_frame
never returns more than max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which only lowers it.
So   B <= max(1, floor(W*H*9/4 / 16384)),  B <= H/2,
and a workgroup's lanes step through the frame by stride = 256 * B items: 16 x 2 pixel groups on the vector path (gx_n = W/16 per row
pair, `groups` in all, the carried walk by += dby, gx += dgx with dby = stride / gx_n, dgx = stride % gx_n and a wrap when gx >= gx_n),
2 x 2 pixel blocks on the byte path."""
import math
import re

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import ORDER_BGR, ORDER_RGB
from test_gpu_nv12_to_bgr import ROOT, SENT, ORDERS, EQ, Nv12In, BgrOut, check, expected, rand_frames, stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small batches leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def max_pairs_lds_f32():
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "clahe.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+kMaxPairsLdsF32\s*=\s*(\d+)\s*;", src).group(1))


def layout_terms(w, h, si, di):
    """The eight values nv12_bgr_aligned16 ORs together, relative to the (16-byte aligned) allocations, from the keyword arguments of
    Nv12In (si) and BgrOut (di) alone: y base, uv base, out base, y_pitch, uv_pitch, out_pitch, in_frame, out_frame."""
    yp, up = si.get("y_pitch") or w, si.get("uv_pitch") or w
    uv_off = yp * h + si.get("plane_gap", 0)
    op = di.get("pitch") or 3 * w
    return {"y": si.get("off", 0), "uv": si.get("off", 0) + uv_off, "out": di.get("off", 0), "y_pitch": yp, "uv_pitch": up,
            "out_pitch": op, "in_frame": uv_off + up * (h // 2) + si.get("frame_gap", 0), "out_frame": op * h + di.get("frame_gap", 0)}


def misaligned(terms):
    return sorted(k for k, v in terms.items() if v % 16)


def build(w, h, n, si, di):
    """The two allocations of a layout; what layout_terms said about it holds for the real addresses."""
    src, dst = Nv12In(w, h, n, **si), BgrOut(w, h, n, **di)
    t = layout_terms(w, h, si, di)
    base_i, base_o = src.buf.data_ptr(), dst.buf.data_ptr()
    real = {"y": src.y_ptr - base_i, "uv": src.uv_ptr - base_i, "out": dst.ptr - base_o, "y_pitch": src.y_pitch, "uv_pitch": src.uv_pitch,
            "out_pitch": dst.pitch, "in_frame": src.fstride, "out_frame": dst.fstride}
    assert real == t, (real, t)
    return src, dst


# ---- 1. LUT-apply and decode loops past their first step -------------------------------------------------------------------------
PITCHED_112 = (dict(y_pitch=128, uv_pitch=144, plane_gap=32, frame_gap=48, off=16), dict(pitch=352, frame_gap=64, off=32))
ODD_66 = (dict(y_pitch=67, uv_pitch=69, plane_gap=3, frame_gap=5, off=1), dict(pitch=201, frame_gap=7, off=1))
LOOP_SHAPES = [
    # id, W, H, n, Nv12In layout, BgrOut layout, vector path
    # bytes/16384 = 1.9: B = 1, stride 256; gx_n 6, groups 432, dby 42, dgx 4: the wrap fires whenever gx >= 2, the second step is partial
    ("96x144-tight", 96, 144, 1, {}, {}, True),
    # the same walk in every frame; the kernel takes the frames last-to-first
    ("96x144-three-frames", 96, 144, 3, {}, {}, True),
    # bytes/16384 = 2.46: B = 2, stride 512; gx_n 7, groups 560, dby 73, dgx 1; pitches, plane gap, frame gaps and bases multiples of 16
    ("112x160-pitched", 112, 160, 2, *PITCHED_112, True),
    # bytes/16384 = 4.5 but H/2 = 2 rows: B = 2, stride 512; gx_n 512, groups 1024, dby 1, dgx 0: every lane steps straight down one row pair
    ("8192x4", 8192, 4, 1, {}, {}, True),
    # bytes/16384 = 4.5, H/2 = 4: B = 4, stride 1024; gx_n 257, groups 1028, dby 3, dgx 253: four lanes take a second step, and wrap
    ("4112x8", 4112, 8, 1, {}, {}, True),
    # byte path, bytes/16384 = 0.3: B = 1; 33 x 17 = 561 blocks of 2 x 2 for 256 lanes: three steps, the last of 49 lanes
    ("66x34-odd", 66, 34, 2, *ODD_66, False),
    # W % 16 == 0 and one term off: vec == 0; 48 x 72 = 3456 blocks, B = 1: thirteen full steps and a half one
    ("96x144-out-base+1", 96, 144, 1, {}, dict(off=1), False),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,w,h,n,si,di,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_equalize_loops_past_first_step(c, name, w, h, n, si, di, vec, order):
    """equalizeHist: nv12_to_bgr_kernel<ORDER, true> where a lane owns more than one group / block (see the module docstring and the
    table above for stride, dby and dgx of each shape)."""
    assert (w % 16 == 0 and not misaligned(layout_terms(w, h, si, di))) == vec
    bound = max(1, w * h * 9 // 4 // 16384)
    assert (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2), "the shape would not loop"
    src, dst = build(w, h, n, si, di)
    check(c, rand_frames(w, h, n, 101), w, h, EQ, order, src, dst, (1, 0))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("di", [{}, dict(off=1)], ids=["vector", "byte"])
def test_decode_only_loops_past_first_step(c, di, order):
    """nv12_to_bgr_kernel<ORDER, false>, the second pass of the CLAHE fallback, at 96 x 144: 144 % 5 != 0, so a 4 x 5 grid pads by
    REFLECT_101 and the call goes two-pass.  Aligned output: the luma comes from 16-byte aligned tight scratch planes and the decode is
    the vector walk of 96x144-tight (first-to-last frame order); output base + 1: the byte walk."""
    w, h, n = 96, 144, 2
    src, dst = build(w, h, n, {}, di)
    check(c, rand_frames(w, h, n, 102), w, h, ("clahe", (2.0, 4, 5)), order, src, dst, (0, 1))


# ---- 2. CLAHE one-pass geometry --------------------------------------------------------------------------------------------------
K = max_pairs_lds_f32()
ONEPASS_SHAPES = [
    # W, H, tiles_x, tiles_y, clip, expected counters
    (32, 20, 2, 2, 2.0, (1, 0)),            # tile 16 x 10: band 1 starts at row 5, the row pair (4, 5) lies in two bands
    (48, 30, 3, 2, 2.0, (1, 0)),            # tile 16 x 15: the pair (22, 23) straddles; 3 groups, 85 phases, lane 255 idle
    (32, 12, 2, 2, 2.0, (1, 0)),            # tile 16 x 6: one sub-band per band; the pair (2, 3) straddles
    (96, 16, 2, 2, 2.0, (1, 0)),            # tile_w 48: three groups per tile, the middle one with both neighbours in one tile
    (4112, 8, 1, 1, 2.0, (1, 0)),           # 257 groups: two column segments, the second of one group
    (4112, 8, 1, 2, 2.0, (1, 0)),           # the same with tile_h 4: three bands
    (16 * (K - 1), 12, K - 1, 2, 2.0, (1, 0)),   # the largest pair table: tiles_x + 1 == kMaxPairsLdsF32, 60 KiB of dynamic LDS
    (16 * K, 12, K, 2, 2.0, (0, 1)),        # one tile wider: the fallback takes over, the same exactness
    (64, 32, 2, 4, 0.0, (1, 0)),            # no clipping
    (64, 32, 2, 4, 40.0, (1, 0)),           # a clip limit above every bin
]


def test_band_edges_of_the_shapes():
    """The straddling row pairs named above, from the kernel's own f32 expression floor(y * inv_th - 0.5)."""
    def band(y, th):
        inv = np.float32(1.0) / np.float32(th)
        return int(np.floor(np.float32(np.float32(y) * inv) - np.float32(0.5)))
    assert band(4, 10) != band(5, 10) and band(22, 15) != band(23, 15) and band(2, 6) != band(3, 6)
    assert all(band(2 * r, th) == band(2 * r + 1, th) for th in (8, 16) for r in range(16))
    assert 4112 // 16 == 257 and 16 * K <= 256


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("w,h,tx,ty,clip,want", ONEPASS_SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}x{s[3]}-clip{s[4]:g}" for s in ONEPASS_SHAPES])
def test_clahe_onepass_geometry(c, w, h, tx, ty, clip, want, order):
    n = 2
    src, dst = build(w, h, n, {}, {})
    check(c, rand_frames(w, h, n, 201), w, h, ("clahe", (clip, tx, ty)), order, src, dst, want)


@pytest.mark.parametrize("order", ORDERS)
def test_clahe_onepass_pitched_with_guards(c, order):
    """48 x 30, 3 x 2 (odd tile height, three groups) with every pitch and stride a multiple of 16 and larger than its row: the pitch
    padding, the plane gap and the frame gaps keep their pattern."""
    w, h, n = 48, 30, 2
    si, di = dict(y_pitch=64, uv_pitch=80, plane_gap=32, frame_gap=48, off=16), dict(pitch=160, frame_gap=64, off=16)
    assert not misaligned(layout_terms(w, h, si, di))
    src, dst = build(w, h, n, si, di)
    check(c, rand_frames(w, h, n, 202), w, h, ("clahe", (2.0, 3, 2)), order, src, dst, (1, 0))


# ---- 3. one alignment term at a time ---------------------------------------------------------------------------------------------
ONE_TERM = [
    # the term, Nv12In layout, BgrOut layout (64 x 32: 32 rows make y_pitch * H and out_pitch * H multiples of 16 whatever the pitch,
    # and 16 chroma rows do the same for uv_pitch)
    ("y", dict(off=1, plane_gap=15, frame_gap=1), {}),
    ("uv", dict(plane_gap=8, frame_gap=8), {}),
    ("out", {}, dict(off=1)),
    ("y_pitch", dict(y_pitch=72), {}),
    ("uv_pitch", dict(uv_pitch=65), {}),
    ("out_pitch", {}, dict(pitch=193)),
    ("in_frame", dict(frame_gap=8), {}),
    ("out_frame", {}, dict(frame_gap=1)),
]


@pytest.mark.parametrize("term,si,di", ONE_TERM, ids=[t[0] for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, term, si, di):
    """64 x 32, CLAHE 4 x 2, two frames is one-pass when everything is aligned.  Each layout leaves seven of the eight terms of
    nv12_bgr_aligned16 multiples of 16 and breaks the eighth, by 1 or by 8 bytes: CLAHE takes the fallback, equalizeHist the byte path."""
    w, h, n = 64, 32, 2
    assert not misaligned(layout_terms(w, h, {}, {}))
    assert misaligned(layout_terms(w, h, si, di)) == [term]
    src, dst = build(w, h, n, si, di)
    frames = rand_frames(w, h, n, 301)
    check(c, frames, w, h, ("clahe", (2.0, 4, 2)), ORDER_BGR, src, dst, (0, 1))
    check(c, frames, w, h, EQ, ORDER_RGB, src, dst, (1, 0))


def test_every_term_aligned_is_onepass(c):
    """The control of the eight cases above."""
    w, h, n = 64, 32, 2
    src, dst = build(w, h, n, {}, {})
    check(c, rand_frames(w, h, n, 301), w, h, ("clahe", (2.0, 4, 2)), ORDER_BGR, src, dst, (1, 0))


# ---- 4. seeded random sweep ------------------------------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 32, 48


def draw_case(rng):
    """One case: W even in [2, 256] (about half of them multiples of 16), H even in [2, 64], 1..3 frames, the op, a tile grid in
    [1, 16] x [1, 5], a clip limit, the order and a layout.  Most CLAHE cases with W % 16 == 0 get a frame their grid divides into tiles
    of a multiple of 16 columns, or the one-pass kernel would hardly ever be drawn; three quarters of the layouts are aligned."""
    kind = "clahe" if rng.random() < 0.55 else "eq"
    tx, ty = int(rng.integers(1, 17)), int(rng.integers(1, 6))
    clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
    n, order = int(rng.integers(1, 4)), int(rng.integers(0, 2))
    w, h = 2 * int(rng.integers(1, 129)), 2 * int(rng.integers(1, 33))
    if rng.random() < 0.5:
        w = 16 * int(rng.integers(1, 17))
        if kind == "clahe" and rng.random() < 0.85:
            w = 16 * tx * int(rng.integers(1, 16 // tx + 1))
            m = 2 * ty // math.gcd(2, ty)
            h = m * int(rng.integers(1, 64 // m + 1))
    if rng.random() < 0.75:
        def up16(v):
            return (v + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
        si = dict(y_pitch=up16(w), uv_pitch=up16(w), plane_gap=16 * int(rng.integers(0, 3)), frame_gap=16 * int(rng.integers(0, 3)),
                  off=16 * int(rng.integers(0, 3)))
        di = dict(pitch=up16(3 * w), frame_gap=16 * int(rng.integers(0, 3)), off=16 * int(rng.integers(0, 3)))
    else:
        si = dict(y_pitch=w + int(rng.integers(0, 40)), uv_pitch=w + int(rng.integers(0, 40)), plane_gap=int(rng.integers(0, 40)),
                  frame_gap=int(rng.integers(0, 40)), off=int(rng.integers(0, 40)))
        di = dict(pitch=3 * w + int(rng.integers(0, 40)), frame_gap=int(rng.integers(0, 40)), off=int(rng.integers(0, 40)))
    return dict(kind=kind, w=w, h=h, n=n, tx=tx, ty=ty, clip=clip, order=order, si=si, di=di)


def classify(case, max_pairs):
    """The documented conditions (include/mi_lumaeq.h, host/nv12_bgr.inc.hpp), restated: the class of a case and its counter delta.
    clahe_fp_contract is off in this module's context."""
    w, h, tx, ty = case["w"], case["h"], case["tx"], case["ty"]
    aligned = not misaligned(layout_terms(w, h, case["si"], case["di"]))
    if case["kind"] == "eq":
        return ("eq-vector" if aligned and w % 16 == 0 else "eq-byte"), (1, 0)
    onepass = w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= max_pairs and aligned
    return ("clahe-onepass", (1, 0)) if onepass else ("clahe-twopass", (0, 1))


def sweep_cases():
    rng = np.random.default_rng(SWEEP_SEED)
    return [draw_case(rng) for _ in range(SWEEP_CASES)]


def test_seeded_random_sweep(c):
    cases = sweep_cases()
    classes = [classify(k, K) for k in cases]
    count = {name: sum(1 for cl, _ in classes if cl == name) for name in ("eq-vector", "eq-byte", "clahe-onepass", "clahe-twopass")}
    assert len(cases) == 48 and min(count.values()) >= 8, count
    assert {k["order"] for k in cases} == {ORDER_BGR, ORDER_RGB}
    c.set_option("clahe_fp_contract", 0)
    for i, (k, (_, want)) in enumerate(zip(cases, classes)):
        w, h, n = k["w"], k["h"], k["n"]
        assert w % 2 == 0 and h % 2 == 0 and 2 <= w <= 256 and 2 <= h <= 64 and 1 <= n <= 3
        src, dst = build(w, h, n, k["si"], k["di"])
        op = EQ if k["kind"] == "eq" else ("clahe", (k["clip"], k["tx"], k["ty"]))
        check(c, rand_frames(w, h, n, 400 + i), w, h, op, k["order"], src, dst, want)


# ---- 5. host form at shapes that loop and at an unaligned UV plane ---------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(34, 18), (96, 144)])
def test_host_form_shapes(w, h):
    """34 x 18: the Y plane of the staged frame is 612 bytes, so its UV plane starts 4 bytes past a 16-byte boundary (byte accesses; no
    grid gives tiles of a multiple of 16 columns: CLAHE goes two-pass).  96 x 144: the staged frame and image are aligned, the vector
    walk loops as in 96x144-tight, CLAHE 1 x 1 and 3 x 2 are one-pass.  Pageable memory, out rows an odd number of bytes apart: only the
    3*W bytes of each row are written."""
    frame = rand_frames(w, h, 1, 501)[0]
    ops = [(EQ, (1, 0))] + [(("clahe", (2.0, tx, ty)), (0, 1) if w == 34 else (1, 0)) for tx, ty in ((1, 1), (3, 2))]
    with mi_lumaeq.Context(0) as c:
        for op, want_stats in ops:
            for order in ORDERS:
                want = expected(frame, w, h, op, order)
                padded = np.full((h, 3 * w + 25), SENT, np.uint8)
                assert padded.strides[0] % 2 == 1
                out = padded[:, : 3 * w].reshape(h, w, 3)
                assert np.shares_memory(out, padded)
                src = frame.copy()
                before = stats(c)
                if op is EQ:
                    got = c.equalize_hist_nv12_to_bgr(src, w, h, order, out=out)
                else:
                    got = c.clahe_nv12_to_bgr(src, w, h, order, *op[1], out=out)
                after = stats(c)
                bad = np.flatnonzero(out != want)
                assert got is out and bad.size == 0, (op, order, bad.size, bad[:8])
                assert (padded[:, 3 * w:] == SENT).all() and np.array_equal(src, frame)
                assert (after[0] - before[0], after[1] - before[1]) == want_stats, (op, before, after)
        assert c.get_stat("error_drains") == 0
