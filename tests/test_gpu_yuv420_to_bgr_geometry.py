"""Planar 4:2:0 in, BGR / RGB out at the shapes where the kernels of kernels/yuv420_bgr.hip.h repeat themselves and where the host
chooses between them: the alignment rule one term at a time (the Y and output terms multiples of 16, the chroma terms of 8), grid-stride
loops past their first step, the CLAHE one-pass geometry of tests/test_gpu_nv12_to_bgr_geometry.py with planar chroma, and a seeded
random sweep.  The helpers of tests/test_gpu_yuv420_to_bgr.py are used here unchanged; every comparison is exact, on the whole
sentinel-filled allocations of both sides, and every call asserts its (onepass, twopass) and (vec, bytes) counter deltas.

The grid of yuv420_to_bgr_kernel is that of nv12_to_bgr_kernel: B = min(blocks_per_frame(W*H*9/4 bytes, H/2 rows, n, 2048),
ceil(items / 256)) with B <= max(1, floor(W*H*9/4 / 16384)) and B <= H/2, and a workgroup's lanes step through the frame by
stride = 256 * B items: 16 x 2 pixel groups on the vector path (gx_n = W/16 per row pair, the carried walk by += dby, gx += dgx with a
wrap when gx >= gx_n), 2 x 2 pixel blocks on the byte path.  The module docstring of the NV12 geometry test derives the bound."""
import math

import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import ORDER_BGR, ORDER_RGB
from test_gpu_yuv420 import EQ, Side
from test_gpu_nv12_to_bgr import BgrOut
from test_gpu_nv12_to_bgr_geometry import ONEPASS_SHAPES, K
from test_gpu_yuv420_to_bgr import ORDERS, ONE, TWO, VEC, BYTES, check

pytestmark = pytest.mark.gpu
TERMS16 = ("y", "y_pitch", "frame_stride", "out", "out_pitch", "out_frame")
TERMS8 = ("c0", "c1", "c_pitch")


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


def layout_terms(w, h, fmt, si, di):
    """The nine values the alignment rule looks at, relative to the (16-byte aligned) allocations, from the keyword arguments of Side
    (si; fmt "i420" or "yv12") and BgrOut (di) alone."""
    yp, cp = si.get("y_pitch") or w, si.get("c_pitch") or w // 2
    a = yp * h + si.get("gap0", 0)
    b = a + cp * (h // 2) + si.get("gap1", 0)
    off = si.get("off", 0)
    u, v = (a, b) if fmt == "i420" else (b, a)
    op = di.get("pitch") or 3 * w
    return {"y": off, "c0": off + u, "c1": off + v, "y_pitch": yp, "c_pitch": cp, "frame_stride": b + cp * (h // 2) + si.get("frame_gap", 0),
            "out": di.get("off", 0), "out_pitch": op, "out_frame": op * h + di.get("frame_gap", 0)}


def misaligned(terms):
    """the terms that break the rule: multiples of 16 for the Y and output side, of 8 for the chroma"""
    assert set(terms) == set(TERMS16 + TERMS8)
    return sorted([k for k in TERMS16 if terms[k] % 16] + [k for k in TERMS8 if terms[k] % 8])


def build(w, h, n, fmt, si, di):
    """The two allocations of a layout; what layout_terms said about it holds for the real addresses."""
    src, dst = Side(w, h, n, fmt, **si), BgrOut(w, h, n, **di)
    p = src.planes()
    real = {"y": p.y - src.base, "c0": p.c0 - src.base, "c1": p.c1 - src.base, "y_pitch": p.y_pitch, "c_pitch": p.c_pitch,
            "frame_stride": p.frame_stride, "out": dst.ptr - dst.buf.data_ptr(), "out_pitch": dst.pitch, "out_frame": dst.fstride}
    assert real == layout_terms(w, h, fmt, si, di), real
    assert src.base % 16 == 0 and dst.buf.data_ptr() % 16 == 0
    return src, dst


# ---- 2. the multiples-of-8 rule --------------------------------------------------------------------------------------------------
# 64 x 32: the Y plane is 2048 bytes and a tight chroma plane 512, so the gaps below say directly what each plane's address is
CHROMA8 = dict(c_pitch=40, gap0=8, gap1=0, frame_gap=8)           # c0 = 2056, c1 = 2696, c_pitch = 40: multiples of 8, none of 16
ONE_TERM = [
    # the term, by how much, Side layout, BgrOut layout
    ("y", 8, dict(off=8), {}),                                    # the chroma planes follow it to multiples of 8
    ("y", 1, dict(off=1, gap0=7, frame_gap=9), {}),
    ("c0", 4, dict(gap0=4, gap1=4, frame_gap=8), {}),
    ("c1", 4, dict(gap1=4, frame_gap=12), {}),
    ("out", 1, {}, dict(off=1)),
    ("out", 8, {}, dict(off=8)),
    ("y_pitch", 8, dict(y_pitch=72), {}),
    ("c_pitch", 4, dict(c_pitch=36), {}),
    ("out_pitch", 1, {}, dict(pitch=193)),
    ("frame_stride", 8, dict(frame_gap=8), {}),
    ("out_frame", 1, {}, dict(frame_gap=1)),
    ("out_frame", 8, {}, dict(frame_gap=8)),
]


def test_every_term_aligned_is_onepass_and_vector(c):
    """The control of the cases below, with every term a multiple of 16 and with the chroma terms multiples of 8 only."""
    w, h, n = 64, 32, 2
    for fmt in ("i420", "yv12"):
        assert not misaligned(layout_terms(w, h, fmt, {}, {}))
        t = layout_terms(w, h, fmt, CHROMA8, {})
        assert not misaligned(t) and all(t[k] % 16 == 8 for k in TERMS8) and all(t[k] % 16 == 0 for k in TERMS16)
        for si in ({}, CHROMA8):
            src, dst = build(w, h, n, fmt, si, {})
            check(c, w, h, n, 301, ("clahe", (2.0, 4, 2)), ORDER_BGR, src, dst, (ONE, VEC))
            check(c, w, h, n, 301, EQ, ORDER_RGB, src, dst, (ONE, VEC))


@pytest.mark.parametrize("term,by,si,di", ONE_TERM, ids=[f"{t[0]}+{t[1]}" for t in ONE_TERM])
def test_one_alignment_term_at_a_time(c, term, by, si, di):
    """64 x 32, CLAHE 4 x 2, two frames is one-pass on the vector path when the rule holds.  Each layout keeps eight of the nine terms
    and breaks the ninth -- a chroma term by 4, another by 1 or 8: CLAHE takes the fallback, both ops write pixels on the byte path."""
    w, h, n = 64, 32, 2
    t = layout_terms(w, h, "i420", si, di)
    assert misaligned(t) == [term] and t[term] % (8 if term in TERMS8 else 16) == by
    src, dst = build(w, h, n, "i420", si, di)
    check(c, w, h, n, 301, ("clahe", (2.0, 4, 2)), ORDER_BGR, src, dst, (TWO, BYTES))
    check(c, w, h, n, 301, EQ, ORDER_RGB, src, dst, (ONE, BYTES))


# ---- 3. loops past their first step ----------------------------------------------------------------------------------------------
# 112 x 160: Y rows at 128, chroma rows at 72 (a multiple of 8, not of 16); 40 bytes behind the Y plane put U, and V 5760 bytes behind
# it, 8 past a 16-byte boundary in every frame (the frame stride is a multiple of 16)
PITCHED_112 = (dict(y_pitch=128, c_pitch=72, gap0=40, gap1=0, frame_gap=24, off=16), dict(pitch=352, frame_gap=64, off=32))
ODD_66 = (dict(y_pitch=67, c_pitch=35, gap0=3, gap1=5, frame_gap=5, off=1), dict(pitch=201, frame_gap=7, off=1))
LOOP_SHAPES = [
    # id, W, H, n, Side layout, BgrOut layout, vector path  (stride, dby and dgx as in the NV12 geometry test's table)
    ("96x144-tight", 96, 144, 1, {}, {}, True),                    # B = 1, stride 256; gx_n 6, groups 432: the wrap fires, the second step is partial
    ("96x144-three-frames", 96, 144, 3, {}, {}, True),             # the same walk in every frame, last-to-first
    ("112x160-pitched", 112, 160, 2, *PITCHED_112, True),          # B = 2, stride 512; gx_n 7, groups 560, dby 73, dgx 1
    ("8192x4", 8192, 4, 1, {}, {}, True),                          # B = 2, stride 512; gx_n 512: every lane steps straight down one row pair
    ("4112x8", 4112, 8, 1, {}, {}, True),                          # B = 4, stride 1024; gx_n 257, dby 3, dgx 253; c_pitch 2056 is 8 mod 16
    ("66x34-odd", 66, 34, 2, *ODD_66, False),                      # byte path: 561 blocks for 256 lanes, three steps
    ("96x144-c1+4", 96, 144, 1, dict(gap1=4, frame_gap=12), {}, False),   # W % 16 == 0 and one chroma term off by 4: 3456 blocks, B = 1
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,w,h,n,si,di,vec", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_equalize_loops_past_first_step(c, name, w, h, n, si, di, vec, order):
    """equalizeHist: yuv420_to_bgr_kernel<ORDER, true> where a lane owns more than one group / block."""
    fmt = "i420" if order == ORDER_BGR else "yv12"
    t = layout_terms(w, h, fmt, si, di)
    assert (w % 16 == 0 and not misaligned(t)) == vec
    if name == "112x160-pitched":
        assert t["c0"] % 16 == 8 and t["c1"] % 16 == 8 and t["frame_stride"] % 16 == 0 and t["c_pitch"] == 72
    if name == "96x144-c1+4":
        assert misaligned(layout_terms(w, h, "i420", si, di)) == ["c1"]
    bound = max(1, w * h * 9 // 4 // 16384)
    assert (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2), "the shape would not loop"
    src, dst = build(w, h, n, fmt, si, di)
    check(c, w, h, n, 101, EQ, order, src, dst, (ONE, VEC if vec else BYTES))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("di,vec", [({}, True), (dict(off=1), False)], ids=["vector", "byte"])
def test_decode_only_loops_past_first_step(c, di, vec, order):
    """yuv420_to_bgr_kernel<ORDER, false>, the second pass of the CLAHE fallback, at 96 x 144: 144 % 5 != 0, so a 4 x 5 grid pads by
    REFLECT_101 and the call goes two-pass.  Aligned: the luma comes from 16-byte aligned tight scratch planes and the decode is the
    vector walk of 96x144-tight (first-to-last frame order); output base + 1: the byte walk."""
    w, h, n = 96, 144, 2
    src, dst = build(w, h, n, "i420", {}, di)
    check(c, w, h, n, 102, ("clahe", (2.0, 4, 5)), order, src, dst, (TWO, VEC if vec else BYTES))


# ---- 4. CLAHE one-pass geometry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("w,h,tx,ty,clip,want", ONEPASS_SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}x{s[3]}-clip{s[4]:g}" for s in ONEPASS_SHAPES])
def test_clahe_onepass_geometry(c, w, h, tx, ty, clip, want, order):
    """The shapes of the NV12 geometry test (straddling row pairs, three groups per tile, two column segments, the largest pair table
    tiles_x + 1 == kMaxPairsLdsF32 and one tile wider, which goes two-pass) on tight I420 / YV12 frames: every one satisfies the rule
    (several with chroma terms that are multiples of 8 only), so the NV12 form's counters are the expected ones."""
    n = 2
    fmt = "i420" if order == ORDER_BGR else "yv12"
    assert not misaligned(layout_terms(w, h, fmt, {}, {}))
    assert [s for s in ONEPASS_SHAPES if s[5] == TWO] == [(16 * K, 12, K, 2, 2.0, TWO)]
    src, dst = build(w, h, n, fmt, {}, {})
    check(c, w, h, n, 201, ("clahe", (clip, tx, ty)), order, src, dst, (want, VEC))


@pytest.mark.parametrize("order", ORDERS)
def test_clahe_onepass_pitched_with_guards(c, order):
    """48 x 30, 3 x 2 (odd tile height, three groups) with every pitch larger than its row, chroma terms 8 past a 16-byte boundary:
    the pitch padding, the plane gaps and the frame gaps keep their pattern."""
    w, h, n = 48, 30, 2
    si, di = dict(y_pitch=64, c_pitch=40, gap0=24, gap1=8, frame_gap=16, off=16), dict(pitch=160, frame_gap=64, off=16)
    t = layout_terms(w, h, "i420", si, di)
    assert not misaligned(t) and all(t[k] % 16 == 8 for k in TERMS8)
    src, dst = build(w, h, n, "i420", si, di)
    check(c, w, h, n, 202, ("clahe", (2.0, 3, 2)), order, src, dst, (ONE, VEC))


# ---- 11. seeded random sweep -----------------------------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 2, 48


def draw_case(rng):
    """One case in the manner of the NV12 geometry test: W even in [2, 256] (about half of them multiples of 16), H even in [2, 64],
    1..3 frames, the op, a tile grid in [1, 16] x [1, 5], a clip limit, the order, I420 or YV12 and a layout.  Most CLAHE cases with
    W % 16 == 0 get a frame their grid divides into tiles of a multiple of 16 columns; three quarters of the layouts satisfy the rule,
    with chroma terms that are any multiple of 8."""
    kind = "clahe" if rng.random() < 0.55 else "eq"
    tx, ty = int(rng.integers(1, 17)), int(rng.integers(1, 6))
    clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
    n, order = int(rng.integers(1, 4)), int(rng.integers(0, 2))
    fmt = "i420" if rng.random() < 0.5 else "yv12"
    w, h = 2 * int(rng.integers(1, 129)), 2 * int(rng.integers(1, 33))
    if rng.random() < 0.5:
        w = 16 * int(rng.integers(1, 17))
        if kind == "clahe" and rng.random() < 0.85:
            w = 16 * tx * int(rng.integers(1, 16 // tx + 1))
            m = 2 * ty // math.gcd(2, ty)
            h = m * int(rng.integers(1, 64 // m + 1))
    if rng.random() < 0.75:
        yp = (w + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
        cp = (w // 2 + 7) // 8 * 8 + 8 * int(rng.integers(0, 3))
        si = dict(y_pitch=yp, c_pitch=cp, off=16 * int(rng.integers(0, 3)))
        si["gap0"] = (-(yp * h)) % 8 + 8 * int(rng.integers(0, 4))
        si["gap1"] = (-(cp * (h // 2))) % 8 + 8 * int(rng.integers(0, 4))
        si["frame_gap"] = (-layout_terms(w, h, fmt, si, {})["frame_stride"]) % 16 + 16 * int(rng.integers(0, 3))
        di = dict(pitch=(3 * w + 15) // 16 * 16 + 16 * int(rng.integers(0, 3)), frame_gap=16 * int(rng.integers(0, 3)),
                  off=16 * int(rng.integers(0, 3)))
    else:
        si = dict(y_pitch=w + int(rng.integers(0, 40)), c_pitch=w // 2 + int(rng.integers(0, 40)), gap0=int(rng.integers(0, 40)),
                  gap1=int(rng.integers(0, 40)), frame_gap=int(rng.integers(0, 40)), off=int(rng.integers(0, 40)))
        di = dict(pitch=3 * w + int(rng.integers(0, 40)), frame_gap=int(rng.integers(0, 40)), off=int(rng.integers(0, 40)))
    return dict(kind=kind, w=w, h=h, n=n, tx=tx, ty=ty, clip=clip, order=order, fmt=fmt, si=si, di=di)


def classify(case, max_pairs):
    """The documented conditions (include/mi_lumaeq.h), restated: the class of a case and its counter deltas.  clahe_fp_contract is off
    in this module's context."""
    w, h, tx, ty = case["w"], case["h"], case["tx"], case["ty"]
    vec = w % 16 == 0 and not misaligned(layout_terms(w, h, case["fmt"], case["si"], case["di"]))
    walk = VEC if vec else BYTES
    if case["kind"] == "eq":
        return ("eq-vector" if vec else "eq-byte"), (ONE, walk)
    onepass = w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= max_pairs and vec
    return ("clahe-onepass", (ONE, VEC)) if onepass else ("clahe-twopass", (TWO, walk))


def sweep_cases(seed=SWEEP_SEED):
    rng = np.random.default_rng(seed)
    return [draw_case(rng) for _ in range(SWEEP_CASES)]


def class_counts(cases):
    classes = [classify(k, K)[0] for k in cases]
    return {name: classes.count(name) for name in ("eq-vector", "eq-byte", "clahe-onepass", "clahe-twopass")}


def test_seeded_random_sweep(c):
    cases = sweep_cases()
    count = class_counts(cases)
    assert len(cases) == 48 and min(count.values()) >= 8, count
    assert {k["order"] for k in cases} == {ORDER_BGR, ORDER_RGB} and {k["fmt"] for k in cases} == {"i420", "yv12"}
    c.set_option("clahe_fp_contract", 0)
    for i, k in enumerate(cases):
        w, h, n = k["w"], k["h"], k["n"]
        assert w % 2 == 0 and h % 2 == 0 and 2 <= w <= 256 and 2 <= h <= 64 and 1 <= n <= 3
        src, dst = build(w, h, n, k["fmt"], k["si"], k["di"])
        op = EQ if k["kind"] == "eq" else ("clahe", (k["clip"], k["tx"], k["ty"]))
        check(c, w, h, n, 400 + i, op, k["order"], src, dst, classify(k, K)[1])
