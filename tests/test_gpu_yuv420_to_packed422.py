"""4:2:0 frames (NV12 / I420 / YV12) in, pitched packed 4:2:2 frames (YUY2 / UYVY) out on the GPU:
mi_equalize_hist_yuv420_to_packed422_batch_dev, mi_clahe_yuv420_to_packed422_batch_dev and their host forms.  Expected bytes
(yuv420_packed422_ref.expected): the Y plane mapped by oracle.equalize_hist / oracle.clahe, input chroma row r under output rows 2r and
2r+1 (MI_UV_COPY) or 128 (MI_UV_FILL128), interleaved by format; tests/test_yuv420_to_packed422_abi.py backs the builder on the CPU.
Planes hold full-range random bytes, U and V drawn independently, so a swapped U / V, a shifted chroma row or an identity map cannot
pass.  Every side of a call lives in a sentinel-filled allocation with 64 guard bytes and the WHOLE allocation is compared, input and
output: every comparison in this file is exact.  After every call the test asserts which of the four counters moved, by the header's
rules restated in yuv420_packed422_ref.misaligned / onepass_clahe.

How many workgroups yuv420_to_packed422_kernel gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by it.  launch_yuv420_to_packed422 takes
B = min(blocks_per_frame(W*H*7/4 bytes, H/2 rows, n, 2048), ceil(items / 256)), and blocks_per_frame never returns more than
max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows -- whatever the CU count, which only lowers it.  So
B <= max(1, floor(W*H*7/4 / 16384)),  B <= H/2, and the 256 lanes of a workgroup step through the frame by stride = 256 * B items:
16 x 2 pixel groups on the vector path (gx_n = W/16 per row pair, the carried walk by += dby, gx += dgx with a wrap when gx >= gx_n),
2 x 2 blocks on the byte path."""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import xfer, UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY
from yuv420_packed422_ref import (SENT, COUNTERS, SRC_FMTS, P422Out, Side, content, expected, expected_frame, misaligned, onepass_clahe, _ref)

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
FMTS = [FMT_YUY2, FMT_UYVY]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)
OTHER_STATS = ("fused_fallbacks", "fused_frames_repaired", "fused_hard_errors", "fused_demotions", "nv12_bgr_onepass", "nv12_bgr_twopass",
               "yuv420_bgr_onepass", "yuv420_bgr_twopass", "yuv420_bgr_vec", "yuv420_bgr_bytes", "yuv420_chroma_vec", "yuv420_chroma_bytes",
               "bgr_packed422_vec", "bgr_packed422_bytes")


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in COUNTERS)


def delta(before, after):
    return tuple(a - b for a, b in zip(after, before))


def want_counters(op, src, dst, uv_mode, contract=False):
    """(onepass, twopass, vec, bytes) one call with work to do must move, by the header's rules."""
    vec = not misaligned(src, dst, uv_mode)
    one = op[0] == "eq" or onepass_clahe(src, dst, op[1], uv_mode, contract)
    return (int(one), int(not one), int(vec), int(not vec))


def run(c, op, src, dst, fmt, uv_mode, n=None, st=None, planes=None):
    kind, cfg = op
    a = planes or (src.planes() if uv_mode == UV_COPY else src.planes(c0=None, c1=None, c_pitch=0))
    kw = dict(dst.kw(), stream=stream() if st is None else st)
    n = src.n if n is None else n
    if kind == "eq":
        c.equalize_hist_yuv420_to_packed422_batch_dev(a, dst.ptr, src.w, src.h, n, fmt, uv_mode, **kw)
    else:
        c.clahe_yuv420_to_packed422_batch_dev(a, dst.ptr, src.w, src.h, n, fmt, uv_mode, *cfg, **kw)


def check(c, w, h, n, seed, op, fmt, uv_mode, src, dst, contract=False):
    """One call on the uploaded content: the whole output allocation is the reference's image of it, the whole input allocation is
    what was uploaded, and exactly one counter of each pair moved -- the one the header's rule names.  Under MI_UV_FILL128 the
    descriptor carries NULL chroma pointers."""
    frames = content(w, h, n, seed)
    src.upload(frames)
    dst.clear()
    before = counters(c)
    run(c, op, src, dst, fmt, uv_mode)
    torch.cuda.synchronize()
    ok, nbad, where = dst.same(expected(w, h, n, seed, op, fmt, uv_mode, contract))
    assert ok, (w, h, src.fmt, op, fmt, uv_mode, nbad, where)
    assert np.array_equal(src.host(), src.image(frames)), "the input allocation was written"
    want = want_counters(op, src, dst, uv_mode, contract)
    assert delta(before, counters(c)) == want, (src.fmt, op, fmt, uv_mode, before, counters(c), want)
    return want


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small batches leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    _ref.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. smallest frames ----------------------------------------------------------------------------------------------------------
SMALLEST = [
    # W, H, the CLAHE grids, (onepass, twopass, vec, bytes) of equalizeHist and of the first grid
    (2, 2, [(2.0, 1, 1)], (1, 0, 0, 1), (0, 1, 0, 1)),                  # one 2 x 2 block, byte path; no grid gives 16-column tiles: two-pass
    (16, 2, [(2.0, 1, 1)], (1, 0, 1, 0), (1, 0, 1, 0)),                 # one 16 x 2 group; I420: U and V are 8 bytes each, V at 8 mod 16; 1 x 1 one-pass
    (18, 4, [(2.0, 1, 2), (2.0, 2, 1)], (1, 0, 0, 1), (0, 1, 0, 1)),    # W % 4 == 2: ragged rows, byte path
    (48, 6, [(2.0, 3, 3), (2.0, 2, 2)], (1, 0, 1, 0), (1, 0, 1, 0)),    # gx_n = 3; 3 x 3: tile 16 x 2, one-pass; 2 x 2: tile_w 24, two-pass
]


@pytest.mark.parametrize("src_fmt", SRC_FMTS)
@pytest.mark.parametrize("w,h,grids,want_eq,want_cl", SMALLEST, ids=[f"{s[0]}x{s[1]}" for s in SMALLEST])
def test_smallest_frames(c, w, h, grids, want_eq, want_cl, src_fmt):
    n = 3
    src, dst = Side(w, h, n, src_fmt), P422Out(w, h, n)
    for fmt in FMTS:
        for uv_mode in UV_MODES:
            assert check(c, w, h, n, 51, EQ, fmt, uv_mode, src, dst) == want_eq
            for k, cfg in enumerate(grids):
                got = check(c, w, h, n, 51, ("clahe", cfg), fmt, uv_mode, src, dst)
                assert k or got == want_cl, (cfg, got)


# ---- 2. parity matrix on pitched layouts -----------------------------------------------------------------------------------------
def layouts(w, h, planar):
    """tight; pitches that are multiples of 16; pitch + 4 at an offset of 4; gaps between planes and frames (multiples of 16)."""
    r = w // 2 if planar else w
    up = lambda v: (v + 31) & ~15  # noqa: E731
    return {
        "tight": ({}, {}),
        "pitch16": (dict(y_pitch=up(w), c_pitch=up(r)), dict(pitch=up(2 * w))),
        "pitch+4": (dict(y_pitch=w + 4, c_pitch=r + 4, off=4), dict(pitch=2 * w + 4, off=4)),
        "gaps": (dict(gap0=32, gap1=16, frame_gap=48, off=16), dict(frame_gap=32, off=16)),
    }


PARITY_OPS_64 = [EQ, ("clahe", (2.0, 4, 4)), ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 3, 5)), ("clahe", (2.0, 1, 1))]
PARITY_OPS_66 = [EQ, ("clahe", (2.0, 3, 2)), ("clahe", (2.0, 2, 2))]


@pytest.mark.parametrize("src_fmt", SRC_FMTS)
@pytest.mark.parametrize("layout", ["tight", "pitch16", "pitch+4", "gaps"])
@pytest.mark.parametrize("w,h,ops", [(64, 32, PARITY_OPS_64), (66, 34, PARITY_OPS_66)], ids=["64x32", "66x34"])
def test_parity_matrix(c, w, h, ops, layout, src_fmt):
    """64 x 32 with the grids 4 x 4 (tile 16 x 8), 2 x 2 and 1 x 1 (one-pass on aligned layouts), 3 x 5 (REFLECT_101: two-pass); 66 x 34:
    the byte path, two-pass by width.  Both formats; the UV mode alternates with the format so that every op meets both."""
    n = 2
    si, do = layouts(w, h, src_fmt != "nv12")[layout]
    src, dst = Side(w, h, n, src_fmt, **si), P422Out(w, h, n, **do)
    seen = set()
    for k, op in enumerate(ops):
        for fmt in FMTS:
            uv_mode = UV_MODES[(k + fmt) % 2]
            seen.add(check(c, w, h, n, 52, op, fmt, uv_mode, src, dst))
    if w == 64 and layout in ("tight", "pitch16", "gaps"):
        assert seen == {(1, 0, 1, 0), (0, 1, 1, 0)}, seen             # one-pass and two-pass (3 x 5), all on the groups
    else:
        assert seen == {(1, 0, 0, 1), (0, 1, 0, 1)}, seen             # equalizeHist is one pass; every CLAHE falls back; all on bytes


@pytest.mark.parametrize("src_fmt", ["nv12", "i420"])
def test_clahe_fp_contract_goes_two_pass(src_fmt):
    """The option sends a one-pass shape through the planar CLAHE's FMA bodies and the pack alone; it is restored afterwards."""
    w, h, n = 64, 32, 2
    src, dst = Side(w, h, n, src_fmt), P422Out(w, h, n)
    with mi_lumaeq.Context(0) as c:
        c.set_option("clahe_fp_contract", 1)
        try:
            for fmt, uv_mode in ((FMT_YUY2, UV_COPY), (FMT_UYVY, UV_FILL128)):
                assert check(c, w, h, n, 53, ("clahe", (2.0, 4, 4)), fmt, uv_mode, src, dst, contract=True) == (0, 1, 1, 0)
        finally:
            c.set_option("clahe_fp_contract", 0)
        assert check(c, w, h, n, 53, ("clahe", (2.0, 4, 4)), FMT_YUY2, UV_COPY, src, dst) == (1, 0, 1, 0)


# ---- 3. one alignment term at a time ---------------------------------------------------------------------------------------------
# 64 x 8 x 2 frames.  nv12 tight: Y 512, UV 256, frame 768; i420 tight: Y 512, U 128, V 128, frame 768; out tight: pitch 128, frame 1024
ONE_TERM = [
    # the broken term (None: every term holds), source format, Side layout, P422Out layout
    (None, "nv12", {}, {}),
    ("y", "nv12", dict(off=8, gap0=8, frame_gap=8), {}),                        # y 8; c0 528; frame 784
    ("y_pitch", "nv12", dict(y_pitch=72), {}),                                  # c0 576; frame 832
    ("c0", "nv12", dict(gap0=8, frame_gap=8), {}),                              # c0 520; frame 784
    ("c_pitch", "nv12", dict(c_pitch=72), {}),                                  # frame 512 + 288 = 800
    ("frame_stride", "nv12", dict(frame_gap=8), {}),                            # 776
    ("out", "nv12", {}, dict(off=4)),
    ("out_pitch", "nv12", {}, dict(pitch=136)),                                 # 136 = 8 (mod 16); frame 1088
    ("out_frame", "nv12", {}, dict(frame_gap=4)),
    (None, "i420", {}, {}),
    (None, "i420", dict(gap0=8, frame_gap=8), {}),                              # c0 520, c1 648: both at 8 mod 16 -- still the groups
    ("y", "i420", dict(off=4, gap0=4, frame_gap=12), {}),                       # y 4; c0 520; c1 648; frame 784
    ("y_pitch", "i420", dict(y_pitch=72), {}),                                  # c0 576; c1 704; frame 832
    ("c0", "i420", dict(gap0=4, gap1=4, frame_gap=8), {}),                      # c0 516; c1 648; frame 784
    ("c1", "i420", dict(gap1=4, frame_gap=12), {}),                             # c1 644; frame 784
    ("c_pitch", "i420", dict(c_pitch=36), {}),                                  # U 144; c1 656; frame 800
    ("frame_stride", "i420", dict(frame_gap=8), {}),
    ("out", "i420", {}, dict(off=8)),
    (None, "yv12", dict(gap0=8, frame_gap=8), {}),                              # V first: c1 520, c0 648
    ("c0", "yv12", dict(gap1=4, frame_gap=12), {}),                             # the U plane is the second one
]


@pytest.mark.parametrize("term,src_fmt,si,do", ONE_TERM, ids=[f"{t[1]}-{t[0]}-{k}" for k, t in enumerate(ONE_TERM)])
def test_one_alignment_term_at_a_time(c, term, src_fmt, si, do):
    """Exactly one term misses its multiple (16; 8 for the planar chroma terms), the output terms at 4 or 8 mod 16 as the packed forms'
    rule of multiples of 4 allows: the byte walk, the same bytes, the same untouched guards, "_bytes" moves instead of "_vec" and a
    one-pass CLAHE shape goes two-pass.  None does: the groups, and planar chroma planes at 8 mod 16 stay on them."""
    w, h, n = 64, 8, 2
    src, dst = Side(w, h, n, src_fmt, **si), P422Out(w, h, n, **do)
    assert misaligned(src, dst) == ([term] if term else []), misaligned(src, dst)
    want = (1, 0, 1, 0) if term is None else (1, 0, 0, 1)
    assert check(c, w, h, n, 54, EQ, FMT_YUY2, UV_COPY, src, dst) == want
    want = (1, 0, 1, 0) if term is None else (0, 1, 0, 1)
    assert check(c, w, h, n, 54, ("clahe", (2.0, 2, 2)), FMT_UYVY, UV_COPY, src, dst) == want


# ---- 4. loops past their first step ----------------------------------------------------------------------------------------------
LOOP_SHAPES = [
    # id, W, H, n, source format, Side layout, P422Out layout
    # bytes/16384 = 1.4: B = 1, stride 256; gx_n 4, 400 groups: a full and a partial second step
    ("64x200-nv12", 64, 200, 2, "nv12", {}, {}),
    ("64x200-i420", 64, 200, 2, "i420", {}, {}),
    # bytes/16384 = 1.75: B = 1, stride 256; gx_n 257, 514 groups: two full steps, two lanes take a third, and the walk wraps
    ("4112x4-nv12", 4112, 4, 1, "nv12", {}, {}),
    # byte path: 3200 blocks of 2 x 2, B = 1: twelve full steps and a half one
    ("64x200-out+4", 64, 200, 1, "yv12", {}, dict(off=4)),
    # byte path, nothing aligned: 33 x 17 = 561 blocks, B = 1: three steps
    ("66x34-odd", 66, 34, 2, "nv12", dict(y_pitch=67, c_pitch=69, gap0=3, frame_gap=5, off=1), dict(pitch=136, frame_gap=12, off=4)),
]


@pytest.mark.parametrize("name,w,h,n,src_fmt,si,do", LOOP_SHAPES, ids=[s[0] for s in LOOP_SHAPES])
def test_loops_past_their_first_step(c, name, w, h, n, src_fmt, si, do):
    """yuv420_to_packed422_kernel where a lane owns more than one group / block: with the LUT (equalizeHist) and without it (the pack
    alone behind the two-pass CLAHE: a 3 x 3 grid divides none of the heights)."""
    src, dst = Side(w, h, n, src_fmt, **si), P422Out(w, h, n, **do)
    vec = not misaligned(src, dst)
    bound = max(1, w * h * 7 // 4 // 16384)
    assert (w * h // 32 if vec else w * h // 4) > 256 * min(bound, h // 2), "the shape would not loop"
    assert check(c, w, h, n, 55, EQ, FMT_YUY2, UV_COPY, src, dst)[:2] == (1, 0)
    assert check(c, w, h, n, 55, ("clahe", (2.0, 3, 3)), FMT_UYVY, UV_COPY, src, dst)[:2] == (0, 1)


INTERP_SHAPES = [
    # W, H, tiles_x, tiles_y
    (4112, 4, 1, 2),          # 257 groups of 16 columns: two column segments, the second of one group; tile_h 2, three bands
    (64, 64, 2, 2),           # tile_h 32: (32 + 2 * kBandMargin) / 8 = 5 sub-bands a band are allowed, and a single frame asks for them
    (32, 20, 2, 2),           # tile 16 x 10: band 1 starts at row 5, the row pair (4, 5) lies in two bands: each row loads chroma row 2
    (224, 12, 14, 2),         # the largest pair table: tiles_x + 1 == kMaxPairsLdsF32, 60 KiB of dynamic LDS
    (240, 12, 15, 2),         # one tile wider: the fallback takes over
]


@pytest.mark.parametrize("src_fmt", ["nv12", "i420"])
@pytest.mark.parametrize("w,h,tx,ty", INTERP_SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}x{s[3]}" for s in INTERP_SHAPES])
def test_interpolation_kernel_geometry(c, w, h, tx, ty, src_fmt):
    """yuv420_packed422_clahe_interp_kernel where its column segments, sub-bands and pair tables repeat."""
    n = 1
    src, dst = Side(w, h, n, src_fmt), P422Out(w, h, n)
    want = (0, 1, 1, 0) if tx == 15 else (1, 0, 1, 0)
    assert check(c, w, h, n, 56, ("clahe", (2.0, tx, ty)), FMT_YUY2, UV_COPY, src, dst) == want
    assert check(c, w, h, n, 56, ("clahe", (2.0, tx, ty)), FMT_UYVY, UV_FILL128, src, dst) == want


# ---- 5. histogram isolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 3, 3)), ("clahe", (2.0, 2, 2))], ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_histograms_do_not_leak_across_frames(c, op):
    """n = 5 frames of different content equal five n = 1 calls, byte for byte (and the reference)."""
    w, h, n = 48, 6, 5
    frames = content(w, h, n, 57)
    src, dst = Side(w, h, n, "i420"), P422Out(w, h, n)
    check(c, w, h, n, 57, op, FMT_YUY2, UV_COPY, src, dst)
    batch = dst.host()
    one_src, one_dst = Side(w, h, 1, "i420"), P422Out(w, h, 1)
    for k in range(n):
        one_src.upload([frames[k]])
        one_dst.clear()
        run(c, op, one_src, one_dst, FMT_YUY2, UV_COPY)
        torch.cuda.synchronize()
        single = one_dst.host()[: dst.fstride]
        assert np.array_equal(single, batch[k * dst.fstride: (k + 1) * dst.fstride]), (op, k)


# ---- 6. composition with the library's own pieces --------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 4)), ("clahe", (2.0, 3, 5))], ids=["eq", "clahe-onepass", "clahe-twopass"])
def test_composition_with_the_librarys_own_pieces(c, op):
    """The luma bytes equal mi_*_u8_batch_dev on the Y planes; an INTERLEAVED and a PLANAR input holding the same samples give
    identical frames; YV12 equals I420 with the addresses exchanged."""
    w, h, n = 64, 32, 3
    frames = content(w, h, n, 58)
    outs = {}
    for src_fmt in SRC_FMTS:
        src, dst = Side(w, h, n, src_fmt).upload(frames), P422Out(w, h, n)
        run(c, op, src, dst, FMT_YUY2, UV_COPY)
        torch.cuda.synchronize()
        outs[src_fmt] = dst.host()
    assert np.array_equal(outs["nv12"], outs["i420"]) and np.array_equal(outs["i420"], outs["yv12"])
    # a YV12 frame laid out by hand: an I420 allocation whose first chroma plane holds V and whose second holds U, with c0 and c1 exchanged
    src, dst = Side(w, h, n, "i420").upload([(y, v, u) for y, u, v in frames]), P422Out(w, h, n)
    _, first, second = src.offsets()
    run(c, op, src, dst, FMT_YUY2, UV_COPY, planes=src.planes(c0=src.base + second, c1=src.base + first))
    torch.cuda.synchronize()
    assert np.array_equal(dst.host(), outs["i420"])
    # the luma: the planar form on the Y planes
    d_y = xfer.to_device(np.stack([f[0] for f in frames]))
    d_m = torch.full_like(d_y, SENT)
    if op is EQ:
        c.equalize_hist_batch_dev(d_y, d_m, w, h, n, stream=stream())
    else:
        c.clahe_batch_dev(d_y, d_m, w, h, n, *op[1], stream=stream())
    torch.cuda.synchronize()
    got = outs["nv12"][: n * 2 * w * h].reshape(n, h, 2 * w)
    assert np.array_equal(got[:, :, 0::2], xfer.to_host(d_m).reshape(n, h, w)), op
    assert not np.array_equal(got[:, :, 0::2], np.stack([f[0] for f in frames])), "the luma was not mapped"


# ---- 7. chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,src_fmt", [(2, 2, "nv12"), (16, 2, "i420")], ids=["2x2-nv12", "16x2-i420"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 1, 1))], ids=["eq", "clahe-1x1"])
def test_chunking(c, op, w, h, src_fmt):
    """Two frames past the chunk of 256: two launch sequences, the second of two frames; every frame distinct, every frame checked."""
    n = 258
    check(c, w, h, n, 59, op, FMT_UYVY, UV_COPY, Side(w, h, n, src_fmt), P422Out(w, h, n))


# ---- 8. launch contract ----------------------------------------------------------------------------------------------------------
def launches(c):
    return {k: v["launches"] for k, v in c.profile_read(reset=False).items()}


@pytest.mark.parametrize("src_fmt", ["nv12", "i420"])
def test_launch_contract(src_fmt):
    """equalizeHist: one MI_K_HIST, one MI_K_EQ_LUT and one MI_K_LUT_APPLY launch per chunk, for either uv_mode, and nothing else.
    One-pass CLAHE: what mi_clahe_u8_batch_dev launches for the Y planes (its interpolation replaced one for one by the new kernel in
    the same slot) and no MI_K_COLOR; two-pass CLAHE: the same plus one MI_K_COLOR per chunk.  Fused and sibling counters untouched."""
    w, h = 64, 32
    with mi_lumaeq.Context(0) as c:
        before = {k: c.get_stat(k) for k in OTHER_STATS}
        c.set_profiling(1)
        for n, chunks in ((2, 1), (258, 2)):
            src, dst = Side(w, h, n, src_fmt), P422Out(w, h, n)
            for uv_mode in UV_MODES:
                c.profile_read(reset=True)
                check(c, w, h, n, 60, EQ, FMT_YUY2, uv_mode, src, dst)
                got = launches(c)
                want = {"hist_partial_kernel": chunks, "equalize_lut_kernel": chunks, "lut_apply_kernel": chunks}
                assert len(got) == 10 and got == {k: want.get(k, 0) for k in mi_lumaeq.KERNEL_NAMES}, (n, uv_mode, got)
        n = 2
        src, dst = Side(w, h, n, src_fmt), P422Out(w, h, n)
        d_y = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        for cfg, two in (((2.0, 4, 4), 0), ((2.0, 3, 5), 1)):
            c.profile_read(reset=True)
            c.clahe_batch_dev(d_y, torch.empty_like(d_y), w, h, n, *cfg, stream=stream())
            torch.cuda.synchronize()
            planar = launches(c)
            assert planar["color_kernel"] == 0 and planar["clahe_interp_kernel"] == 1, planar
            c.profile_read(reset=True)
            assert check(c, w, h, n, 60, ("clahe", cfg), FMT_UYVY, UV_COPY, src, dst)[:2] == (1 - two, two)
            got = launches(c)
            assert got == dict(planar, color_kernel=two), (cfg, got, planar)
        c.set_profiling(0)
        assert {k: c.get_stat(k) for k in OTHER_STATS} == before


# ---- 9. errors, zero sizes, busy, hipGraph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_fmt", ["nv12", "i420"])
def test_errors_and_zero_sizes_enqueue_nothing(src_fmt):
    w, h, n = 32, 16, 2
    frames = content(w, h, n, 61)
    src = Side(w, h, n, src_fmt, y_pitch=48, c_pitch=40, frame_gap=16).upload(frames)
    dst = P422Out(w, h, n, pitch=80, frame_gap=16)
    good = src.planes()
    row = src.row
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        before = counters(c)
        base = dict(ctx=hd, planes={}, o=dst.ptr, op=dst.pitch, fo=dst.fstride, w=w, h=h, n=n, fmt=FMT_YUY2, uvm=UV_COPY)

        def args(kw):
            a = dict(base)
            a.update(kw)
            p = None if a["planes"] is None else ctypes.byref(src.planes(**a["planes"]))
            return (a["ctx"], p, a["o"], a["op"], a["fo"], a["w"], a["h"], a["n"], a["fmt"], a["uvm"])

        def eq(**kw):
            return L.mi_equalize_hist_yuv420_to_packed422_batch_dev(*args(kw), stream())

        def cl(tx=2, ty=2, **kw):
            return L.mi_clahe_yuv420_to_packed422_batch_dev(*args(kw), 2.0, tx, ty, stream())
        bad = [dict(ctx=None), dict(planes=None), dict(planes=dict(y=None)), dict(planes=dict(c0=None)), dict(o=None),     # null pointers
               dict(planes=dict(chroma=2)), dict(planes=dict(chroma=-1)),
               dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),
               dict(w=-2), dict(h=-2), dict(n=-1),                                            # negative sizes
               dict(w=31), dict(h=15), dict(w=31, h=0), dict(h=15, n=0), dict(h=15, w=0),      # odd sizes, also when another size is 0
               dict(planes=dict(y_pitch=w - 1)), dict(planes=dict(c_pitch=row - 1)), dict(op=2 * w - 4),       # a pitch below its row
               dict(o=dst.ptr + 2), dict(op=dst.pitch + 2), dict(fo=dst.fstride + 2),          # an output term that is no multiple of 4
               dict(o=good.y), dict(o=good.c0)]                                               # no in-place form
        if src.planar:
            bad += [dict(planes=dict(c1=None)), dict(o=good.c1)]
        for kw in bad:
            assert eq(**kw) == BAD_ARG, kw
            assert cl(**kw) == BAD_ARG, kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert cl(tx, ty) == BAD_ARG, (tx, ty)
            assert cl(tx, ty, n=0) == BAD_ARG, (tx, ty)
        for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, o=None, planes=dict(y=None, c0=None))):   # zero sizes: MI_OK, nothing written
            assert eq(**kw) == 0 and cl(**kw) == 0, kw
        # sizes and tile grids the planar forms refuse: their status
        big = dict(w=(1 << 24) + 2, h=2, op=1 << 26, fo=1 << 27, planes=dict(y_pitch=1 << 25, c_pitch=1 << 25, frame_stride=1 << 27))
        planar = L.mi_equalize_hist_u8_batch_dev(hd, dst.ptr, 1 << 25, 1 << 27, dst.ptr, 1 << 25, 1 << 27, big["w"], 2, 1, stream())
        assert planar == UNSUPPORTED and eq(**big) == planar and cl(**big) == planar
        planar = L.mi_clahe_u8_batch_dev(hd, dst.ptr, dst.pitch, dst.fstride, dst.ptr, dst.pitch, dst.fstride, w, h, 1, 2.0, 2048, 1024, stream())
        assert planar == UNSUPPORTED and cl(2048, 1024) == planar
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote"
        assert np.array_equal(src.host(), src.image(frames)), "a refused or empty call wrote the input"
        assert all(v == 0 for v in launches(c).values()), launches(c)
        assert counters(c) == before
        c.set_profiling(0)
        # MI_UV_FILL128 with NULL chroma pointers (and a c_pitch that would be refused) succeeds, and the context still works
        check(c, w, h, n, 61, EQ, FMT_UYVY, UV_FILL128, src, dst)
        check(c, w, h, n, 61, ("clahe", (2.0, 2, 2)), FMT_YUY2, UV_COPY, src, dst)


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    src = Side(w, h, 1, "nv12").upload(content(w, h, 1, 62))
    dst = P422Out(w, h, 1)
    with mi_lumaeq.Context(0) as c:
        before = counters(c)
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 2, 2))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, src, dst, FMT_YUY2, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused call wrote"
        assert counters(c) == before
        check(c, w, h, 1, 62, EQ, FMT_YUY2, UV_COPY, src, dst)                           # and the context still works


def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist, one one-pass and one two-pass CLAHE call captured on a single stream (one
    linear chain, no parallel branches) and two replays onto fresh inputs: the bytes of an eager call."""
    w, h, n = 64, 32, 3
    src = Side(w, h, n, "i420", gap0=32, gap1=16, frame_gap=48, off=16)
    mk = lambda: P422Out(w, h, n, frame_gap=32, off=16)  # noqa: E731
    calls = ((EQ, mk(), FMT_YUY2, UV_COPY), (("clahe", (2.0, 4, 4)), mk(), FMT_UYVY, UV_COPY), (("clahe", (2.0, 3, 5)), mk(), FMT_YUY2, UV_FILL128))
    with mi_lumaeq.Context(0) as c:
        src.upload(content(w, h, n, 63))
        for op, dst, fmt, uv_mode in calls:                                              # the eager calls size the scratch
            dst.clear()
            run(c, op, src, dst, fmt, uv_mode)
            torch.cuda.synchronize()
            assert dst.same(expected(w, h, n, 63, op, fmt, uv_mode))[0], ("eager", op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            for op, dst, fmt, uv_mode in calls:
                run(c, op, src, dst, fmt, uv_mode, st=st)
        for rep in range(2):
            fresh = content(w, h, n, 64 + rep)
            src.upload(fresh)
            for _, dst, _, _ in calls:
                dst.clear()
            g.replay()
            torch.cuda.synchronize()
            for op, dst, fmt, uv_mode in calls:
                assert dst.same(expected(w, h, n, 64 + rep, op, fmt, uv_mode))[0], ("graph replay", op, rep)
            assert np.array_equal(src.host(), src.image(fresh))


# ---- 10. host forms --------------------------------------------------------------------------------------------------------------
def pinned_like(a):
    t = torch.empty(a.size, dtype=torch.uint8).pin_memory()
    v = t.numpy()
    v[:] = a.reshape(-1)
    return t, v


@pytest.mark.parametrize("src_fmt", SRC_FMTS)
@pytest.mark.parametrize("w,h", [(2, 2), (18, 4), (64, 32)])
def test_host_forms(w, h, src_fmt):
    """A pitched host frame with gaps at an offset in, and a tight pinned one; a new tight H x 2W frame out, a caller's padded view at an
    odd address whose padding and guards stay untouched, and a tight pinned frame: both ops, both formats, both UV modes; the source is
    unchanged; the counters name the tight, aligned device copy (W % 16 == 0: the groups; 64 x 32 with a 2 x 2 grid: one pass)."""
    planes = content(w, h, 1, 65)[0]
    pitched = Side(w, h, 1, src_fmt, y_pitch=w + 3, c_pitch=w + 5, gap0=7, gap1=3, off=1, dev=False).upload([planes])
    tight = Side(w, h, 1, src_fmt, dev=False).upload([planes])
    keep, pin = pinned_like(tight.buf[: w * h * 3 // 2])
    opitch = 2 * w + 5
    cl = ("clahe", (2.0, 2, 2) if w == 64 else (2.0, 1, 2))
    with mi_lumaeq.Context(0) as c:
        for op in (EQ, cl):
            for fmt in FMTS:
                for uv_mode in UV_MODES:
                    want = expected_frame(planes, op, fmt, uv_mode)
                    vec = w % 16 == 0
                    one = op is EQ or vec
                    cnt = (int(one), int(not one), int(vec), int(not vec))

                    def call(frame, out=None):
                        before = counters(c)
                        if op is EQ:
                            r = c.equalize_hist_yuv420_to_packed422(frame, w, h, src_fmt, fmt, uv_mode, out=out)
                        else:
                            r = c.clahe_yuv420_to_packed422(frame, w, h, src_fmt, fmt, uv_mode, *op[1], out=out)
                        assert delta(before, counters(c)) == cnt, (op, fmt, uv_mode, before, counters(c))
                        return r
                    a = pitched.planes(frame_stride=12345) if uv_mode == UV_COPY else pitched.planes(c0=None, c1=None, c_pitch=0)
                    got = call(a)
                    assert got.shape == (h, 2 * w) and np.array_equal(got, want), (op, fmt, uv_mode, "pitched in")
                    assert np.array_equal(call(pin), want), (op, fmt, uv_mode, "pinned tight in")
                    buf = np.full(h * opitch + 1 + 64, SENT, np.uint8)
                    oview = buf[1: 1 + h * opitch].reshape(h, opitch)[:, : 2 * w]
                    assert oview.ctypes.data % 2 == 1
                    assert call(tight.buf[: w * h * 3 // 2], out=oview) is oview
                    ref = np.full(buf.size, SENT, np.uint8)
                    ref[1: 1 + h * opitch].reshape(h, opitch)[:, : 2 * w] = want
                    assert np.array_equal(buf, ref), (op, fmt, uv_mode, "padded host view")
                    okeep, opin = pinned_like(np.full(h * 2 * w, SENT, np.uint8))
                    call(pin, out=opin.reshape(h, 2 * w))
                    assert np.array_equal(opin.reshape(h, 2 * w), want), (op, fmt, uv_mode, "pinned tight out")
                    del okeep
        assert np.array_equal(pitched.host(), pitched.image([planes])) and np.array_equal(tight.host(), tight.image([planes]))
        assert np.array_equal(pin, tight.buf[: w * h * 3 // 2]), "the source was written"
        assert c.get_stat("error_drains") == 0
    del keep


def test_host_form_errors():
    w, h = 32, 16
    planes = content(w, h, 1, 66)[0]
    src = Side(w, h, 1, "i420", dev=False).upload([planes])
    out = np.full(h * 2 * w, SENT, np.uint8)
    op = out.ctypes.data
    src0 = src.host()
    good = src.planes()
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        before = counters(c)
        base = dict(ctx=hd, planes={}, o=op, op=2 * w, w=w, h=h, fmt=FMT_UYVY, uvm=UV_COPY)

        def args(kw):
            a = dict(base)
            a.update(kw)
            p = None if a["planes"] is None else ctypes.byref(src.planes(**a["planes"]))
            return (a["ctx"], p, a["o"], a["op"], a["w"], a["h"], a["fmt"], a["uvm"])
        for kw in (dict(ctx=None), dict(planes=None), dict(planes=dict(y=None)), dict(planes=dict(c0=None)), dict(planes=dict(c1=None)),
                   dict(o=None), dict(planes=dict(chroma=2)), dict(planes=dict(y_pitch=w - 1)), dict(planes=dict(c_pitch=w // 2 - 1)),
                   dict(op=2 * w - 1), dict(w=w - 1), dict(h=h - 1), dict(w=-2), dict(h=-2), dict(fmt=1), dict(fmt=4), dict(uvm=2),
                   dict(o=good.y), dict(o=good.c0), dict(o=good.c1), dict(w=w - 1, h=0), dict(h=h - 1, w=0)):
            assert L.mi_equalize_hist_yuv420_to_packed422(*args(kw)) == BAD_ARG, kw
            assert L.mi_clahe_yuv420_to_packed422(*args(kw), 2.0, 2, 2) == BAD_ARG, kw
        assert L.mi_clahe_yuv420_to_packed422(*args({}), 2.0, 0, 2) == BAD_ARG
        assert L.mi_clahe_yuv420_to_packed422(*args({}), 2.0, 2048, 1024) == UNSUPPORTED
        assert L.mi_equalize_hist_yuv420_to_packed422(*args(dict(w=0))) == 0
        assert L.mi_equalize_hist_yuv420_to_packed422(*args(dict(h=0))) == 0
        assert (out == SENT).all() and np.array_equal(src.host(), src0) and c.get_stat("error_drains") == 0
        assert counters(c) == before
