"""Packed 4:2:2 in (YUY2 / UYVY) -- packed, NV12, BGR / RGB and planar 4:2:0 (I420 / YV12) out -- at the shapes where the kernels of
kernels/packed422.hip.h, packed422_nv12.hip.h, packed422_bgr.hip.h and packed422_yuv420.hip.h repeat themselves: source and destination rows at different 16-byte phases, carried
(row, slot) walks past their first step, bands without rows, rows shorter than their head, frame lists whose frames each have their
own phase, and a seeded sweep with a class census.  test_gpu_packed422.py, test_gpu_packed422_to_nv12.py and test_gpu_packed422_to_bgr.py
cover layouts, errors, graphs and the big sizes with one layout for both sides of a call; their Batch / Nv12Out / BgrOut classes, their
expected_frame / expected_planes builders, run and planar_status are used here unchanged (as P, N and B), and packed422_bgr_ref.expected
builds the images; the planar 4:2:0 form takes PlanarOut, expected_planes and run of test_gpu_packed422_to_yuv420.py (as Y) the same
way.  Every comparison is exact: the whole sentinel-filled output allocation(s), 64 guard bytes included, against the
image built from oracle.equalize_hist / oracle.clahe, and the whole input allocation against what was uploaded.  Luma and chroma are
full-range bytes of np.random.default_rng, drawn independently; every batch (every pair of calls on a one-frame batch) holds one such
frame and one compressed to (x // 3) + 40, on which a dword that was not mapped, or mapped twice, cannot equal its expected value.

How many workgroups a frame gets (B) is not observable and no test asserts it, but the shapes of group 2 are chosen by it.
equalize422_dev takes B = blocks_per_frame(2*W*H bytes, units, n, cap) with units = H rows (W::apply_rows: H / 2 row pairs for the NV12
apply), and blocks_per_frame never returns more than max(1, floor(bytes / 16384)) nor, for units > 1, more than units -- whatever the
CU count, which only lowers it.  So
    B <= max(1, floor(2*W*H / 16384)),   B <= H when H > 1 (H / 2 when H / 2 > 1 for the NV12 apply),
and workgroup b of B takes the band [units * b / B, units * (b + 1) / B), which is EMPTY for some b when units == 1 and B > 1.  A band
is walked as items, a step at a time, the position carried from step to step (row += drow; slot += dslot; wrap when slot >= S):
    hist422_partial, lut_apply422   items (row, slot), S = ((W/2 + 3) >> 2) + 1 slots a row, step 4 * 256 (four loads in flight);
                                     drow = 256 / S, dslot = 256 % S; the apply cuts its slots at the DESTINATION row
    tile_hist422                    items (row, slot) over the dwords of one tile, step 4 * 512, one workgroup a tile (the row split of
                                     launch_tile_luts422 is 1 below 65536 pixels a tile)
    lut_apply422_nv12               items (row pair, group), G = (W/2 + 7) >> 3 groups of 16 columns, step 256
    lut_apply422_bgr                items (row, group), the same G, step 256 (kThreads lanes, one item a lane and step; a group is
                                     two 16-byte loads, 16 pixels decoded, 48 bytes stored; the last group of a row may be ragged)
    lut_apply422_yuv420             lut_apply422_nv12's walk; a group leaves as two 16-byte Y stores and an 8-byte store into the U and
                                     into the V row, the ragged last group of a row as a dword, a 2-byte store and a byte
tests/packed422_geometry_cases.py holds the shapes with these numbers worked out next to each, and
tests/test_packed422_geometry_shapes.py asserts them on the CPU."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import packed422_bgr_ref as ref
import packed422_geometry_cases as g
import test_gpu_packed422 as P
import test_gpu_packed422_to_nv12 as N
import test_gpu_packed422_to_bgr as B
import test_gpu_packed422_to_yuv420 as Y                # helpers only: PlanarOut, expected_planes, run
from mi_lumaeq.capi import BgrYuv420FrameDev, CHROMA_PLANAR
from mi_lumaeq import UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

pytestmark = pytest.mark.gpu
SENT = P.SENT
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]
ORDERS = [ORDER_BGR, ORDER_RGB]
KEY = "packed422-geometry"
assert (g.FMT_YUY2, g.FMT_UYVY, g.UV_FILL128, g.UV_COPY) == (FMT_YUY2, FMT_UYVY, UV_FILL128, UV_COPY) and N.SENT == B.SENT == Y.SENT == SENT


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small batches leave nothing cached in torch's allocator for the modules that run after it, and its reference
    planes leave the caches of the modules whose builders it used."""
    yield
    _content.clear()
    _mapped.clear()
    for cache in (P._ref_cache, N._ref_cache):
        for k in [k for k in cache if isinstance(k[0], tuple) and isinstance(k[0][0], tuple) and k[0][0][:1] == (KEY,)]:
            del cache[k]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- content and references ------------------------------------------------------------------------------------------------------
_content, _mapped = {}, {}


def content(w, h, n, fmt, seed, flip=False):
    """n frames of independent full-range luma and chroma bytes; every second one (the first when `flip`) compressed to x // 3 + 40."""
    key = (w, h, n, fmt, seed, flip)
    if key not in _content:
        rng = np.random.default_rng([seed, w, h, n])
        off = fmt - 2
        frames = []
        for k in range(n):
            f = np.empty((h, 2 * w), np.uint8)
            f[:, off::2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
            f[:, 1 - off::2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
            frames.append(f // 3 + 40 if (k & 1) != flip else f)
        _content[key] = frames
    return _content[key], (KEY,) + key


def variants(n):
    """A batch of two or more frames holds both kinds of content; a one-frame batch is run once with each."""
    return (False,) if n > 1 else (False, True)


def mapped(key, frame, w, fmt, op):
    k = (key, op)
    if k not in _mapped:
        _mapped[k] = ref.mapped_luma(ref.luma(frame, w, fmt), op[0], op[1])
    return _mapped[k]


def first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return int(bad.size), bad[:8].tolist()


def align4(x):
    return (x + 3) & ~3


# ---- the four forms, each with a source layout and a destination layout of its own -----------------------------------------------
def check_packed(c, w, h, n, seed, fmt, uv, op, sl, dl, in_place=False):
    """sl, dl: (pitch - 2W, gap between frames, base offset) of the source and of the destination batch."""
    for flip in variants(n):
        frames, key = content(w, h, n, fmt, seed, flip)
        src = P.Batch(w, h, n, sl).upload(frames)
        dst = src if in_place else P.Batch(w, h, n, dl)
        P.run(c, op[0], op[1], src, dst, fmt, uv)
        torch.cuda.synchronize()
        want = dst.image([P.expected_frame(f, w, fmt, op[0], op[1], uv, (key, k)) for k, f in enumerate(frames)])
        got = dst.host()
        why = dict(form="packed in place" if in_place else "packed", w=w, h=h, n=n, fmt=fmt, uv=uv, op=op, src=sl, dst=dl, flip=flip)
        assert np.array_equal(got, want), (why, first_bad(got, want))
        if not in_place:
            got = src.host()
            assert np.array_equal(got, src.image(frames)), (why, "the input allocation was written", first_bad(got, src.image(frames)))


def nv12_layout(w, h, y_extra, uv_extra, y_off, uv_phase, gap=0):
    """An Nv12Out layout whose Y plane starts y_off bytes into its allocation and whose UV plane, in the same allocation behind a gap of
    at least `gap` bytes, starts at uv_phase modulo 16."""
    ysz = (align4(w) + y_extra) * h
    return (y_extra, uv_extra, "gap", gap + (uv_phase - y_off - ysz - gap) % 16, y_off)


def check_nv12(c, w, h, n, seed, fmt, uv, op, sl, dl):
    """sl as check_packed; dl: an Nv12Out layout (y_pitch - align4(W), uv_pitch - align4(W), where the UV plane lies, gap, offset)."""
    for flip in variants(n):
        frames, key = content(w, h, n, fmt, seed, flip)
        src = N.Batch(w, h, n, sl).upload(frames)
        dst = N.Nv12Out(w, h, n, dl)
        N.run(c, op[0], op[1], src, dst, fmt, uv)
        torch.cuda.synchronize()
        want = dst.image([N.expected_planes(f, w, fmt, op[0], op[1], uv, (key, k)) for k, f in enumerate(frames)])
        why = dict(form="nv12", w=w, h=h, n=n, fmt=fmt, uv=uv, op=op, src=sl, dst=dl, flip=flip)
        for bi, (got, wnt) in enumerate(zip(dst.host(), want)):
            assert np.array_equal(got, wnt), (why, "allocation", bi, first_bad(got, wnt))
        got = src.host()
        assert np.array_equal(got, src.image(frames)), (why, "the input allocation was written", first_bad(got, src.image(frames)))


class BgrAt(B.BgrOut):
    """BgrOut with the base offset, the pitch and the gap between images given as numbers."""

    def __init__(self, w, h, n, off, pitch, gap):
        self.w, self.h, self.n, self.off, self.pitch = w, h, n, off, pitch
        self.fstride = pitch * h + gap
        self.total = off + self.fstride * n + 64
        self.buf = torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0 and pitch >= 3 * w


def bgr_wide(w, off=4, extra=4, gap=8):
    """(off, pitch, gap) with every term a multiple of 4: vector stores."""
    return (off, align4(3 * w) + extra, gap)


def bgr_bytes(w, off=1, gap=3):
    """An odd base and an odd pitch: byte stores."""
    return (off, 3 * w + 1, gap)


def check_bgr(c, w, h, n, seed, fmt, order, op, sl, dl):
    """sl as check_packed; dl: (base offset, pitch, gap between images) of the BgrAt allocation."""
    for flip in variants(n):
        frames, key = content(w, h, n, fmt, seed, flip)
        src = B.Batch(w, h, n, sl).upload(frames)
        dst = BgrAt(w, h, n, *dl)
        B.run(c, op[0], op[1], src, dst, fmt, order)
        torch.cuda.synchronize()
        want = dst.image([ref.expected(f, w, fmt, order, op[0], op[1], False, mapped((key, k), f, w, fmt, op)) for k, f in enumerate(frames)])
        got = dst.host()
        why = dict(form="bgr", w=w, h=h, n=n, fmt=fmt, order=order, op=op, src=sl, dst=dl, flip=flip)
        assert np.array_equal(got, want), (why, first_bad(got, want))
        got = src.host()
        assert np.array_equal(got, src.image(frames)), (why, "the input allocation was written", first_bad(got, src.image(frames)))


def planar_out(w, h, n, dl):
    """dl: (kind, y_off, y_pitch - align4(W), c_pitch - align4(W / 2), (phase of the first chroma plane, of the second)) of a PlanarOut."""
    kind, y_off, ye, ce, phases = dl
    return Y.PlanarOut(w, h, n, kind, y_off=y_off, ye=ye, ce=ce, phases=phases)


def check_yuv420(c, w, h, n, seed, fmt, uv, op, sl, dl):
    """sl as check_packed; dl as planar_out takes it.  Every allocation of the three planes, and the input's, compared whole."""
    for flip in variants(n):
        frames, key = content(w, h, n, fmt, seed, flip)
        src = N.Batch(w, h, n, sl).upload(frames)
        dst = planar_out(w, h, n, dl)
        Y.run(c, op[0], op[1], src, dst.planes(), fmt, uv)
        torch.cuda.synchronize()
        want = dst.image([Y.expected_planes(f, w, fmt, op[0], op[1], uv, (key, k)) for k, f in enumerate(frames)])
        why = dict(form="yuv420", w=w, h=h, n=n, fmt=fmt, uv=uv, op=op, src=sl, dst=dl, flip=flip)
        for bi, (got, wnt) in enumerate(zip(dst.host(), want)):
            assert np.array_equal(got, wnt), (why, "allocation", bi, first_bad(got, wnt))
        got = src.host()
        assert np.array_equal(got, src.image(frames)), (why, "the input allocation was written", first_bad(got, src.image(frames)))


# ---- 1. phase matrix -------------------------------------------------------------------------------------------------------------
def phase_src(off):
    return (g.PHASE_SRC["extra"], g.PHASE_SRC["gap"], off)


@pytest.mark.parametrize("src_off", g.PHASES)
def test_phase_matrix_packed(c, src_off):
    """40 x 6 x 2 frames, source pitch 2W + 4, destination pitch 2W + 8: with the base offsets crossed, every row of a call has its own
    pair of phases.  lut_apply422 cuts its slots at the destination row and loads the source wherever that puts it; the interpolation
    kernels read and write unaligned-capable vectors (two full groups) and dwords (the ragged group of 8 columns)."""
    w, h, n = g.PHASE_W, g.PHASE_H, g.PHASE_N
    for di, dst_off in enumerate(g.PHASES):
        for fmt in FMTS:
            for oi, op in enumerate(g.PHASE_OPS):
                uv = UVS[(src_off // 4 + di + fmt + oi) % 2]
                check_packed(c, w, h, n, 11, fmt, uv, op, phase_src(src_off), (g.PHASE_DST["extra"], g.PHASE_DST["gap"], dst_off))


@pytest.mark.parametrize("off", g.PHASES)
def test_phase_matrix_packed_in_place(c, off):
    """src is dst: the same rows, so the same phase on both sides, at each base offset."""
    w, h, n = g.PHASE_W, g.PHASE_H, g.PHASE_N
    for fmt in FMTS:
        for oi, op in enumerate(g.PHASE_OPS):
            check_packed(c, w, h, n, 12, fmt, UVS[(off // 4 + fmt + oi) % 2], op, phase_src(off), phase_src(off), in_place=True)


@pytest.mark.parametrize("src_off", g.PHASES)
def test_phase_matrix_nv12(c, src_off):
    """The source offset crossed with the Y plane's; the UV plane at a third phase (the first of 0, 4, 8, 12 that neither has, shifted by
    the format), Y pitch W + 4 and UV pitch W + 12."""
    w, h, n = g.PHASE_W, g.PHASE_H, g.PHASE_N
    for di, y_off in enumerate(g.PHASES):
        for fmt in FMTS:
            third = [p for p in g.PHASES if p not in (src_off, y_off)][fmt - 2]
            for oi, op in enumerate(g.PHASE_OPS):
                uv = UVS[(src_off // 4 + di + fmt + oi) % 2]
                check_nv12(c, w, h, n, 13, fmt, uv, op, phase_src(src_off), nv12_layout(w, h, 4, 12, y_off, third, gap=g.PHASE_DST["gap"]))


@pytest.mark.parametrize("src_off", g.PHASES)
def test_phase_matrix_bgr(c, src_off):
    """The source offset crossed with the image's base: 0, 4 and 16 with a pitch of 3W + 4 (vector stores at 4-byte alignment), 1 with a
    pitch of 3W + 1 (byte stores)."""
    w, h, n = g.PHASE_W, g.PHASE_H, g.PHASE_N
    for di, base in enumerate(g.BGR_BASES):
        dl = bgr_bytes(w, off=base) if base & 3 else bgr_wide(w, off=base, gap=g.PHASE_DST["gap"])
        for fmt in FMTS:
            for oi, op in enumerate(g.PHASE_OPS):
                check_bgr(c, w, h, n, 14, fmt, ORDERS[(src_off // 4 + di + fmt + oi) % 2], op, phase_src(src_off), dl)


@pytest.mark.parametrize("src_off", g.PHASES)
def test_phase_matrix_yuv420(c, src_off):
    """The source offset crossed with the Y plane's; U and V at the first two of 0, 4, 8, 12 that neither has, V's address below U's
    (YV12 order) for UYVY.  Y pitch W + 4 and chroma pitch W / 2 + 4: the Y phase advances by 12 a row, the chroma phases by 8."""
    w, h, n = g.PHASE_W, g.PHASE_H, g.PHASE_N
    ye, ce = g.PHASE_YUV420["ye"], g.PHASE_YUV420["ce"]
    for di, y_off in enumerate(g.PHASES):
        rest = tuple(p for p in g.PHASES if p not in (src_off, y_off))[:2]
        for fmt in FMTS:
            kind = "one" if fmt == FMT_YUY2 else "yv12"
            for oi, op in enumerate(g.PHASE_OPS):
                uv = UVS[(src_off // 4 + di + fmt + oi) % 2]
                check_yuv420(c, w, h, n, 15, fmt, uv, op, phase_src(src_off), (kind, y_off, ye, ce, rest))


@pytest.mark.parametrize("w", g.TAIL_WIDTHS)
def test_every_chroma_tail_length_yuv420(c, w):
    """33 .. 40 macropixels a row: the last group of a row holds 1, 2, ..., 8 macropixels, so store_c_tail, load422_tail and the
    ragged branch of the interpolation run at every length (a dword, a 2-byte store and a byte in every combination), through the LUT
    apply, the LDS interpolation and the wide-grid kernel, with both UV modes and both formats."""
    h, n = g.TAIL_H, g.TAIL_N
    assert g.tail_dwords(w // 2) == (w - 64) // 2
    for op in g.TAIL_OPS:
        for fmt in FMTS:
            for uv in UVS:
                check_yuv420(c, w, h, n, 16, fmt, uv, op, g.P4, g.TAIL_DST)


# ---- 2. walks past their first step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", g.LOOP_SHAPES, ids=[s["id"] for s in g.LOOP_SHAPES])
def test_walks_past_their_first_step(c, shape):
    """The table of packed422_geometry_cases.LOOP_SHAPES: S, drow, dslot, items and steps of every shape stand next to it there, and
    test_packed422_geometry_shapes.py asserts on the CPU that each loops.  equalizeHist runs the histogram and the apply walk of the
    form; the CLAHE grid runs the tile histograms and the interpolation at the same shape and layouts."""
    w, h, n, form = shape["w"], shape["h"], shape["n"], shape["form"]
    for walk in shape["walks"]:
        items, _, step, _ = g.walk(walk, w, h)
        assert items > step, "the shape would not loop"
    for oi, op in enumerate(shape["ops"]):
        for fmt in FMTS:
            k = (oi + fmt) % 2
            if form == "packed":
                check_packed(c, w, h, n, 21, fmt, UVS[k], op, shape["sl"], shape["dl"])
            elif form == "nv12":
                check_nv12(c, w, h, n, 22, fmt, UVS[k], op, shape["sl"], nv12_layout(w, h, 4, 12, 4, 8, gap=8))
            elif form == "yuv420":
                check_yuv420(c, w, h, n, 25, fmt, UVS[k], op, shape["sl"], shape["dl"])
            else:
                check_bgr(c, w, h, n, 23, fmt, ORDERS[k], op, shape["sl"], bgr_wide(w))
                check_bgr(c, w, h, n, 23, fmt, ORDERS[1 - k], op, shape["sl"], bgr_bytes(w))


@pytest.mark.parametrize("shape", g.TILE_SHAPES, ids=[s["id"] for s in g.TILE_SHAPES])
def test_tile_histogram_walk(c, shape):
    """tile_hist422_body on the largest tile a size allows (one step with a partly live fourth load at 200 rows, a second step at 232)
    and on tiles that start and end on odd columns with a reflected column and row; source rows at every phase (pitch 2W + 4)."""
    w, h = shape["w"], shape["h"]
    op = ("clahe", (2.0,) + shape["grid"])
    for fmt in FMTS:
        check_packed(c, w, h, 1, 24, fmt, UVS[fmt % 2], op, g.P4, (8, 0, 12))


# ---- 3. rows shorter than their head ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", g.HEAD_WIDTHS)
def test_rows_shorter_than_their_head(c, w):
    """One, two and three macropixels a row, eight rows, three frames; source pitch 2W + 4 at offset 4, destination pitch 2W + 12 at
    offset 12: rows that lie wholly before their first 16-byte boundary, next to rows that cross it.  NV12 out: UV rows of 2, 4 and 6
    bytes, a single 2-byte store, a dword, a dword and a 2-byte store.  Planar 4:2:0 out: chroma rows of 1, 2 and 3 bytes (a byte; a
    2-byte store; a 2-byte store and a byte) at a chroma pitch of 4 or 8, the planes at offsets 12 / 8 / 4."""
    h, n = g.HEAD_H, g.HEAD_N
    for oi, op in enumerate(g.HEAD_OPS):
        for fmt in FMTS:
            uv = UVS[(oi + fmt + w // 2) % 2]
            check_packed(c, w, h, n, 31, fmt, uv, op, g.HEAD_SRC, g.HEAD_DST)
            check_nv12(c, w, h, n, 32, fmt, uv, op, g.HEAD_SRC, nv12_layout(w, h, 12, 4, 12, 8))
            check_yuv420(c, w, h, n, 33, fmt, uv, op, g.HEAD_SRC, g.head_yuv420(w))


# ---- 4. frame lists --------------------------------------------------------------------------------------------------------------
def list_frames(w, h, fmt, seed):
    """Four frames of one list, and each as the single frame of a batch (the key names its reference)."""
    frames, key = content(w, h, 4, fmt, seed)
    return frames, [(key, k) for k in range(4)]


@pytest.mark.parametrize("in_place", [False, True], ids=["pitches-differ", "one-frame-in-place"])
def test_frame_list_packed(c, in_place):
    """Four frames, each in its own allocation: `in` at offsets 0, 4, 8, 12, `out` at 12 - 4k.  Pitches 2W + 4 in and 2W + 8 out; or, with
    equal pitches (an in-place frame needs them), frame 2 in place.  The list call gives the reference and, byte for byte, what four
    single-frame batch calls give."""
    w, h = g.PHASE_W, g.PHASE_H
    se, de = 4, 4 if in_place else 8
    for fmt in FMTS:
        frames, keys = list_frames(w, h, fmt, 41)
        for oi, op in enumerate(g.PHASE_OPS):
            uv = UVS[(oi + fmt + in_place) % 2]
            srcs = [P.Batch(w, h, 1, (se, 0, off)).upload([f]) for off, f in zip(g.PHASES, frames)]
            dsts = [P.Batch(w, h, 1, (de, 0, 12 - 4 * k)) for k in range(4)]
            if in_place:
                dsts[2] = srcs[2]
            ins, outs = [s.dev.data_ptr() for s in srcs], [d.dev.data_ptr() for d in dsts]
            kw = dict(in_pitch=srcs[0].pitch, out_pitch=dsts[0].pitch, stream=P.stream())
            if op[0] == "eq":
                c.equalize_hist_packed422_frames(ins, outs, w, h, fmt, uv, **kw)
            else:
                c.clahe_packed422_frames(ins, outs, w, h, fmt, uv, *op[1], **kw)
            torch.cuda.synchronize()
            for k, (f, s, d) in enumerate(zip(frames, srcs, dsts)):
                why = dict(form="packed list", fmt=fmt, uv=uv, op=op, frame=k, src=(se, 0, s.off), dst=(de, 0, d.off), in_place=d is s)
                want = d.image([P.expected_frame(f, w, fmt, op[0], op[1], uv, keys[k])])
                got = d.host()
                assert np.array_equal(got, want), (why, first_bad(got, want))
                if d is not s:
                    assert np.array_equal(s.host(), s.image([f])), (why, "the input allocation was written")
                one_src = P.Batch(w, h, 1, (se, 0, s.off)).upload([f])
                one_dst = one_src if d is s else P.Batch(w, h, 1, (de, 0, d.off))
                P.run(c, op[0], op[1], one_src, one_dst, fmt, uv)
                torch.cuda.synchronize()
                assert np.array_equal(one_dst.host(), got), (why, "the list call and the batch call differ", first_bad(one_dst.host(), got))


def test_frame_list_nv12(c):
    """Four frames: `in` at offsets 0, 4, 8, 12, the Y plane one phase on, the UV plane two phases on."""
    w, h = g.PHASE_W, g.PHASE_H
    for fmt in FMTS:
        frames, keys = list_frames(w, h, fmt, 42)
        for oi, op in enumerate(g.PHASE_OPS):
            uv = UVS[(oi + fmt) % 2]
            srcs = [N.Batch(w, h, 1, (4, 0, off)).upload([f]) for off, f in zip(g.PHASES, frames)]
            lays = [nv12_layout(w, h, 4, 12, g.PHASES[(k + 1) % 4], g.PHASES[(k + 2) % 4]) for k in range(4)]
            dsts = [N.Nv12Out(w, h, 1, lay) for lay in lays]
            kw = dict(in_pitch=srcs[0].pitch, y_pitch=dsts[0].y_pitch, uv_pitch=dsts[0].uv_pitch, stream=N.stream())
            a = ([s.dev.data_ptr() for s in srcs], [d.y_ptr for d in dsts], [d.uv_ptr for d in dsts], w, h, fmt, uv)
            if op[0] == "eq":
                c.equalize_hist_packed422_to_nv12_frames(*a, **kw)
            else:
                c.clahe_packed422_to_nv12_frames(*a, *op[1], **kw)
            torch.cuda.synchronize()
            for k, (f, s, d) in enumerate(zip(frames, srcs, dsts)):
                why = dict(form="nv12 list", fmt=fmt, uv=uv, op=op, frame=k, src=(4, 0, s.off), dst=lays[k])
                want = d.image([N.expected_planes(f, w, fmt, op[0], op[1], uv, keys[k])])
                got = d.host()
                assert np.array_equal(got[0], want[0]), (why, first_bad(got[0], want[0]))
                assert np.array_equal(s.host(), s.image([f])), (why, "the input allocation was written")
                one_dst = N.Nv12Out(w, h, 1, lays[k])
                N.run(c, op[0], op[1], s, one_dst, fmt, uv)
                torch.cuda.synchronize()
                assert np.array_equal(one_dst.host()[0], got[0]), (why, "the list call and the batch call differ")


def test_frame_list_bgr(c):
    """Four frames: `in` at offsets 0, 4, 8, 12, the images at bases 0, 1, 4 and 16 with one pitch of 3W + 4: the frame at base 1 takes
    the byte stores, its neighbours in the same launch the vector stores."""
    w, h = g.PHASE_W, g.PHASE_H
    pitch = 3 * w + 4
    for fmt in FMTS:
        frames, keys = list_frames(w, h, fmt, 43)
        for oi, op in enumerate(g.PHASE_OPS):
            order = ORDERS[(oi + fmt) % 2]
            srcs = [B.Batch(w, h, 1, (4, 0, off)).upload([f]) for off, f in zip(g.PHASES, frames)]
            dsts = [BgrAt(w, h, 1, base, pitch, 0) for base in g.BGR_BASES]
            a = ([s.ptr for s in srcs], [d.ptr for d in dsts], w, h, fmt, order)
            kw = dict(in_pitch=srcs[0].pitch, out_pitch=pitch, stream=B.stream())
            if op[0] == "eq":
                c.equalize_hist_packed422_to_bgr_frames(*a, **kw)
            else:
                c.clahe_packed422_to_bgr_frames(*a, *op[1], **kw)
            torch.cuda.synchronize()
            for k, (f, s, d) in enumerate(zip(frames, srcs, dsts)):
                why = dict(form="bgr list", fmt=fmt, order=order, op=op, frame=k, src=(4, 0, s.off), dst=(d.off, pitch, 0))
                want = d.image([ref.expected(f, w, fmt, order, op[0], op[1], False, mapped(keys[k], f, w, fmt, op))])
                got = d.host()
                assert np.array_equal(got, want), (why, first_bad(got, want))
                assert np.array_equal(s.host(), s.image([f])), (why, "the input allocation was written")
                one_dst = BgrAt(w, h, 1, d.off, pitch, 0)
                B.run(c, op[0], op[1], s, one_dst, fmt, order)
                torch.cuda.synchronize()
                assert np.array_equal(one_dst.host(), got), (why, "the list call and the batch call differ")


def yuv420_list_call(c, w, h, kind, fmt, uv, op, seed):
    """One list call on four frames -- `in` at offsets 0, 4, 8, 12; the planes of frame k one, two and three phases on, in three
    allocations ("own") or with the U and V rows side by side in one pitched plane ("side": V = U + W / 2) -- compared per frame with
    the oracle's image over the whole allocations, and with a single-frame batch call at the same phases."""
    frames, keys = list_frames(w, h, fmt, seed)
    srcs = [N.Batch(w, h, 1, (4, 0, off)).upload([f]) for off, f in zip(g.PHASES, frames)]
    lays = [(kind, g.PHASES[(k + 1) % 4], 4, 4, (g.PHASES[(k + 2) % 4], g.PHASES[(k + 3) % 4])) for k in range(4)]
    dsts = [planar_out(w, h, 1, lay) for lay in lays]
    if kind == "side":
        assert all(d.c_pitch == w and d.ptr("v") == d.ptr("u") + w // 2 for d in dsts)
    entries = [BgrYuv420FrameDev(s.dev.data_ptr(), d.ptr("y"), d.ptr("u"), d.ptr("v")) for s, d in zip(srcs, dsts)]
    a = (entries, w, h, srcs[0].pitch, dsts[0].y_pitch, dsts[0].c_pitch, CHROMA_PLANAR, fmt, uv)
    if op[0] == "eq":
        c.equalize_hist_packed422_to_yuv420_frames_dev(*a, stream=Y.stream())
    else:
        c.clahe_packed422_to_yuv420_frames_dev(*a, *op[1], stream=Y.stream())
    torch.cuda.synchronize()
    for k, (f, s, d) in enumerate(zip(frames, srcs, dsts)):
        why = dict(form="yuv420 list", w=w, h=h, fmt=fmt, uv=uv, op=op, frame=k, src=(4, 0, s.off), dst=lays[k])
        want = d.image([Y.expected_planes(f, w, fmt, op[0], op[1], uv, keys[k])])
        got = d.host()
        for bi, (gt, wnt) in enumerate(zip(got, want)):
            assert np.array_equal(gt, wnt), (why, "allocation", bi, first_bad(gt, wnt))
        assert np.array_equal(s.host(), s.image([f])), (why, "the input allocation was written")
        one_dst = planar_out(w, h, 1, lays[k])
        Y.run(c, op[0], op[1], s, one_dst.planes(), fmt, uv)
        torch.cuda.synchronize()
        for gt, one in zip(got, one_dst.host()):
            assert np.array_equal(one, gt), (why, "the list call and the batch call differ", first_bad(one, gt))


@pytest.mark.parametrize("kind", ["own", "side"], ids=["own-planes", "side-by-side"])
def test_frame_list_yuv420(c, kind):
    """40 x 6: two full groups and a ragged one of 4 macropixels; W / 2 = 20 is a multiple of 4, so the form accepts c_pitch = W with
    c1 = c0 + W / 2.  Own planes also at 62 x 6, whose last group holds 7 macropixels: the table launches of the LUT apply, the LDS
    interpolation and the wide-grid kernel run load422_tail and the dword, 2-byte and byte stores of store_c_tail."""
    w, h = g.PHASE_W, g.PHASE_H
    for fmt in FMTS:
        for oi, op in enumerate(g.PHASE_OPS):
            yuv420_list_call(c, w, h, kind, fmt, UVS[(oi + fmt) % 2], op, 44)
            if kind == "own":
                assert g.tail_dwords(62 // 2) == 7
                yuv420_list_call(c, 62, h, kind, fmt, UVS[(oi + fmt + 1) % 2], op, 45)


# ---- 5. seeded sweep -------------------------------------------------------------------------------------------------------------
def sweep_layouts(case):
    """The two layouts of a case in the terms of its form's classes."""
    w, h, dl = case["w"], case["h"], case["dl"]
    if case["form"] == "packed":
        return case["sl"], dl
    if case["form"] == "nv12":
        if case["uv_own"]:
            return case["sl"], (dl[0], case["uv_extra"], "own", dl[1], dl[2])
        return case["sl"], nv12_layout(w, h, dl[0], case["uv_extra"], dl[2], case["uv_phase"], gap=dl[1])
    if case["form"] == "yuv420":
        return case["sl"], g.yuv420_layout(case)
    if case["byte"]:
        return case["sl"], (dl[2] + 1, 3 * w + dl[0] + 1, dl[1] + 3)
    return case["sl"], (dl[2], align4(3 * w) + dl[0], dl[1])


def untouched(form, dst):
    return np.array_equal(dst.host(), dst.image()) if form == "packed" else dst.same()


@pytest.mark.parametrize("form", g.FORMS)
def test_seeded_sweep(c, form):
    """48 cases of one fixed seed for each output form (the same draws for all four), named by classify(): the census is a condition
    on the generator, asserted here and, without a GPU, in test_packed422_geometry_shapes.py.  A case the planar form refuses gives that
    form's status and leaves the output allocation(s) -- all three planes' -- and the input untouched."""
    cases = g.sweep_cases(form)
    assert g.census_holds(cases), {k: v[0] for k, v in g.census(cases).items()}
    check = {"packed": check_packed, "nv12": check_nv12, "bgr": check_bgr, "yuv420": check_yuv420}[form]
    M = {"packed": P, "nv12": N, "bgr": B, "yuv420": N}[form]
    for i, case in enumerate(cases):
        w, h, n, fmt, op = case["w"], case["h"], case["n"], case["fmt"], g.op_of(case)
        sl, dl = sweep_layouts(case)
        status = N.planar_status(c, w, h, n, op[0], op[1])
        if g.classify(case) != "refused-by-planar-form":
            assert status == 0, (i, case, status)
            check(c, w, h, n, 500 + i, fmt, case["uv"], op, sl, dl)
            continue
        assert status != 0, (i, case)
        frames, _ = content(w, h, n, fmt, 500 + i)
        src = M.Batch(w, h, n, sl).upload(frames)
        if form == "yuv420":
            dst = planar_out(w, h, n, dl)
        else:
            dst = BgrAt(w, h, n, *dl) if form == "bgr" else (P.Batch if form == "packed" else N.Nv12Out)(w, h, n, dl)
        with pytest.raises(mi_lumaeq.MiError) as e:
            if form == "yuv420":
                Y.run(c, op[0], op[1], src, dst.planes(), fmt, case["uv"])
            else:
                M.run(c, op[0], op[1], src, dst, fmt, case["uv"])
        torch.cuda.synchronize()
        assert e.value.status == status, (i, case, e.value.status, status)
        assert untouched(form, dst), (i, case, "a refused call wrote")
        assert np.array_equal(src.host(), src.image(frames)), (i, case, "a refused call wrote the input")


def test_zz_fused_counters_stay_zero(c):
    torch.cuda.synchronize()
    assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
