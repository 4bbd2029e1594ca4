"""Packed 4:2:2 frames in (YUY2 / UYVY), interleaved BGR / RGB images out on a LIST of device frames:
mi_equalize_hist_packed422_to_bgr_frames_dev and mi_clahe_packed422_to_bgr_frames_dev.  The expected image is
tests/packed422_bgr_ref.py (the oracle's luma in the call's arithmetic mode, decoded with every row's OWN chroma), and the batch form
run on the same pixels.  Every frame and every image lives in a sentinel-filled allocation of its own, at a padded pitch and a base of
its own; the WHOLE allocation is compared, the inputs must read unchanged, and every comparison in this file is exact bytes.
The statistics "packed422_bgr_list_frames_wide" / "packed422_bgr_list_frames_bytes" count the frames by store path under the header's
rule, restated in wide_frames() below."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mi_lumaeq
import clahe_u8_rungs
import packed422_bgr_ref as ref
import test_gpu_packed422_interp_paths as interp_paths          # the seven rung shapes and the four option pairs are read from there
from mi_lumaeq import synth, UV_COPY, FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

pytestmark = pytest.mark.gpu
BAD_ARG = 1
SENT = 0x5A
DISTS = ["D1", "D2", "D3"]
FMTS = [FMT_YUY2, FMT_UYVY]
ORDERS = [ORDER_BGR, ORDER_RGB]
OPS = [("eq", None), ("clahe", (2.0, 2, 2))]
STATS = ("packed422_bgr_list_frames_wide", "packed422_bgr_list_frames_bytes")
SLACK = 48                                                       # sentinel bytes behind the last row of every allocation
# input: (pitch - 2W, base offsets from a 16-byte boundary, taken in turn); every base and pitch a multiple of 4
IN_LAYOUTS = [(4, (4, 8, 12)), (36, (8, 0, 4)), (0, (12, 4, 0))]
# output: name -> (pitch from W, base offsets taken in turn).  wide: everything a multiple of 4; mixed: pitch a multiple of 4, bases
# of every residue; odd: pitch 3W + 1; tight: pitch 3W (2 mod 4 when W % 4 == 2)
OUT_LAYOUTS = ["wide", "mixed", "odd", "tight"]


def stream():
    return torch.cuda.current_stream().cuda_stream


def out_layout(w, name):
    if name == "wide":
        return (3 * w + 3) // 4 * 4 + 4, (4, 16, 8)
    if name == "mixed":
        return (3 * w + 3) // 4 * 4 + 8, (0, 1, 2, 3, 4)
    if name == "odd":
        return 3 * w + 1, (5, 0, 3)
    return 3 * w, (0, 6, 1)


def wide_frames(pitch, ptrs):
    """The header's rule: out_pitch and the frame's own `out` are multiples of 4."""
    return sum(1 for p in ptrs if pitch % 4 == 0 and p % 4 == 0)


class Pool:
    """n sentinel-filled device allocations, one per frame: `h` rows of `row` payload bytes at `pitch`, frame k `offs[k % len]` bytes
    into its allocation."""

    def __init__(self, n, h, row, pitch, offs):
        self.n, self.h, self.row, self.pitch = n, h, row, pitch
        self.offs = [offs[k % len(offs)] for k in range(n)]
        self.total = max(offs) + pitch * h + SLACK
        self.bufs = [torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.ptrs = [b.data_ptr() + o for b, o in zip(self.bufs, self.offs)]

    def image(self, payloads=None):
        """What the n allocations hold: sentinels, and payloads[k] (h x >= row bytes) in frame k's rows."""
        a = np.full((self.n, self.total), SENT, np.uint8)
        if payloads is not None:
            for k, p in enumerate(payloads):
                o = self.offs[k]
                a[k, o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : self.row] = p.reshape(self.h, -1)[:, : self.row]
        return a

    def upload(self, payloads):
        a = self.image(payloads)
        for k, b in enumerate(self.bufs):
            b.copy_(torch.from_numpy(a[k]))
        return self

    def host(self):
        return torch.stack(self.bufs).cpu().numpy() if self.n else np.zeros((0, self.total), np.uint8)

    def same(self, payloads=None):
        return np.array_equal(self.host(), self.image(payloads))


def in_pool(frames, w, h, li=0):
    extra, offs = IN_LAYOUTS[li % len(IN_LAYOUTS)]
    return Pool(len(frames), h, 2 * w, 2 * w + extra, offs).upload(frames)


def out_pool(n, w, h, lo="wide"):
    pitch, offs = out_layout(w, lo)
    return Pool(n, h, 3 * w, pitch, offs)


def run_list(c, op, cfg, src, dst, w, h, fmt, order, st=None):
    kw = dict(in_pitch=src.pitch, out_pitch=dst.pitch, stream=stream() if st is None else st)
    if op == "eq":
        c.equalize_hist_packed422_to_bgr_frames(src.ptrs, dst.ptrs, w, h, fmt, order, **kw)
    else:
        c.clahe_packed422_to_bgr_frames(src.ptrs, dst.ptrs, w, h, fmt, order, *cfg, **kw)


def run_batch(c, op, cfg, frames, w, h, fmt, order):
    """The batch form on the same pixels, tight in one allocation per side; returns the n images (n x h x w x 3)."""
    n = len(frames)
    d_in = torch.from_numpy(np.stack([np.ascontiguousarray(f[:, : 2 * w]) for f in frames])).to("cuda:0")
    d_out = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda:0")
    if op == "eq":
        c.equalize_hist_packed422_to_bgr_batch_dev(d_in, d_out, w, h, n, fmt, order, stream=stream())
    else:
        c.clahe_packed422_to_bgr_batch_dev(d_in, d_out, w, h, n, fmt, order, *cfg, stream=stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


_frames, _luma = {}, {}


def frames_of(w, h, fmt, n=3, seed=100):
    k = (w, h, fmt, n, seed)
    if k not in _frames:
        _frames[k] = [synth.packed422_frame(w, h, fmt, DISTS[i % 3], seed + i) for i in range(n)]
    return _frames[k]


def expected(key, frames, w, fmt, order, op, cfg, contract=False):
    """The reference images of a list of frames; the oracle's luma is computed once per (content, op, arithmetic mode) and shared."""
    out = []
    for k, f in enumerate(frames):
        lk = (key, w, f.shape[0], fmt, k, op, cfg, bool(contract))
        if lk not in _luma:
            _luma[lk] = ref.mapped_luma(ref.luma(f, w, fmt), op, cfg, contract)
        out.append(ref.expected(f, w, fmt, order, op, cfg, contract, _luma[lk]))
    return out


def check_list(c, frames, w, h, fmt, order, op, cfg, li, lo, key, contract=False, against_batch=True):
    why = (w, h, fmt, order, op, cfg, li, lo, contract)
    src = in_pool(frames, w, h, li)
    dst = out_pool(len(frames), w, h, lo)
    batch = None
    if against_batch:
        try:
            batch = run_batch(c, op, cfg, frames, w, h, fmt, order)
        except mi_lumaeq.MiError as e:                # a size / grid pair the batch form refuses: the same status, nothing written
            with pytest.raises(mi_lumaeq.MiError) as e2:
                run_list(c, op, cfg, src, dst, w, h, fmt, order)
            torch.cuda.synchronize()
            assert e2.value.status == e.status, (why, e2.value.status, e.status)
            assert dst.same() and src.same(frames), (why, "a refused call wrote")
            return
    run_list(c, op, cfg, src, dst, w, h, fmt, order)
    torch.cuda.synchronize()
    want = expected(key, frames, w, fmt, order, op, cfg, contract)
    got, img = dst.host(), dst.image(want)
    assert np.array_equal(got, img), (why, int((got != img).sum()), np.argwhere(got != img)[:8])
    assert src.same(frames), (why, "an input allocation was written")
    if batch is not None:
        assert np.array_equal(batch, np.stack(want)), (why, "the batch form differs from the reference")


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


# ---- 1. the grid against the reference and the batch form ------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 14, 16, 18, 30, 32, 50])
def test_grid_against_reference_and_batch(c, w):
    """W = 2, 14: no full 16-column group; 16, 32: exact groups; 18, 30, 50: groups plus a ragged tail.  H = 1, 2, 3, 5: single rows and
    odd heights.  Both formats x both orders x both ops, three frames of different content a list, padded pitches and a base of its
    own per frame; the four output layouts and three input layouts take turns."""
    i = 0
    for h in (1, 2, 3, 5):
        for fmt in FMTS:
            frames = frames_of(w, h, fmt)
            for order in ORDERS:
                for op, cfg in OPS:
                    check_list(c, frames, w, h, fmt, order, op, cfg, i, OUT_LAYOUTS[i % 4], "grid")
                    i += 1
    assert i == 32


# ---- 2. both store paths in one list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [18, 32])
def test_mixed_store_paths_in_one_list(c, w):
    """Images 0, 4, 1, 2 and 3 bytes past a 16-byte boundary.  With out_pitch a multiple of 4 the first two frames store wide and the
    other three bytes, in one launch; with out_pitch = 3W + 1 all five store bytes.  W = 18 has a ragged last group, W = 32 a full one.
    The two statistics move by exactly those counts."""
    h, offs = 5, (0, 4, 1, 2, 3)
    for fi, fmt in enumerate(FMTS):
        frames = frames_of(w, h, fmt, 5, 200)
        for op, cfg in OPS:
            order = ORDERS[fi]
            want = expected("mixed", frames, w, fmt, order, op, cfg)
            for pitch, n_wide in (((3 * w + 3) // 4 * 4 + 4, 2), (3 * w + 1, 0)):
                src = in_pool(frames, w, h, fi)
                dst = Pool(5, h, 3 * w, pitch, offs)
                assert wide_frames(pitch, dst.ptrs) == n_wide
                before = [c.get_stat(s) for s in STATS]
                run_list(c, op, cfg, src, dst, w, h, fmt, order)
                torch.cuda.synchronize()
                after = [c.get_stat(s) for s in STATS]
                assert [a - b for a, b in zip(after, before)] == [n_wide, 5 - n_wide], (w, fmt, op, pitch)
                assert dst.same(want), (w, fmt, op, pitch)
                assert src.same(frames)


# ---- 3. table indexing and chunk edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_table_indexing_and_chunk_edges(c, n):
    """A chunk is 128 frames: one short chunk, one frame short of a chunk, exactly one, one more, two and one.  Every frame has content
    of its own, so a frame written from another's table entry, LUT or histogram shows."""
    w, h = 16, 2
    rng = np.random.default_rng(7)
    all_frames = [rng.integers(0, 256, (h, 2 * w), dtype=np.uint8) for _ in range(257)]
    frames = all_frames[:n]
    src = in_pool(frames, w, h, 0)
    for oi, (op, cfg) in enumerate(OPS):
        dst = out_pool(n, w, h, "mixed")
        before = [c.get_stat(s) for s in STATS]
        run_list(c, op, cfg, src, dst, w, h, FMT_YUY2 + oi, ORDERS[oi])
        torch.cuda.synchronize()
        nw = wide_frames(dst.pitch, dst.ptrs)
        assert [c.get_stat(s) - b for s, b in zip(STATS, before)] == [nw, n - nw]
        want = expected("chunks", frames, w, FMT_YUY2 + oi, ORDERS[oi], op, cfg)
        got, img = dst.host(), dst.image(want)
        assert np.array_equal(got, img), (n, op, sorted(set(np.argwhere(got != img)[:, 0].tolist()))[:8])
    assert src.same(frames)


# ---- 4. the apply kernel's item loop goes round ------------------------------------------------------------------------------------------
def test_apply_loop_past_its_first_item(c):
    """64 x 130: one workgroup per frame, 130 * 4 = 520 (row, group) items for 256 lanes: every lane takes a second item, eight a third."""
    w, h = 64, 130
    for fi, fmt in enumerate(FMTS):
        frames = frames_of(w, h, fmt, 2, 300)
        for k, lo in enumerate(("wide", "odd")):
            check_list(c, frames, w, h, fmt, ORDERS[(fi + k) % 2], "eq", None, fi + k, lo, "loop")


# ---- 5. every rung of the CLAHE interpolation ladder, other grids ----------------------------------------------------------------------
def rung_frame(shape, fmt, k):
    w, h = shape[:2]
    f = synth.packed422_frame(w, h, fmt, DISTS[k], 500 + k)
    if shape in interp_paths.MODE_SHAPES:
        f = f.copy()
        f[:, fmt - 2:2 * w:2] = clahe_u8_rungs.content(w, h, 100 + k)
    return f


@pytest.mark.parametrize("shape", interp_paths.SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_every_rung(c, shape):
    """Two frames a list; both formats and both orders, clahe_float_tables and clahe_fp_contract both ways, the wide and the byte store
    path: every *_frames_kernel instantiation of the interpolation runs.  The bytes are the reference's in the call's arithmetic mode
    and the batch form's."""
    w, h, tx, ty = shape
    cfg = (interp_paths.CLIP, tx, ty)
    assert len(interp_paths.SHAPES) == 7 and len(interp_paths.OPTIONS) == 4
    try:
        for fmt in FMTS:
            frames = [rung_frame(shape, fmt, k) for k in range(2)]
            for float_tables, contract in interp_paths.OPTIONS:
                c.set_option("clahe_float_tables", float_tables)
                c.set_option("clahe_fp_contract", contract)
                for oi, order in enumerate(ORDERS):
                    for k, lo in enumerate(("wide", "odd")):
                        check_list(c, frames, w, h, fmt, order, "clahe", cfg, oi + k, lo, ("rung", shape), contract,
                                   against_batch=(k == 0))
    finally:
        c.set_option("clahe_float_tables", 1)
        c.set_option("clahe_fp_contract", 0)


@pytest.mark.parametrize("w,h,cfg", [(50, 13, (2.0, 3, 5)), (50, 13, (0.0, 3, 5)), (64, 48, (2.0, 64, 2))])
def test_other_grids(c, w, h, cfg):
    """50 x 13 at 3 x 5: a grid that does not divide the frame (REFLECT_101 padding), with clip 2.0 and with clip 0 (the unclipped
    histogram); 64 x 48 at 64 x 2: 65 pairs, the wide-grid fallback that reads the LUTs from global memory."""
    for fi, fmt in enumerate(FMTS):
        frames = frames_of(w, h, fmt, 2, 400)
        for oi, order in enumerate(ORDERS):
            check_list(c, frames, w, h, fmt, order, "clahe", cfg, fi + oi, OUT_LAYOUTS[(2 * fi + oi) % 4], "grids")


# ---- 6. every row keeps its own chroma ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_per_row_chroma(c, fmt):
    """Even rows with strong chroma, odd rows with chroma 128 (the frame of the batch test), through both ops of the list form: the
    result is the batch form's and differs from what packed -> NV12 (MI_UV_COPY) followed by cvt_color_420(YUV2BGR_NV12) returns."""
    w, h = 48, 6
    frames = [ref.alternating_chroma_frame(w, h, fmt, 11), ref.alternating_chroma_frame(w, h, fmt, 12)]
    src = in_pool(frames, w, h, 0)
    d_in = torch.from_numpy(frames[0]).to("cuda:0")
    nv12 = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")
    two = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0")
    for op, cfg in OPS:
        dst = out_pool(2, w, h, "wide")
        run_list(c, op, cfg, src, dst, w, h, fmt, ORDER_BGR)
        torch.cuda.synchronize()
        batch = run_batch(c, op, cfg, frames, w, h, fmt, ORDER_BGR)
        assert dst.same(list(batch)), (fmt, op, "the list form differs from the batch form")
        assert np.array_equal(batch[0], ref.expected(frames[0], w, fmt, ORDER_BGR, op, cfg))
        if op == "eq":
            c.equalize_hist_packed422_to_nv12_batch_dev(d_in, nv12, None, w, h, 1, fmt, UV_COPY, stream=stream())
        else:
            c.clahe_packed422_to_nv12_batch_dev(d_in, nv12, None, w, h, 1, fmt, UV_COPY, *cfg, stream=stream())
        c.cvt_color_420_batch_dev(nv12, two, w, h, 1, mi_lumaeq.COLOR_YUV2BGR_NV12, stream=stream())
        torch.cuda.synchronize()
        two_h = two.cpu().numpy()
        got = dst.host()[0, dst.offs[0]: dst.offs[0] + dst.pitch * h].reshape(h, dst.pitch)[:, : 3 * w].reshape(h, w, 3)
        assert not np.array_equal(two_h[0::2], got[0::2]) and not np.array_equal(two_h[1::2], got[1::2]), (fmt, op)
    assert src.same(frames)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(c):
    w, h, n = 32, 6, 4
    frames = frames_of(w, h, FMT_YUY2, n, 700)
    src = in_pool(frames, w, h, 0)
    dst = out_pool(n, w, h, "wide")
    L, hd = c._L, c._h
    Entry = mi_lumaeq.Packed422BgrFrameDev
    good = [(src.ptrs[k], dst.ptrs[k]) for k in range(n)]
    base = dict(n=n, w=w, h=h, ip=src.pitch, op=dst.pitch, fmt=FMT_YUY2, order=ORDER_BGR)

    def table(entries):
        arr = (Entry * max(1, len(entries)))()
        for k, (i, o) in enumerate(entries):
            arr[k] = Entry(i, o)
        return arr

    def args(entries=good, null_list=False, **kw):
        a = dict(base)
        a.update(kw)
        return (hd, None if null_list else table(entries), a["n"], a["w"], a["h"], a["ip"], a["op"], a["fmt"], a["order"])

    def both(**kw):
        return (L.mi_equalize_hist_packed422_to_bgr_frames_dev(*args(**kw), stream()),
                L.mi_clahe_packed422_to_bgr_frames_dev(*args(**kw), 2.0, 2, 2, stream()))

    def with_entry(k, i=None, o=None):
        e = list(good)
        e[k] = (e[k][0] if i is None else i, e[k][1] if o is None else o)
        return e

    stats0 = [c.get_stat(s) for s in STATS]
    bad = [dict(null_list=True),
           dict(entries=with_entry(0, i=0)), dict(entries=with_entry(0, o=0)),                          # null in / out, first and last
           dict(entries=[(None, good[0][1])] + good[1:]), dict(entries=good[:-1] + [(good[-1][0], None)]),
           dict(entries=good[:-1] + [(None, good[-1][1])]),
           dict(entries=with_entry(2, i=good[2][0] + 2)), dict(entries=with_entry(1, i=good[1][0] + 1)),  # in not a multiple of 4, index > 0
           dict(ip=2 * w + 2), dict(ip=2 * w + 1), dict(ip=2 * w - 4),                                   # in_pitch
           dict(op=3 * w - 1), dict(op=3 * w - 4),                                                       # out_pitch < 3W
           dict(order=2), dict(order=-1), dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1),           # order, format
           dict(w=w - 1), dict(w=w - 1, h=0), dict(w=w - 1, n=0), dict(w=1),                             # odd width, also next to a zero size
           dict(w=-2), dict(h=-1), dict(n=-1),                                                           # negative sizes
           dict(entries=with_entry(2, o=good[2][0] + 8)),                                                # an image inside its own input
           dict(entries=with_entry(n - 1, o=good[n - 1][0] + src.pitch * (h - 1) + 2 * w - 1)),          # ... meeting its last byte
           dict(entries=with_entry(1, o=good[1][0]))]                                                    # in == out
    for kw in bad:
        assert both(**kw) == (BAD_ARG, BAD_ARG), kw
    for tx, ty in ((0, 2), (2, 0), (-1, 2)):
        assert L.mi_clahe_packed422_to_bgr_frames_dev(*args(), 2.0, tx, ty, stream()) == BAD_ARG
    # nothing to do: MI_OK, nothing written -- also with a null list when there are no frames
    for kw in (dict(n=0), dict(n=0, null_list=True), dict(w=0), dict(h=0)):
        assert both(**kw) == (0, 0), kw
    torch.cuda.synchronize()
    assert dst.same(), "a refused or empty call wrote"
    assert src.same(frames), "a refused or empty call wrote an input"
    assert [c.get_stat(s) for s in STATS] == stats0, "a refused or empty call was counted"
    # an image may lie next to its input, and the same input may feed two images: legal, and the context still works
    dst2 = out_pool(n, w, h, "odd")
    src2 = SimpleNamespace(ptrs=[src.ptrs[0]] * n, pitch=src.pitch)
    run_list(c, "clahe", (2.0, 2, 2), src2, dst2, w, h, FMT_YUY2, ORDER_RGB)
    torch.cuda.synchronize()
    assert dst2.same(expected("refuse", frames[:1], w, FMT_YUY2, ORDER_RGB, "clahe", (2.0, 2, 2)) * n)
    assert dst.same() and src.same(frames)


# ---- 8. streams, profiling, the pipe -----------------------------------------------------------------------------------------------------
def test_streams(c):
    w, h = 64, 9
    frames = frames_of(w, h, FMT_UYVY, 3, 900)
    src = in_pool(frames, w, h, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for st in (side.cuda_stream, mi_lumaeq.STREAM_CTX):
        for op, cfg in (("eq", None), ("clahe", (2.0, 4, 3))):
            dst = out_pool(3, w, h, "mixed")
            torch.cuda.synchronize()
            run_list(c, op, cfg, src, dst, w, h, FMT_UYVY, ORDER_RGB, st=st)
            if st == side.cuda_stream:
                side.synchronize()
            else:
                c.synchronize(mi_lumaeq.STREAM_CTX)
            assert dst.same(expected("streams", frames, w, FMT_UYVY, ORDER_RGB, op, cfg)), (st, op)
    assert src.same(frames)


def test_launch_accounting():
    """The list form charges the slots the batch form charges, with the same counts (three frames: one chunk)."""
    w, h = 64, 48
    frames = frames_of(w, h, FMT_YUY2, 3, 1000)
    src = in_pool(frames, w, h, 0)
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (2.0, 64, 2))):
            c.profile_read(reset=True)
            run_batch(c, op, cfg, frames, w, h, FMT_YUY2, ORDER_BGR)
            batch = c.profile_read(reset=True)
            dst = out_pool(3, w, h, "wide")
            run_list(c, op, cfg, src, dst, w, h, FMT_YUY2, ORDER_BGR)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            assert len(prof) == 10
            for k in mi_lumaeq.KERNEL_NAMES:
                assert prof[k]["launches"] == batch[k]["launches"], (op, cfg, k, prof[k], batch[k])
            if op == "eq":
                for k in mi_lumaeq.KERNEL_NAMES:
                    want = 1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0
                    assert prof[k]["launches"] == want, (k, prof[k])
            else:
                assert prof["tile_hist_kernel"]["launches"] == 1 and prof["clahe_interp_kernel"]["launches"] == 1, prof
                assert prof["lut_apply_kernel"]["launches"] == 0 and prof["hist_partial_kernel"]["launches"] == 0
            assert dst.same(expected("prof", frames, w, FMT_YUY2, ORDER_BGR, op, cfg))
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    frames = frames_of(w, h, FMT_YUY2, 1, 1100)
    src = in_pool(frames, w, h, 0)
    dst = out_pool(1, w, h, "tight")
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run_list(c, op, cfg, src, dst, w, h, FMT_YUY2, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same(), "a refused call wrote"
        assert [c.get_stat(s) for s in STATS] == [0, 0]
