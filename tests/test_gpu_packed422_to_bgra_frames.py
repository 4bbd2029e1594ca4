"""Packed 4:2:2 frames in (YUY2 / UYVY), four-channel BGRA / RGBA images (CV_8UC4, A = 255) out on a LIST of device frames:
mi_equalize_hist_packed422_to_bgra_frames_dev and mi_clahe_packed422_to_bgra_frames_dev.  The expected image is
tests/packed422_bgra_ref.py (the three-channel reference with a fourth channel of 255), and the batch form run on the same pixels one
frame a call.  Every frame and every image lives in a sentinel-filled allocation of its own, at a padded pitch and a base of its own;
the WHOLE allocation is compared, the inputs must read unchanged, and every comparison in this file is exact bytes.  The statistics
"packed422_bgra_list_frames_wide" / "packed422_bgra_list_frames_bytes" count the frames by store path under the header's rule
(packed422_bgra_ref.frame_wide); no other counter of this form or of its neighbours moves on a list call."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mi_lumaeq
import packed422_bgra_ref as ref
from packed422_bgra_ref import SENT, EQ, CL22, CL54, CL642, COUNTERS, FOREIGN, FMT_YUY2, FMT_UYVY, ORDER_BGR, ORDER_RGB

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
FMTS = [FMT_YUY2, FMT_UYVY]
ORDERS = [ORDER_BGR, ORDER_RGB]
SLACK = 48                                                       # sentinel bytes behind the last row of every allocation


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small allocations leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def counters(c):
    return [c.get_stat(s) for s in COUNTERS + FOREIGN]


def moved(c, before):
    return tuple(a - b for a, b in zip(counters(c), before))


class Pool:
    """n sentinel-filled device allocations, one per frame: `h` rows of `row` payload bytes at `pitch`, frame k `offs[k % len]` bytes
    into its allocation (every allocation starts at a multiple of 16)."""

    def __init__(self, n, h, row, pitch, offs):
        self.n, self.h, self.row, self.pitch = n, h, row, pitch
        self.offs = [offs[k % len(offs)] for k in range(n)]
        self.total = max(offs) + pitch * h + SLACK
        self.bufs = [torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.ptrs = [b.data_ptr() + o for b, o in zip(self.bufs, self.offs)]

    def image(self, payloads=None):
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
        return torch.stack(self.bufs).cpu().numpy()

    def same(self, payloads=None):
        return np.array_equal(self.host(), self.image(payloads))


def run_list(c, op, src, dst, w, h, fmt, order, st=None):
    kw = dict(in_pitch=src.pitch, out_pitch=dst.pitch, stream=stream() if st is None else st)
    if op[0] == "eq":
        c.equalize_hist_packed422_to_bgra_frames(src.ptrs, dst.ptrs, w, h, fmt, order, **kw)
    else:
        c.clahe_packed422_to_bgra_frames(src.ptrs, dst.ptrs, w, h, fmt, order, *op[1], **kw)


def run_batch_one_by_one(c, op, frames, w, h, fmt, order):
    """The batch form, n_frames = 1 a call, tight on both sides; returns the images (n x h x w x 4)."""
    outs = []
    for f in frames:
        d_in = torch.from_numpy(np.ascontiguousarray(f[:, : 2 * w])).to("cuda:0")
        d_out = torch.full((h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
        if op[0] == "eq":
            c.equalize_hist_packed422_to_bgra_batch_dev(d_in, d_out, w, h, 1, fmt, order, stream=stream())
        else:
            c.clahe_packed422_to_bgra_batch_dev(d_in, d_out, w, h, 1, fmt, order, *op[1], stream=stream())
        torch.cuda.synchronize()
        outs.append(d_out.cpu().numpy())
    return outs


_luma = {}


def expected(key, frames, w, fmt, order, op, contract=False):
    out = []
    for k, f in enumerate(frames):
        lk = (key, w, f.shape[0], fmt, k, op, bool(contract))
        if lk not in _luma:
            _luma[lk] = ref.mapped_luma(ref.luma(f, w, fmt), op[0], op[1], contract)
        out.append(ref.expected(f, w, fmt, order, op[0], op[1], contract, _luma[lk]))
    return out


def four_frames(w, h, fmt, seed):
    """Independent random Y, U, V, and (frame 1) the alternating-chroma frame that a shared chroma row cannot pass."""
    fs = [ref.random_frame(w, h, fmt, seed + i) for i in range(4)]
    fs[1] = ref.alternating_chroma_frame(w, h, fmt, seed + 1)
    return fs


# ---- 1. both store paths and every input phase in one list ---------------------------------------------------------------------------
@pytest.mark.parametrize("op", [EQ, CL22, CL54, CL642], ids=["eq", "clahe2x2", "clahe5x4-pads", "clahe64x2-global"])
def test_four_frames_at_offsets_0_1_4_16(c, op):
    """Four frames of 40 x 6 (two full 16-column groups and a ragged one) whose images sit 0, 1, 4 and 16 bytes past a 16-byte boundary,
    in one call: three wide frames and one byte frame, by counter; the inputs at phases 0, 4, 8, 12.  Every image is the oracle's, and
    the whole result is that of four n_frames = 1 batch calls.  The LDS rungs run with clahe_float_tables and clahe_fp_contract both
    ways: every *_frames_kernel instantiation runs."""
    w, h = 40, 6
    options = ref.OPTIONS if op in ref.LDS_OPS else ref.OPTIONS[:1]
    try:
        for fi, fmt in enumerate(FMTS):
            frames = four_frames(w, h, fmt, 100)
            src = Pool(4, h, 2 * w, 2 * w + 4, (0, 4, 8, 12)).upload(frames)
            for float_tables, contract in options:
                c.set_option("clahe_float_tables", float_tables)
                c.set_option("clahe_fp_contract", contract)
                for order in ORDERS:
                    dst = Pool(4, h, 4 * w, 4 * w + 16, (0, 1, 4, 16))
                    assert [ref.frame_wide(p, dst.pitch) for p in dst.ptrs] == [True, False, True, True]
                    before = counters(c)
                    run_list(c, op, src, dst, w, h, fmt, order)
                    torch.cuda.synchronize()
                    assert moved(c, before) == (0, 0, 3, 1) + (0,) * 8, (op, fmt, order)
                    want = expected("four", frames, w, fmt, order, op, contract)
                    got, img = dst.host(), dst.image(want)
                    assert np.array_equal(got, img), (op, fmt, order, float_tables, contract, np.argwhere(got != img)[:8])
                    assert src.same(frames), "an input allocation was written"
                    batch = run_batch_one_by_one(c, op, frames, w, h, fmt, order)
                    assert dst.same(batch), (op, fmt, order, "the list form differs from four batch calls")
    finally:
        c.set_option("clahe_float_tables", 1)
        c.set_option("clahe_fp_contract", 0)


def test_odd_pitch_makes_every_frame_a_byte_frame(c):
    w, h = 40, 6
    frames = four_frames(w, h, FMT_UYVY, 150)
    src = Pool(4, h, 2 * w, 2 * w, (0, 4, 8, 12)).upload(frames)
    for op in (EQ, CL22, CL642):
        dst = Pool(4, h, 4 * w, 4 * w + 1, (0, 1, 4, 16))
        before = counters(c)
        run_list(c, op, src, dst, w, h, FMT_UYVY, ORDER_RGB)
        torch.cuda.synchronize()
        assert moved(c, before) == (0, 0, 0, 4) + (0,) * 8, op
        assert dst.same(expected("oddpitch", frames, w, FMT_UYVY, ORDER_RGB, op)), op
    assert src.same(frames)


# ---- 2. the 128-frame chunk ------------------------------------------------------------------------------------------------------------
def test_130_frames_cross_the_chunk(c):
    """130 frames of 16 x 2: a chunk of 128 and one of 2.  Every frame has content of its own, so a frame written from another's table
    entry, LUT or histogram shows; entry 129 reads the input of entry 3 again (the same input in two entries)."""
    w, h, n = 16, 2, 130
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (h, 2 * w), dtype=np.uint8) for _ in range(n - 1)]
    src = Pool(n - 1, h, 2 * w, 2 * w + 4, (0, 4, 8, 12)).upload(frames)
    ins = SimpleNamespace(ptrs=src.ptrs + [src.ptrs[3]], pitch=src.pitch)
    for oi, op in enumerate((EQ, CL22)):
        fmt, order = FMTS[oi], ORDERS[oi]
        dst = Pool(n, h, 4 * w, 4 * w + 8, (0, 1, 2, 3, 4))
        nw = sum(ref.frame_wide(p, dst.pitch) for p in dst.ptrs)
        assert nw == 2 * 26
        before = counters(c)
        run_list(c, op, ins, dst, w, h, fmt, order)
        torch.cuda.synchronize()
        assert moved(c, before) == (0, 0, nw, n - nw) + (0,) * 8, op
        want = expected("chunk", frames, w, fmt, order, op)
        want = want + [want[3]]
        got, img = dst.host(), dst.image(want)
        assert np.array_equal(got, img), (op, sorted(set(np.argwhere(got != img)[:, 0].tolist()))[:8])
    assert src.same(frames)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(c):
    w, h, n = 32, 6, 4
    frames = four_frames(w, h, FMT_YUY2, 700)
    src = Pool(n, h, 2 * w, 2 * w + 4, (4, 8, 12)).upload(frames)
    dst = Pool(n, h, 4 * w, 4 * w + 4, (4, 16, 8))
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
        return (L.mi_equalize_hist_packed422_to_bgra_frames_dev(*args(**kw), stream()),
                L.mi_clahe_packed422_to_bgra_frames_dev(*args(**kw), 2.0, 2, 2, stream()))

    def with_entry(k, i=None, o=None):
        e = list(good)
        e[k] = (e[k][0] if i is None else i, e[k][1] if o is None else o)
        return e

    before = counters(c)
    last = n - 1
    bad = [dict(null_list=True),
           # a bad LAST entry: null out, null in, `in` not a multiple of 4, the image's rows meeting the rows of its own input
           dict(entries=good[:-1] + [(good[last][0], None)]), dict(entries=good[:-1] + [(None, good[last][1])]),
           dict(entries=with_entry(last, i=good[last][0] + 2)), dict(entries=with_entry(last, i=good[last][0] + 1)),
           dict(entries=with_entry(last, o=good[last][0] + 8)),                                          # an image inside its own input
           dict(entries=with_entry(last, o=good[last][0] + src.pitch * (h - 1) + 2 * w - 1)),            # ... meeting its last byte
           dict(entries=with_entry(last, o=good[last][0] - dst.pitch * (h - 1) - 4 * w + 1)),            # ... its last byte meeting the first
           dict(entries=with_entry(last, o=good[last][0])),                                              # in == out
           dict(entries=with_entry(0, i=0)), dict(entries=with_entry(0, o=0)),                           # the first entry
           dict(ip=2 * w + 2), dict(ip=2 * w + 1), dict(ip=2 * w - 4),                                   # in_pitch
           dict(op=4 * w - 1), dict(op=4 * w - 4), dict(op=3 * w),                                       # out_pitch < 4W
           dict(order=2), dict(order=-1), dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1),           # order, format
           dict(w=w - 1), dict(w=w - 1, h=0), dict(w=w - 1, n=0), dict(w=1),                             # odd width, also next to a zero size
           dict(w=-2), dict(h=-1), dict(n=-1)]                                                           # negative sizes
    for kw in bad:
        assert both(**kw) == (BAD_ARG, BAD_ARG), kw
    for tx, ty in ((0, 2), (2, 0), (-1, 2)):
        assert L.mi_clahe_packed422_to_bgra_frames_dev(*args(), 2.0, tx, ty, stream()) == BAD_ARG
    # the grids and heights the batch form refuses
    assert L.mi_clahe_packed422_to_bgra_frames_dev(*args(), 2.0, 512, 256, stream()) == UNSUPPORTED
    assert L.mi_clahe_packed422_to_bgra_frames_dev(*args(w=64, h=65536, ip=128, op=256), 2.0, 64, 1, stream()) == UNSUPPORTED
    # nothing to do: MI_OK, nothing written -- also with a null list when there are no frames
    for kw in (dict(n=0), dict(n=0, null_list=True), dict(w=0), dict(h=0)):
        assert both(**kw) == (0, 0), kw
    torch.cuda.synchronize()
    assert dst.same(), "a refused or empty call wrote"
    assert src.same(frames), "a refused or empty call wrote an input"
    assert not any(moved(c, before)), "a refused or empty call was counted"
    # and the context still works
    run_list(c, CL22, src, dst, w, h, FMT_YUY2, ORDER_RGB)
    torch.cuda.synchronize()
    assert dst.same(expected("refuse", frames, w, FMT_YUY2, ORDER_RGB, CL22)) and src.same(frames)


# ---- 4. streams, hipGraph, profiling, the pipe -----------------------------------------------------------------------------------------
def test_streams_and_graph():
    """A side stream, MI_STREAM_CTX, then one call captured behind its eager twin and replayed twice onto new content."""
    w, h = 40, 6
    frames = four_frames(w, h, FMT_UYVY, 900)
    src = Pool(4, h, 2 * w, 2 * w + 4, (0, 4, 8, 12)).upload(frames)
    with mi_lumaeq.Context(0) as c:
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        for st in (side.cuda_stream, mi_lumaeq.STREAM_CTX):
            for op in (EQ, CL22):
                dst = Pool(4, h, 4 * w, 4 * w + 16, (0, 1, 4, 16))
                torch.cuda.synchronize()
                run_list(c, op, src, dst, w, h, FMT_UYVY, ORDER_RGB, st=st)
                if st == side.cuda_stream:
                    side.synchronize()
                else:
                    c.synchronize(mi_lumaeq.STREAM_CTX)
                assert dst.same(expected("streams", frames, w, FMT_UYVY, ORDER_RGB, op)), (st, op)
        for op in (EQ, CL22):
            dst = Pool(4, h, 4 * w, 4 * w + 16, (0, 1, 4, 16))
            run_list(c, op, src, dst, w, h, FMT_UYVY, ORDER_BGR)            # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run_list(c, op, src, dst, w, h, FMT_UYVY, ORDER_BGR, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                fresh = four_frames(w, h, FMT_UYVY, 910 + 10 * rep)
                src.upload(fresh)
                for b in dst.bufs:
                    b.fill_(SENT)
                g.replay()
                torch.cuda.synchronize()
                assert dst.same(expected(("graph", rep), fresh, w, FMT_UYVY, ORDER_BGR, op)), ("graph replay", op, rep)
                assert src.same(fresh)
            src.upload(frames)


def test_launch_accounting():
    """The list form charges the slots the batch form charges, with the same counts (three frames: one chunk)."""
    w, h = 64, 48
    frames = four_frames(w, h, FMT_YUY2, 1000)[:3]
    src = Pool(3, h, 2 * w, 2 * w + 4, (4, 8, 12)).upload(frames)
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for op in (EQ, ("clahe", (2.0, 8, 8)), CL642):
            dst = Pool(3, h, 4 * w, 4 * w + 4, (4, 16, 8))
            c.profile_read(reset=True)
            run_list(c, op, src, dst, w, h, FMT_YUY2, ORDER_BGR)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            assert len(prof) == 10
            if op[0] == "eq":
                for k in mi_lumaeq.KERNEL_NAMES:
                    want = 1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0
                    assert prof[k]["launches"] == want, (k, prof[k])
            else:
                for k in ("equalize_fused_kernel", "fused_finish_kernel", "color_kernel", "analyze_diff_kernel", "hist_partial_kernel",
                          "equalize_lut_kernel", "lut_apply_kernel"):
                    assert prof[k]["launches"] == 0, (op, k, prof[k])
                assert prof["tile_hist_kernel"]["launches"] == 1 and prof["clahe_interp_kernel"]["launches"] == 1, prof
            assert dst.same(expected("prof", frames, w, FMT_YUY2, ORDER_BGR, op))
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = mi_lumaeq.synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    frames = four_frames(w, h, FMT_YUY2, 1100)[:1]
    src = Pool(1, h, 2 * w, 2 * w, (0,)).upload(frames)
    dst = Pool(1, h, 4 * w, 4 * w, (0,))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op in (EQ, ("clahe", (2.0, 8, 8))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run_list(c, op, src, dst, w, h, FMT_YUY2, ORDER_BGR)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert dst.same(), "a refused call wrote"
        assert not any(counters(c))
