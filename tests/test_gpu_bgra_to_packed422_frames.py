"""Four-channel BGRA / RGBA (CV_8UC4) images in, pitched packed 4:2:2 frames (YUY2 / UYVY) out on a LIST of device frames:
mi_equalize_hist_bgra_to_packed422_frames_dev and mi_clahe_bgra_to_packed422_frames_dev.  Expected bytes: bgra_packed422_ref (the
three-channel reference on the image with its fourth byte removed, which tests/test_bgra_to_packed422_abi.py backs on the CPU), the
oracle's work computed once per image and shared.  Every image and every output frame is a sentinel-filled torch allocation of its own
with guard bytes before and behind the payload; the WHOLE allocation is compared, inputs included, and every comparison is exact bytes.
The frames of a list have distinct full-range random content, the fourth byte included.  After every call the deltas of the four
counters "bgra_packed422_vec" / "bgra_packed422_bytes" / "bgra_packed422_list_frames_vec" / "bgra_packed422_list_frames_bytes" are
asserted, by the header's rule restated in bgra_packed422_ref.frame_vec, and no bgr_packed422* counter may move.

How many workgroups stage 1 gets per frame (B) is not observable and no test asserts it, but the shapes of
test_loops_past_their_first_step are chosen by the documented bound: launch_bgra_to_packed422 computes
B = min(blocks_per_frame(W*H*3 bytes, H rows, n, 2048), ceil(items / 256)) with items counted by what the SHAPE allows (16-pixel
groups when W % 16 == 0 and both pitches are multiples of 16, else macropixels), and blocks_per_frame never returns more than
max(1, floor(bytes / 16384)) nor, for rows > 1, more than rows: B <= 2 at 8192 x 2, B <= 3 at 4112 x 4, B = 1 at 66 x 35 (the module
docstring of tests/test_gpu_bgra_to_packed422.py says which lanes take a second step for every such B).  A frame off the 16-byte grid
in a launch whose shape allows the groups walks W*H/2 macropixels with the stride of the vector grid: 8224 macropixels at 4112 x 4, at
most 768 a step."""
import numpy as np
import pytest
import torch

import mi_lumaeq
from mi_lumaeq import ORDER_BGR, ORDER_RGB, UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY
from bgra_packed422_ref import (SENT, COUNTERS, LIST_COUNTERS, SIBLING_COUNTERS, BgraIn, P422Out, convert, mapped_luma, pack, rand_images4,
                                first3, frame_vec)

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
ORDERS = [ORDER_BGR, ORDER_RGB]
FMTS = [FMT_YUY2, FMT_UYVY]
UV_MODES = [UV_COPY, UV_FILL128]
EQ = ("eq", None)
ALL = COUNTERS + LIST_COUNTERS
GUARD, SLACK = 32, 48                                            # sentinel bytes before the first and behind the last row of an allocation
CHUNK = 128                                                      # kPacked422FramesPerLaunch (tests/test_bgra_to_packed422_frames_abi.py pins it)
_ref = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def counters(c):
    return tuple(c.get_stat(k) for k in ALL)


def siblings(c):
    return tuple(c.get_stat(k) for k in SIBLING_COUNTERS)


def expected(img, op, order, fmt, uv_mode, contract=False):
    """bgra_packed422_ref.expected with the conversion and the mapped luma of an image computed once: they do not depend on the format
    or the UV mode."""
    img = first3(img)
    key = (img.shape, img.tobytes(), order)
    if key not in _ref:
        _ref[key] = convert(img, order)
    y, uv = _ref[key]
    mkey = key + (op, contract)
    if mkey not in _ref:
        _ref[mkey] = mapped_luma(y, op, contract)
    return pack(_ref[mkey], uv if uv_mode == UV_COPY else np.full_like(uv, 128), fmt)


class Pool:
    """n sentinel-filled device allocations, one per frame: `h` rows of `row` payload bytes at `pitch`; the payload of allocation k
    starts GUARD + offs[k % len] bytes in, GUARD being a multiple of 16 and every allocation 16-byte aligned."""

    def __init__(self, n, h, row, pitch, offs=(0,)):
        self.n, self.h, self.row, self.pitch = n, h, row, pitch
        self.offs = [GUARD + offs[k % len(offs)] for k in range(n)]
        self.total = max(self.offs) + pitch * h + SLACK
        self.bufs = [torch.full((self.total,), SENT, dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.ptrs = [b.data_ptr() + o for b, o in zip(self.bufs, self.offs)]

    def image(self, payloads=None):
        """What the n allocations hold: sentinels, and payloads[k] (h x row bytes) in the rows of allocation k."""
        a = np.full((self.n, self.total), SENT, np.uint8)
        for k, p in enumerate(payloads or []):
            o = self.offs[k]
            a[k, o: o + self.pitch * self.h].reshape(self.h, self.pitch)[:, : self.row] = p.reshape(self.h, self.row)
        return a

    def upload(self, payloads):
        a = self.image(payloads)
        for k, b in enumerate(self.bufs):
            b.copy_(torch.from_numpy(a[k]))
        return self

    def clear(self):
        for b in self.bufs:
            b.fill_(SENT)

    def host(self):
        return torch.stack(self.bufs).cpu().numpy() if self.n else np.zeros((0, self.total), np.uint8)

    def same(self, payloads=None):
        got, want = self.host(), self.image(payloads)
        return np.array_equal(got, want), int((got != want).sum()), np.argwhere(got != want)[:8].tolist()


def pools(images, w, h, in_pitch=None, out_pitch=None, in_offs=(0,), out_offs=(0,)):
    n = len(images)
    return (Pool(n, h, 4 * w, in_pitch or 4 * w, in_offs).upload(images), Pool(n, h, 2 * w, out_pitch or 2 * w, out_offs))


def vec_frames(w, in_pitch, out_pitch, ins, outs):
    return sum(1 for i, o in zip(ins, outs) if frame_vec(w, in_pitch, out_pitch, i, o))


def run(c, op, ins, outs, w, h, order, fmt, uv_mode, in_pitch, out_pitch, st=None):
    kind, cfg = op
    kw = dict(in_pitch=in_pitch, out_pitch=out_pitch, stream=stream() if st is None else st)
    if kind == "eq":
        c.equalize_hist_bgra_to_packed422_frames(ins, outs, w, h, order, fmt, uv_mode, **kw)
    else:
        c.clahe_bgra_to_packed422_frames(ins, outs, w, h, order, fmt, uv_mode, *cfg, **kw)


def check(c, images, op, order, fmt, uv_mode, src, dst, w, h, contract=False, n_vec=None, sync=None, st=None):
    """One list call on the uploaded `images`: every output allocation is the reference's image of it, every input allocation is what
    was uploaded, the two list counters moved by the frames on each walk -- n_frames in total -- while the per-call pair and the
    three-channel form's counters stood still."""
    dst.clear()
    torch.cuda.synchronize()                                     # the call may run on another stream than the fill
    before, sib = counters(c), siblings(c)
    run(c, op, src.ptrs, dst.ptrs, w, h, order, fmt, uv_mode, src.pitch, dst.pitch, st=st)
    (sync or torch.cuda.synchronize)()
    why = (w, h, op, order, fmt, uv_mode)
    ok, nbad, where = dst.same([expected(img, op, order, fmt, uv_mode, contract) for img in images])
    assert ok, (why, nbad, where)
    assert src.same(images)[0], (why, "an input allocation was written")
    nv = vec_frames(w, src.pitch, dst.pitch, src.ptrs, dst.ptrs)
    assert n_vec is None or nv == n_vec, (why, nv, n_vec)
    after = counters(c)
    assert tuple(a - b for a, b in zip(after, before)) == (0, 0, nv, len(images) - nv), (why, before, after)
    assert siblings(c) == sib, "a three-channel counter moved"


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small allocations leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    _ref.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
PARITY = [
    # id, W, H, frames, in_pitch, out_pitch, in offsets, out offsets, frames on the vector walk, the ops: equalizeHist, a CLAHE grid
    # that divides the frame and one that does not
    ("16x1", 16, 1, 1, None, None, (0,), (0,), 1, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 3, 1))]),       # one vector group
    ("2x1", 2, 1, 1, None, None, (0,), (0,), 0, [EQ, ("clahe", (2.0, 1, 1)), ("clahe", (2.0, 2, 1))]),         # one macropixel
    ("48x5", 48, 5, 2, None, None, (0,), (0,), 2, [EQ, ("clahe", (2.0, 3, 5)), ("clahe", (2.0, 5, 4))]),       # gx_n = 3, odd height
    ("66x35-odd", 66, 35, 2, 265, 136, (1, 5), (4, 12), 0, [EQ, ("clahe", (2.0, 3, 5)), ("clahe", (3.0, 4, 3))]),   # nothing aligned
    ("64x32-pitched", 64, 32, 2, 272, 144, (0, 16), (16, 48), 2, [EQ, ("clahe", (2.0, 4, 2)), ("clahe", (4.0, 5, 3))]),
]


@pytest.mark.parametrize("name,w,h,n,ip,op_,io,oo,n_vec,ops", PARITY, ids=[p[0] for p in PARITY])
def test_parity(c, name, w, h, n, ip, op_, io, oo, n_vec, ops):
    images = rand_images4(w, h, n, 131)
    src, dst = pools(images, w, h, ip, op_, io, oo)
    for op in ops:
        for order in ORDERS:
            for fmt in FMTS:
                for uv_mode in UV_MODES:
                    check(c, images, op, order, fmt, uv_mode, src, dst, w, h, n_vec=n_vec)


# ---- 2. the walk is each frame's own ---------------------------------------------------------------------------------------------
SKEW_IN, SKEW_OUT = (0, 8, 0, 8, 0), (0, 0, 4, 4, 0)             # aligned, image at +8, frame at +4, both skewed, aligned


def test_per_frame_walk(c):
    """Five frames in one list, one launch: the two aligned ones take the 16-pixel groups, the other three the macropixels; the
    counters move by exactly those numbers, five in total."""
    w, h = 32, 3
    images = rand_images4(w, h, 5, 132)
    src, dst = pools(images, w, h, None, None, SKEW_IN, SKEW_OUT)
    for op, order, fmt, uv_mode in ((EQ, ORDER_BGR, FMT_YUY2, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_RGB, FMT_UYVY, UV_FILL128)):
        check(c, images, op, order, fmt, uv_mode, src, dst, w, h, n_vec=2)


@pytest.mark.parametrize("term,w,ip,op_", [("in_pitch", 32, 136, 64), ("out_pitch", 32, 128, 72), ("width", 24, 96, 48)])
def test_one_shape_term_at_a_time(c, term, w, ip, op_):
    """One term of the shape misses 16 (every other one a multiple of 16): no frame of the list takes the groups, aligned or not."""
    h = 3
    assert [t for t, v in (("in_pitch", ip), ("out_pitch", op_), ("width", w)) if v % 16] == [term]
    images = rand_images4(w, h, 4, 133)
    src, dst = pools(images, w, h, ip, op_, SKEW_IN, SKEW_OUT)
    assert src.ptrs[0] % 16 == 0 and dst.ptrs[0] % 16 == 0
    for op, order, fmt, uv_mode in ((EQ, ORDER_RGB, FMT_UYVY, UV_COPY), (("clahe", (2.0, 2, 2)), ORDER_BGR, FMT_YUY2, UV_FILL128)):
        check(c, images, op, order, fmt, uv_mode, src, dst, w, h, n_vec=0)


# ---- 3. equal to the batch form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=["yuy2", "uyvy"])
@pytest.mark.parametrize("op", [EQ, ("clahe", (2.0, 4, 2))], ids=["eq", "clahe"])
def test_equal_to_the_batch_form(c, op, fmt):
    """Each frame's bytes equal the batch form's for that frame alone: a list built from the addresses of a strided batch layout
    (padded rows, gaps between frames) gives byte for byte what n batch calls of one frame each write into the same layout -- the whole
    allocation -- and both are the reference."""
    w, h, n = 64, 32, 3
    images = rand_images4(w, h, n, 134)
    src = BgraIn(w, h, n, pitch=272, frame_gap=64, off=32).upload(images)
    one, two = (P422Out(w, h, n, pitch=144, frame_gap=32, off=16) for _ in range(2))
    before = counters(c)
    for f in range(n):                                            # frame f alone
        kw = dict(src.kw(), **one.kw(), stream=stream())
        i, o = src.ptr + f * src.fstride, one.ptr + f * one.fstride
        if op is EQ:
            c.equalize_hist_bgra_to_packed422_batch_dev(i, o, w, h, 1, ORDER_RGB, fmt, UV_COPY, **kw)
        else:
            c.clahe_bgra_to_packed422_batch_dev(i, o, w, h, 1, ORDER_RGB, fmt, UV_COPY, *op[1], **kw)
    mid = counters(c)
    run(c, op, [src.ptr + f * src.fstride for f in range(n)], [two.ptr + f * two.fstride for f in range(n)], w, h, ORDER_RGB, fmt, UV_COPY,
        src.pitch, two.pitch)
    torch.cuda.synchronize()
    after = counters(c)
    assert np.array_equal(one.host(), two.host()), (op, fmt)
    assert two.same([expected(img, op, ORDER_RGB, fmt, UV_COPY) for img in images])[0], (op, fmt)
    assert np.array_equal(src.host(), src.image(images))
    assert tuple(a - b for a, b in zip(mid, before)) == (n, 0, 0, 0) and tuple(a - b for a, b in zip(after, mid)) == (0, 0, n, 0)


# ---- 4. chunk seam -----------------------------------------------------------------------------------------------------------------
def test_chunk_seam(c):
    """One frame more than a chunk of 128: two launch sequences, the second of one frame.  The list order is a fixed permutation of the
    allocation order.  Equal 16 x 2 frames would have equal histograms, so the frames around the seam get disjoint luma ranges (middle,
    dark, bright pixels: Y = 16 + 0.86 * grey stays inside 93..162, 16..85 and 170..236): a partial or a LUT taken from the neighbour's
    index cannot pass.  Every frame, the seam frames and the last among them, is compared exactly."""
    w, h, n = 16, 2, CHUNK + 1
    images = rand_images4(w, h, n, 135)
    rng = np.random.default_rng(136)
    for idx, (lo, hi) in ((CHUNK - 2, (90, 170)), (CHUNK - 1, (0, 80)), (CHUNK, (180, 256))):
        images[idx][:, :, :3] = rng.integers(lo, hi, (h, w, 3), dtype=np.uint8)
    lumas = [convert(first3(images[i]))[0] for i in (CHUNK - 1, CHUNK - 2, CHUNK)]
    assert lumas[0].max() < lumas[1].min() and lumas[1].max() < lumas[2].min()
    perm = [(37 * i + 5) % n for i in range(n)]                  # list entry i lives in allocation perm[i]
    assert sorted(perm) == list(range(n)) and perm != list(range(n))
    alloc_images = [None] * n
    for i, a in enumerate(perm):
        alloc_images[a] = images[i]
    src, dst = pools(alloc_images, w, h)
    ins, outs = [src.ptrs[a] for a in perm], [dst.ptrs[a] for a in perm]
    for op, order, fmt in ((EQ, ORDER_RGB, FMT_UYVY), (("clahe", (2.0, 2, 1)), ORDER_BGR, FMT_YUY2)):
        dst.clear()
        before = counters(c)
        run(c, op, ins, outs, w, h, order, fmt, UV_COPY, src.pitch, dst.pitch)
        torch.cuda.synchronize()
        ok, nbad, where = dst.same([expected(img, op, order, fmt, UV_COPY) for img in alloc_images])
        assert ok, (op, nbad, sorted({perm.index(a) for a, _ in where}))
        assert tuple(a - b for a, b in zip(counters(c), before)) == (0, 0, n, 0)
    assert src.same(alloc_images)[0]


# ---- 5. loops past their first step ------------------------------------------------------------------------------------------------
LOOPS = [
    # id, W, H, in_pitch, out_pitch, in offsets of the two frames, out offsets, frames on the vector walk, the bound on B
    ("8192x2", 8192, 2, None, None, (0,), (0,), 2, 2),
    ("4112x4", 4112, 4, None, None, (0,), (0,), 2, 3),
    ("66x35-odd", 66, 35, 265, 136, (1, 5), (4, 12), 0, 1),
    ("4112x4-one-skewed", 4112, 4, None, None, (0, 8), (0,), 1, 3),  # a byte-walk frame stepping with the vector grid's stride
]


@pytest.mark.parametrize("name,w,h,ip,op_,io,oo,n_vec,bmax", LOOPS, ids=[s[0] for s in LOOPS])
def test_loops_past_their_first_step(c, name, w, h, ip, op_, io, oo, n_vec, bmax):
    """Stage 1 where a lane owns more than one group / macropixel: with the histogram (equalizeHist, U and V computed) and without it
    (CLAHE 2 x 2, chroma filled)."""
    images = rand_images4(w, h, 2, 137)
    src, dst = pools(images, w, h, ip, op_, io, oo)
    shape_vec = w % 16 == 0 and src.pitch % 16 == 0 and dst.pitch % 16 == 0
    bound = min(max(1, w * h * 3 // 16384), h)
    assert bound == bmax
    assert (w * h // 16 if shape_vec else w * h // 2) > 256 * bound, "the shape would not loop"
    if shape_vec and n_vec < 2:
        assert w * h // 2 > 256 * bound, "the byte-walk frame would not loop"
    for order, fmt in ((ORDER_BGR, FMT_YUY2), (ORDER_RGB, FMT_UYVY)):
        check(c, images, EQ, order, fmt, UV_COPY, src, dst, w, h, n_vec=n_vec)
        check(c, images, ("clahe", (2.0, 2, 2)), order, fmt, UV_FILL128, src, dst, w, h, n_vec=n_vec)


# ---- 6. one image, several output frames -------------------------------------------------------------------------------------------
def test_same_image_in_several_entries(c):
    w, h = 48, 5
    images = rand_images4(w, h, 2, 138)
    src = Pool(2, h, 4 * w, 208).upload(images)
    dst3 = Pool(3, h, 2 * w, 112)
    for op in (EQ, ("clahe", (2.0, 3, 2))):
        dst3.clear()
        before = counters(c)
        run(c, op, [src.ptrs[0], src.ptrs[1], src.ptrs[0]], dst3.ptrs, w, h, ORDER_BGR, FMT_YUY2, UV_COPY, src.pitch, dst3.pitch)
        torch.cuda.synchronize()
        want = [expected(images[k], op, ORDER_BGR, FMT_YUY2, UV_COPY) for k in (0, 1, 0)]
        assert dst3.same(want)[0], op
        assert src.same(images)[0], "an input allocation was written"
        assert tuple(a - b for a, b in zip(counters(c), before)) == (0, 0, 3, 0)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    w, h, n = 32, 6, 3
    images = rand_images4(w, h, n, 139)
    src, dst = pools(images, w, h, 144, 80)
    Entry = mi_lumaeq.BgrPacked422FrameDev
    good = [(src.ptrs[k], dst.ptrs[k]) for k in range(n)]
    base = dict(n=n, w=w, h=h, ip=src.pitch, op=dst.pitch, order=ORDER_BGR, fmt=FMT_YUY2, uvm=UV_COPY)
    with mi_lumaeq.Context(0) as c:
        L, hd = c._L, c._h
        c.set_profiling(1)
        c.profile_read(reset=True)
        before, sib = counters(c), siblings(c)

        def table(entries):
            arr = (Entry * max(1, len(entries)))()
            for k, (i, o) in enumerate(entries):
                arr[k] = Entry(i, o)
            return arr

        def args(entries=good, null_list=False, **kw):
            a = dict(base)
            a.update(kw)
            return (hd, None if null_list else table(entries), a["n"], a["w"], a["h"], a["ip"], a["op"], a["order"], a["fmt"], a["uvm"])

        def both(tx=2, ty=2, **kw):
            return (L.mi_equalize_hist_bgra_to_packed422_frames_dev(*args(**kw), stream()),
                    L.mi_clahe_bgra_to_packed422_frames_dev(*args(**kw), 2.0, tx, ty, stream()))

        def last(i=None, o=None):
            return good[:-1] + [(good[-1][0] if i is None else i, good[-1][1] if o is None else o)]

        inside = good[-1][0] + 8                                  # a multiple of 4 inside the last image's rows
        assert inside % 4 == 0
        bad = [dict(null_list=True),                                                                  # a null list with n > 0
               dict(entries=good[:-1] + [(None, good[-1][1])]), dict(entries=good[:-1] + [(good[-1][0], None)]),   # null in / out, last entry
               dict(entries=last(o=good[-1][1] + 2)),                                                 # out at +2, last entry
               dict(op=dst.pitch + 2),                                                                # out_pitch 2 mod 4
               dict(w=w - 1), dict(w=w - 1, h=0), dict(w=w - 1, n=0),                                 # an odd width, also next to a zero size
               dict(ip=4 * w - 1), dict(ip=3 * w), dict(op=2 * w - 4),                                # a pitch below its row
               dict(entries=last(o=inside)),                                                          # an image whose rows meet its own frame
               dict(entries=last(o=good[-1][0])),                                                     # ... starting at the same byte
               dict(entries=last(o=good[-1][0] + 3 * w + 4)),                                         # ... in the fourth quarter of its 4W-byte row
               dict(entries=last(i=good[-1][1] + dst.pitch * (h - 1) + 2 * w - 1)),                   # ... meeting its last byte
               dict(order=2), dict(order=-1), dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),
               dict(w=-2), dict(h=-1), dict(n=-1)]                                                    # negative sizes
        for kw in bad:
            assert both(**kw) == (BAD_ARG, BAD_ARG), kw
        for tx, ty in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert L.mi_clahe_bgra_to_packed422_frames_dev(*args(), 2.0, tx, ty, stream()) == BAD_ARG, (tx, ty)
        # a size and a tile grid the three-channel list form refuses: its status
        big = dict(w=(1 << 24) + 2, h=2, ip=1 << 27, op=1 << 26)
        sib_big = L.mi_clahe_bgr_to_packed422_frames_dev(*args(**big), 2.0, 2, 2, stream())
        assert sib_big == UNSUPPORTED and both(**big) == (sib_big, sib_big)
        sib_tiles = L.mi_clahe_bgr_to_packed422_frames_dev(*args(), 2.0, 2048, 1024, stream())
        assert sib_tiles == UNSUPPORTED and L.mi_clahe_bgra_to_packed422_frames_dev(*args(), 2.0, 2048, 1024, stream()) == sib_tiles
        # nothing to do: MI_OK, nothing written -- also with a null list when there are no frames
        for kw in (dict(n=0, null_list=True), dict(n=0), dict(w=0), dict(h=0)):
            assert both(**kw) == (0, 0), kw
        torch.cuda.synchronize()
        assert dst.same()[0], "a refused or empty call wrote: a bad last entry must leave every output allocation untouched"
        assert src.same(images)[0], "a refused or empty call wrote an input"
        assert all(v["launches"] == 0 for v in c.profile_read(reset=False).values())
        assert counters(c) == before, "a refused or empty call was counted"
        assert siblings(c) == sib
        c.set_profiling(0)
        # an image next to its frame is legal, and the context still works
        check(c, images, EQ, ORDER_RGB, FMT_UYVY, UV_FILL128, src, dst, w, h, n_vec=n)


# ---- 8. streams, options, hipGraph -------------------------------------------------------------------------------------------------
def test_streams(c):
    w, h = 64, 9
    images = rand_images4(w, h, 3, 140)
    src, dst = pools(images, w, h, 272, 144, (0, 16, 4), (0,))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    check(c, images, EQ, ORDER_RGB, FMT_UYVY, UV_COPY, src, dst, w, h, n_vec=2, st=side.cuda_stream, sync=side.synchronize)
    check(c, images, ("clahe", (2.0, 4, 3)), ORDER_BGR, FMT_YUY2, UV_FILL128, src, dst, w, h, n_vec=2, st=mi_lumaeq.STREAM_CTX,
          sync=lambda: c.synchronize(mi_lumaeq.STREAM_CTX))


def test_clahe_fp_contract():
    """The option reaches stage 2 of a list call: the bytes are the reference's in that arithmetic mode (the option is restored)."""
    w, h = 66, 35
    images = rand_images4(w, h, 2, 141)
    src, dst = pools(images, w, h, 265, 136, (1, 5), (4, 12))
    with mi_lumaeq.Context(0) as c:
        c.set_option("clahe_fp_contract", 1)
        try:
            check(c, images, ("clahe", (2.0, 3, 2)), ORDER_RGB, FMT_UYVY, UV_COPY, src, dst, w, h, contract=True, n_vec=0)
        finally:
            c.set_option("clahe_fp_contract", 0)
        check(c, images, ("clahe", (2.0, 3, 2)), ORDER_RGB, FMT_UYVY, UV_COPY, src, dst, w, h, n_vec=0)


def test_graph_capture_and_replay():
    """One eager call of each shape, then one equalizeHist and one CLAHE list call captured on a single stream (one linear chain, no
    parallel branches) and one replay onto fresh inputs at the captured addresses: the bytes of an eager call."""
    w, h, n = 64, 32, 2
    cl = ("clahe", (2.0, 4, 2))
    images = rand_images4(w, h, n, 142)
    src, dst_eq = pools(images, w, h, 272, 144, (0, 8), (0,))
    dst_cl = Pool(n, h, 2 * w, 144)
    calls = ((EQ, dst_eq, FMT_YUY2, UV_COPY), (cl, dst_cl, FMT_UYVY, UV_FILL128))
    with mi_lumaeq.Context(0) as c:
        for op, dst, fmt, uv_mode in calls:                                              # the eager calls size the scratch
            check(c, images, op, ORDER_BGR, fmt, uv_mode, src, dst, w, h, n_vec=1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            for op, dst, fmt, uv_mode in calls:
                run(c, op, src.ptrs, dst.ptrs, w, h, ORDER_BGR, fmt, uv_mode, src.pitch, dst.pitch, st=st)
        fresh = rand_images4(w, h, n, 143)
        src.upload(fresh)
        dst_eq.clear()
        dst_cl.clear()
        g.replay()
        torch.cuda.synchronize()
        for op, dst, fmt, uv_mode in calls:
            assert dst.same([expected(img, op, ORDER_BGR, fmt, uv_mode) for img in fresh])[0], ("graph replay", op)
        assert src.same(fresh)[0]


def test_binding_derives_the_pitches_from_tensors(c):
    """H x W x 4 image tensors that are views of padded rows and H x pitch frame tensors: the pitches are the tensors' row strides."""
    w, h, n = 32, 4, 2
    images = rand_images4(w, h, n, 144)
    ins, outs, bufs = [], [], []
    for img in images:
        b = torch.full((h, 144), SENT, dtype=torch.uint8, device="cuda:0")
        v = b.as_strided((h, w, 4), (144, 4, 1))                 # an H x W x 4 view of the padded rows
        v.copy_(torch.from_numpy(img))
        o = torch.full((h, 80), SENT, dtype=torch.uint8, device="cuda:0")
        ins.append(v)
        outs.append(o[:, : 2 * w])
        bufs.append((b, o))
    before = counters(c)
    c.equalize_hist_bgra_to_packed422_frames(ins, outs, w, h, stream=stream())
    torch.cuda.synchronize()
    for img, (b, o) in zip(images, bufs):
        want = np.full((h, 80), SENT, np.uint8)
        want[:, : 2 * w] = expected(img, EQ, ORDER_BGR, FMT_YUY2, UV_COPY)
        assert np.array_equal(o.cpu().numpy(), want)
        keep = np.full((h, 144), SENT, np.uint8)
        keep[:, : 4 * w] = img.reshape(h, 4 * w)
        assert np.array_equal(b.cpu().numpy(), keep)
    assert tuple(a - b for a, b in zip(counters(c), before)) == (0, 0, n, 0)
