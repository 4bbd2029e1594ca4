"""Packed 4:2:2 frames in (YUY2 / UYVY), NV12 frames out on LISTS of device frames: mi_equalize_hist_packed422_to_nv12_frames_dev and
mi_clahe_packed422_to_nv12_frames_dev.  The expected Y plane is oracle.equalize_hist / oracle.clahe on the gathered luma; the expected
UV plane is 128 (MI_UV_FILL128) or the rounding mean (a + b + 1) >> 1 of input chroma rows 2r and 2r+1 (MI_UV_COPY).  Every frame
lives in three torch allocations of its own (input, Y, UV), sentinel-filled, with padded pitches and bases 4 / 8 / 12 bytes past a
16-byte boundary that vary per frame within one list; the WHOLE allocations are compared and the inputs must be unchanged: every
comparison in this file is exact bytes."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
from mi_lumaeq import synth, UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 2
SENT = 0x5A
DISTS = ["D1", "D2", "D3", "D4", "D5"]
CLAHE_CONFIGS = [(2.0, 8, 8), (3.0, 4, 4), (0.0, 3, 5), (2.0, 16, 16), (2.0, 64, 2)]      # the last takes the wide-grid fallback
OPS = [("eq", None)] + [("clahe", cfg) for cfg in CLAHE_CONFIGS]
FMTS = [FMT_YUY2, FMT_UYVY]
UVS = [UV_COPY, UV_FILL128]
OFFS = (4, 8, 12)                                                                        # bytes past a 16-byte boundary


def stream():
    return torch.cuda.current_stream().cuda_stream


def align4(x):
    return (x + 3) & ~3


def luma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, fmt - 2:2 * w:2])


def chroma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, 3 - fmt:2 * w:2])


def uv_mean(c):
    """The header's chroma rule: UV row r is the per-byte rounding mean of chroma rows 2r and 2r+1."""
    a, b = c[0::2], c[1::2]
    return ((a.astype(np.uint16) + b + 1) >> 1).astype(np.uint8)


_ref_cache = {}


def y_ref(y, op, cfg, key=None):
    """The oracle's plane; `key` names the content so that one plane is computed once per op (default arithmetic mode only)."""
    k = None if key is None else (key, op, cfg)
    if k in _ref_cache:
        return _ref_cache[k]
    r = oracle.equalize_hist(y) if op == "eq" else oracle.clahe(y, *cfg)
    if k is not None:
        _ref_cache[k] = r
    return r


def expected_planes(frame, w, fmt, op, cfg, uv_mode, key=None):
    h = frame.shape[0]
    uv = uv_mean(chroma(frame, w, fmt)) if uv_mode == UV_COPY else np.full((h // 2, w), 128, np.uint8)
    return y_ref(luma(frame, w, fmt), op, cfg, key), uv


def dev_buf(size):
    b = torch.full((size,), SENT, dtype=torch.uint8, device="cuda:0")
    assert b.data_ptr() % 16 == 0
    return b


class Pool:
    """n frames of a list.  Every plane is placed as (buffer, byte offset); the default gives every frame three sentinel-filled
    allocations of its own -- the input (H rows of 2W bytes at in_pitch), the Y plane (H rows of W bytes at y_pitch) and the UV plane
    (H/2 rows at uv_pitch) -- whose bases lie 4 / 8 / 12 bytes past a 16-byte boundary, a different triple for every frame."""

    def __init__(self, w, h, n, extra=(12, 4, 20), tight=False):
        self.w, self.h, self.n = w, h, n
        if tight:
            self.in_pitch, self.y_pitch, self.uv_pitch = 2 * w, w, w
        else:
            self.in_pitch, self.y_pitch, self.uv_pitch = 2 * w + extra[0], align4(w) + extra[1], align4(w) + extra[2]
        self.bufs, self.in_at, self.y_at, self.uv_at = [], [], [], []
        for k in range(n):
            for at, size, off in ((self.in_at, self.in_pitch * h, OFFS[k % 3]), (self.y_at, self.y_pitch * h, OFFS[(k + 1) % 3]),
                                  (self.uv_at, self.uv_pitch * (h // 2), OFFS[(k + 2 + k // 3) % 3])):
                at.append((len(self.bufs), off))
                self.bufs.append(dev_buf(16 + size + 64))

    def ptr(self, at):
        return self.bufs[at[0]].data_ptr() + at[1]

    def ptrs(self):
        return ([self.ptr(a) for a in self.in_at], [self.ptr(a) for a in self.y_at], [self.ptr(a) for a in self.uv_at])

    def image(self, frames=None, planes=None):
        """All allocations, concatenated, as they must read with `frames` in the inputs and `planes` = [(Y, UV), ...] in the outputs
        (None: the sentinel)."""
        imgs = [np.full(b.numel(), SENT, np.uint8) for b in self.bufs]

        def paint(at, pitch, rows, width, px):
            bi, o = at
            imgs[bi][o: o + pitch * rows].reshape(rows, pitch)[:, :width] = px[:, :width]
        if frames is not None:
            for k in range(len(self.in_at)):
                paint(self.in_at[k], self.in_pitch, self.h, frames[k].shape[1], frames[k])
        if planes is not None:
            for k, (y, uv) in enumerate(planes):
                paint(self.y_at[k], self.y_pitch, self.h, self.w, y)
                paint(self.uv_at[k], self.uv_pitch, self.h // 2, self.w, uv)
        return np.concatenate(imgs)

    def upload(self, frames):
        self.frames = frames
        img = torch.from_numpy(self.image(frames)).to("cuda:0")
        o = 0
        for b in self.bufs:
            b.copy_(img[o: o + b.numel()])
            o += b.numel()
        return self

    def clear_outputs(self):
        for at in (self.y_at, self.uv_at):
            for bi, _ in at:
                self.bufs[bi].fill_(SENT)

    def host(self):
        return torch.cat(self.bufs).cpu().numpy()

    def same(self, planes=None):
        """The whole of every allocation: the inputs as uploaded, the outputs `planes` (None: untouched), the sentinel elsewhere."""
        return np.array_equal(self.host(), self.image(self.frames, planes))

    def diff(self, planes=None):
        got, want = self.host(), self.image(self.frames, planes)
        bad = np.flatnonzero(got != want)
        return int(bad.size), bad[:8]

    def kw(self):
        return {"in_pitch": self.in_pitch, "y_pitch": self.y_pitch, "uv_pitch": self.uv_pitch}


def run(c, op, cfg, pool, fmt, uv_mode, st=None):
    i, y, uv = pool.ptrs()
    kw = dict(pool.kw(), stream=stream() if st is None else st)
    if op == "eq":
        c.equalize_hist_packed422_to_nv12_frames(i, y, uv, pool.w, pool.h, fmt, uv_mode, **kw)
    else:
        c.clahe_packed422_to_nv12_frames(i, y, uv, pool.w, pool.h, fmt, uv_mode, *cfg, **kw)


_planar_cache = {}


def planar_status(c, w, h, n, op, cfg):
    """What the planar form answers for this size / grid pair (0 = accepted)."""
    k = (w, h, n, op, cfg)
    if k not in _planar_cache:
        a = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        status = 0
        try:
            if op == "eq":
                c.equalize_hist_batch_dev(a, b, w, h, n, stream=stream())
            else:
                c.clahe_batch_dev(a, b, w, h, n, *cfg, stream=stream())
        except mi_lumaeq.MiError as e:
            status = e.status
        finally:
            torch.cuda.synchronize()
        _planar_cache[k] = status
    return _planar_cache[k]


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


def make_frames(w, h, fmt, dists, first):
    return [synth.packed422_frame(w, h, fmt, d, first + k) for k, d in enumerate(dists)]


# ---- 1. small sizes, full matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 48), (62, 46), (2, 2), (4098, 4)])
def test_small_sizes_full_matrix(c, w, h):
    """Every format x uv_mode x op on D1-D5, five frames at five alignment triples in one list.  62 x 46: W % 4 == 2 (a 2-byte row
    tail) and no tile grid divides it; 2 x 2: one macropixel, one row pair; 4098 x 4: rows of many groups plus a ragged one;
    (2.0, 64, 2) takes the wide-grid kernel.  A size / grid pair the planar form refuses: the same status, nothing written."""
    pool = Pool(w, h, len(DISTS))
    for fmt in FMTS:
        frames = make_frames(w, h, fmt, DISTS, 100)
        pool.upload(frames)
        for uv_mode in UVS:
            for op, cfg in OPS:
                pool.clear_outputs()
                status = planar_status(c, w, h, len(frames), op, cfg)
                if status != 0:
                    with pytest.raises(mi_lumaeq.MiError) as e:
                        run(c, op, cfg, pool, fmt, uv_mode)
                    torch.cuda.synchronize()
                    assert e.value.status == status, (w, h, op, cfg, e.value.status, status)
                    assert pool.same(), "a refused call wrote"
                    continue
                run(c, op, cfg, pool, fmt, uv_mode)
                torch.cuda.synchronize()
                want = [expected_planes(f, w, fmt, op, cfg, uv_mode, ("small", w, h, k, fmt)) for k, f in enumerate(frames)]
                assert pool.same(want), (w, h, fmt, uv_mode, op, cfg, pool.diff(want))


# ---- 2. identity with the batch form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 129, 258])
def test_identity_with_the_batch_form(c, n):
    """The same pixels through mi_*_packed422_to_nv12_batch_dev (one tight allocation) and through the list: the same bytes, across
    a chunk boundary of a 64-entry and of a 128-entry table (twice at n = 258), under both CLAHE arithmetic modes."""
    w, h = 320, 90
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1412 + n)
    x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
    x[: n // 2 + 1, :, :] = (x[: n // 2 + 1, :, :] // 3) + 40                      # half of the frames low-contrast
    nv12 = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")   # tight: UV directly behind Y, all defaults
    pool = Pool(w, h, n).upload(list(x.cpu().numpy()))
    try:
        for fmt in FMTS:
            for op, cfg, contracts in (("eq", None, (0,)), ("clahe", (2.0, 8, 8), (0, 1)), ("clahe", (3.0, 5, 3), (0, 1))):
                for contract in contracts:
                    c.set_option("clahe_fp_contract", contract)
                    nv12.fill_(SENT)
                    pool.clear_outputs()
                    if op == "eq":
                        c.equalize_hist_packed422_to_nv12_batch_dev(x, nv12, None, w, h, n, fmt, UV_COPY, stream=stream())
                    else:
                        c.clahe_packed422_to_nv12_batch_dev(x, nv12, None, w, h, n, fmt, UV_COPY, *cfg, stream=stream())
                    run(c, op, cfg, pool, fmt, UV_COPY)
                    torch.cuda.synchronize()
                    ref = nv12.cpu().numpy()
                    want = [(ref[k, :h], ref[k, h:]) for k in range(n)]
                    assert pool.same(want), (n, fmt, contract, op, cfg, pool.diff(want))
    finally:
        c.set_option("clahe_fp_contract", 0)


# ---- 3. list semantics -----------------------------------------------------------------------------------------------------------
def test_list_semantics(c):
    """The same input in several entries going to distinct outputs; the Y planes of all frames in ONE pool allocation and the UV
    planes in another; the frames of the list at different alignments modulo 16."""
    w, h, n = 64, 48, 5
    src = make_frames(w, h, FMT_YUY2, DISTS[:2], 300)
    pool = Pool(w, h, 2)                                  # two inputs (their own Y / UV allocations stay unused)
    ysz, usz = pool.y_pitch * h + 4, pool.uv_pitch * (h // 2) + 12          # strides of the plane pools: 4 and 12 mod 16 apart
    ybuf, ubuf = len(pool.bufs), len(pool.bufs) + 1
    pool.bufs += [dev_buf(16 + ysz * n + 64), dev_buf(16 + usz * n + 64)]
    which = [0, 1, 0, 0, 1]
    pool.in_at = [pool.in_at[i] for i in which]
    pool.y_at = [(ybuf, 8 + k * ysz) for k in range(n)]
    pool.uv_at = [(ubuf, 4 + k * usz) for k in range(n)]
    assert len({pool.ptr(a) % 16 for a in pool.y_at}) > 1 and len({pool.ptr(a) % 16 for a in pool.uv_at}) > 1
    assert len({pool.ptr(a) % 16 for a in pool.in_at}) > 1
    frames = [src[i] for i in which]
    pool.upload(frames)
    for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8)), ("clahe", (2.0, 64, 2))):
        for uv_mode in UVS:
            pool.clear_outputs()
            run(c, op, cfg, pool, FMT_YUY2, uv_mode)
            torch.cuda.synchronize()
            want = [expected_planes(f, w, FMT_YUY2, op, cfg, uv_mode, ("sem", which[k])) for k, f in enumerate(frames)]
            assert pool.same(want), (op, cfg, uv_mode, pool.diff(want))


# ---- 4. chroma rounding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_chroma_rounding(c, fmt):
    """Row pairs (0, 1), (254, 255), (255, 255), (0, 255), (7, 8), (128, 128) in NEIGHBOURING chroma bytes (a carry or borrow between the
    bytes of a 4-byte-at-once mean would show), in both row orders, through full 16-column groups and a ragged one (W = 38), through
    the LDS-table and the wide-grid kernel."""
    w, h = 38, 4
    pairs = [(0, 1), (254, 255), (255, 255), (0, 255), (7, 8), (128, 128)]
    mean = [1, 255, 255, 128, 8, 128]
    a = np.array([p[0] for p in pairs], np.uint8)[np.arange(w) % 6]
    b = np.array([p[1] for p in pairs], np.uint8)[np.arange(w) % 6]
    frame = synth.packed422_frame(w, h, fmt, "D2", 900)
    frame[:, 3 - fmt::2] = np.stack([a, b, b, a])
    want_uv = np.tile(np.array(mean, np.uint8)[np.arange(w) % 6], (h // 2, 1))
    assert np.array_equal(uv_mean(chroma(frame, w, fmt)), want_uv)
    pool = Pool(w, h, 2).upload([frame, frame])
    for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 64, 2))):
        assert planar_status(c, w, h, 1, op, cfg) == 0, (op, cfg)       # LDS-table kernel (full and ragged groups), wide-grid kernel
        pool.clear_outputs()
        run(c, op, cfg, pool, fmt, UV_COPY)
        torch.cuda.synchronize()
        want = [(y_ref(luma(frame, w, fmt), op, cfg), want_uv)] * 2
        assert pool.same(want), (fmt, op, cfg, pool.diff(want))


# ---- 5. launch accounting --------------------------------------------------------------------------------------------------------
def test_launch_accounting():
    w, h, n = 64, 48, 3
    frames = make_frames(w, h, FMT_YUY2, DISTS[:n], 1000)
    pool = Pool(w, h, n).upload(frames)
    big = Pool(w, h, 130).upload([frames[k % n] for k in range(130)])
    with mi_lumaeq.Context(0) as c:
        c.set_profiling(1)
        for uv_mode in UVS:
            c.profile_read(reset=True)
            run(c, "eq", None, pool, FMT_YUY2, uv_mode)
            torch.cuda.synchronize()
            prof = c.profile_read(reset=True)
            assert len(prof) == 10
            for k in mi_lumaeq.KERNEL_NAMES:
                want = 1 if k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel") else 0
                assert prof[k]["launches"] == want, (uv_mode, k, prof[k])
            assert pool.same([expected_planes(f, w, FMT_YUY2, "eq", None, uv_mode) for f in frames])
        for cfg in ((2.0, 8, 8), (2.0, 64, 2)):
            assert planar_status(c, w, h, n, "clahe", cfg) == 0
            for uv_mode in UVS:
                c.profile_read(reset=True)
                run(c, "clahe", cfg, pool, FMT_YUY2, uv_mode)
                torch.cuda.synchronize()
                prof = c.profile_read(reset=True)
                for k in mi_lumaeq.KERNEL_NAMES:
                    want = 1 if k in ("tile_hist_kernel", "clahe_interp_kernel") else 0
                    assert prof[k]["launches"] == want, (cfg, uv_mode, k, prof[k])
        # 130 frames: two chunks of a 128-entry table, three of a 64-entry one -- every stage of a chunk with the same chunk
        c.profile_read(reset=True)
        run(c, "eq", None, big, FMT_YUY2, UV_COPY)
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
        counts = [prof[k]["launches"] for k in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel")]
        assert counts[0] == counts[1] == counts[2] and counts[0] in (2, 3), counts
        for k in mi_lumaeq.KERNEL_NAMES:
            if k not in ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel"):
                assert prof[k]["launches"] == 0, (k, prof[k])
        assert big.same([expected_planes(frames[k % n], w, FMT_YUY2, "eq", None, UV_COPY, ("acct", k % n)) for k in range(130)])
        c.set_profiling(0)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(c):
    w, h, n = 64, 48, 3
    frames = make_frames(w, h, FMT_YUY2, DISTS[:n], 700)
    pool = Pool(w, h, n).upload(frames)
    L, hd = c._L, c._h
    Entry = mi_lumaeq.Packed422Nv12FrameDev
    ins, ys, uvs = pool.ptrs()
    base = dict(n=n, w=w, h=h, ipitch=pool.in_pitch, ypitch=pool.y_pitch, uvpitch=pool.uv_pitch, fmt=FMT_YUY2, uvm=UV_COPY,
                null_list=False, entry=None)

    def args(kw):
        a = dict(base)
        a.update(kw)
        arr = (Entry * n)(*[Entry(ins[k], ys[k], uvs[k]) for k in range(n)])
        if a["entry"] is not None:                        # replace the LAST entry: every earlier frame is fine
            e = dict(i=ins[n - 1], y=ys[n - 1], uv=uvs[n - 1])
            e.update(a["entry"])
            arr[n - 1] = Entry(e["i"], e["y"], e["uv"])
        lst = None if a["null_list"] else arr
        return (hd, lst, a["n"], a["w"], a["h"], a["ipitch"], a["ypitch"], a["uvpitch"], a["fmt"], a["uvm"])

    def eq(**kw):
        return L.mi_equalize_hist_packed422_to_nv12_frames_dev(*args(kw), stream())

    def cl(tx=8, ty=8, **kw):
        return L.mi_clahe_packed422_to_nv12_frames_dev(*args(kw), 2.0, tx, ty, stream())
    i2, y2, uv2 = ins[n - 1], ys[n - 1], uvs[n - 1]
    bad = [dict(null_list=True),                                                                  # a null list with n_frames > 0
           dict(entry=dict(i=None)), dict(entry=dict(y=None)), dict(entry=dict(uv=None)),         # a null address
           dict(w=63), dict(h=47), dict(w=63, h=47), dict(w=0, h=47), dict(n=0, h=47), dict(w=63, h=0), dict(w=63, n=0),   # odd sizes
           dict(w=-2), dict(h=-2), dict(h=-1), dict(n=-1),                                        # negative sizes
           dict(fmt=0), dict(fmt=1), dict(fmt=4), dict(fmt=-1), dict(uvm=2), dict(uvm=-1),         # format, uv_mode
           dict(ipitch=2 * w - 4), dict(ypitch=w - 4), dict(uvpitch=w - 4),                       # pitches too small
           dict(ipitch=2 * w + 2), dict(ypitch=w + 2), dict(uvpitch=w + 6),                       # pitches, not multiples of 4
           dict(entry=dict(i=i2 + 2)), dict(entry=dict(y=y2 + 2)), dict(entry=dict(uv=uv2 + 1)),  # addresses, not multiples of 4
           dict(entry=dict(y=i2)), dict(entry=dict(uv=i2)),                                       # no in-place form
           dict(entry=dict(y=i2 + 2 * pool.in_pitch)), dict(entry=dict(uv=i2 + 4 * pool.in_pitch + 8)),     # output rows meet input rows
           dict(entry=dict(uv=y2)), dict(entry=dict(uv=y2 + 8 * pool.y_pitch)), dict(entry=dict(uv=y2 + 4))]    # Y rows meet UV rows
    # (every overlapping plane above lies inside the larger allocation it is pointed into)
    for kw in bad:
        assert eq(**kw) == BAD_ARG, kw
        assert cl(**kw) == BAD_ARG, kw
    for tx, ty in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert cl(tx, ty) == BAD_ARG
    # sizes the planar forms refuse: their status (width * height = 2^31; nothing is dereferenced, the shape is refused first)
    big = dict(w=65536, h=32768, ipitch=2 * 65536, ypitch=65536, uvpitch=65536)
    assert eq(**big) == UNSUPPORTED and cl(**big) == UNSUPPORTED
    # the documented consequence: a tight NV12 pitch with W % 4 == 2 is not a multiple of 4
    assert eq(w=62, ypitch=62, uvpitch=62) == BAD_ARG
    assert cl(w=62, ypitch=62, uvpitch=62) == BAD_ARG
    # zero sizes: MI_OK, nothing written (a null list with no frames included)
    for kw in (dict(w=0), dict(h=0), dict(n=0), dict(n=0, null_list=True)):
        assert eq(**kw) == 0 and cl(**kw) == 0, kw
    torch.cuda.synchronize()
    assert pool.same(), "a refused or empty call wrote"
    # the same W % 4 == 2 frames with padded pitches are accepted (the same buffers: the pitches are wide enough for 64 columns)
    assert eq(w=62) == 0
    torch.cuda.synchronize()
    cut = [np.ascontiguousarray(f[:, :124]) for f in frames]
    want = [expected_planes(f, 62, FMT_YUY2, "eq", None, UV_COPY) for f in cut]
    pool.w = 62
    assert pool.same(want), pool.diff(want)
    pool.w = w
    # and the context still works
    pool.clear_outputs()
    run(c, "clahe", (2.0, 8, 8), pool, FMT_YUY2, UV_COPY)
    torch.cuda.synchronize()
    assert pool.same([expected_planes(f, w, FMT_YUY2, "clahe", (2.0, 8, 8), UV_COPY) for f in frames])


# ---- 7. busy ---------------------------------------------------------------------------------------------------------------------
def test_busy_while_a_pipe_has_frames_pending():
    w, h = 64, 48
    frame = synth.nv12_frame(w, h, "D1", 1)
    out = np.zeros_like(frame)
    pool = Pool(w, h, 2).upload(make_frames(w, h, FMT_YUY2, ["D1", "D2"], 1100))
    with mi_lumaeq.Context(0) as c:
        with mi_lumaeq.Pipe(c, w, h, depth=2) as pipe:
            assert pipe.submit(frame, out, 1)
            for op, cfg in (("eq", None), ("clahe", (2.0, 8, 8))):
                with pytest.raises(mi_lumaeq.MiError) as e:
                    run(c, op, cfg, pool, FMT_YUY2, UV_COPY)
                assert e.value.status == mi_lumaeq.ERR_BUSY
            assert pipe.wait()[0] == 1
        torch.cuda.synchronize()
        assert pool.same(), "a refused call wrote"


# ---- 8. hipGraph -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    """One eager call of the shape, then capture and two replays on fresh inputs (the frame table is part of the captured launches:
    the same buffers, new contents)."""
    w, h, n = 640, 360, 3
    fmt = FMT_UYVY
    frames = make_frames(w, h, fmt, DISTS[:n], 800)
    pool = Pool(w, h, n, extra=(36, 8, 24)).upload(frames)
    with mi_lumaeq.Context(0) as c:
        for op, cfg, uv_mode in (("eq", None, UV_COPY), ("clahe", (3.0, 4, 4), UV_COPY), ("clahe", (2.0, 8, 8), UV_FILL128)):
            pool.clear_outputs()
            run(c, op, cfg, pool, fmt, uv_mode)                        # the eager call of the captured shape sizes the scratch
            torch.cuda.synchronize()
            assert pool.same([expected_planes(f, w, fmt, op, cfg, uv_mode) for f in frames]), ("eager", op)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(c, op, cfg, pool, fmt, uv_mode, st=torch.cuda.current_stream().cuda_stream)
            for rep in range(2):
                fresh = make_frames(w, h, fmt, [DISTS[(k + 2 + rep) % 5] for k in range(n)], 850 + 10 * rep)
                pool.upload(fresh)                                     # also resets the outputs to the sentinel
                g.replay()
                torch.cuda.synchronize()
                assert pool.same([expected_planes(f, w, fmt, op, cfg, uv_mode) for f in fresh]), ("graph replay", op, rep)
            pool.upload(frames)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
