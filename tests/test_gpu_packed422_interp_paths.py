"""Every rung of the CLAHE interpolation ladder on packed 4:2:2 input (YUY2 / UYVY), through every device form: packed out, NV12 out
and planar 4:2:0 out (I420 / YV12), each as a strided batch and as a list of frames.  The host picks the interpolation kernel from
(writer, list or batch, float or quad tables, clahe_fp_contract, format, LDS or global tables); the sizes below are the smallest that
reach each branch of that choice, and the options clahe_float_tables and clahe_fp_contract are set both ways, so that every instantiation runs.  64 x 8 and
128 x 8 have tiles of 4 x 4 and 2 x 4 pixels: 1 / tile is exact there, FMA and mul + add round alike and both arithmetic modes give the
same bytes, so those two rungs cannot tell an FMA body from a plain one.  96 x 10 and 192 x 10 (tiles 6 x 5 and 3 x 5) reach the same
two kernels on shapes where the modes differ; their luma is tests/clahe_u8_rungs.py content, on which the test first shows that they do.

    kMaxPairsLdsF32 = 15, kMaxPairsLds = 63, kInterpPx = 16, clahe_seg_pairs = 9 (default); pairs = tiles_x + 1
    64 x 48,   8 x 8:   9 pairs <= 15: one float table; uchar quads when clahe_float_tables = 0
    1792 x 8,  16 x 2:  17 pairs > 15, tile_w = 112: (9 - 3) * 112 / 16 = 42 >= 40 column groups per segment, so float tables on
                        column segments (112 groups in ceil(112 / 42) = 3 segments); quads in one segment when clahe_float_tables = 0
    1790 x 8,  16 x 2:  17 pairs > 15, the width pads to 1792: tile_w = 112 and 42 groups a segment again, so float tables on column
                        segments: 112 groups in 3 segments of 38, 38 and 36, and the LAST group (x0 = 1776, 7 macropixels) is ragged in
                        the last segment: the dword-by-dword branch with p0 != 0 and blockIdx.z > 0.  With clahe_float_tables = 0
                        the same shape is the ragged quad path in one segment
    64 x 8,    16 x 2:  17 pairs > 15, tile_w = 4: (9 - 3) * 4 / 16 = 1 < 40, quads whatever clahe_float_tables says
    128 x 8,   64 x 2:  65 pairs > 63: the global-LUT kernel
    96 x 10,   16 x 2:  17 pairs > 15, tile_w = 6: (9 - 3) * 6 / 16 = 2 < 40, quads again, on tiles that are no power of two
    192 x 10,  64 x 2:  65 pairs > 63: the global-LUT kernel again, tile_w = 3

How many column segments plan_interp422 makes is not observable: the rungs are chosen from its arithmetic, restated above, and the
segment count is not asserted against the library.  The float-table rungs (64 x 48, 1792 x 8, 1790 x 8) are the only ones that run the
float-table bodies, so the test first shows that the two arithmetic modes differ on their D1 / D2 / D3 content too.

The expected luma is oracle.clahe on the gathered luma in the arithmetic mode of the call (oracle.set_fp_contract); chroma is copied
(packed out), the rounding mean of each row pair (NV12 out), or the even (U) and odd (V) columns of that mean (planar out).  Every plane
lies in a sentinel-filled allocation at a padded pitch, the WHOLE allocations are compared, and every comparison is exact bytes."""
import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
import clahe_u8_rungs
from mi_lumaeq import synth, UV_COPY, FMT_YUY2, FMT_UYVY
from mi_lumaeq.capi import Yuv420Planes, BgrYuv420FrameDev, CHROMA_PLANAR

pytestmark = pytest.mark.gpu
SENT = 0x5A
N = 3
DISTS = ["D1", "D2", "D3"]
CLIP = 2.0
# (width, height, tiles_x, tiles_y): plain float tables, column-segment float tables, quad fallback of a wide grid, global LUTs;
# then the last two again on tiles where the arithmetic mode shows; then column segments whose last group is ragged
SHAPES = [(64, 48, 8, 8), (1792, 8, 16, 2), (64, 8, 16, 2), (128, 8, 64, 2), (96, 10, 16, 2), (192, 10, 64, 2), (1790, 8, 16, 2)]
MODE_SHAPES = SHAPES[4:6]                                        # luma from clahe_u8_rungs.content, not from D1 / D2 / D3
FLOAT_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[6]]                 # the rungs that run float tables: the modes differ on D1 / D2 / D3 there
FORMS = ["packed_batch", "packed_list", "nv12_batch", "nv12_list", "yuv420_batch", "yuv420_list"]
FMTS = [FMT_YUY2, FMT_UYVY]
# (clahe_float_tables, clahe_fp_contract); the first is the default pair, whose bytes the other pair with fp_contract 0 must repeat
OPTIONS = [(1, 0), (0, 0), (1, 1), (0, 1)]
OFFS = (4, 8, 12)                                                # bytes past a 16-byte boundary
OFFS4 = (0, 4, 8, 12)                                            # the planar list: in, Y, U and V of a frame each at its own


def stream():
    return torch.cuda.current_stream().cuda_stream


def align4(x):
    return (x + 3) & ~3


def up16(x):
    return (x + 15) & ~15


def luma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, fmt - 2:2 * w:2])


def chroma(frame, w, fmt):
    return np.ascontiguousarray(frame[:, 3 - fmt:2 * w:2])


def uv_mean(c):
    """The header's chroma rule: UV row r is the per-byte rounding mean of chroma rows 2r and 2r+1."""
    a, b = c[0::2], c[1::2]
    return ((a.astype(np.uint16) + b + 1) >> 1).astype(np.uint8)


_ref_cache = {}


def y_plane(shape, k):
    """The luma of frame k of a shape."""
    w, h = shape[:2]
    return clahe_u8_rungs.content(w, h, 100 + k) if shape in MODE_SHAPES else synth.y_plane(w, h, DISTS[k], 500 + k)


def packed_frame(shape, fmt, k):
    w, h = shape[:2]
    f = synth.packed422_frame(w, h, fmt, DISTS[k], 500 + k)
    if shape in MODE_SHAPES:
        f = f.copy()
        f[:, fmt - 2:2 * w:2] = y_plane(shape, k)
    return f


def y_ref(shape, k, contract):
    """oracle.clahe on the luma of frame k of a shape (the same plane in both formats), computed once per arithmetic mode."""
    key = (shape, k, contract)
    if key not in _ref_cache:
        w, h, tx, ty = shape
        old = oracle.set_fp_contract(bool(contract))
        try:
            _ref_cache[key] = oracle.clahe(y_plane(shape, k), CLIP, tx, ty)
        finally:
            oracle.set_fp_contract(old)
    return _ref_cache[key]


class Layout:
    """Sentinel-filled device allocations and the planes placed in them, each as (allocation, byte offset, pitch)."""

    def __init__(self):
        self.bufs = []

    def alloc(self, size):
        b = torch.full((size,), SENT, dtype=torch.uint8, device="cuda:0")
        assert b.data_ptr() % 16 == 0
        self.bufs.append(b)
        return len(self.bufs) - 1

    def batch(self, pitch, fstride, off):
        """N planes in one allocation, `fstride` bytes apart, the first `off` bytes in."""
        b = self.alloc(off + fstride * N + 64)
        return [(b, off + k * fstride, pitch) for k in range(N)]

    def frames(self, rows, pitch, first, offs=OFFS):
        """N planes, each in an allocation of its own at its own offset."""
        offs = [offs[(first + k) % len(offs)] for k in range(N)]
        return [(self.alloc(o + pitch * rows + 64), o, pitch) for o in offs]

    def planes3(self, h, y_pitch, c_pitch):
        """N frames of three planes (H rows, H / 2, H / 2) in ONE allocation with one frame stride: Y, U and V start 4, 8 and 12 bytes
        past a 16-byte boundary, and the stride is 4 past one, so every frame's planes have phases of their own."""
        y_at = OFFS[0]
        u_at = up16(y_at + y_pitch * h) + OFFS[1]
        v_at = up16(u_at + c_pitch * (h // 2)) + OFFS[2]
        fstride = up16(v_at + c_pitch * (h // 2) - y_at) + 4
        b = self.alloc(y_at + fstride * N + 64)
        return fstride, [[(b, at + k * fstride, pitch) for k in range(N)] for at, pitch in ((y_at, y_pitch), (u_at, c_pitch), (v_at, c_pitch))]

    def ptr(self, at):
        return self.bufs[at[0]].data_ptr() + at[1]

    def image(self, painted):
        """All allocations, concatenated, as they must read with `painted` = [(plane, pixels), ...] in them."""
        imgs = [np.full(b.numel(), SENT, np.uint8) for b in self.bufs]
        for (bi, off, pitch), px in painted:
            rows, wb = px.shape
            imgs[bi][off: off + pitch * rows].reshape(rows, pitch)[:, :wb] = px
        return np.concatenate(imgs)

    def upload(self, painted):
        img = torch.from_numpy(self.image(painted)).to("cuda:0")
        o = 0
        for b in self.bufs:
            b.copy_(img[o: o + b.numel()])
            o += b.numel()

    def host(self):
        return torch.cat(self.bufs).cpu().numpy()


class Case:
    """One form on one shape: where its inputs and outputs lie, how it is called, what it must write."""

    def __init__(self, form, shape):
        self.form, self.shape = form, shape
        w, h = shape[:2]
        self.nv12, self.yuv420, self.list = form.startswith("nv12"), form.startswith("yuv420"), form.endswith("list")
        self.lay = lay = Layout()
        self.in_pitch = 2 * w + 4
        self.in_frame = self.in_pitch * h + 20
        self.ins = lay.frames(h, self.in_pitch, 0) if self.list else lay.batch(self.in_pitch, self.in_frame, 4)
        if self.nv12:
            self.y_pitch, self.uv_pitch = align4(w) + 4, align4(w) + 20
            self.out_frame = self.y_pitch * h + 12                          # one frame stride for both planes
            if self.list:
                self.ys, self.uvs = lay.frames(h, self.y_pitch, 1), lay.frames(h // 2, self.uv_pitch, 2)
            else:
                self.ys = lay.batch(self.y_pitch, self.out_frame, 8)
                self.uvs = lay.batch(self.uv_pitch, self.out_frame, 12)
        elif self.yuv420:
            self.y_pitch, self.c_pitch = align4(w) + 4, align4(w // 2) + 12
            if self.list:                                                   # frame 0: in at 4, Y at 8, U at 12, V at 0
                self.ys = lay.frames(h, self.y_pitch, 2, OFFS4)
                self.us, self.vs = lay.frames(h // 2, self.c_pitch, 3, OFFS4), lay.frames(h // 2, self.c_pitch, 0, OFFS4)
            else:
                self.out_frame, (self.ys, self.us, self.vs) = lay.planes3(h, self.y_pitch, self.c_pitch)
        else:
            self.out_pitch = 2 * w + 36
            self.out_frame = self.out_pitch * h
            self.outs = lay.frames(h, self.out_pitch, 1) if self.list else lay.batch(self.out_pitch, self.out_frame, 8)

    def call(self, c, fmt):
        w, h, tx, ty = self.shape
        p = self.lay.ptr
        ins = [p(a) for a in self.ins]
        if self.nv12:
            ys, uvs = [p(a) for a in self.ys], [p(a) for a in self.uvs]
            if self.list:
                c.clahe_packed422_to_nv12_frames(ins, ys, uvs, w, h, fmt, UV_COPY, CLIP, tx, ty, in_pitch=self.in_pitch,
                                                 y_pitch=self.y_pitch, uv_pitch=self.uv_pitch, stream=stream())
            else:
                c.clahe_packed422_to_nv12_batch_dev(ins[0], ys[0], uvs[0], w, h, N, fmt, UV_COPY, CLIP, tx, ty, in_pitch=self.in_pitch,
                                                    in_frame=self.in_frame, y_pitch=self.y_pitch, uv_pitch=self.uv_pitch,
                                                    out_frame=self.out_frame, stream=stream())
        elif self.yuv420:
            ys, us, vs = [p(a) for a in self.ys], [p(a) for a in self.us], [p(a) for a in self.vs]
            if self.list:
                entries = [BgrYuv420FrameDev(*a) for a in zip(ins, ys, us, vs)]
                c.clahe_packed422_to_yuv420_frames_dev(entries, w, h, self.in_pitch, self.y_pitch, self.c_pitch, CHROMA_PLANAR, fmt, UV_COPY,
                                                       CLIP, tx, ty, stream=stream())
            else:
                planes = Yuv420Planes(ys[0], self.y_pitch, us[0], vs[0], self.c_pitch, self.out_frame, CHROMA_PLANAR)
                c.clahe_packed422_to_yuv420_batch_dev(ins[0], planes, w, h, N, fmt, UV_COPY, CLIP, tx, ty, in_pitch=self.in_pitch,
                                                      in_frame=self.in_frame, stream=stream())
        else:
            outs = [p(a) for a in self.outs]
            if self.list:
                c.clahe_packed422_frames(ins, outs, w, h, fmt, UV_COPY, CLIP, tx, ty, in_pitch=self.in_pitch,
                                         out_pitch=self.out_pitch, stream=stream())
            else:
                c.clahe_packed422_batch_dev(ins[0], outs[0], w, h, N, fmt, UV_COPY, CLIP, tx, ty, in_pitch=self.in_pitch,
                                            in_frame=self.in_frame, out_pitch=self.out_pitch, out_frame=self.out_frame, stream=stream())

    def expected(self, frames, fmt, contract):
        """The inputs as uploaded and the outputs of a call, as Layout.image takes them."""
        w = self.shape[0]
        painted = list(zip(self.ins, frames))
        for k, f in enumerate(frames):
            y = y_ref(self.shape, k, contract)
            if self.nv12:
                painted += [(self.ys[k], y), (self.uvs[k], uv_mean(chroma(f, w, fmt)))]
            elif self.yuv420:
                uv = uv_mean(chroma(f, w, fmt))
                painted += [(self.ys[k], y), (self.us[k], uv[:, 0::2]), (self.vs[k], uv[:, 1::2])]
            else:
                out = f.copy()
                out[:, fmt - 2::2] = y
                painted.append((self.outs[k], out))
        return painted


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_every_rung(c, shape, form):
    """Three frames per call; both formats, MI_UV_COPY, clahe_float_tables and clahe_fp_contract both ways.  The bytes are the
    oracle's in the call's arithmetic mode, and with clahe_fp_contract = 0 also those of the default tables (the same bytes on
    every path)."""
    w, h = shape[:2]
    if shape in MODE_SHAPES or shape in FLOAT_SHAPES:            # the two arithmetic modes are told apart on this shape
        assert any(not np.array_equal(y_ref(shape, k, 0), y_ref(shape, k, 1)) for k in range(N)), (shape, "both modes give the same bytes")
    case = Case(form, shape)
    try:
        for fmt in FMTS:
            frames = [packed_frame(shape, fmt, k) for k in range(N)]
            assert all(np.array_equal(luma(f, w, fmt), y_plane(shape, k)) for k, f in enumerate(frames))
            default = None
            for float_tables, contract in OPTIONS:
                why = (form, shape, fmt, float_tables, contract)
                c.set_option("clahe_float_tables", float_tables)
                c.set_option("clahe_fp_contract", contract)
                case.lay.upload(list(zip(case.ins, frames)))                # also resets the outputs to the sentinel
                case.call(c, fmt)
                torch.cuda.synchronize()
                got, want = case.lay.host(), case.lay.image(case.expected(frames, fmt, contract))
                bad = np.flatnonzero(got != want)
                print(why, "differing bytes:", bad.size, "first:", bad[:1])
                assert bad.size == 0, (why, int(bad.size), bad[:8])
                if (float_tables, contract) == (1, 0):
                    default = got
                elif contract == 0:
                    assert np.array_equal(got, default), (why, "differs from clahe_float_tables = 1")
    finally:
        c.set_option("clahe_float_tables", 1)
        c.set_option("clahe_fp_contract", 0)
