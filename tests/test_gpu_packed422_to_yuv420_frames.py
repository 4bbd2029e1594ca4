"""Packed 4:2:2 frames in (YUY2 / UYVY), planar 4:2:0 frames out on LISTS of device frames: mi_equalize_hist_packed422_to_yuv420_frames_dev
and mi_clahe_packed422_to_yuv420_frames_dev.  70 frames of 32 x 4 cross the 64-frame chunk of the list; every plane of every frame lies
in a sentinel-filled allocation of its own at a base 0 / 4 / 8 / 12 bytes past a 16-byte boundary that varies within the list.  Per
frame the bytes equal a batch call with n_frames = 1 (whose bytes tests/test_gpu_packed422_to_yuv420.py pins to the oracle); the WHOLE
of every allocation is compared: exact bytes."""
import ctypes

import numpy as np
import pytest
import torch

import mi_lumaeq
import test_gpu_packed422_to_nv12 as nv                 # helpers only
import test_gpu_packed422_to_yuv420 as pl               # helpers only: PlanarOut, run
from mi_lumaeq import UV_FILL128, UV_COPY, FMT_YUY2, FMT_UYVY
from mi_lumaeq.capi import BgrYuv420FrameDev, CHROMA_INTERLEAVED, CHROMA_PLANAR

pytestmark = pytest.mark.gpu
BAD_ARG = 1
SENT = nv.SENT
OFFS = (0, 4, 8, 12)
W, H, N, DISTINCT = 32, 4, 70, 7
CASES = [("eq", None, UV_COPY, FMT_YUY2), ("clahe", (2.0, 2, 2), UV_COPY, FMT_UYVY), ("clahe", pl.WIDE, UV_FILL128, FMT_YUY2),
         ("eq", None, UV_FILL128, FMT_UYVY), ("clahe", (3.0, 4, 2), UV_COPY, FMT_YUY2)]
stream = nv.stream


def dev_buf(size):
    b = torch.full((size,), SENT, dtype=torch.uint8, device="cuda:0")
    assert b.data_ptr() % 16 == 0
    return b


class Pool:
    """n frames, four allocations each: the input (H rows of 2W bytes at in_pitch), Y (H x W at y_pitch), U and V (H/2 x W/2 at c_pitch).
    Frame k holds content k % DISTINCT; `alias` = (k, j) makes entry k read entry j's input allocation."""

    def __init__(self, w, h, n, frames, alias=None):
        self.w, self.h, self.n, self.frames = w, h, n, frames
        self.in_pitch, self.y_pitch, self.c_pitch = 2 * w + 12, nv.align4(w) + 4, nv.align4(w // 2) + 4
        self.ins, self.outs = [], []                    # (buffer, offset) per frame; (y, u, v) triples of them
        for k in range(n):
            o = OFFS[k % 4]
            b = dev_buf(o + self.in_pitch * h + 64)
            img = np.full(b.numel(), SENT, np.uint8)
            img[o: o + self.in_pitch * h].reshape(h, self.in_pitch)[:, : 2 * w] = frames[k % len(frames)]
            b.copy_(torch.from_numpy(img))
            self.ins.append((b, o))
            self.outs.append(tuple((dev_buf(OFFS[(k + j) % 4] + pitch * rows + 64), OFFS[(k + j) % 4])
                                   for j, (pitch, rows) in enumerate(((self.y_pitch, h), (self.c_pitch, h // 2), (self.c_pitch, h // 2)), 1)))
        if alias:
            k, j = alias
            assert k % len(frames) == j % len(frames)
            self.ins[k] = self.ins[j]
        self.in_image = torch.cat([b for b, _ in self.ins]).cpu().numpy()

    def entries(self):
        arr = (BgrYuv420FrameDev * self.n)()
        for k in range(self.n):
            (ib, io), ((yb, yo), (ub, uo), (vb, vo)) = self.ins[k], self.outs[k]
            arr[k] = BgrYuv420FrameDev(ib.data_ptr() + io, yb.data_ptr() + yo, ub.data_ptr() + uo, vb.data_ptr() + vo)
        return arr

    def clear(self):
        for t in self.outs:
            for b, _ in t:
                b.fill_(SENT)

    def host(self):
        return torch.cat([b for t in self.outs for b, _ in t]).cpu().numpy()

    def image(self, planes=None):
        """Every output allocation, concatenated, with planes[k % len(planes)] = (Y, U, V) in frame k (None: untouched)."""
        imgs = []
        for k, t in enumerate(self.outs):
            for j, ((b, o), pitch, rows, cols) in enumerate(zip(t, (self.y_pitch, self.c_pitch, self.c_pitch), (self.h, self.h // 2, self.h // 2),
                                                               (self.w, self.w // 2, self.w // 2))):
                img = np.full(b.numel(), SENT, np.uint8)
                if planes is not None:
                    img[o: o + pitch * rows].reshape(rows, pitch)[:, :cols] = planes[k % len(planes)][j]
                imgs.append(img)
        return np.concatenate(imgs)

    def inputs_unchanged(self):
        return np.array_equal(torch.cat([b for b, _ in self.ins]).cpu().numpy(), self.in_image)


def run_list(c, op, cfg, pool, arr, fmt, uv_mode, chroma=CHROMA_PLANAR):
    a = (arr, pool.w, pool.h, pool.in_pitch, pool.y_pitch, pool.c_pitch, chroma, fmt, uv_mode)
    if op == "eq":
        c.equalize_hist_packed422_to_yuv420_frames_dev(*a, stream=stream())
    else:
        c.clahe_packed422_to_yuv420_frames_dev(*a, *cfg, stream=stream())


def batch_planes(c, frames, w, h, fmt, op, cfg, uv_mode):
    """(Y, U, V) of every frame from a batch call with n_frames = 1."""
    out = []
    for f in frames:
        src = nv.Batch(w, h, 1, nv.LAYOUTS[0]).upload([f])
        dst = pl.PlanarOut(w, h, 1, "one")
        pl.run(c, op, cfg, src, dst.planes(), fmt, uv_mode)
        torch.cuda.synchronize()
        out.append(tuple(dst.plane(name, 0) for name in ("y", "u", "v")))
    return out


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        yield ctx


@pytest.mark.parametrize("op,cfg,uv_mode,fmt", CASES)
def test_seventy_frames_cross_the_chunk(c, op, cfg, uv_mode, fmt):
    """70 frames in two chunks (64 + 6); entry 69 reads the input allocation of entry 6 (the same input in two entries)."""
    assert nv.planar_status(c, W, H, 1, op, cfg) == 0
    frames = nv.make_frames(W, H, fmt, [nv.DISTS[k % 5] for k in range(DISTINCT)], 1200)
    pool = Pool(W, H, N, frames, alias=(69, 6))
    want = batch_planes(c, frames, W, H, fmt, op, cfg, uv_mode)
    run_list(c, op, cfg, pool, pool.entries(), fmt, uv_mode)
    torch.cuda.synchronize()
    got, exp = pool.host(), pool.image(want)
    assert np.array_equal(got, exp), (op, cfg, uv_mode, fmt, int((got != exp).sum()), np.flatnonzero(got != exp)[:8])
    assert pool.inputs_unchanged(), "an input allocation was written"


def test_interleaved_list_is_the_nv12_list_form(c):
    """out_chroma = MI_CHROMA_INTERLEAVED: the call is mi_*_packed422_to_nv12_frames_dev on {in, y, c0}; c1 is ignored."""
    n, fmt = 5, FMT_YUY2
    frames = nv.make_frames(W, H, fmt, nv.DISTS, 1300)
    ins = [dev_buf(2 * W * H) for _ in range(n)]
    for b, f in zip(ins, frames):
        b.copy_(torch.from_numpy(f.ravel()))
    for op, cfg in (("eq", None), ("clahe", (2.0, 2, 2))):
        ys = [[dev_buf(W * H + 64) for _ in range(n)] for _ in range(2)]
        uvs = [[dev_buf(W * H // 2 + 64) for _ in range(n)] for _ in range(2)]
        if op == "eq":
            c.equalize_hist_packed422_to_nv12_frames(ins, ys[0], uvs[0], W, H, fmt, UV_COPY, in_pitch=2 * W, y_pitch=W, uv_pitch=W, stream=stream())
        else:
            c.clahe_packed422_to_nv12_frames(ins, ys[0], uvs[0], W, H, fmt, UV_COPY, *cfg, in_pitch=2 * W, y_pitch=W, uv_pitch=W, stream=stream())
        arr = [BgrYuv420FrameDev(ins[k].data_ptr(), ys[1][k].data_ptr(), uvs[1][k].data_ptr(), None) for k in range(n)]
        a = (arr, W, H, 2 * W, W, W, CHROMA_INTERLEAVED, fmt, UV_COPY)
        if op == "eq":
            c.equalize_hist_packed422_to_yuv420_frames_dev(*a, stream=stream())
        else:
            c.clahe_packed422_to_yuv420_frames_dev(*a, *cfg, stream=stream())
        torch.cuda.synchronize()
        for k in range(n):
            assert torch.equal(ys[0][k], ys[1][k]) and torch.equal(uvs[0][k], uvs[1][k]), (op, k)
            assert not bool((ys[1][k][: W * H] == SENT).all())


def test_a_bad_last_entry_refuses_the_call(c):
    """Nothing is enqueued unless every frame passes the checks: frame 0's outputs stay untouched."""
    fmt = FMT_YUY2
    frames = nv.make_frames(W, H, fmt, [nv.DISTS[k % 5] for k in range(DISTINCT)], 1200)
    pool = Pool(W, H, N, frames)
    good = pool.entries()
    last = good[N - 1]
    in_ptr = last.in_
    bad_last = [BgrYuv420FrameDev(last.in_, last.y, last.c0, None),                                  # a null c1
                BgrYuv420FrameDev(last.in_, last.y + 2, last.c0, last.c1),                           # an address = 2 mod 4
                BgrYuv420FrameDev(last.in_, last.y, last.c0, last.c1 + 2),
                BgrYuv420FrameDev(last.in_, in_ptr + pool.in_pitch + 8, last.c0, last.c1),           # Y meets the rows of its own input
                BgrYuv420FrameDev(last.in_, last.y, last.c0, last.c0),                               # U and V at one address
                BgrYuv420FrameDev(None, last.y, last.c0, last.c1)]
    L, hd = c._L, c._h
    for e in bad_last:
        arr = (BgrYuv420FrameDev * N)(*list(good))
        arr[N - 1] = e
        a = (hd, arr, N, W, H, pool.in_pitch, pool.y_pitch, pool.c_pitch, CHROMA_PLANAR, fmt, UV_COPY)
        assert L.mi_equalize_hist_packed422_to_yuv420_frames_dev(*a, stream()) == BAD_ARG
        assert L.mi_clahe_packed422_to_yuv420_frames_dev(*a, ctypes.c_double(2.0), 2, 2, stream()) == BAD_ARG
    a = (hd, good, N, W, H, pool.in_pitch, pool.y_pitch, pool.c_pitch)
    assert L.mi_equalize_hist_packed422_to_yuv420_frames_dev(*a, 2, fmt, UV_COPY, stream()) == BAD_ARG       # a chroma other than the two
    assert L.mi_equalize_hist_packed422_to_yuv420_frames_dev(hd, None, N, W, H, pool.in_pitch, pool.y_pitch, pool.c_pitch, CHROMA_PLANAR,
                                                            fmt, UV_COPY, stream()) == BAD_ARG
    assert L.mi_equalize_hist_packed422_to_yuv420_frames_dev(hd, good, N, W, H, pool.in_pitch, pool.y_pitch, pool.c_pitch + 2, CHROMA_PLANAR,
                                                            fmt, UV_COPY, stream()) == BAD_ARG
    assert L.mi_equalize_hist_packed422_to_yuv420_frames_dev(hd, good, 0, W, H, pool.in_pitch, pool.y_pitch, pool.c_pitch, CHROMA_PLANAR,
                                                            fmt, UV_COPY, stream()) == 0
    torch.cuda.synchronize()
    got = pool.host()
    assert np.array_equal(got, pool.image()), "a refused or empty call wrote"
    assert pool.inputs_unchanged()
    # and the context still works on the good list
    want = batch_planes(c, frames, W, H, fmt, "eq", None, UV_COPY)
    run_list(c, "eq", None, pool, good, fmt, UV_COPY)
    torch.cuda.synchronize()
    assert np.array_equal(pool.host(), pool.image(want))
