"""Pitched, guarded layouts for the strided device batch forms (every *_batch_dev entry takes a row pitch and a frame stride per side).

A `Side` is one side of a call -- n frames of `rows` x `row_bytes` bytes at `off + k * frame_stride`, rows `pitch` bytes apart -- inside
ONE uint8 allocation filled with a sentinel, 64 guard bytes behind the last row.  A test uploads `image(frames)`, runs the call on
`ptr` / `pitch` / `frame_stride`, and hands the sides with the images they must now hold to `assert_sides`, which compares whole
allocations: a byte stored into row padding, into the gap between frames or behind the last frame fails like a wrong pixel does, and
so does an input that was written.  tests/test_strided_layouts.py shows on a numpy stand-in for the device that planted pitch and
stride faults are caught.  A plain module, like tests/color_mutants.py."""
from __future__ import annotations

import numpy as np

SENTINEL = 0x5A
GUARD = 64


def _align(x: int, a: int) -> int:
    return (x + a - 1) // a * a


class Side:
    def __init__(self, rows, row_bytes, pitch, off, n, frame_stride, name=""):
        assert pitch >= row_bytes and (n <= 1 or frame_stride >= (rows - 1) * pitch + row_bytes), "frames must not overlap"
        self.rows, self.row_bytes, self.pitch, self.off, self.n, self.frame_stride = rows, row_bytes, pitch, off, n, frame_stride
        self.name = name
        self.end = off + (n - 1) * frame_stride + (rows - 1) * pitch + row_bytes        # one past the last image byte
        self.nbytes = self.end + GUARD
        self.buf = None                                                                  # the allocation: a torch uint8 tensor

    def __repr__(self):
        return (f"Side({self.name or '?'}: {self.n} x {self.rows} rows of {self.row_bytes} B, pitch {self.pitch}, off {self.off}, "
                f"frame stride {self.frame_stride}, {self.nbytes} B)")

    # ---- what the allocation must read ----
    def image(self, frames=None) -> np.ndarray:
        """The whole allocation as it must read with `frames` (n arrays of rows x row_bytes bytes, any dtype) in it; None: untouched."""
        a = np.full(self.nbytes, SENTINEL, np.uint8)
        if frames is not None:
            assert len(frames) == self.n, (len(frames), self.n)
            for k, f in enumerate(frames):
                f = np.ascontiguousarray(f)
                self.frame_view(a, k)[:] = f.view(np.uint8).reshape(self.rows, self.row_bytes)
        return a

    def frame_view(self, a: np.ndarray, k: int) -> np.ndarray:
        """Frame k of a host copy of the allocation: a rows x row_bytes view (writable when `a` is)."""
        base = self.off + k * self.frame_stride
        return np.lib.stride_tricks.as_strided(a[base:], (self.rows, self.row_bytes), (self.pitch, 1))

    def where(self, o: int) -> str:
        """Offset in the allocation -> "frame k row r col c", or what kind of byte outside every image it is."""
        if o >= self.end:
            return f"guard +{o - self.end}"
        if o < self.off:
            return f"gap before frame 0 (+{o})"
        k = min((o - self.off) // self.frame_stride, self.n - 1) if self.n > 1 else 0
        r, c = divmod(o - self.off - k * self.frame_stride, self.pitch)
        if r >= self.rows or (r == self.rows - 1 and c >= self.row_bytes):
            return f"gap behind frame {k} (+{o - self.off - k * self.frame_stride - (self.rows - 1) * self.pitch - self.row_bytes})"
        if c >= self.row_bytes:
            return f"padding of frame {k} row {r} (+{c - self.row_bytes})"
        return f"frame {k} row {r} col {c}"

    # ---- the allocation ----
    def upload(self, frames=None, device="cuda:0"):
        """(Re)create the allocation on `device` holding image(frames); "cpu" serves the numpy stand-in of the CPU tests."""
        import torch
        img = self.image(frames)
        if str(device) == "cpu":
            self.buf = torch.from_numpy(img)
        else:
            from mi_lumaeq import xfer
            self.buf = xfer.to_device(img, device)
        return self

    @property
    def ptr(self) -> int:
        """Address of frame 0."""
        return int(self.buf.data_ptr()) + self.off

    def download(self) -> np.ndarray:
        from mi_lumaeq import xfer
        return xfer.to_host(self.buf)


def assert_sides(got, want, why):
    """got: a Side or a sequence of Sides (uploaded, the call done and synchronised); want: for each the image() it must hold now.
    Whole allocations, byte for byte; a failure names the first differing offsets by frame / row / column or padding / gap / guard."""
    if isinstance(got, Side):
        got, want = [got], [want]
    assert len(got) == len(want)
    msgs = []
    for side, w in zip(got, want):
        g = side.download()
        assert g.shape == w.shape == (side.nbytes,), (side, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        if bad.size:
            first = ", ".join(f"@{int(o)} {side.where(int(o))}: got 0x{int(g[o]):02x} want 0x{int(w[o]):02x}" for o in bad[:6])
            msgs.append(f"{side!r}: {bad.size} bytes differ; first {first}")
    assert not msgs, f"{why}: " + " | ".join(msgs)


# ---- the four layout classes ----
def make_side(cls, rows, row_bytes, n, elem=1, variant=0, name=None) -> Side:
    """cls: "T" tight pitch, tight stride, off 0;  "Tgap" tight pitch, stride rows * pitch + 5 (flattened addressing, every frame at
    another alignment);  "A16" pitch align(row_bytes, 16) + 16, off 16, stride a multiple of 16 (row-wise, every row 16-byte aligned);
    "U" pitch row_bytes + 1, off 3, stride rows * pitch + 7 (row alignment walks through the residues).  elem = 2 (16-bit planes):
    everything stays even -- Tgap gap 6; U pitch row_bytes + 2, off 2, gap 6.  variant 1: another pitch of the same class (A16, U)."""
    assert elem in (1, 2) and row_bytes % elem == 0
    if cls == "T":
        pitch, off, gap = row_bytes, 0, 0
    elif cls == "Tgap":
        pitch, off, gap = row_bytes, 0, 5 if elem == 1 else 6
    elif cls == "A16":
        pitch, off, gap = _align(row_bytes, 16) + 16 * (1 + variant), 16, 32
    elif cls == "U":
        pitch, off, gap = (row_bytes + 1 + 2 * variant, 3, 7) if elem == 1 else (row_bytes + 2 + 4 * variant, 2, 6)
    else:
        raise ValueError(cls)
    return Side(rows, row_bytes, pitch, off, n, rows * pitch + gap, name or (cls if not variant else f"{cls}'"))


# source class, destination class; None = in place (ONE Side is both).  Equal classes get different pitches (variant 1 on the destination).
PAIRINGS = {
    "T-A16": ("T", "A16"), "A16-T": ("A16", "T"), "A16-A16": ("A16", "A16"), "U-A16": ("U", "A16"), "A16-U": ("A16", "U"),
    "U-U": ("U", "U"), "Tgap-Tgap": ("Tgap", "Tgap"), "inplace-A16": ("A16", None), "inplace-U": ("U", None),
}


def make_pair(pairing, rows, row_bytes, n, elem=1, dst_rows=None, dst_row_bytes=None):
    """(src, dst) Sides of PAIRINGS[pairing]; dst is src when in place."""
    s, d = PAIRINGS[pairing]
    src = make_side(s, rows, row_bytes, n, elem)
    if d is None:
        assert dst_rows in (None, rows) and dst_row_bytes in (None, row_bytes)
        return src, src
    return src, make_side(d, dst_rows or rows, dst_row_bytes or row_bytes, n, elem, variant=1 if d == s and d in ("A16", "U") else 0)
