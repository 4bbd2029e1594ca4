"""tests/strided_layouts.py on a numpy stand-in for the device: the whole-allocation comparer passes a correct strided op on every
pairing of layouts and fails each of five planted pitch / stride / overrun faults.  No GPU."""
import numpy as np
import pytest

import strided_layouts as L

ROWS, ROW_BYTES, N = 5, 50, 3


def ref_op(frame):
    """The reference op of the stand-in device: a byte map that is no identity and never yields a constant row."""
    return (frame.astype(np.uint16) * 7 + 13).astype(np.uint8)


def frames_for(rows=ROWS, row_bytes=ROW_BYTES, n=N, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (rows, row_bytes), dtype=np.uint8) for _ in range(n)]


def fake_device_op(src, dst, fault=None):
    """ref_op from Side `src` into Side `dst` (dst may be src) on their "cpu" allocations, addressed the way a kernel does: from the
    two frame-0 addresses with pitches and frame strides.  `fault` plants one wrong term."""
    s, d = src.buf.numpy(), dst.buf.numpy()
    d_pitch, d_frame = dst.pitch, dst.frame_stride
    if fault == "dst_pitch_ignored":
        d_pitch = dst.row_bytes
    elif fault == "src_pitch_for_dst":
        d_pitch = src.pitch
    elif fault == "frame_stride_is_rows_x_pitch":
        d_frame = dst.rows * dst.pitch
    for k in range(src.n):
        for r in range(src.rows):
            so = src.off + k * src.frame_stride + r * src.pitch
            do = dst.off + k * d_frame + r * d_pitch
            out = ref_op(s[so:so + src.row_bytes])
            keep = max(0, min(dst.row_bytes, d.size - do))      # a store past the allocation lands in memory no test can see
            d[do:do + keep] = out[:keep]
            if fault == "one_byte_past_row_end" and do + dst.row_bytes < d.size:
                d[do + dst.row_bytes] = out[-1] ^ 0xFF if (out[-1] ^ 0xFF) != L.SENTINEL else 0
    if fault == "one_byte_into_guard":
        d[dst.end + 17] = 0


def run(pairing, fault=None):
    frames = frames_for()
    src, dst = L.make_pair(pairing, ROWS, ROW_BYTES, N)
    src.upload(frames, "cpu")
    if dst is not src:
        dst.upload(None, "cpu")
    fake_device_op(src, dst, fault)
    want = [ref_op(f) for f in frames]
    if dst is src:
        L.assert_sides(src, src.image(want), f"{pairing} {fault}")
    else:
        L.assert_sides([src, dst], [src.image(frames), dst.image(want)], f"{pairing} {fault}")


@pytest.mark.parametrize("pairing", list(L.PAIRINGS))
def test_correct_strided_op_passes(pairing):
    run(pairing)


# where each fault changes an address at all: a tight destination has no pitch to ignore, in place the two pitches are one
FAULT_CASES = (
    [("dst_pitch_ignored", p) for p in ("T-A16", "A16-A16", "U-A16", "A16-U", "U-U", "inplace-A16", "inplace-U")]
    + [("src_pitch_for_dst", p) for p in ("T-A16", "A16-T", "A16-A16", "U-A16", "A16-U", "U-U")]
    + [("frame_stride_is_rows_x_pitch", p) for p in ("T-A16", "A16-A16", "U-A16", "A16-U", "U-U", "Tgap-Tgap", "inplace-A16", "inplace-U")]
    + [("one_byte_past_row_end", p) for p in L.PAIRINGS]
    + [("one_byte_into_guard", p) for p in L.PAIRINGS])


@pytest.mark.parametrize("fault,pairing", FAULT_CASES, ids=lambda v: v)
def test_planted_fault_is_caught(fault, pairing):
    with pytest.raises(AssertionError, match="bytes differ"):
        run(pairing, fault)


def test_a_written_input_is_caught():
    frames = frames_for()
    src, dst = L.make_pair("A16-U", ROWS, ROW_BYTES, N)
    src.upload(frames, "cpu"); dst.upload(None, "cpu")
    fake_device_op(src, dst)
    src.buf.numpy()[src.off + src.frame_stride + 2 * src.pitch + 7] ^= 1
    with pytest.raises(AssertionError, match=r"Side\(A16.*1 bytes differ.*frame 1 row 2 col 7"):
        L.assert_sides([src, dst], [src.image(frames), dst.image([ref_op(f) for f in frames])], "input written")


def test_failure_names_padding_gap_and_guard():
    s = L.make_side("U", ROWS, ROW_BYTES, N)
    assert s.where(0) == "gap before frame 0 (+0)"
    assert s.where(s.off) == "frame 0 row 0 col 0"
    assert s.where(s.off + ROW_BYTES) == "padding of frame 0 row 0 (+0)"
    assert s.where(s.off + s.frame_stride + 3 * s.pitch + 9) == "frame 1 row 3 col 9"
    last = s.off + s.frame_stride + (ROWS - 1) * s.pitch + ROW_BYTES
    assert s.where(last - 1) == f"frame 1 row {ROWS - 1} col {ROW_BYTES - 1}"
    assert s.where(last) == "gap behind frame 1 (+0)"
    assert s.where(s.off + 2 * s.frame_stride - 1).startswith("gap behind frame 1")
    assert s.where(s.end - 1) == f"frame 2 row {ROWS - 1} col {ROW_BYTES - 1}"
    assert s.where(s.end) == "guard +0" and s.where(s.nbytes - 1) == f"guard +{L.GUARD - 1}"
    s.upload(None, "cpu")
    s.buf.numpy()[s.end + 5] = 1
    with pytest.raises(AssertionError, match=r"guard \+5: got 0x01 want 0x5a"):
        L.assert_sides(s, s.image(None), "guard")


def test_layout_classes_are_what_they_say():
    for elem in (1, 2):
        rb = ROW_BYTES * elem
        t, tg, a, a2, u, u2 = (L.make_side(c, ROWS, rb, N, elem, v) for c, v in
                               [("T", 0), ("Tgap", 0), ("A16", 0), ("A16", 1), ("U", 0), ("U", 1)])
        assert (t.pitch, t.off, t.frame_stride) == (rb, 0, ROWS * rb)
        assert (tg.pitch, tg.off, tg.frame_stride) == (rb, 0, ROWS * rb + (5 if elem == 1 else 6))
        for s in (a, a2):
            assert s.pitch >= rb + 16 and s.pitch % 16 == 0 and s.off == 16 and s.frame_stride % 16 == 0 and s.frame_stride > ROWS * s.pitch
        assert a.pitch != a2.pitch and u.pitch != u2.pitch
        if elem == 1:
            assert (u.pitch, u.off, u.frame_stride) == (rb + 1, 3, ROWS * (rb + 1) + 7)
            # rows of one frame start at more than two residues mod 16, an aligned one among all frames' rows or not: vector and byte rows mix
            res = {(u.off + k * u.frame_stride + r * u.pitch) % 16 for k in range(N) for r in range(ROWS)}
            assert len(res) >= 5
        else:
            assert (u.pitch, u.off, u.frame_stride) == (rb + 2, 2, ROWS * (rb + 2) + 6)
        for s in (t, tg, a, a2, u, u2):
            assert all(v % elem == 0 for v in (s.pitch, s.off, s.frame_stride))
            img = s.image(None)
            assert img.shape == (s.nbytes,) and (img == L.SENTINEL).all() and s.nbytes == s.end + L.GUARD
            filled = s.image([np.full((ROWS, rb), k + 1, np.uint8) for k in range(N)])
            assert int((filled != L.SENTINEL).sum()) == N * ROWS * rb
            assert (L.Side.frame_view(s, filled, 2) == 3).all()
    with pytest.raises(AssertionError):
        L.Side(4, 8, 8, 0, 2, 16)                      # overlapping frames
