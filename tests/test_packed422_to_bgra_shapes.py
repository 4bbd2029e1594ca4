"""CPU checks behind tests/test_gpu_packed422_to_bgra.py and tests/test_gpu_packed422_to_bgra_frames.py: the shapes of
tests/packed422_bgra_ref.py do what their comments claim, by the walks restated in tests/packed422_geometry_cases.py (the new LUT-apply
kernel keeps lut_apply422_bgr_body's walk) and by the interpolation plan restated in tests/clahe_u8_rungs.py.  Nothing here needs a GPU
or the library."""
import re
from pathlib import Path

import numpy as np
import pytest

import clahe_u8_rungs as rungs
import packed422_bgra_ref as ref
import packed422_geometry_cases as g

ROOT = Path(__file__).resolve().parents[1]
KERNELS = ROOT / "opencv-opencl_amd" / "csrc" / "kernels"


def _code(name):
    return re.sub(r"\s+", "", re.sub(r"//[^\n]*", "", (KERNELS / name).read_text()))


def test_the_apply_kernel_keeps_the_three_channel_walk():
    """The carried (row, group) walk of the four-channel LUT-apply kernels is lut_apply422_bgr_body's because it IS that body: one
    text in packed422_bgr.hip.h, a template on the block type and a store policy, which both forms' kernels wrap -- with 64 bytes a
    group and 4 a pixel out as Store422Bgra's constants where Store422Bgr has 48 and 3."""
    bgr, bgra = _code("packed422_bgr.hip.h"), _code("packed422_bgra.hip.h")
    for piece in ("constintG=(p.dwords+7)>>3;", "constlonglongitems=(longlong)(r1-r0)*G;", "introw=t/G,grp=t-row*G;",
                  "constintdrow=kThreads/G,dgrp=kThreads-drow*G;", "for(longlongit=t;it<items;it+=kThreads){",
                  "row+=drow;grp+=dgrp;if(grp>=G){grp-=G;++row;}", "constintnd=min(8,p.dwords-8*grp);",
                  "constuint8_t*s=src0+(longlong)row*p.src_step+32LL*grp;",
                  "uint8_t*d=out0+(longlong)row*p.out_step+(longlong)S::kGroupBytes*grp;",
                  "uint8_t*dst=fr.out_of(f)+(longlong)S::kPxBytes*x0;"):
        assert bgr.count(piece) == 1 and piece not in bgra, piece
    for body in ("lut_apply422_bgr_body", "clahe_interp422_bgr_body"):
        assert len(re.findall(r"void" + body + r"\(constBlock&p,constFrames&fr,", bgr)) == 1, body
        assert "void" + body not in bgra and "void" + body.replace("bgr", "bgra") not in bgra, body
    assert "template<intORDER>structStore422Bgr{staticconstexprintkPxBytes=3,kGroupBytes=48;" in bgr
    assert "template<intORDER>structStore422Bgra{staticconstexprintkPxBytes=4,kGroupBytes=64;" in bgra
    # every entry of the four-channel form wraps the shared body with its own policy and its own two address policies
    for body in ("lut_apply422_bgr_body<OFF,", "clahe_interp422_bgr_body<FT,FMA,OFF,"):
        assert bgra.count(body + "Store422Bgra<ORDER>>(p,Strided422Bgra{p},") == 1, body
        assert bgra.count(body + "Store422Bgra<ORDER>>(p,Table422Bgra{l,p},") == 1, body
        assert bgr.count(body + "Store422Bgr<ORDER>>(p,Strided422Bgr{p},") == 1, body
        assert bgr.count(body + "Store422Bgr<ORDER>>(p,Table422Bgr{l,p},") == 1, body
    assert g.groups422(33) == 5 and g.groups422(8193) == 1025


def test_parity_shapes_have_the_groups_their_comments_name():
    """(full 16-column groups, macropixels of the ragged last group) of every parity shape."""
    want = {(2, 1): (0, 1), (16, 1): (1, 0), (18, 3): (1, 1), (30, 5): (1, 7), (40, 6): (2, 4), (66, 34): (4, 1)}
    assert [tuple(s) for s in ref.PARITY_SHAPES] == list(want)
    for (w, h), (full, nd) in want.items():
        dwords = w // 2
        assert (dwords // 8, dwords % 8) == (full, nd), (w, h)
        assert g.groups422(dwords) == full + (1 if nd else 0)
        assert g.bands_bound(w, h, h) == 1                        # one band: a band of one row for the one-row shapes
    assert 2 * 4 == 8                                             # the ragged group of 40 x 6 holds 8 columns


def test_parity_ops_take_the_paths_their_names_say():
    (_, cfg22), (_, cfg54), (_, cfg642) = ref.CL22, ref.CL54, ref.CL642
    assert ref.K_MAX_PAIRS == rungs.K_MAX_PAIRS
    assert cfg22[1] + 1 <= rungs.K_MAX_PAIRS_F32 and cfg54[1] + 1 <= rungs.K_MAX_PAIRS_F32      # LDS tables, float when the option is on
    assert cfg642[1] + 1 > rungs.K_MAX_PAIRS                                                      # 65 pairs: LUTs from global memory
    for w, h in ref.PARITY_SHAPES:
        assert (w % cfg54[1] or h % cfg54[2]), (w, h, "5 x 4 divides the frame: no REFLECT_101 padding")
    assert 66 % 2 == 0 and 34 % 2 == 0 and 40 % 2 == 0 and 6 % 2 == 0                           # 2 x 2 divides the two larger shapes
    assert set(ref.OPTIONS) == {(ft, fma) for ft in (0, 1) for fma in (0, 1)}
    assert set(ref.LDS_OPS) == {ref.CL22, ref.CL54} and ref.PARITY_OPS == [ref.EQ, ref.CL22, ref.CL54, ref.CL642]


def test_loop_shapes_loop():
    by = {s[0]: s for s in ref.LOOP_SHAPES}
    # 66 x 386: up to three bands, G = 5, the smallest band 128 rows: 640 items, three steps of 256; the group index wraps (dgrp = 1)
    assert g.walk("lut_apply422_bgr", 66, 386) == (640, 5, 256, 3)
    assert 256 // 5 == 51 and 256 - 51 * 5 == 1 and 640 > 2 * 256
    assert by["66x386x2"][3] == 2
    # 16386 x 1: G = 1025 > 256, drow = 0: a lane walks along the row; B may be 2 and band 0 is then empty
    assert g.walk("lut_apply422_bgr", 16386, 1) == (1025, 1025, 256, 2)
    assert 256 // 1025 == 0 and [(1 * k // 2, 1 * (k + 1) // 2) for k in range(2)] == [(0, 0), (0, 1)]
    assert 1025 == 4 * 256 + 1 and 8193 - 8 * 1024 == 1           # five steps, the last of one item; the last group holds one macropixel
    # the two CLAHE shapes: 4 column groups, so 64 phases; a lane's rows are 64 apart
    assert by["1040x44-cl22"][1:4] == (1040, 44, 1) and by["1040x44-cl22"][4] == ref.CL22 and 1040 == 65 * 16
    for name, w in (("64x200-cl22", 64), ("62x200-cl22", 62)):
        _, ww, h, n, (_, cfg) = by[name]
        assert (ww, h, n) == (w, 200, 1) and cfg == (2.0, 2, 2)
        ngroups = (w + rungs.K_INTERP_PX - 1) // rungs.K_INTERP_PX
        assert ngroups == 4 and rungs.K_THREADS // ngroups == 64
    assert 62 // 2 - 8 * 3 == 7                                   # the ragged group of 62 x 200: nd = 7, over every row


def rows_per_lane(w, h, tx, ty, cu, nf=1):
    """The rows every (band, sub-band, phase) of the LDS interpolation owns: interp_stage's bands and sub-bands and the bodies' row trim
    and first row (kernels/clahe.hip.h, kernels/packed422_bgra.hip.h) restated, the tile coordinate in float32 as the kernel has it."""
    plan = rungs.interp_plan(w, h, tx, ty, nf, cu)
    tile_h = g.clahe_tile(w, h, tx, ty)[1]
    inv_th = np.float32(1.0) / np.float32(tile_h)

    def ty1_of(y):
        return int(np.floor(np.float32(y) * inv_th - np.float32(0.5)))
    margin, out = rungs.K_BAND_MARGIN, []
    for band in range(ty + 1):
        lo = max(0, int((2 * band - 1) * tile_h / 2) - margin)                 # C++ division truncates toward zero
        hi = min(h, ((2 * band + 1) * tile_h + 1) // 2 + margin)
        nrows = max(0, hi - lo)
        for sub in range(plan.subs):
            y_lo, y_hi = lo + nrows * sub // plan.subs, lo + nrows * (sub + 1) // plan.subs
            a_lo, a_hi = y_lo, y_hi
            while a_lo < a_hi and ty1_of(a_lo) != band - 1:
                a_lo += 1
            while a_hi > a_lo and ty1_of(a_hi - 1) != band - 1:
                a_hi -= 1
            for phase in range(plan.phases):
                y0 = a_lo + (phase - (a_lo - y_lo) % plan.phases) % plan.phases
                out.append(len(range(y0, a_hi, plan.phases)))
    return plan, out


@pytest.mark.parametrize("cu", [64, 256, 304])
def test_which_row_loop_the_clahe_shapes_run(cu):
    """Every row is owned once.  64 x 200 and 62 x 200 at 2 x 2: 64 phases and sub-bands of about 8 rows, so a lane owns at most one
    row: the one-row loop alone (full groups in the first three column groups, the ragged branch in the fourth of 62 x 200).
    1040 x 44: 3 phases, and lanes that own two rows (the two-rows-in-flight loop, no tail) and three (that loop, then its tail)."""
    for w, h in ((64, 200), (62, 200)):
        plan, rows = rows_per_lane(w, h, 2, 2, cu)
        assert plan.kind == "float" and (plan.groups, plan.segs, plan.phases) == (4, 1, 64) and plan.subs >= 8
        assert sum(rows) == h and max(rows) == 1
    plan, rows = rows_per_lane(1040, 44, 2, 2, cu)
    assert (plan.groups, plan.segs, plan.phases, plan.subs) == (65, 1, 3, 3)
    assert sum(rows) == 44 and 2 in rows and 3 in rows


def test_rule_terms_of_the_gpu_test():
    """32 x 4, two frames: the control layout has every term a multiple of 16; +4 keeps a term a multiple of 4, +1 does not."""
    w, h = 32, 4
    pitch = 4 * w + 16
    fstride = pitch * h + 16
    assert pitch % 16 == 0 and fstride % 16 == 0
    for by, wide in ((4, True), (1, False)):
        assert ref.frame_wide(0x1000 + by, pitch, fstride) == wide
        assert ref.frame_wide(0x1000, pitch + by, fstride) == wide
        assert ref.frame_wide(0x1000, pitch, fstride + by) == wide
    # frames stay apart when only the frame stride moves, and rows when only the pitch does
    assert fstride + 1 >= pitch * h and pitch + 1 >= 4 * w


def test_list_offsets_of_the_gpu_test():
    """Images 0, 1, 4 and 16 bytes past a 16-byte boundary at a pitch that is a multiple of 4: three wide frames, one byte frame;
    130 frames at offsets 0 .. 4 in turn: 52 wide."""
    pitch = 4 * 40 + 16
    assert [ref.frame_wide(0x2000 + o, pitch) for o in (0, 1, 4, 16)] == [True, False, True, True]
    assert not any(ref.frame_wide(0x2000 + o, pitch + 1) for o in (0, 1, 4, 16))
    assert sum(ref.frame_wide(0x2000 + k % 5, 4 * 16 + 8) for k in range(130)) == 52
    p422 = (KERNELS / "packed422.hip.h").read_text()
    assert int(re.search(r"#define\s+MI_PACKED422_FRAMES_PER_LAUNCH\s+(\d+)", p422).group(1)) == 128 < 130
