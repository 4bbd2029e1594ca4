"""CPU checks behind tests/test_gpu_packed422_geometry.py: slots422 / slot422 of kernels/packed422.hip.h restated in Python partition
a row; the shapes of the GPU module's loop table loop by the bounds of its docstring alone; 16386 x 1 admits a band without rows; the
short-row layouts hold rows that end before their first 16-byte boundary; and the committed sweep seed gives the census the GPU module
asserts.  Nothing here needs a GPU or the library."""
import re
from pathlib import Path

import pytest

import packed422_geometry_cases as g

ROOT = Path(__file__).resolve().parents[1]
KERNELS = ROOT / "opencv-opencl_amd" / "csrc" / "kernels"


def test_restated_slot_arithmetic_is_the_headers():
    """The two expressions this module restates are still the header's, character for character (spaces aside)."""
    src = re.sub(r"\s+", "", (KERNELS / "packed422.hip.h").read_text())
    assert "intslots422(intdwords){return((dwords+3)>>2)+1;}" in src
    assert "constinthd=(int)(((16-((uintptr_t)row&15))&15)>>2);" in src
    assert "a=max(hd-4+4*k,0),b=min(hd+4*k,dwords);" in src
    assert "s.d0=a;s.n=max(b-a,0);" in src


def test_restated_planar_apply_walk_is_the_headers():
    """walk("lut_apply422_yuv420") takes lut_apply422_nv12's numbers: the planar writer's header still cuts row pairs into groups of
    eight macropixels and steps by kThreads items."""
    src = re.sub(r"\s+", "", (KERNELS / "packed422_yuv420.hip.h").read_text())
    body = src[src.index("voidlut_apply422_yuv420_body("): src.index("voidlut_apply422_yuv420_kernel(")]
    assert "constintG=(p.dwords+7)>>3;" in body
    assert "it+=kThreads" in body
    assert "pairs=p.rows>>1" in body
    assert "constintnd=min(8,p.dwords-8*grp);" in body
    for w, h in ((66, 386), (16386, 2), (62, 200)):
        assert g.walk("lut_apply422_yuv420", w, h) == g.walk("lut_apply422_nv12", w, h)


def test_tail_widths_give_every_tail_length():
    """33 .. 40 macropixels a row: the last group of a row holds 1, 2, ..., 8 of them, in that order."""
    assert [g.tail_dwords(w // 2) for w in g.TAIL_WIDTHS] == [1, 2, 3, 4, 5, 6, 7, 8]
    assert {min(8, w // 2 - 8 * (g.groups422(w // 2) - 1)) for w in g.TAIL_WIDTHS} == set(range(1, 9))
    kind, y_off, ye, ce, phases = g.TAIL_DST
    assert (y_off,) + phases == (4, 8, 12) and ye > 0 and ce > 0
    # the short rows: chroma rows of 1, 2 and 3 bytes at a pitch of 4 or 8, planes at 12 / 8 / 4
    for w in g.HEAD_WIDTHS:
        kind, y_off, ye, ce, phases = g.head_yuv420(w)
        assert (y_off,) + phases == (12, 8, 4) and ((w // 2 + 3) & ~3) + ce in (4, 8)
    assert {((w // 2 + 3) & ~3) + g.head_yuv420(w)[3] for w in g.HEAD_WIDTHS} == {4, 8}


@pytest.mark.parametrize("phase", g.PHASES)
def test_slots_partition_a_row(phase):
    """For every row phase and 1..40 dwords: the slots tile [0, dwords) once and in order, only the first and the last non-empty slot
    are ragged, and every full slot starts on a 16-byte boundary of the row it was cut for."""
    for base in (phase, phase + 4096):
        for dwords in range(1, 41):
            slots = [g.slot422(base, dwords, k) for k in range(g.slots422(dwords))]
            live = [(d0, n) for d0, n in slots if n]
            assert all(0 <= n <= 4 for _, n in slots)
            at = 0
            for d0, n in live:                                      # once and in order
                assert d0 == at, (phase, dwords, slots)
                at += n
            assert at == dwords, (phase, dwords, slots)
            idx = [k for k, (_, n) in enumerate(slots) if n]
            assert idx == list(range(idx[0], idx[0] + len(idx))), "an empty slot between two live ones"
            assert all(n == 4 for _, n in live[1:-1]), (phase, dwords, slots)
            assert all((base + 4 * d0) % 16 == 0 for d0, n in live if n == 4), (phase, dwords, slots)
            # one slot more would be empty: slots422 is enough
            assert g.slot422(base, dwords, g.slots422(dwords))[1] == 0
            # a row shorter than its head is one ragged slot
            if dwords < g.head422(base):
                assert live == [(0, dwords)]


def test_slot_cut_depends_on_the_row_it_is_cut_for():
    """What the phase matrix is for: the same dwords cut for a row at another phase give other slots."""
    assert [g.slot422(0, 20, k) for k in range(6)] != [g.slot422(4, 20, k) for k in range(6)]
    assert g.slot422(4, 20, 0) == (0, 3) and g.slot422(0, 20, 0) == (0, 0) and g.slot422(0, 20, 1) == (0, 4)


@pytest.mark.parametrize("shape", g.LOOP_SHAPES, ids=[s["id"] for s in g.LOOP_SHAPES])
def test_loop_shapes_loop(shape):
    """items per band > step for every walk a shape names, with B at its upper bound and in the smallest band that has rows."""
    for kernel in shape["walks"]:
        items, per, step, b = g.walk(kernel, shape["w"], shape["h"])
        assert items > step, (shape["id"], kernel, items, step, b)


def test_loop_table_says_what_its_comments_say():
    by = {s["id"]: s for s in g.LOOP_SHAPES}

    def w(name, kernel):
        return g.walk(kernel, by[name]["w"], by[name]["h"])
    assert w("64x200-tight", "lut_apply422") == (1800, 9, 1024, 1)
    assert w("66x200", "hist422_partial") == (2000, 10, 1024, 1)
    assert w("64x386-two-frames", "lut_apply422") == (128 * 9, 9, 1024, 3)
    assert w("4098x3", "lut_apply422") == (1542, 514, 1024, 1) and 256 // 514 == 0             # drow == 0
    assert w("16386x1", "lut_apply422") == (2050, 2050, 1024, 2)
    assert w("16386x2-nv12", "lut_apply422_nv12") == (1025, 1025, 256, 4)
    assert w("16386x2-nv12", "hist422_partial") == (2050, 2050, 1024, 2)
    assert w("64x200-nv12", "lut_apply422_nv12") == (400, 4, 256, 1)
    assert w("62x200-nv12", "lut_apply422_nv12") == (400, 4, 256, 1) and 31 - 8 * 3 == 7
    assert w("66x200-nv12", "lut_apply422_nv12") == (500, 5, 256, 1) and 33 - 8 * 4 == 1
    assert w("66x386-bgr", "lut_apply422_bgr") == (640, 5, 256, 3)
    assert w("66x386-yuv420", "lut_apply422_yuv420") == (320, 5, 256, 3) and 193 * 1 // 3 == 64 and 256 // 5 == 51 and 256 % 5 == 1
    assert w("66x386-yuv420", "hist422_partial") == (1280, 10, 1024, 3)
    assert by["66x386-yuv420"]["n"] == 2 and by["66x386-yuv420"]["sl"][1] == 4               # frames 4 bytes apart
    assert w("16386x2-yuv420", "lut_apply422_yuv420") == (1025, 1025, 256, 4)
    assert w("16386x2-yuv420", "hist422_partial") == (2050, 2050, 1024, 2)
    sl, dl = by["16386x2-yuv420"]["sl"], by["16386x2-yuv420"]["dl"]
    assert len({sl[2], dl[1]} | set(dl[4])) == 4                                             # source, Y, U and V at four phases
    # both forms and the packed walks with drow == 0 and drow > 0 are there
    assert {s["form"] for s in g.LOOP_SHAPES} == set(g.FORMS)


def test_one_row_frame_admits_a_band_without_rows():
    assert g.bands_bound(16386, 1, 1) == 2                       # rows == 1 does not cap B
    bands = [(1 * k // 2, 1 * (k + 1) // 2) for k in range(2)]
    assert bands == [(0, 0), (0, 1)]                             # r0 == r1 in the first workgroup
    assert g.bands_bound(16386, 2, 1) == 4 and g.bands_bound(16386, 2, 2) == 2
    assert g.bands_bound(16384, 1, 1) == 2 and g.bands_bound(16382, 1, 1) == 1


@pytest.mark.parametrize("shape", g.TILE_SHAPES, ids=[s["id"] for s in g.TILE_SHAPES])
def test_tile_shapes(shape):
    """A second step of tile_hist422_body needs more than 2048 items.  64 x 200 and 66 x 200 stay below (1800 and 2000: one step with
    a partly live fourth load), which is why the table also holds the same widths at 232 rows."""
    items, per, step, b = g.walk("tile_hist422", shape["w"], shape["h"], shape["grid"])
    assert step == 2048 and b == 1
    assert (items > step) == shape["loops"], (shape["id"], items)
    if not shape["loops"] and shape["grid"] == (1, 1):
        assert 3 * 512 < items <= step                           # the fourth load of the only step is live in some lanes, not in all
    if shape["id"] == "62x200-3x1":
        tw, th = g.clahe_tile(62, 200, 3, 1)
        assert (tw, th) == (21, 201) and 3 * tw - 62 == 1        # odd tile starts, one reflected column, one reflected row


@pytest.mark.parametrize("w", g.HEAD_WIDTHS)
def test_short_rows(w):
    """The phase changes from every row to the next on at least one side (W = 2: the destination pitch is 16; W = 6: the source pitch
    is; W = 4: both change), so source and destination phases differ by more than one amount; for W = 2 and 4 some rows on either side
    lie wholly before their first 16-byte boundary (a row of three dwords never does: a head is at most three dwords)."""
    sides = [g.row_addresses(w, g.HEAD_H, g.HEAD_N, layout) for layout in (g.HEAD_SRC, g.HEAD_DST)]
    steps = [all(rows[k] % 16 != rows[k + 1] % 16 for k in range(g.HEAD_H - 1)) for rows in sides]
    assert any(steps) and (all(steps) or w != 4), (w, steps)
    assert len({(s - d) % 16 for s, d in zip(*sides)}) >= 2
    for rows in sides:
        assert all(a % 4 == 0 for a in rows)
        short = [a for a in rows if w // 2 < g.head422(a)]
        assert bool(short) == (w < 6), (w, short)


def test_phase_matrix_pitches_advance_differently():
    src = g.row_addresses(g.PHASE_W, g.PHASE_H, g.PHASE_N, (g.PHASE_SRC["extra"], g.PHASE_SRC["gap"], 0))
    dst = g.row_addresses(g.PHASE_W, g.PHASE_H, g.PHASE_N, (g.PHASE_DST["extra"], g.PHASE_DST["gap"], 0))
    diff = {(s - d) % 16 for s, d in zip(src, dst)}
    assert diff == {0, 4, 8, 12}                                 # every relative phase, at every pair of base offsets
    assert g.PHASE_W // 2 == 20 and g.groups422(20) == 3 and 20 - 16 == 4


def test_sweep_census_holds_for_the_committed_seed():
    for form in g.FORMS:
        cases = g.sweep_cases(form)
        assert g.census_holds(cases), (form, {k: v[0] for k, v in g.census(cases).items()})
        cen = g.census(cases)
        assert all(cen[k][0] >= 6 for k in g.CLASSES[:4]) and 1 <= cen[g.CLASSES[4]][0] <= 4
        for c in cases:
            assert c["w"] % 2 == 0 and 2 <= c["w"] <= 160 and 1 <= c["h"] <= 48 and 1 <= c["n"] <= 3
            assert form not in ("nv12", "yuv420") or c["h"] % 2 == 0
            assert all(v % 4 == 0 for v in c["sl"] + c["dl"])
        assert sum(c["w"] % 16 == 0 for c in cases) >= 16 and sum(c["w"] % 4 == 2 for c in cases) >= 8
    # every form draws the same numbers
    a, b = g.sweep_cases("packed"), g.sweep_cases("bgr")
    assert [(c["w"], c["h"], c["sl"], c["dl"]) for c in a] == [(c["w"], c["h"], c["sl"], c["dl"]) for c in b]
    assert g.sweep_cases("packed") == g.sweep_cases("packed")


def test_sweep_yuv420_draws_what_the_other_forms_draw():
    """The planar 4:2:0 form adds no draw: its cases have the widths and layouts of `packed`, the heights of `nv12`, hence the census
    of both; its chroma planes come from the four numbers every form draws last, and all of them are multiples of 4."""
    y, p, n = g.sweep_cases("yuv420"), g.sweep_cases("packed"), g.sweep_cases("nv12")
    assert [(c["w"], c["sl"], c["dl"]) for c in y] == [(c["w"], c["sl"], c["dl"]) for c in p]
    assert [c["h"] for c in y] == [c["h"] for c in n]
    keys = ("n", "kind", "tx", "ty", "clip", "fmt", "uv")
    assert [[c[k] for k in keys] for c in y] == [[c[k] for k in keys] for c in p]
    assert [(c["c_extra"], c["u_phase"], c["c_own"]) for c in y] == [(c["uv_extra"], c["uv_phase"], c["uv_own"]) for c in n]
    assert [c["yv12"] for c in y] == [c["byte"] for c in g.sweep_cases("bgr")]
    assert [g.census(y)[k][0] for k in g.CLASSES] == [7, 17, 14, 7, 3] == [g.census(p)[k][0] for k in g.CLASSES]
    kinds = set()
    for c in y:
        kind, y_off, ye, ce, (pa, pb) = g.yuv420_layout(c)
        kinds.add(kind)
        c_pitch = ((c["w"] // 2 + 3) & ~3) + ce
        assert c_pitch % 4 == 0 and c_pitch >= c["w"] // 2 and all(v % 4 == 0 and 0 <= v < 16 for v in (pa, pb)) and y_off % 4 == 0 and ye % 4 == 0
        assert (pa - pb) % 16 in (4, 12)                         # V = U + 4 or U - 4 modulo 16: never the same phase
        u = pb if kind == "yv12" else pa
        assert u == c["u_phase"]
    assert kinds == {"one", "yv12", "own"}
