"""Shapes and cases of tests/test_gpu_packed422_geometry.py, and the arithmetic they rest on, in plain Python: no GPU, no torch.
tests/test_packed422_geometry_shapes.py asserts on the CPU that the shapes do what their comments say; the GPU module runs them.

The walks of kernels/packed422*.hip.h restated (W even, dwords = W / 2 macropixels a row):
  slots422 / slot422      a row is cut into S = ((dwords + 3) >> 2) + 1 slots at the 16-byte boundaries of the row it is cut FOR
  hist422_partial         band of rows, (row, slot) items, 256 lanes, four loads in flight: a step is 4 * 256 items
  lut_apply422            the same walk cut at the destination row, a step is 4 * 256 items
  lut_apply422_nv12       band of row PAIRS, (pair, group) items with G = (dwords + 7) >> 3 groups of 16 columns, a step is 256 items
  lut_apply422_bgr        band of rows, (row, group) items with the same G, a step is 256 items
  lut_apply422_yuv420     (kernels/packed422_yuv420.hip.h) lut_apply422_nv12's arithmetic: row pairs, the same G, a step is 256 items
  tile_hist422            one tile per workgroup (512 lanes), (row, slot) items over the tile's dwords, a step is 4 * 512 items
A band is rows [units * b / B, units * (b + 1) / B); B <= max(1, floor(2*W*H / 16384)) and, when units > 1, B <= units."""
import numpy as np

FMT_YUY2, FMT_UYVY = 2, 3
UV_FILL128, UV_COPY = 0, 1
FORMS = ("packed", "nv12", "bgr", "yuv420")
EQ = ("eq", None)


# ---- the kernels' arithmetic -----------------------------------------------------------------------------------------------------
def head422(addr):
    """Dwords of a row at `addr` that lie before its first 16-byte boundary (slot422's hd)."""
    return ((16 - (addr & 15)) & 15) >> 2


def slots422(dwords):
    return ((dwords + 3) >> 2) + 1


def slot422(addr, dwords, k):
    """(d0, n) of slot k of a row of `dwords` dwords at byte address `addr`."""
    hd = head422(addr)
    a, b = max(hd - 4 + 4 * k, 0), min(hd + 4 * k, dwords)
    return a, max(b - a, 0)


def groups422(dwords):
    return (dwords + 7) >> 3


def bands_bound(w, h, units):
    """The largest B blocks_per_frame can return for a W x H packed frame cut into `units` rows or row pairs."""
    b = max(1, 2 * w * h // 16384)
    return min(b, units) if units > 1 else b


def smallest_band(units, b):
    """Units of the smallest band that has any (units == 1 with B > 1 leaves bands without rows)."""
    return min(x for x in (units * (k + 1) // b - units * k // b for k in range(b)) if x)


def clahe_tile(w, h, tx, ty):
    """(tile_w, tile_h) of clahe_geometry: both axes pad when either is indivisible."""
    if w % tx or h % ty:
        return (w + tx - w % tx) // tx, (h + ty - h % ty) // ty
    return w // tx, h // ty


def walk(kernel, w, h, grid=None):
    """(items in the smallest non-empty band with B at its upper bound, items per unit, step, B bound) of one kernel's walk.
    tile_hist422: the row split of launch_tile_luts422 is taken to be 1 (it is for every tile below 65536 pixels), the tile is tile
    (0, 0), and its rows are those of the padded tile."""
    dwords = w // 2
    if kernel in ("hist422_partial", "lut_apply422"):
        units, per, step = h, slots422(dwords), 4 * 256
    elif kernel in ("lut_apply422_nv12", "lut_apply422_yuv420"):
        units, per, step = h // 2, groups422(dwords), 256
    elif kernel == "lut_apply422_bgr":
        units, per, step = h, groups422(dwords), 256
    elif kernel == "tile_hist422":
        tw, th = clahe_tile(w, h, *grid)
        assert tw * th < 65536
        return th * slots422((min(tw, w) + 1) >> 1), slots422((min(tw, w) + 1) >> 1), 4 * 512, 1
    else:
        raise ValueError(kernel)
    b = bands_bound(w, h, units)
    return smallest_band(units, b) * per, per, step, b


# ---- group 1: phase matrix -------------------------------------------------------------------------------------------------------
PHASES = (0, 4, 8, 12)
PHASE_W, PHASE_H, PHASE_N = 40, 6, 2            # 20 dwords: two full 16-column groups and a ragged one of 8 columns
PHASE_SRC = dict(extra=4, gap=4)                # pitch 2W + 4: the source phase advances by 4 a row
PHASE_DST = dict(extra=8, gap=12)               # pitch 2W + 8: the destination phase advances by 8 a row
PHASE_OPS = (EQ, ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 64, 2)))      # LUT apply; LDS interpolation; the wide-grid kernel
BGR_BASES = (0, 1, 4, 16)
# planar 4:2:0 out: y_pitch W + 4 = 44 (the Y phase advances by 12 a row), c_pitch W / 2 + 4 = 24 (the chroma phases advance by 8)
PHASE_YUV420 = dict(ye=4, ce=4)

# every length of the ragged chroma tail: 33 .. 40 macropixels a row, so the last group of a row holds 1, 2, ..., 8
TAIL_WIDTHS = (66, 68, 70, 72, 74, 76, 78, 80)
TAIL_H, TAIL_N = 4, 2
TAIL_OPS = (EQ, ("clahe", (2.0, 2, 2)), ("clahe", (2.0, 64, 2)))
TAIL_DST = ("one", 4, 4, 4, (8, 12))            # a planar layout (below): Y / U / V at phases 4 / 8 / 12, padded pitches


def tail_dwords(dwords):
    """Macropixels in the last group of a row: the nd of the writers' last (pair, group) item."""
    return min(8, dwords - 8 * (groups422(dwords) - 1))


# ---- group 2: walks past their first step ----------------------------------------------------------------------------------------
# (extra, gap, off) as the Batch class of the packed-in test modules takes them; a planar 4:2:0 destination is
# (kind, y_off, y_pitch - align4(W), c_pitch - align4(W / 2), (phase of the first chroma plane, of the second)) as
# test_gpu_packed422_to_yuv420.PlanarOut takes them
TIGHT, P4 = (0, 0, 0), (4, 0, 4)
CL22 = ("clahe", (2.0, 2, 2))
LOOP_SHAPES = [
    # id, form, W, H, n, source layout, destination layout (packed out; the other forms build theirs from it), ops, the walks that repeat
    # B = 1; S = 9, drow 28, dslot 4: 1800 items, one full step, then 776 items: loads 0..2 full, the fourth live in lanes 0..7 only
    dict(id="64x200-tight", form="packed", w=64, h=200, n=1, sl=TIGHT, dl=TIGHT, ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422")),
    # the same walk with every row at another phase: source rows step by 4 from 4, destination rows likewise; src and dst differ
    dict(id="64x200-pitch+4", form="packed", w=64, h=200, n=1, sl=P4, dl=(4, 0, 12), ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422")),
    # B = 1; 33 dwords, S = 10, drow 25, dslot 6: 2000 items, two steps; a row at phase 0 has slots of 4 x 8 + 1, its last slot is ragged
    dict(id="66x200", form="packed", w=66, h=200, n=1, sl=TIGHT, dl=(8, 0, 4), ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422")),
    # 2WH / 16384 = 3.01: up to three bands of 128 / 129 / 129 rows, S = 9: 1152 / 1161 / 1161 items, two steps each; frame 2 is 4 bytes
    # past the end of frame 1, so its phase differs
    dict(id="64x386-two-frames", form="packed", w=64, h=386, n=2, sl=(0, 4, 0), dl=(0, 4, 8), ops=(EQ, CL22),
         walks=("hist422_partial", "lut_apply422")),
    # B = 1; S = 514 > 256: drow 0, dslot 256, 1542 items: a lane walks along one row and wraps into the next, two steps
    dict(id="4098x3", form="packed", w=4098, h=3, n=1, sl=(4, 0, 4), dl=(12, 0, 8), ops=(EQ, ("clahe", (2.0, 2, 1))),
         walks=("hist422_partial", "lut_apply422")),
    # 32772 bytes in one row: B may be 2, and then band 0 has no rows (it publishes an all-zero partial and writes nothing); S = 2050,
    # drow 0, dslot 256: 2050 items, three steps, the third of two items
    dict(id="16386x1", form="packed", w=16386, h=1, n=1, sl=TIGHT, dl=(0, 0, 4), ops=(EQ,), walks=("hist422_partial", "lut_apply422")),
    # one row pair: the apply grid may have four bands, three of them without a pair; G = 1025, dpr 0, dgrp 256: five steps.  The
    # histogram has two bands of one row, 2050 items each
    dict(id="16386x2-nv12", form="nv12", w=16386, h=2, n=1, sl=TIGHT, dl=TIGHT, ops=(EQ, ("clahe", (2.0, 2, 1))),
         walks=("hist422_partial", "lut_apply422_nv12")),
    # B = 1, 100 pairs; G = 4, dpr 64, dgrp 0: 400 items, two steps of 256
    dict(id="64x200-nv12", form="nv12", w=64, h=200, n=1, sl=P4, dl=TIGHT, ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422_nv12")),
    # 31 dwords: G = 4, the last group ragged with 7 dwords: 14 bytes a plane row, three dwords and a 2-byte tail store
    dict(id="62x200-nv12", form="nv12", w=62, h=200, n=1, sl=P4, dl=TIGHT, ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422_nv12")),
    # 33 dwords: G = 5, dpr 51, dgrp 1: 500 items; the last group holds one dword, a single 2-byte store
    dict(id="66x200-nv12", form="nv12", w=66, h=200, n=1, sl=P4, dl=TIGHT, ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422_nv12")),
    # lut_apply422_bgr steps by 256 (row, group) items.  2WH / 16384 = 3.1: up to three bands of 128 / 129 / 129 rows; G = 5, drow 51,
    # dgrp 1: 640 / 645 / 645 items, three steps each, and the group wraps into the next row; two frames
    dict(id="66x386-bgr", form="bgr", w=66, h=386, n=2, sl=(4, 4, 4), dl=TIGHT, ops=(EQ, CL22), walks=("hist422_partial", "lut_apply422_bgr")),
    # lut_apply422_yuv420 steps by 256 (row pair, group) items.  193 row pairs in up to three bands of 64 / 64 / 65; G = 5, dpr 51,
    # dgrp 1: 320 / 320 / 325 items, two steps each, and the group wraps into the next pair; two frames 4 bytes apart
    dict(id="66x386-yuv420", form="yuv420", w=66, h=386, n=2, sl=(4, 4, 4), dl=("one", 4, 4, 4, (8, 12)), ops=(EQ, CL22),
         walks=("hist422_partial", "lut_apply422_yuv420")),
    # as 16386x2-nv12 -- one row pair, up to four apply bands, three of them without a pair; G = 1025, five steps -- with the source
    # and the three planes each at a phase of its own
    dict(id="16386x2-yuv420", form="yuv420", w=16386, h=2, n=1, sl=P4, dl=("one", 8, 4, 4, (12, 0)), ops=(EQ, ("clahe", (2.0, 2, 1))),
         walks=("hist422_partial", "lut_apply422_yuv420")),
]

# tile_hist422_body: CLAHE with a 1 x 1 grid, the largest tile a size allows.  The row split of launch_tile_luts422 is not observable; it
# is taken to be 1, which the host code gives every tile of fewer than 65536 pixels.  A step is 4 * 512 = 2048 items.
TILE_SHAPES = [
    # id, W, H, grid, second step
    # tile 64 x 200, 32 dwords, RS = 9: 1800 items -- ONE step, whose fourth load is live in lanes 0..263 only
    dict(id="64x200-1x1", w=64, h=200, grid=(1, 1), loops=False),
    # tile 66 x 200, 33 dwords, RS = 10: 2000 items -- one step, the fourth load live in lanes 0..463
    dict(id="66x200-1x1", w=66, h=200, grid=(1, 1), loops=False),
    # RS = 9, drow 56, dslot 8: 2088 items, a second step of 40 items
    dict(id="64x232-1x1", w=64, h=232, grid=(1, 1), loops=True),
    # RS = 10, drow 51, dslot 2: 2320 items, a second step of 272 items
    dict(id="66x232-1x1", w=66, h=232, grid=(1, 1), loops=True),
    # 62 x 200 at 3 x 1 pads to 63 x 201: tile_w 21, tiles start at columns 0, 21, 42.  Tile 0 ends and tile 1 starts inside dword 10
    # (odd_last / odd_first), tile 2 has 20 columns inside the frame and one reflected column; row 200 is reflected
    dict(id="62x200-3x1", w=62, h=200, grid=(3, 1), loops=False),
]


# ---- group 3: rows shorter than their head ---------------------------------------------------------------------------------------
HEAD_WIDTHS = (2, 4, 6)
HEAD_H, HEAD_N = 8, 3
HEAD_SRC = (4, 4, 4)           # pitch 2W + 4 at offset 4, frames 4 bytes apart
HEAD_DST = (12, 8, 12)         # pitch 2W + 12 at offset 12
HEAD_OPS = (EQ, ("clahe", (2.0, 1, 1)))


def head_yuv420(w):
    """Planar 4:2:0 out on the short rows: chroma rows of 1, 2 and 3 bytes (a byte; a 2-byte store; a 2-byte store and a byte) at a
    chroma pitch of 8, 4 and 8; Y / U / V at offsets 12 / 8 / 4."""
    return ("one", 12, 12, 4 * ((w // 2) & 1), (8, 4))


def row_addresses(w, h, n, layout):
    """Byte addresses (relative to a 16-byte aligned allocation) of every row of a batch in a (extra, gap, off) layout."""
    extra, gap, off = layout
    pitch = 2 * w + extra
    return [off + f * (pitch * h + gap) + r * pitch for f in range(n) for r in range(h)]


# ---- group 5: seeded sweep -------------------------------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 3, 48      # the smallest seed whose 48 cases meet census_holds for every form
REFUSED_GRID = (2048, 1024)            # more tiles than the planar form accepts
CLASSES = ("eq", "clahe-lds", "clahe-lds-ragged", "clahe-wide-grid", "refused-by-planar-form")


def draw_case(rng, form):
    """One case.  W even in [2, 160]: half of the cases force a multiple of 16, a quarter W % 4 == 2.  H in [1, 48] (rounded up to
    even for NV12 out), 1..3 frames, the op, a grid in [1, 16] x [1, 5] with tiles_x = 64 one time in eight (and, one time in sixteen,
    a grid the planar form refuses), a clip limit, the format, the UV mode (BGR out: the channel order), and two independent layouts:
    pitch paddings in 4 * [0, 10], offsets and gaps in 4 * [0, 7].  Every form draws the same numbers from the same seed.  Planar
    4:2:0 out rounds H up to even too, and takes its chroma planes from extra2, phase2, own and byte alone (yuv420_layout)."""
    w = 2 * int(rng.integers(1, 81))
    u = rng.random()
    if u < 0.5:
        w = 16 * int(rng.integers(1, 11))
    elif u < 0.75:
        w = 4 * int(rng.integers(0, 40)) + 2
    h = int(rng.integers(1, 49))
    if form in ("nv12", "yuv420"):
        h += h & 1
    n = int(rng.integers(1, 4))
    kind = "clahe" if rng.random() < 0.8 else "eq"
    tx, ty = int(rng.integers(1, 17)), int(rng.integers(1, 6))
    if rng.integers(0, 8) == 0:
        tx = 64
    if rng.integers(0, 16) == 0:
        tx, ty = REFUSED_GRID
    clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
    fmt, uv = int(rng.integers(2, 4)), int(rng.integers(0, 2))

    def m4(hi):
        return 4 * int(rng.integers(0, hi + 1))
    sl = (m4(10), m4(7), m4(7))
    dl = (m4(10), m4(7), m4(7))
    extra2, phase2, own, byte = m4(10), m4(3), bool(rng.integers(0, 2)), rng.integers(0, 4) == 0
    case = dict(form=form, w=w, h=h, n=n, kind=kind, tx=tx, ty=ty, clip=clip, fmt=fmt, uv=uv, sl=sl, dl=dl)
    if form == "nv12":          # the UV plane: its own pitch padding, its own phase, behind the Y plane or in its own allocation
        case.update(uv_extra=extra2, uv_phase=phase2, uv_own=own)
    if form == "bgr":           # one case in four moves the image to an odd base and an odd pitch: byte stores
        case.update(byte=bool(byte))
    if form == "yuv420":        # the chroma planes: their pitch padding, the U phase, one allocation or three, YV12 order
        case.update(c_extra=extra2, u_phase=phase2, c_own=own, yv12=bool(byte))
    return case


def yuv420_layout(case):
    """The planar destination of a yuv420 sweep case, as LOOP_SHAPES writes one: Y from dl (pitch padding and offset), the chroma
    pitch padded by c_extra, U at u_phase, V four bytes on (modulo 16) or, when c_extra is an odd multiple of 4, four bytes back; the
    planes in three allocations (c_own), or in one, where yv12 puts V's address below U's."""
    u = case["u_phase"]
    v = (u + (4 if (case["c_extra"] >> 2) & 1 == 0 else 12)) % 16
    kind = "own" if case["c_own"] else ("yv12" if case["yv12"] else "one")
    return (kind, case["dl"][2], case["dl"][0], case["c_extra"], (v, u) if kind == "yv12" else (u, v))


def sweep_cases(form, seed=SWEEP_SEED):
    rng = np.random.default_rng(seed)
    return [draw_case(rng, form) for _ in range(SWEEP_CASES)]


def op_of(case):
    return EQ if case["kind"] == "eq" else ("clahe", (case["clip"], case["tx"], case["ty"]))


def classify(case):
    """The header's rules restated: equalizeHist takes the LUT-apply kernel; a CLAHE grid of more than 65535 tiles is refused as
    the planar form refuses it; tiles_x > 62 takes the wide-grid kernel (one macropixel a thread, LUTs from global memory); every other
    grid the LDS interpolation, whose last group of a row is ragged when W is no multiple of 16."""
    if case["kind"] == "eq":
        return "eq"
    if case["tx"] * case["ty"] > 65535:
        return "refused-by-planar-form"
    if case["tx"] > 62:
        return "clahe-wide-grid"
    return "clahe-lds" if case["w"] % 16 == 0 else "clahe-lds-ragged"


def census(cases):
    """class -> (count, formats seen, UV modes / orders seen)"""
    out = {k: [0, set(), set()] for k in CLASSES}
    for c in cases:
        e = out[classify(c)]
        e[0] += 1
        e[1].add(c["fmt"])
        e[2].add(c["uv"])
    return out


def census_holds(cases):
    cen = census(cases)
    if len(cases) != SWEEP_CASES:
        return False
    for k, (count, fmts, uvs) in cen.items():
        if k == "refused-by-planar-form":
            if not 1 <= count <= 4:
                return False
        elif count < 6:
            return False
        if fmts != {FMT_YUY2, FMT_UYVY} or uvs != {0, 1}:
            return False
    return True
