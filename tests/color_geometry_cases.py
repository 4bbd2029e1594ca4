"""Shapes and cases of tests/test_gpu_color_geometry.py, and the host arithmetic they rest on, in plain Python: no GPU, no torch.
tests/test_color_geometry_shapes.py asserts on the CPU, for every CU count from 64 to 1024, that each case reaches what it records; the
GPU module runs the cases after asserting that its device's CU count lies in that range.

Restated from host/color.inc.hpp and host/context.inc.hpp (cu = the device's CU count, n = frames of the launch):
  blocks_per_frame(bytes, rows, n, cap)   min(ceil(8 cu / n), max(1, bytes / 16384), rows if rows > 1, cap), at least 1
  one-pass BGR CLAHE (bgr_luma_dev)       shape_ok; S row slices of a tile; `subs` sub-bands, `groups` lanes a row, `segs` column
                                          segments and `phases` rows in flight of bgr_clahe_interp_kernel
  launch_color                            bx workgroups a row of color_kernel, rows flattened to one when both pitches are 3 W
  cvt420_dev                              bx workgroups a frame of cvt420_kernel
and from the kernels (kernels/color.hip.h, kernels/color_clahe.hip.h) the walks the cases are chosen by:
  bgr_tile_hist_kernel<512>   (row, slot) items of a slice, slots = tile_w / 16, two items in flight: a step is 2 * 512 items; the walk is
                              carried by row += drow, slot += dslot with drow = 512 / slots, dslot = 512 % slots and a wrap
  bgr_luma_hist / apply       16-pixel groups of the flattened frame, a step is 512 B groups; the ragged tail and unaligned frames go a
                              pixel a lane
  nv12_bgr_hist / apply       16 x 2 groups (vector) or 2 x 2 blocks (byte), a step is 512 B items; the vector walk is carried by
                              by += dby, gx += dgx with a wrap
  cvt420_kernel<0/1>          the same two bodies with 256 lanes
  color_kernel<0/1>           rows by gridDim.y, 16-pixel groups by 256 bx lanes, the tail and unaligned rows a pixel a lane

WHERE EACH PROPERTY IS REACHED (the tables below say it again, case by case, as `reach`):
  second item in flight (`two`) in some lanes only   a: 1072x8-1x1 (24 lanes), 1040x16-1x1 (8 lanes of either slice)
  tile-histogram steps 1 / 2 / 3 / 5                 a: 1072x8-1x1 / 2096x8-1x1 / 4128x16-1x2 / 8208x8-1x1
  a last step with `two` false                       a: 2096x8-1x1 (24 lanes), 4128x16-1x2 (16), 8208x8-1x1 (8)
  the (row, slot) wrap before a live item            a: 2096x8-1x1 (drow 3, dslot 119), 4128x16-1x2, 8208x8-1x1; the second items of
                                                     1072x8-1x1 and 1040x16-1x1 lie in lanes that do not wrap, 64x44-2x1 has dslot 0
  drow = 0 (more slots than lanes)                   a: 8208x8-1x1 (513 slots, dslot 512)
  uneven slices                                      a: 64x44-2x1 (S = 5: 8, 9, 9, 9, 9 rows)
  the LUT written directly (S = 1)                   a: 1072x8, 2096x8, 4128x16, 8208x8;  b: 80x21, 224x12
  partials and tile_lut_kernel (S > 1)               a: 1040x16-1x1 (S = 2), 64x44-2x1 (S = 5);  b: 64x32-2x1 (S = 4)
  segs = 2 / segs = 3                                a: 4128x16-1x2 (second segment of two groups) / 8208x8-1x1 (third of one group)
  phases = 1 with idle lanes                         a: 2096x8-1x1 (131 groups: lanes 131..255 idle)
  phases > 1 with an idle lane                       b: 80x21-5x3 (5 groups, 51 phases, lane 255 idle), odd band edges (tile_h 7)
  the 15-pair table, 60 KiB of LDS                   b: 224x12-14x2
  planes because of the pair table                   b: 240x12-15x2
  planes because tile_w % 16 != 0                    b: 72x12-3x2
  planes because of clahe_fp_contract                b: 64x32-2x4-contract
  planes because of REFLECT_101 padding              b: 64x30-2x4
  planes because of alignment                        b: 64x32-2x4-base+4
  fused equalizeHist, a second step in some lanes    c: 112x96 (160 lanes), 50x218 (169 lanes)
  the ragged tail                                    c: 50x218 (4 pixels)
  the empty partial                                  c: 128x128 (B = 3, the third workgroup starts at group 1024 of 1024)
  the byte body of the fused kernels                 c: 50x218-base+1 (22 steps)
  NV12 vector walk, second step, wrap                d: 112x160 (48 lanes, dgx 1, wrap at gx 6), 144x144 (136 lanes, dgx 8)
  NV12 byte walk                                     d: 66x34 (two steps), 96x144-base+1 (seven steps)
  one workgroup a frame: cvt420 vector / byte        e: 96x96 (288 groups, dby 42, dgx 4, 32 lanes step twice) / 66x34 (three steps)
  mixed vector and byte frames of color_kernel       e: 67x63 (frame k is aligned iff k % 16 == 0: 263 groups on 256 lanes and a
                                                     13-pixel tail; every other frame 17 byte steps)
  the second row step of color_kernel                f: 16x65540 (rows 65535..65539)"""

import functools

# ---- constants of the headers (tests/test_color_geometry_shapes.py parses the headers and compares) ------------------------------
K_THREADS = 256                 # kernels/common.hip.h kThreads
K_MAX_PAIRS_LDS_F32 = 15        # kernels/clahe.hip.h
K_INTERP_PX = 16                # kernels/clahe.hip.h
K_BAND_MARGIN = 4               # kernels/clahe.hip.h
K_BGR_THREADS = 512             # kernels/color.hip.h
K_NV12_THREADS = 512            # kernels/color.hip.h
K_MAX_GRID_Y = 65535            # host/context.inc.hpp
TILE_NT = 512                   # host/color.inc.hpp launches bgr_tile_hist_kernel<512>
CU_MIN, CU_MAX = 64, 1024       # the CU counts the tables are checked for
FRAMES_PER_CU = 8               # group e: n = 8 * cu_count frames makes every grid one workgroup a frame

OP_EQUALIZE, OP_CLAHE = 0, 1
COLOR_BGR2YUV, COLOR_YUV2BGR, COLOR_YUV2BGR_NV12, COLOR_BGR2YUV_I420 = 82, 84, 93, 128


def ceil_div(a, b):
    return (a + b - 1) // b


def c_div(a, b):
    """C's integer division: it truncates towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- host formulas ---------------------------------------------------------------------------------------------------------------
def blocks_per_frame(cu, bytes_per_frame, rows, n, cap):
    b = min(ceil_div(cu * 8, n), max(1, bytes_per_frame // 16384))
    if rows > 1:
        b = min(b, rows)
    return max(1, min(b, cap))


def clahe_tile(w, h, tx, ty):
    """(tile_w, tile_h) of clahe_geometry: both axes pad when either is indivisible."""
    if w % tx or h % ty:
        return (w + tx - w % tx) // tx, (h + ty - h % ty) // ty
    return w // tx, h // ty


def shape_ok(w, h, tx, ty, contract=False, aligned=True):
    """bgr_luma_dev's shape_ok, term by term: None when the one-pass kernels run, else the first term that sends the call through the
    planes.  `aligned`: both bases, both pitches and both frame strides are multiples of 16."""
    tile_w, _ = clahe_tile(w, h, tx, ty)
    if contract:
        return "contract"
    if w % tx or h % ty:
        return "padding"
    if tile_w % 16:
        return "tile_w"
    if tx + 1 > K_MAX_PAIRS_LDS_F32:
        return "pairs"
    if tx * ty > K_MAX_GRID_Y:
        return "tiles"
    if w // K_INTERP_PX > K_THREADS * K_MAX_GRID_Y:
        return "width"
    if not aligned:
        return "alignment"
    return None


@functools.lru_cache(maxsize=None)
def carried_walk(first_lanes, stride, per_row, total):
    """The incremental (row, column) walk all these kernels use, lane by lane as they write it:
        row = i / per_row, col = i % per_row;  loop: [wrap: col >= per_row -> col -= per_row, ++row]  body  i += stride, row += drow, col += dcol
    Returns (steps of the longest lane, lanes in that last step, wraps fired in live items, walk_is_divmod)."""
    drow, dcol = stride // per_row, stride % per_row
    steps = last = wraps = 0
    ok = True
    for t in range(first_lanes[0], first_lanes[1]):
        i, row, col, k = t, t // per_row, t % per_row, 0
        while i < total:
            if col >= per_row:
                col -= per_row
                row += 1
                wraps += 1
            ok = ok and (row, col) == divmod(i, per_row)
            k += 1
            i, row, col = i + stride, row + drow, col + dcol
        if k > steps:
            steps, last = k, 1
        elif k == steps and k:
            last += 1
    return steps, last, wraps, ok


@functools.lru_cache(maxsize=None)
def tile_hist_walk(items, slots, nt=TILE_NT):
    """bgr_tile_hist_kernel's loop over one slice: item_ptr() is called twice a step whether or not the second item is live, and wraps
    after the increment.  Returns dict(steps, last_lanes: lanes in the last step, last_two: those of them whose second item is live,
    two_some: some step has `two` true in some lanes and false in others, wraps: wraps whose position a live item then uses, ok: every
    live item is divmod(it, slots))."""
    drow, dslot = nt // slots, nt % slots
    steps = ceil_div(items, 2 * nt)
    last_lanes = last_two = wraps = 0
    ok, two_some = True, False
    for k in range(steps):
        twos = 0
        lanes = 0
        for t in range(nt):
            it = t + 2 * nt * k
            if it >= items:
                continue
            lanes += 1
            twos += it + nt < items
        two_some = two_some or 0 < twos < lanes
        if k == steps - 1:
            last_lanes, last_two = lanes, twos
    for t in range(min(nt, items)):
        row, slot = t // slots, t % slots
        it = t
        while it < items:
            for live in (True, it + nt < items):                   # p0, then p1
                if live:
                    ok = ok and (row, slot) == divmod(it, slots)
                row, slot = row + drow, slot + dslot
                if slot >= slots:
                    slot -= slots
                    row += 1
                    wraps += it + nt < items                         # the wrapped position is that of this lane's next item
                it += nt
    return dict(steps=steps, last_lanes=last_lanes, last_two=last_two, two_some=two_some, wraps=wraps, ok=ok, drow=drow, dslot=dslot)      # read, never changed


def onepass_plan(cu, w, h, tx, ty, n):
    """The launch geometry of the one-pass BGR CLAHE for a batch of n (<= 65535) frames."""
    tile_w, tile_h = clahe_tile(w, h, tx, ty)
    tiles = tx * ty
    want = ceil_div(cu * 8, tiles * n)
    s = max(1, min(want, max(1, tile_h // 8), 64))
    slices = [tile_h * (k + 1) // s - tile_h * k // s for k in range(s)]
    slots = tile_w // 16
    ngroups = w // K_INTERP_PX
    groups = min(ngroups, K_THREADS)
    segs = ceil_div(ngroups, groups)
    bands = ty + 1
    want = ceil_div(cu * 8, bands * n * segs)
    subs = max(1, min(want, max(1, (tile_h + 2 * K_BAND_MARGIN) // 8), 64))
    phases = K_THREADS // groups
    band_rows = []
    for band in range(bands):
        lo = max(0, c_div((2 * band - 1) * tile_h, 2) - K_BAND_MARGIN)
        hi = min(h, c_div((2 * band + 1) * tile_h + 1, 2) + K_BAND_MARGIN)
        band_rows.append(max(0, hi - lo))
    return dict(S=s, slices=slices, slots=slots, items=[r * slots for r in slices], groups=groups, segs=segs,
                last_seg_groups=ngroups - (segs - 1) * groups, phases=phases, idle_lanes=K_THREADS - phases * groups, subs=subs,
                bands=bands, band_rows=band_rows, lds_bytes=(tx + 1) * 256 * 16, tile_lut=s > 1)


def color_job_rows(w, h, src_pitch, dst_pitch):
    """(rows, row_px) of color_job(): one row of W * H pixels when both pitches are 3 W (or H == 1)."""
    if (src_pitch == 3 * w and dst_pitch == 3 * w) or h == 1:
        return 1, w * h
    return h, w


def color_bx(cu, rows, row_px, n):
    """(gy, bx) of launch_color."""
    gy = min(rows, 65535)
    bx = ceil_div(cu * 8, gy * n)
    return gy, max(1, min(bx, (row_px // 16 + K_THREADS - 1) // K_THREADS + 1))


def cvt420_bx(cu, w, h, n, vec):
    blocks = (w // 2) * (h // 2)
    bx = max(1, min(ceil_div(cu * 8, n), ceil_div(blocks, K_THREADS)))
    if vec:
        bx = max(1, min(bx, ceil_div(blocks // 8, K_THREADS)))
    return bx


def flat_walk(total, lanes):
    """A plain grid-stride loop of `lanes` lanes over `total` items: (steps, lanes in the last step)."""
    steps = ceil_div(total, lanes)
    return steps, (total - (steps - 1) * lanes if steps else 0)


# ---- a. bgr_tile_hist_kernel<512>: items, steps and slices -----------------------------------------------------------------------
# OP_CLAHE, clip 2.0, aligned tight layout (pitch 3 W, frames H * 3 W apart, everything a multiple of 16), two frames, out of place and
# in place.  reach: S, the slice heights, slots, items a slice, steps of the tile-histogram loop, lanes of the last step and how many of
# them have a live second item, drow / dslot, segs, groups of the last segment, phases, idle lanes of the interpolation, subs
A_N = 2
A_CLIP = 2.0
TILE_HIST_SHAPES = [
    dict(id="1072x8-1x1", w=1072, h=8, tx=1, ty=1,
         reach=dict(S=1, slices=[8], slots=67, items=[536], steps=1, last_lanes=512, last_two=24, drow=7, dslot=43, segs=1,
                    last_seg_groups=67, phases=3, idle_lanes=55, subs=2)),
    dict(id="1040x16-1x1", w=1040, h=16, tx=1, ty=1,
         reach=dict(S=2, slices=[8, 8], slots=65, items=[520, 520], steps=1, last_lanes=512, last_two=8, drow=7, dslot=57, segs=1,
                    last_seg_groups=65, phases=3, idle_lanes=61, subs=3)),
    dict(id="2096x8-1x1", w=2096, h=8, tx=1, ty=1,
         reach=dict(S=1, slices=[8], slots=131, items=[1048], steps=2, last_lanes=24, last_two=0, drow=3, dslot=119, segs=1,
                    last_seg_groups=131, phases=1, idle_lanes=125, subs=2)),
    dict(id="4128x16-1x2", w=4128, h=16, tx=1, ty=2,
         reach=dict(S=1, slices=[8], slots=258, items=[2064], steps=3, last_lanes=16, last_two=0, drow=1, dslot=254, segs=2,
                    last_seg_groups=2, phases=1, idle_lanes=0, subs=2)),
    dict(id="8208x8-1x1", w=8208, h=8, tx=1, ty=1,
         reach=dict(S=1, slices=[8], slots=513, items=[4104], steps=5, last_lanes=8, last_two=0, drow=0, dslot=512, segs=3,
                    last_seg_groups=1, phases=1, idle_lanes=0, subs=2)),
    dict(id="64x44-2x1", w=64, h=44, tx=2, ty=1,
         reach=dict(S=5, slices=[8, 9, 9, 9, 9], slots=2, items=[16, 18, 18, 18, 18], steps=1, last_lanes=18, last_two=0, drow=256,
                    dslot=0, segs=1, last_seg_groups=4, phases=64, idle_lanes=0, subs=6, band_rows=[26, 26])),
]

# ---- b. bgr_clahe_interp_kernel: bands, phases and the hand-over to planes -------------------------------------------------------
# path: "onepass" or "planes"; why: shape_ok's answer; contract: clahe_fp_contract and the oracle's fp_contract on for the call;
# off: byte offset of both bases in their allocations; n frames; inplace
B_N = 2
INTERP_CASES = [
    dict(id="80x21-5x3", w=80, h=21, tx=5, ty=3, clip=2.0, path="onepass", why=None,
         reach=dict(S=1, slots=1, groups=5, phases=51, idle_lanes=1, subs=1, bands=4, band_rows=[8, 15, 15, 8], segs=1)),
    dict(id="224x12-14x2", w=224, h=12, tx=14, ty=2, clip=2.0, path="onepass", why=None,
         reach=dict(S=1, groups=14, phases=18, idle_lanes=4, lds_bytes=61440, segs=1)),
    dict(id="240x12-15x2", w=240, h=12, tx=15, ty=2, clip=2.0, path="planes", why="pairs"),
    dict(id="72x12-3x2", w=72, h=12, tx=3, ty=2, clip=2.0, path="planes", why="tile_w"),
    dict(id="64x32-2x4-clip0", w=64, h=32, tx=2, ty=4, clip=0.0, path="onepass", why=None, reach=dict(S=1, subs=2, bands=5)),
    dict(id="64x32-2x4-clip40", w=64, h=32, tx=2, ty=4, clip=40.0, path="onepass", why=None, reach=dict(S=1, subs=2, bands=5)),
    dict(id="64x32-2x1", w=64, h=32, tx=2, ty=1, clip=2.0, path="onepass", why=None,
         reach=dict(S=4, slices=[8, 8, 8, 8], subs=5, bands=2, band_rows=[20, 20], tile_lut=True)),
    dict(id="64x32-2x4-contract", w=64, h=32, tx=2, ty=4, clip=2.0, path="planes", why="contract", contract=True),
    dict(id="64x30-2x4", w=64, h=30, tx=2, ty=4, clip=2.0, path="planes", why="padding"),
    dict(id="64x32-2x4-base+4", w=64, h=32, tx=2, ty=4, clip=2.0, path="planes", why="alignment", off=4),
    dict(id="64x32-2x4-three-inplace", w=64, h=32, tx=2, ty=4, clip=2.0, path="onepass", why=None, n=3, inplace=True,
         reach=dict(S=1, subs=2, bands=5)),
]

# ---- c. fused BGR equalizeHist: bgr_luma_hist_kernel / bgr_luma_apply_kernel -----------------------------------------------------
# Tight pitch (3 W: the frame is one row of W * H pixels), two frames a multiple of 16 bytes apart, both sides at byte offset `off`.
# reach: B of either pass, 16-pixel groups, steps and last-step lanes of the vector loop, tail pixels; off = 1: steps of the byte loop
C_N = 2
EQUALIZE_CASES = [
    dict(id="112x96", w=112, h=96, off=0, reach=dict(B=1, groups=672, steps=2, last_lanes=160, tail=0)),
    dict(id="50x218", w=50, h=218, off=0, reach=dict(B=1, groups=681, steps=2, last_lanes=169, tail=4)),
    dict(id="128x128", w=128, h=128, off=0, reach=dict(B=3, groups=1024, steps=1, last_lanes=1024, tail=0, idle_workgroups=1)),
    dict(id="50x218-base+1", w=50, h=218, off=1, reach=dict(B=1, groups=0, steps=22, last_lanes=148, tail=10900)),
]

# ---- d. nv12_bgr_equalize_batch_dev ----------------------------------------------------------------------------------------------
# extra: (in, out) bytes added to the tight frame stride W * H * 3 / 2, out None = in place; off: byte offset of both bases
# reach: B, items (16 x 2 groups or 2 x 2 blocks), per row (gx_n or W / 2), steps, lanes of the last step, dby / dgx and wraps (vector)
NV12_CASES = [
    dict(id="112x160-strides", w=112, h=160, n=2, off=0, extra=(16, 48), vec=True,
         reach=dict(B=1, items=560, per_row=7, steps=2, last_lanes=48, dby=73, dgx=1, wraps=6)),
    dict(id="144x144-inplace", w=144, h=144, n=2, off=0, extra=(0, None), vec=True,
         reach=dict(B=1, items=648, per_row=9, steps=2, last_lanes=136, dby=56, dgx=8, wraps=120)),
    dict(id="66x34", w=66, h=34, n=2, off=0, extra=(0, 0), vec=False, reach=dict(B=1, items=561, per_row=33, steps=2, last_lanes=49)),
    dict(id="96x144-base+1", w=96, h=144, n=2, off=1, extra=(0, 0), vec=False,
         reach=dict(B=1, items=3456, per_row=48, steps=7, last_lanes=384)),
]

# ---- e. many small frames: one workgroup a frame ---------------------------------------------------------------------------------
# n = FRAMES_PER_CU * cu frames, tight and aligned on both sides.  cvt420: reach as in d with 256 lanes.  color: 67 x 63 frames are
# 12663 = 7 (mod 16) bytes, so frame k starts aligned iff k % 16 == 0
CVT420_MANY = [
    dict(id="96x96", w=96, h=96, vec=True, reach=dict(bx=1, items=288, per_row=6, steps=2, last_lanes=32, dby=42, dgx=4, wraps=20)),
    dict(id="66x34", w=66, h=34, vec=False, reach=dict(bx=1, items=561, per_row=33, steps=3, last_lanes=49)),
]
COLOR_MANY = dict(id="67x63", w=67, h=63,
                  reach=dict(gy=1, bx=1, frame_mod16=7, aligned_every=16, groups=263, vec_steps=2, vec_last_lanes=7, tail=13,
                             byte_steps=17, byte_last_lanes=125))

# ---- f. more rows than the grid has ----------------------------------------------------------------------------------------------
COLOR_ROWS = dict(id="16x65540", w=16, h=65540, pitch=64, n=1, reach=dict(gy=65535, bx=1, second_step_rows=5))


# ---- what a case reaches, from the formulas --------------------------------------------------------------------------------------
def tile_hist_reach(cu, case, n):
    p = onepass_plan(cu, case["w"], case["h"], case["tx"], case["ty"], n)
    walk = tile_hist_walk(max(p["items"]), p["slots"])
    out = dict(p)
    out.update(steps=walk["steps"], last_lanes=walk["last_lanes"], last_two=walk["last_two"], drow=walk["drow"], dslot=walk["dslot"])
    return out


def equalize_reach(cu, case, n):
    w, h = case["w"], case["h"]
    px = w * h
    b = blocks_per_frame(cu, 3 * px, 1, n, 256)
    assert b == blocks_per_frame(cu, 3 * px, 1, n, 2048)            # the apply pass takes the same grid at these sizes
    if case["off"] % 16:
        steps, last = flat_walk(px, K_BGR_THREADS * b)
        return dict(B=b, groups=0, steps=steps, last_lanes=last, tail=px)
    groups = px // 16
    steps, last = flat_walk(groups, K_BGR_THREADS * b)
    out = dict(B=b, groups=groups, steps=steps, last_lanes=last, tail=px - 16 * groups)
    idle = sum(1 for k in range(b) if k * K_BGR_THREADS >= groups and k * K_BGR_THREADS >= px - 16 * groups)
    if idle:
        out["idle_workgroups"] = idle
    return out


def walk_reach(case, b, lanes):
    """The item walk of the NV12 / 4:2:0 kernels with b workgroups of `lanes` lanes a frame."""
    w, h = case["w"], case["h"]
    per_row = w // 16 if case["vec"] else w // 2
    items = per_row * (h // 2)
    stride = b * lanes
    if not case["vec"]:
        steps, last = flat_walk(items, stride)
        return dict(items=items, per_row=per_row, steps=steps, last_lanes=last)
    steps, last, wraps, ok = carried_walk((0, stride), stride, per_row, items)
    assert ok, "the carried walk left divmod"
    return dict(items=items, per_row=per_row, steps=steps, last_lanes=last, dby=stride // per_row, dgx=stride % per_row, wraps=wraps)


def nv12_reach(cu, case):
    w, h, n = case["w"], case["h"], case["n"]
    b = blocks_per_frame(cu, w * h * 3 // 2, 1, n, 256)
    assert b == blocks_per_frame(cu, w * h * 3 // 2, 1, n, 2048)
    return dict(B=b, **walk_reach(case, b, K_NV12_THREADS))


def cvt420_reach(cu, case):
    bx = cvt420_bx(cu, case["w"], case["h"], FRAMES_PER_CU * cu, case["vec"])
    return dict(bx=bx, **walk_reach(case, bx, K_THREADS))


def color_many_reach(cu):
    w, h = COLOR_MANY["w"], COLOR_MANY["h"]
    n = FRAMES_PER_CU * cu
    rows, row_px = color_job_rows(w, h, 3 * w, 3 * w)
    gy, bx = color_bx(cu, rows, row_px, n)
    frame = 3 * w * h
    aligned = [k for k in range(64) if (k * frame) % 16 == 0]
    groups = row_px // 16
    vs, vl = flat_walk(groups, bx * K_THREADS)
    bs, bl = flat_walk(row_px, bx * K_THREADS)
    return dict(gy=gy, bx=bx, frame_mod16=frame % 16, aligned_every=aligned[1] - aligned[0], groups=groups, vec_steps=vs,
                vec_last_lanes=vl, tail=row_px - 16 * groups, byte_steps=bs, byte_last_lanes=bl)


def color_rows_reach(cu):
    k = COLOR_ROWS
    rows, row_px = color_job_rows(k["w"], k["h"], k["pitch"], k["pitch"])
    gy, bx = color_bx(cu, rows, row_px, k["n"])
    return dict(gy=gy, bx=bx, second_step_rows=rows - gy)
