"""The rung table of tests/clahe_u8_rungs.py, checked on the CPU: every rung reaches the branch of the 8-bit CLAHE launch plan it is
there for (on a 256-CU part), and its content lets the oracle see what the GPU tests claim to test."""
import functools

import numpy as np

import oracle
import clahe_u8_rungs as R
from clahe_u8_rungs import RUNGS, HistPlan, InterpPlan

CU = 256

# rung -> (HistPlan, InterpPlan) with the rung's base options, cu = 256.  NV12 heights that differ are listed below.
TABLE = {
    "direct":      (HistPlan(8, 6, 1, 1, 1),      InterpPlan("float", 4, 1, 1, 64)),
    "float":       (HistPlan(20, 22, 1, 0, 1),    InterpPlan("float", 4, 1, 3, 64)),
    "float-pad":   (HistPlan(21, 7, 1, 0, 1),     InterpPlan("float", 4, 1, 1, 64)),
    "beyond":      (HistPlan(3, 3, 1, 1, 1),      InterpPlan("quad", 3, 1, 1, 85)),
    "quad-narrow": (HistPlan(6, 5, 1, 1, 1),      InterpPlan("quad", 6, 1, 1, 42)),
    "seg":         (HistPlan(112, 4, 1, 1, 1),    InterpPlan("float-seg", 38, 3, 1, 6)),
    "global":      (HistPlan(3, 5, 1, 1, 1),      InterpPlan("global", 0, 0, 0, 0)),
    "rows":        (HistPlan(2056, 22, 1, 0, 1),  InterpPlan("float", 256, 2, 3, 1)),
    "loads":       (HistPlan(280, 160, 1, 0, 1),  InterpPlan("float", 35, 1, 21, 7)),
    "split":       (HistPlan(280, 235, 29, 0, 1), InterpPlan("float", 18, 1, 30, 14)),
    "split-pad":   (HistPlan(281, 236, 29, 0, 1), InterpPlan("float", 18, 1, 30, 14)),
    "multi2":      (HistPlan(16, 4, 1, 1, 2),     InterpPlan("float", 8, 1, 1, 32)),
    "multi4":      (HistPlan(16, 4, 1, 1, 4),     InterpPlan("quad", 16, 1, 1, 16)),
    "multi8":      (HistPlan(16, 4, 1, 1, 8),     InterpPlan("quad", 16, 1, 1, 16)),
    "multi-noxcd": (HistPlan(16, 4, 1, 0, 2),     InterpPlan("float", 10, 1, 1, 25)),
    "multi-pad":   (HistPlan(16, 4, 1, 0, 2),     InterpPlan("float", 10, 1, 1, 25)),
}
# (rung, options beyond the base) -> the plan values the option is there to change
OPTION_TABLE = [
    ("seg", {"clahe_seg_pairs": 15}, None, InterpPlan("float-seg", 56, 2, 1, 4)),
    ("seg", {"clahe_seg_pairs": 4}, None, InterpPlan("quad", 112, 1, 1, 2)),
    ("seg", {"clahe_float_tables": 0}, None, InterpPlan("quad", 112, 1, 1, 2)),
    ("quad-narrow", {"clahe_float_tables": 0}, None, InterpPlan("quad", 6, 1, 1, 42)),
    ("float", {"clahe_float_tables": 0}, None, InterpPlan("quad", 4, 1, 3, 64)),
    ("rows", {"clahe_float_tables": 0}, None, InterpPlan("quad", 256, 2, 3, 1)),
    ("direct", {"clahe_xcd_map": 0}, HistPlan(8, 6, 1, 0, 1), None),
    ("direct", {"clahe_hist_threads": 256}, HistPlan(8, 6, 1, 1, 1), None),
    ("multi2", {"clahe_xcd_map": 0}, HistPlan(16, 4, 1, 0, 2), None),
    ("multi4", {"clahe_tiles_per_wg": 0}, HistPlan(16, 4, 1, 1, 2), None),
    ("multi8", {"clahe_hist_threads": 256}, HistPlan(16, 4, 1, 1, 1), None),
    ("split", {"clahe_hist_threads": 256}, HistPlan(280, 235, 29, 0, 1), None),
]


def test_rungs_reach_their_branch_on_256_cus():
    assert set(TABLE) == set(RUNGS)
    for name, r in RUNGS.items():
        got = R.plans(r, r.h, CU, r.base)
        assert got == TABLE[name], (name, got)
        if r.h_nv12 not in (None, r.h):                            # float-pad: 62 x 30 pads to the same 21 x 7 tiles
            assert R.plans(r, r.h_nv12, CU, r.base) == TABLE[name], (name, "NV12 height")
    for name, opts, hist, interp in OPTION_TABLE:
        r = RUNGS[name]
        h, i = R.plans(r, r.h, CU, dict(r.base, **opts))
        assert hist is None or h == hist, (name, opts, h)
        assert interp is None or i == interp, (name, opts, i)
    # what the table says in words
    assert R.K_MAX_PAIRS_F32 < 17 <= R.K_MAX_PAIRS < 65             # 16 tiles across leave the plain float tables, 64 the LDS
    assert 60 % 16 == 12 and 4 * 64 == 256 and 85 * 3 == 255        # float: ragged last group; beyond: lane 255 idle
    assert 280 * 235 >= 65536 and 235 % 29 != 0
    assert (9 - 3) * 6 // 16 == 2 and (9 - 3) * 112 // 16 == 42 and (4 - 3) * 112 // 16 == 7
    assert 280 // 16 == 17 and 280 % 16 == 8 and 512 // 17 == 30 and 512 - 30 * 17 == 2       # loads: slots, ragged bytes, drow, dslot
    assert 512 * 4 < 17 * 160 < 512 * 8 and 256 * 8 < 17 * 160 < 256 * 12                      # second / third round of the four loads
    assert 158 - 9 * 16 == 14 and 70 % 8 != 0
    # every class of each plan is hit
    hists = [TABLE[n][0] for n in TABLE] + [h for _, _, h, _ in OPTION_TABLE if h]
    interps = [TABLE[n][1] for n in TABLE] + [i for _, _, _, i in OPTION_TABLE if i]
    assert {p.kind for p in interps} == {"float", "float-seg", "quad", "global"}
    assert {p.K for p in hists} == {1, 2, 4, 8}
    assert {p.S > 1 for p in hists} == {True, False} and {p.xcd_map for p in hists} == {0, 1}
    assert {(p.K > 1, p.xcd_map) for p in hists} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert any(p.segs > 1 and p.kind == "float" for p in interps) and any(p.subs > 1 for p in interps)
    assert any(p.phases == 1 for p in interps)
    assert R.K256 == {n: TABLE[n][0].K for n, r in RUNGS.items() if r.multi}
    # a 64-frame list is exactly one chunk
    assert all(r.n == R.FRAMES_PER_LAUNCH for r in RUNGS.values() if r.multi)


def test_plan_follows_the_cu_count():
    """The restated plan is a function of the CU count, as the host's is: a part with fewer CUs splits less and fills sooner."""
    assert R.hist_plan(280, 470, 1, 2, 1, 64).S == 29 and R.hist_plan(280, 470, 1, 2, 1, 32).S == 16
    assert R.hist_plan(280, 470, 1, 2, 1, 1).S == 1
    assert R.hist_plan(256, 32, 16, 8, 64, 128, tiles_per_wg=8).K == 8
    assert R.hist_plan(128, 32, 8, 8, 64, 304).K == 1
    assert R.interp_plan(60, 66, 3, 3, 3, 1).subs == 1


@functools.lru_cache(maxsize=None)
def ref(name, h, k, clip, contract):
    r = RUNGS[name]
    old = oracle.set_fp_contract(bool(contract))
    try:
        return oracle.clahe(R.frame(r.w, h, k, r.n), clip, r.tx, r.ty)
    finally:
        oracle.set_fp_contract(old)


def nearest_tile(img, clip, tx, ty):
    """Every pixel through the LUT of its own tile only: what CLAHE would give without interpolation."""
    h, w = img.shape
    tw, th = R.tile_size(w, h, tx, ty)
    luts = oracle.clahe_tile_luts(img, clip, tx, ty)
    tile = (np.arange(h)[:, None] // th) * tx + np.arange(w)[None, :] // tw
    return luts[tile, img]


def test_content_shows_what_the_rungs_test():
    print()
    for name, h, r in [(n, h, r) for n, r in RUNGS.items() for h in sorted({r.h, r.h_nv12 or r.h})]:
        frames = [R.frame(r.w, h, k, r.n) for k in range(r.n)]
        name_h = f"{name} ({r.w}x{h})"
        assert len({f.tobytes() for f in frames}) == r.n, (name, "frames repeat")
        # (a) the interpolation is visible, in every frame
        if r.tx * r.ty > 1:
            shown = [float(np.mean(ref(name, h, k, R.CLIP, 0) != nearest_tile(f, R.CLIP, r.tx, r.ty))) for k, f in enumerate(frames)]
            print(f"{name_h}: interpolation shows in {100 * min(shown):.0f}..{100 * max(shown):.0f} % of the pixels")
            assert min(shown) >= 0.40, (name, shown)
        # (b) the arithmetic mode is visible over the frames the GPU tests run
        differ = sum(int(np.count_nonzero(ref(name, h, k, R.CLIP, 0) != ref(name, h, k, R.CLIP, 1))) for k in range(r.n))
        print(f"{name_h}: the two arithmetic modes differ in {differ} bytes over {r.n} frame(s)")
        runs_contract = any(o.get("clahe_fp_contract") for o, _ in r.variants())
        assert runs_contract == r.contract
        if r.contract:
            assert differ >= 5, (name, differ)
        if r.multi:                                                # 16 x 4 tiles: 1/tile is exact, both modes round alike
            assert differ == 0 and not r.contract, (name, differ)
        # (c) the output is not the input
        same = max(float(np.mean(ref(name, h, k, R.CLIP, 0) == f)) for k, f in enumerate(frames))
        print(f"{name_h}: at most {100 * same:.1f} % of a frame's output bytes equal the input")
        assert same <= 0.05, (name, same)
