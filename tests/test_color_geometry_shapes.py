"""CPU checks behind tests/test_gpu_color_geometry.py: the host formulas of host/color.inc.hpp restated in tests/color_geometry_cases.py
are still the header's, its constants are the headers', and every case of its tables reaches what it records -- loop steps, lanes of the
last step, the wrap, S and the slice heights, segs, phases, one-pass or planes -- for every CU count from 64 to 1024, so the GPU module
may run the tables on any device in that range.  Nothing here needs a GPU or the library."""
import re
from pathlib import Path

import pytest

import color_geometry_cases as g

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "opencv-opencl_amd" / "csrc"
CUS = range(g.CU_MIN, g.CU_MAX + 1)


def constant(header, name):
    src = (CSRC / header).read_text()
    return int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src).group(1))


def squeezed(header):
    return re.sub(r"\s+", "", (CSRC / header).read_text())


def subset(full, want):
    return {k: full[k] for k in want}


def test_constants_are_the_headers():
    assert constant("kernels/clahe.hip.h", "kMaxPairsLdsF32") == g.K_MAX_PAIRS_LDS_F32
    assert constant("kernels/clahe.hip.h", "kInterpPx") == g.K_INTERP_PX
    assert constant("kernels/clahe.hip.h", "kBandMargin") == g.K_BAND_MARGIN
    assert constant("kernels/color.hip.h", "kBgrThreads") == g.K_BGR_THREADS
    assert constant("kernels/color.hip.h", "kNv12Threads") == g.K_NV12_THREADS
    assert constant("kernels/common.hip.h", "kThreads") == g.K_THREADS
    assert constant("host/context.inc.hpp", "kMaxGridY") == g.K_MAX_GRID_Y


def test_restated_host_formulas_are_the_headers():
    """The expressions color_geometry_cases restates, character for character (spaces aside)."""
    ctx = squeezed("host/context.inc.hpp")
    for piece in ("constlonglongtarget=(longlong)c->cu_count*8;", "longlongb=(target+n_frames-1)/n_frames;",
                  "by_bytes=std::max<longlong>(1,bytes_per_frame/16384);", "if(rows>1)b=std::min<longlong>(b,rows);",
                  "b=std::min<longlong>(b,cap);"):
        assert piece in ctx, piece
    host = squeezed("host/color.inc.hpp")
    for piece in (
            # launch_color
            "constintgy=std::min(j.rows,65535);",
            "longlongbx=((longlong)c->cu_count*8+(longlong)gy*n_frames-1)/((longlong)gy*n_frames);",
            "bx=std::max<longlong>(1,std::min<longlong>(bx,(j.row_px/16+kThreads-1)/kThreads+1));",
            # color_job
            "if(contiguous||a.height==1){j.rows=1;j.row_px=(longlong)a.width*a.height;",
            # the fused equalizeHist and the NV12 form
            "blocks_per_frame(c,(longlong)a.width*a.height*3,1,nf,256);", "blocks_per_frame(c,(longlong)a.width*a.height*3,1,nf,2048);",
            "blocks_per_frame(c,ysz*3/2,1,nf,256);", "blocks_per_frame(c,ysz*3/2,1,nf,2048);",
            "dim3(B,1,nf),dim3(kBgrThreads)", "dim3(B2,1,nf),dim3(kBgrThreads)", "dim3(B,nf),dim3(kNv12Threads)", "dim3(B2,nf),dim3(kNv12Threads)",
            # shape_ok
            "constboolshape_ok=!g.contract&&a.width%tx==0&&a.height%ty==0&&g.tile_w%16==0&&tx+1<=kMaxPairsLdsF32&&"
            "tiles<=kMaxGridY&&a.width/kInterpPx<=kThreads*kMaxGridY&&"
            "(((uintptr_t)a.src|(uintptr_t)a.dst|a.src_step|a.dst_step|a.src_frame|a.dst_frame)&15)==0;",
            # S, groups, segs, subs
            "longlongwant=((longlong)c->cu_count*8+(longlong)tiles*nf-1)/((longlong)tiles*nf);",
            "constintS=(int)std::max<longlong>(1,std::min<longlong>({want,(longlong)std::max(1,g.tile_h/8),64LL}));",
            "uint8_t*direct=S==1?c->d_luts:nullptr;", "bgr_tile_hist_kernel<512>,dim3(S,tiles,nf),dim3(512)",
            "constintngroups=a.width/kInterpPx;", "constintgroups=std::min(ngroups,kThreads);", "constintsegs=(ngroups+groups-1)/groups;",
            "constintbands=ty+1;", "want=((longlong)c->cu_count*8+(longlong)bands*nf*segs-1)/((longlong)bands*nf*segs);",
            "constintsubs=(int)std::max<longlong>(1,std::min<longlong>({want,(longlong)std::max(1,(g.tile_h+2*kBandMargin)/8),64LL}));",
            "(size_t)(tx+1)*256*4*sizeof(float)",
            # cvt420_dev
            "constlonglongblocks=(longlong)(width/2)*(height/2);", "longlongbx=((longlong)c->cu_count*8+nf-1)/nf;",
            "bx=std::max<longlong>(1,std::min<longlong>(bx,(blocks+kThreads-1)/kThreads));",
            "if(vec)bx=std::max<longlong>(1,std::min<longlong>(bx,(blocks/8+kThreads-1)/kThreads));"):
        assert piece in host, piece
    kern = squeezed("kernels/color_clahe.hip.h")
    for piece in ("constintslots=g.tile_w>>4;", "constintdrow=NT/slots,dslot=NT-drow*slots;", "for(intit=t;it<items;it+=2*NT){",
                  "constbooltwo=it+NT<items;", "r0=(int)((longlong)g.tile_h*s/S),r1=(int)((longlong)g.tile_h*(s+1)/S);",
                  "constintphases=kThreads/groups;", "constintx0=(blockIdx.z*groups+grp)*kInterpPx;",
                  "(int)max(0LL,((longlong)(2*band-1)*g.tile_h)/2-kBandMargin);",
                  "(int)min((longlong)g.height,((longlong)(2*band+1)*g.tile_h+1)/2+kBandMargin);"):
        assert piece in kern, piece
    color = squeezed("kernels/color.hip.h")
    for piece in ("for(introw=blockIdx.y;row<j.rows;row+=gridDim.y){", "constintstride=(int)gridDim.x*kNv12Threads,dby=stride/gx_n,dgx=stride-dby*gx_n;",
                  "constintstride=(int)gridDim.x*kThreads,dby=stride/gx_n,dgx=stride-dby*gx_n;", "if(gx>=gx_n){gx-=gx_n;++by;}"):
        assert piece in color, piece


def test_blocks_per_frame_bounds():
    for cu in (g.CU_MIN, 256, g.CU_MAX):
        assert g.blocks_per_frame(cu, 16383, 1, 1, 256) == 1 and g.blocks_per_frame(cu, 3 * 16384, 1, 1, 256) == 3
        assert g.blocks_per_frame(cu, 1 << 30, 1, 1, 256) == 256 and g.blocks_per_frame(cu, 1 << 30, 1, 1, 2048) == min(2048, 8 * cu)
        assert g.blocks_per_frame(cu, 1 << 30, 5, 1, 256) == 5 and g.blocks_per_frame(cu, 1 << 30, 1, 16 * cu, 256) == 1
    assert g.c_div(-7, 2) == -3 and g.c_div(7, 2) == 3 and g.c_div(-8, 2) == -4


@pytest.mark.parametrize("case", g.TILE_HIST_SHAPES, ids=[c["id"] for c in g.TILE_HIST_SHAPES])
def test_tile_hist_shapes_reach_what_they_record(case):
    w, h, tx, ty = case["w"], case["h"], case["tx"], case["ty"]
    assert g.shape_ok(w, h, tx, ty) is None and (3 * w) % 16 == 0
    for n in (g.A_N,):
        for cu in CUS:
            got = g.tile_hist_reach(cu, case, n)
            assert subset(got, case["reach"]) == case["reach"], (cu, subset(got, case["reach"]))
    plan = g.onepass_plan(256, w, h, tx, ty, g.A_N)
    for items in set(plan["items"]):
        assert g.tile_hist_walk(items, plan["slots"])["ok"], "a live item of the carried (row, slot) walk is not divmod(it, slots)"


def test_tile_hist_table_covers_the_named_properties():
    by = {c["id"]: c["reach"] for c in g.TILE_HIST_SHAPES}
    walk = {c["id"]: g.tile_hist_walk(max(c["reach"]["items"]), c["reach"]["slots"]) for c in g.TILE_HIST_SHAPES}
    # the second item in flight is live in some lanes and dead in others
    assert walk["1072x8-1x1"]["two_some"] and by["1072x8-1x1"]["last_two"] == 24
    assert walk["1040x16-1x1"]["two_some"] and by["1040x16-1x1"]["last_two"] == 8
    # every step count, and a last step whose second item is dead in every lane
    assert [by[k]["steps"] for k in ("1072x8-1x1", "2096x8-1x1", "4128x16-1x2", "8208x8-1x1")] == [1, 2, 3, 5]
    assert all(by[k]["last_two"] == 0 and 0 < by[k]["last_lanes"] < g.TILE_NT for k in ("2096x8-1x1", "4128x16-1x2", "8208x8-1x1"))
    # a step with both items live in every lane comes before it
    assert 2064 > 2 * g.TILE_NT + 0 and 4104 > 4 * 2 * g.TILE_NT
    # the wrap fires; drow == 0 with more slots than lanes
    assert {k for k in walk if walk[k]["wraps"] > 0} == {"2096x8-1x1", "4128x16-1x2", "8208x8-1x1"}
    assert (by["2096x8-1x1"]["drow"], by["2096x8-1x1"]["dslot"]) == (3, 119)
    assert by["8208x8-1x1"]["slots"] == 513 > g.TILE_NT and (by["8208x8-1x1"]["drow"], by["8208x8-1x1"]["dslot"]) == (0, 512)
    # slices: one, two even ones, five uneven ones; the LUT direct or through partials
    assert by["64x44-2x1"]["slices"] == [8, 9, 9, 9, 9] and by["1040x16-1x1"]["slices"] == [8, 8]
    assert {k for k in by if by[k]["S"] == 1} == {"1072x8-1x1", "2096x8-1x1", "4128x16-1x2", "8208x8-1x1"}
    # column segments and phases of the interpolation
    assert (by["4128x16-1x2"]["segs"], by["4128x16-1x2"]["last_seg_groups"]) == (2, 2)
    assert (by["8208x8-1x1"]["segs"], by["8208x8-1x1"]["last_seg_groups"]) == (3, 1)
    assert (by["2096x8-1x1"]["phases"], by["2096x8-1x1"]["idle_lanes"]) == (1, 125)
    assert by["64x44-2x1"]["subs"] == 6 and by["64x44-2x1"]["band_rows"] == [26, 26]
    assert all(c["w"] <= 4096 or c["reach"]["segs"] > 1 for c in g.TILE_HIST_SHAPES)


@pytest.mark.parametrize("case", g.INTERP_CASES, ids=[c["id"] for c in g.INTERP_CASES])
def test_interp_cases_take_the_path_they_record(case):
    w, h, tx, ty = case["w"], case["h"], case["tx"], case["ty"]
    aligned = case.get("off", 0) % 16 == 0 and (3 * w) % 16 == 0 and (3 * w * h) % 16 == 0
    why = g.shape_ok(w, h, tx, ty, case.get("contract", False), aligned)
    assert why == case["why"] and (why is None) == (case["path"] == "onepass")
    if why is not None:
        # one term alone fails: the same shape with that term mended is one-pass, or the term is a property of the grid
        others = g.shape_ok(w, h, tx, ty, False, True)
        assert others == (None if why in ("contract", "alignment") else why)
        return
    for cu in CUS:
        got = g.onepass_plan(cu, w, h, tx, ty, case.get("n", g.B_N))
        assert subset(got, case["reach"]) == case["reach"], (cu, subset(got, case["reach"]))


def test_interp_table_covers_the_named_properties():
    by = {c["id"]: c for c in g.INTERP_CASES}
    r = by["80x21-5x3"]["reach"]
    assert (r["groups"], r["phases"], r["idle_lanes"]) == (5, 51, 1) and g.clahe_tile(80, 21, 5, 3) == (16, 7)
    assert all((2 * band - 1) * 7 % 2 for band in range(4))                      # every band edge falls between two rows
    r = by["224x12-14x2"]["reach"]
    assert r["lds_bytes"] == 60 * 1024 and by["224x12-14x2"]["tx"] + 1 == g.K_MAX_PAIRS_LDS_F32
    assert by["240x12-15x2"]["tx"] + 1 == g.K_MAX_PAIRS_LDS_F32 + 1
    assert g.clahe_tile(72, 12, 3, 2)[0] == 24
    assert {c["why"] for c in g.INTERP_CASES} == {None, "pairs", "tile_w", "contract", "padding", "alignment"}
    assert {c["clip"] for c in g.INTERP_CASES if c["w"] == 64 and c["path"] == "onepass"} >= {0.0, 40.0}
    assert by["64x32-2x4-three-inplace"]["n"] == 3 and by["64x32-2x4-three-inplace"]["inplace"]
    assert by["64x32-2x1"]["reach"]["S"] == 4 and by["64x32-2x1"]["reach"]["tile_lut"]


@pytest.mark.parametrize("case", g.EQUALIZE_CASES, ids=[c["id"] for c in g.EQUALIZE_CASES])
def test_equalize_cases_reach_what_they_record(case):
    for cu in CUS:
        assert g.equalize_reach(cu, case, g.C_N) == case["reach"], (cu, g.equalize_reach(cu, case, g.C_N))


def test_equalize_table_covers_the_named_properties():
    by = {c["id"]: c["reach"] for c in g.EQUALIZE_CASES}
    assert by["112x96"] == dict(B=1, groups=672, steps=2, last_lanes=160, tail=0)
    assert by["50x218"]["groups"] == 681 and by["50x218"]["tail"] == 4 and by["50x218"]["steps"] == 2
    assert 3 * 128 * 128 == 3 * 16384 and by["128x128"]["B"] == 3 and by["128x128"]["idle_workgroups"] == 1
    assert 2 * g.K_BGR_THREADS == by["128x128"]["groups"]                       # the third workgroup's first group is one past the last
    assert by["50x218-base+1"]["groups"] == 0 and by["50x218-base+1"]["steps"] == 22
    # a frame stride of a multiple of 16 keeps every frame of a case on the body its first frame takes
    for c in g.EQUALIZE_CASES:
        assert equalize_stride(c) % 16 == 0 and equalize_stride(c) >= 3 * c["w"] * c["h"]


def equalize_stride(case):
    """The frame stride the GPU module gives group c: the frame rounded up to 16 bytes, and 16 more."""
    return (3 * case["w"] * case["h"] + 15) // 16 * 16 + 16


@pytest.mark.parametrize("case", g.NV12_CASES, ids=[c["id"] for c in g.NV12_CASES])
def test_nv12_cases_reach_what_they_record(case):
    w, h = case["w"], case["h"]
    frame = w * h * 3 // 2
    strides = [frame + e for e in case["extra"] if e is not None]
    vec = w % 16 == 0 and case["off"] % 16 == 0 and all(s % 16 == 0 for s in strides)
    assert vec == case["vec"]
    for cu in CUS:
        assert g.nv12_reach(cu, case) == case["reach"], (cu, g.nv12_reach(cu, case))


def test_nv12_table_covers_the_named_properties():
    by = {c["id"]: c for c in g.NV12_CASES}
    r = by["112x160-strides"]["reach"]
    assert (r["per_row"], r["items"], r["last_lanes"], r["dgx"]) == (7, 560, 48, 1)
    assert r["wraps"] == len([t for t in range(48) if t % 7 == 6])               # dgx 1: the wrap fires at gx 6 alone
    r = by["144x144-inplace"]["reach"]
    assert (r["per_row"], r["dgx"]) == (9, 8) and r["wraps"] == len([t for t in range(136) if t % 9 >= 1])
    assert by["66x34"]["reach"]["steps"] == 2 and by["96x144-base+1"]["reach"]["steps"] == 7
    assert any(c["extra"][1] is None for c in g.NV12_CASES)                      # one in place
    assert any(c["extra"][1] not in (None, c["extra"][0]) for c in g.NV12_CASES)  # one with two different strides
    assert all(c["n"] >= 2 for c in g.NV12_CASES)


@pytest.mark.parametrize("case", g.CVT420_MANY, ids=[c["id"] for c in g.CVT420_MANY])
def test_many_frames_cvt420_reach_what_they_record(case):
    w, h = case["w"], case["h"]
    assert case["vec"] == (w % 16 == 0 and (3 * w) % 16 == 0 and (3 * w * h) % 16 == 0 and (w * h * 3 // 2) % 16 == 0)
    for cu in CUS:
        assert g.FRAMES_PER_CU * cu <= g.K_MAX_GRID_Y                            # one launch
        assert g.cvt420_reach(cu, case) == case["reach"], (cu, g.cvt420_reach(cu, case))
        assert g.cvt420_bx(cu, w, h, g.FRAMES_PER_CU * cu - 1, case["vec"]) == 2  # one frame fewer and the grid is wider
        assert w * h * 9 // 2 * g.FRAMES_PER_CU * 256 <= 90e6                     # bytes a call moves on a 256-CU device


def test_many_frames_cvt420_table_covers_the_named_properties():
    r = g.CVT420_MANY[0]["reach"]
    assert (r["items"], r["dby"], r["dgx"], r["last_lanes"]) == (288, 42, 4, 32)
    assert r["wraps"] == len([t for t in range(32) if t % 6 >= 2]) > 0
    assert g.CVT420_MANY[1]["reach"]["steps"] == 3


def test_many_frames_color_reaches_what_it_records():
    for cu in CUS:
        assert g.color_many_reach(cu) == g.COLOR_MANY["reach"], (cu, g.color_many_reach(cu))
    r = g.COLOR_MANY["reach"]
    assert r["vec_steps"] == 2 and r["tail"] == 13 and r["byte_steps"] == 17 and r["aligned_every"] == 16
    assert 2 * 3 * 67 * 63 * g.FRAMES_PER_CU * 256 <= 90e6


def test_row_loop_reaches_its_second_step():
    for cu in CUS:
        assert g.color_rows_reach(cu) == g.COLOR_ROWS["reach"], (cu, g.color_rows_reach(cu))
    k = g.COLOR_ROWS
    assert k["pitch"] != 3 * k["w"] and k["pitch"] % 16 == 0                     # row-wise addressing, every row aligned
    assert k["h"] - 65535 == 5
