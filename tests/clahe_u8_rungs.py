"""The rungs of the 8-bit CLAHE launch plan: small shapes that each reach one branch of launch_tile_luts / launch_interp
(csrc/host/clahe.inc.hpp), the content they run on, and the plan itself restated in Python.  No GPU, no test functions: a plain module
like tests/strided_layouts.py, used by tests/test_clahe_u8_rungs.py (CPU), tests/test_gpu_clahe_u8_rungs.py and the 4:2:2 ladder.

hist_plan() and interp_plan() restate the rules written in clahe.inc.hpp and its comments; the constants kMaxPairsLdsF32, kMaxPairsLds,
kInterpPx and kBandMargin are read from kernels/clahe.hip.h, the rest (tiles below 3 * 16 * 512 pixels take two tiles per workgroup,
tiles of 65536 pixels and more are split, 40 column groups per segment at least, 8 workgroups per CU) are the host's own literals."""
from __future__ import annotations

import re
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CLIP = 2.0
FRAMES_PER_LAUNCH = 64                                             # kFramesPerLaunch: a list of 64 frames is exactly one chunk


def _const(name: str) -> int:
    src = (ROOT / "opencv-opencl_amd" / "csrc" / "kernels" / "clahe.hip.h").read_text()
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


K_MAX_PAIRS_F32 = _const("kMaxPairsLdsF32")
K_MAX_PAIRS = _const("kMaxPairsLds")
K_INTERP_PX = _const("kInterpPx")
K_BAND_MARGIN = _const("kBandMargin")
K_THREADS = 256                                                    # the interpolation workgroup (kThreads)


# ---- content ---------------------------------------------------------------------------------------------------------------------
def content(w: int, h: int, seed: int) -> np.ndarray:
    """A ramp over both axes plus 48 levels of noise: neighbouring tiles get different LUTs, so the interpolation weights and the
    arithmetic mode show in the output."""
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    base = x * 160 // max(1, w - 1) + y * 64 // max(1, h - 1)
    noise = np.random.default_rng(seed).integers(0, 48, (h, w))
    return np.clip(base + noise, 0, 255).astype(np.uint8)


def frame(w: int, h: int, k: int, n: int) -> np.ndarray:
    """Frame k of a rung of n frames.  Small rungs: content(seed 100 + k).  The 64-frame rungs draw seven contents and add a per-frame
    offset k % 11, so every frame is distinct (7 and 11 are coprime)."""
    if n <= 7:
        return content(w, h, 100 + k)
    f = content(w, h, 100 + k % 7).astype(np.uint16) + k % 11
    return np.clip(f, 0, 255).astype(np.uint8)


# ---- the plan, restated ----------------------------------------------------------------------------------------------------------
HistPlan = namedtuple("HistPlan", "tile_w tile_h S xcd_map K")
InterpPlan = namedtuple("InterpPlan", "kind groups segs subs phases")


def tile_size(w, h, tx, ty):
    """clahe_geometry: BOTH axes are padded whenever EITHER is indivisible, each by tiles - size % tiles."""
    ew, eh = w, h
    if w % tx or h % ty:
        ew, eh = w + (tx - w % tx), h + (ty - h % ty)
    return ew // tx, eh // ty


def hist_plan(w, h, tx, ty, nf, cu, threads=512, xcd=1, tiles_per_wg=0) -> HistPlan:
    """launch_tile_luts.  S parts per tile (tile_lut_kernel runs iff S > 1), the XCD tile order, K tiles per workgroup
    (tile_hist_multi*_kernel runs iff K > 1)."""
    tile_w, tile_h = tile_size(w, h, tx, ty)
    tiles = tx * ty
    want = cu // (tiles * nf) if tile_w * tile_h >= 65536 else 1
    S = max(1, min(want, max(1, tile_h // 8), 64))
    xcd_map = 1 if xcd and S == 1 and tiles % 8 == 0 else 0
    K = 1
    if S == 1 and threads == 512:
        want_k = tiles_per_wg if tiles_per_wg > 0 else (2 if tile_w * tile_h < 3 * 16 * 512 else 1)
        run = tiles // 8 if xcd_map else tiles
        K = max(1, min(want_k, 8))
        while K > 1 and run % K:
            K -= 1
        while K > 1 and tiles // K * nf < cu * 8:                  # the batch must still fill the chip with workgroups
            K >>= 1
        if K > 1 and run % K:
            K = 1
    return HistPlan(tile_w, tile_h, S, xcd_map, K)


def interp_plan(w, h, tx, ty, nf, cu, float_tables=1, seg_pairs=9) -> InterpPlan:
    """launch_interp.  kind: "float" (f32 pair tables of the whole frame), "float-seg" (f32 tables per column segment), "quad" (uchar
    quads) or "global" (LUTs read from global memory; groups, segs, subs and phases are 0 there).  groups: 16-pixel column groups per
    segment, segs: column segments, subs: sub-bands per band, phases: rows a workgroup walks at once (256 / groups)."""
    tile_w, tile_h = tile_size(w, h, tx, ty)
    npairs = tx + 1
    if npairs > K_MAX_PAIRS:
        return InterpPlan("global", 0, 0, 0, 0)
    ngroups = (w + K_INTERP_PX - 1) // K_INTERP_PX
    groups = min(ngroups, K_THREADS)
    seg_tables = False
    seg_cap = max(4, min(seg_pairs, K_MAX_PAIRS_F32))
    if npairs > K_MAX_PAIRS_F32 and float_tables:
        gmax = (seg_cap - 3) * tile_w // K_INTERP_PX
        if gmax >= 40:
            per = min(groups, gmax)
            nseg = (ngroups + per - 1) // per
            groups = (ngroups + nseg - 1) // nseg
            seg_tables = True
    segs = (ngroups + groups - 1) // groups
    bands = ty + 1
    want = (cu * 8 + bands * nf * segs - 1) // (bands * nf * segs)
    rows_per_band = tile_h + 2 * K_BAND_MARGIN
    subs = max(1, min(want, max(1, rows_per_band // 8), 64))
    if float_tables and (npairs <= K_MAX_PAIRS_F32 or seg_tables):
        kind = "float-seg" if seg_tables else "float"
    else:
        kind = "quad"
    return InterpPlan(kind, groups, segs, subs, K_THREADS // groups)


# ---- the rungs -------------------------------------------------------------------------------------------------------------------
class Rung:
    """w x h (planar form), grid tx x ty, n frames.  h_nv12: the height of the NV12 forms (None: the rung runs planar only).
    contract: whether the GPU tests also run the rung with clahe_fp_contract = 1.  options: extra option sets beyond the rung's
    default ones, each a dict of context options."""

    def __init__(self, name, w, h, tx, ty, n, h_nv12="same", contract=True, base=None, extra=(), clips=(CLIP,), inplace=False):
        self.name, self.w, self.h, self.tx, self.ty, self.n = name, w, h, tx, ty, n
        self.h_nv12 = h if h_nv12 == "same" else h_nv12
        self.contract = contract
        self.base = dict(base or {})                               # options every variant of the rung runs with
        self.extra = tuple(extra)                                  # option sets run at (float_tables 1, contract 0) on top of `base`
        self.clips = tuple(clips)
        self.inplace = inplace
        self.multi = name.startswith("multi")

    def __repr__(self):
        return f"Rung({self.name}: {self.w}x{self.h} {self.tx}x{self.ty} x{self.n})"

    def variants(self):
        """[(options, clip)]: every option set the GPU tests run this rung with.  Options not named are the context's defaults."""
        out = []
        if self.multi:
            out += [(dict(self.base), clip) for clip in self.clips]
        else:
            modes = [(1, 0), (0, 0), (1, 1), (0, 1)] if self.contract else [(1, 0), (0, 0)]
            out += [(dict(self.base, clahe_float_tables=ft, clahe_fp_contract=fc), CLIP) for ft, fc in modes]
            out += [(dict(self.base), clip) for clip in self.clips if clip != CLIP]
        out += [(dict(self.base, **e), CLIP) for e in self.extra]
        return out


MULTI_CLIPS = (0.0, 2.0, 40.0)
RUNGS = {r.name: r for r in [
    Rung("direct", 64, 48, 8, 8, 3, extra=({"clahe_hist_threads": 256}, {"clahe_xcd_map": 0})),
    Rung("float", 60, 66, 3, 3, 3, clips=(0.0, CLIP, 40.0), inplace=True),
    Rung("float-pad", 62, 31, 3, 5, 3, h_nv12=30),
    Rung("beyond", 34, 10, 16, 4, 3),
    Rung("quad-narrow", 96, 10, 16, 2, 3),
    Rung("seg", 1792, 8, 16, 2, 3, extra=({"clahe_seg_pairs": 15}, {"clahe_seg_pairs": 4}), inplace=True),
    Rung("global", 192, 10, 64, 2, 3),
    Rung("rows", 4112, 44, 2, 2, 3),
    Rung("loads", 560, 160, 2, 1, 3, extra=({"clahe_hist_threads": 256},)),
    Rung("split", 280, 470, 1, 2, 1, extra=({"clahe_hist_threads": 256},)),
    Rung("split-pad", 280, 471, 1, 2, 1, h_nv12=None),
    Rung("multi2", 128, 32, 8, 8, 64, contract=False, clips=MULTI_CLIPS, extra=({"clahe_xcd_map": 0},)),
    Rung("multi4", 256, 32, 16, 8, 64, contract=False, clips=MULTI_CLIPS, base={"clahe_tiles_per_wg": 8}),
    Rung("multi8", 256, 64, 16, 16, 64, contract=False, clips=MULTI_CLIPS, base={"clahe_tiles_per_wg": 8}),
    Rung("multi-noxcd", 160, 28, 10, 7, 64, contract=False, clips=MULTI_CLIPS),
    Rung("multi-pad", 158, 26, 10, 7, 64, contract=False, clips=MULTI_CLIPS),
]}

# Tiles per workgroup on a 256-CU part, with each rung's own options.  K cannot be observed from outside the library: the GPU tests
# compute it with hist_plan from the device's CU count and insist on these values before they call.
K256 = {"multi2": 2, "multi4": 4, "multi8": 8, "multi-noxcd": 2, "multi-pad": 2}

# option name -> argument of hist_plan / interp_plan
_HIST_ARGS = {"clahe_hist_threads": "threads", "clahe_xcd_map": "xcd", "clahe_tiles_per_wg": "tiles_per_wg"}
_INTERP_ARGS = {"clahe_float_tables": "float_tables", "clahe_seg_pairs": "seg_pairs"}
DEFAULTS = {"clahe_float_tables": 1, "clahe_fp_contract": 0, "clahe_hist_threads": 512, "clahe_xcd_map": 1, "clahe_tiles_per_wg": 0,
            "clahe_seg_pairs": 9}


def plans(r: Rung, h: int, cu: int, options=None):
    """(HistPlan, InterpPlan) of one call of rung r at height h with the given context options on a `cu`-CU part."""
    o = dict(options or {})
    hk = {_HIST_ARGS[k]: v for k, v in o.items() if k in _HIST_ARGS}
    ik = {_INTERP_ARGS[k]: v for k, v in o.items() if k in _INTERP_ARGS}
    return hist_plan(r.w, h, r.tx, r.ty, r.n, cu, **hk), interp_plan(r.w, h, r.tx, r.ty, r.n, cu, **ik)
