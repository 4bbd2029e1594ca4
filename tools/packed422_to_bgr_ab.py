"""Packed 4:2:2 in, BGR out (mi_*_packed422_to_bgr_batch_dev) against the route a caller had before it and against a ceiling, in ONE
process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (A)  the new form: packed frames in, BGR images out, every row with its own chroma (7 B/px: 2 + 2 read, 3 written)
    (B)  mi_*_packed422_to_nv12_batch_dev (MI_UV_COPY) into an NV12 batch, then mi_cvt_color_420_u8_batch_dev(YUV2BGR_NV12) (10 B/px).
         NOT the same pixels: the first call halves the chroma vertically, so B's images carry 4:2:0 chroma.  The luma channel agrees.
    (C)  the ceiling: mi_*_nv12_to_bgr_batch_dev on frames converted to NV12 beforehand (5.5 B/px; not a route from packed input)
    (A') the new form once more in the same rotation: |A - A'| / A is the run's own spread
64 x 3840x2160 and 256 x 1920x1080 frames per call (1 GiB of packed input: far beyond the 256 MiB Infinity Cache); YUY2 and UYVY;
equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR; tight layouts.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  Inputs never change.  No ratio is fixed in advance: the run
records A against B and says whether the difference exceeds the spread.  After the timed legs each row runs 30 profiled calls of A
and of B and records the p50 time of each kernel role (mi_ctx_profile_read).
    python tools/packed422_to_bgr_ab.py [--out DIR] [--calls N]   -> DIR/r25_packed422_to_bgr_ab.json and .md (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, FMT_YUY2, FMT_UYVY, ORDER_BGR, COLOR_YUV2BGR_NV12  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
FMTS = [(FMT_YUY2, "YUY2"), (FMT_UYVY, "UYVY")]
ROLES = {"equalize": ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel", "color_kernel"),
         "clahe": ("tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel", "color_kernel")}
CLAHE = (2.0, 8, 8)


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def timed(stream, legs, warmup, calls):
    names = list(legs)
    times = {k: [] for k in names}
    for it in range(warmup + calls):
        order = names[it % len(names):] + names[: it % len(names)]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[name]()
            e1.record(stream)
            if it >= warmup:
                times[name].append((e0, e1))
        if it % 20 == 19:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = {}
    for name, ev in times.items():
        ms = [a.elapsed_time(b) for a, b in ev]
        out[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows, lines = [], []
    for w, h, n in CASES:
        for fmt, fname in FMTS:
            off = fmt - 2
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2500 + w + fmt)
            x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
            lane = x[:, :, off::2]
            lane.copy_(lane // 4 + 64)                               # low-contrast luma (~60 populated bins), random chroma
            bgr_a = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")
            bgr_b, bgr_c = torch.empty_like(bgr_a), torch.empty_like(bgr_a)
            nv12 = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")       # B's intermediate
            pre = torch.empty_like(nv12)                                                     # C's input: the same frames as NV12
            pre[:, :h, :].copy_(x[:, :, off::2])
            ch = x[:, :, 1 - off::2]
            pre[:, h:, :].copy_((ch[:, 0::2, :].to(torch.int16) + ch[:, 1::2, :] + 1) >> 1)
            del ch
            for op in ("equalize", "clahe"):
                def leg_a():
                    if op == "equalize":
                        ctx.equalize_hist_packed422_to_bgr_batch_dev(x, bgr_a, w, h, n, fmt, ORDER_BGR, stream=s)
                    else:
                        ctx.clahe_packed422_to_bgr_batch_dev(x, bgr_a, w, h, n, fmt, ORDER_BGR, *CLAHE, stream=s)

                def leg_b():
                    if op == "equalize":
                        ctx.equalize_hist_packed422_to_nv12_batch_dev(x, nv12, None, w, h, n, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_packed422_to_nv12_batch_dev(x, nv12, None, w, h, n, fmt, UV_COPY, *CLAHE, stream=s)
                    ctx.cvt_color_420_batch_dev(nv12, bgr_b, w, h, n, COLOR_YUV2BGR_NV12, stream=s)

                def leg_c():
                    if op == "equalize":
                        ctx.equalize_hist_nv12_to_bgr_batch_dev(pre, None, bgr_c, w, h, n, ORDER_BGR, stream=s)
                    else:
                        ctx.clahe_nv12_to_bgr_batch_dev(pre, None, bgr_c, w, h, n, ORDER_BGR, *CLAHE, stream=s)

                # before anything is timed: B and C are the same pixels in two calls and in one; whether A's bytes differ from theirs
                # (they do wherever the two rows of a pair carry different chroma) is recorded with the row
                leg_a()
                leg_b()
                leg_c()
                torch.cuda.synchronize()
                assert torch.equal(bgr_b, bgr_c), ("B and C differ", w, h, fname, op)
                differs = not torch.equal(bgr_a[0], bgr_b[0])
                legs = {"A_packed_to_bgr": leg_a, "B_to_nv12_then_cvt": leg_b, "C_nv12_to_bgr_ceiling": leg_c, "A2_packed_to_bgr_again": leg_a}
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "format": fname, "order": "BGR", "calls": args.calls,
                       "A_and_B_differ_in_chroma_bytes": differs}
                for name, r in timed(stream, legs, args.warmup, args.calls).items():
                    r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                    res[name] = r
                a, a2 = res["A_packed_to_bgr"]["median_us"], res["A2_packed_to_bgr_again"]["median_us"]
                res["spread"] = abs(a - a2) / a
                res["A_rate_over_B_rate"] = res["B_to_nv12_then_cvt"]["median_us"] / a
                res["A_rate_over_C_rate"] = res["C_nv12_to_bgr_ceiling"]["median_us"] / a
                res["A_ahead_of_B_by_more_than_the_spread"] = res["A_rate_over_B_rate"] - 1.0 > res["spread"]
                px = w * h * n
                res["A_bytes_per_s"] = 7.0 * px / (a * 1e-6)
                ctx.set_profiling(1)
                kern = {}
                for leg, tag in ((leg_a, "A"), (leg_b, "B")):
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        leg()
                    torch.cuda.synchronize()
                    prof = ctx.profile_read(reset=True)
                    for role in ROLES[op]:
                        if prof[role]["launches"]:
                            kern.setdefault(role, {})[tag + "_p50_us"] = prof[role]["p50_ms"] * 1e3
                ctx.set_profiling(0)
                res["kernels"] = kern
                rows.append(res)
                line = (f"{w}x{h} x{n:3d} {fname} {op:8s} " +
                        "  ".join(f"{k.split('_')[0]} {res[k]['median_us']:8.1f} us [{res[k]['p10_us']:.1f} {res[k]['p90_us']:.1f}]" for k in legs) +
                        f"  | A/B {res['A_rate_over_B_rate']:.3f}  A/C {res['A_rate_over_C_rate']:.3f}  spread {res['spread']:.3f}  | " +
                        "  ".join(f"{role} A {v.get('A_p50_us', 0):.1f} B {v.get('B_p50_us', 0):.1f} us" for role, v in kern.items()))
                print(line, flush=True)
                lines.append(line)
            del x, lane, bgr_a, bgr_b, bgr_c, nv12, pre
            torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "note": "A and B do not write the same chroma: B halves it vertically (4:2:0), A keeps every row's own (4:2:2)",
            "bars": "none fixed in advance"}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r25_packed422_to_bgr_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# Packed 4:2:2 in, BGR out: the one-call form against the two-call route and the NV12 ceiling", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one "
          "process, medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR; tight layouts.  Rates are frames per second.  "
          "(A): mi_*_packed422_to_bgr_batch_dev, 7 B/px.  (B): mi_*_packed422_to_nv12_batch_dev + mi_cvt_color_420_u8_batch_dev(YUV2BGR_NV12), "
          "10 B/px -- the routes DIFFER IN CHROMA BYTES: B halves the chroma vertically, A keeps every row's own.  (C): "
          "mi_*_nv12_to_bgr_batch_dev on pre-converted NV12 frames, 5.5 B/px: a ceiling, not a route from packed input.  Spread: the two (A) "
          "legs of the same rotation against each other.  A TB/s: 7 B/px over A's median.  Kernels: p50 of the pixel-writing kernel "
          "(MI_K_LUT_APPLY / MI_K_CLAHE_INTERP) of A and of B, and B's conversion kernel (MI_K_COLOR).", "",
          "| frames | format | op | (A) one call | (B) two calls | (C) NV12 ceiling | A / B | A / C | spread | A TB/s | writer A | writer B | B color |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(k):
            return f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)"
        wr = "lut_apply_kernel" if r["op"] == "equalize" else "clahe_interp_kernel"
        kk = r["kernels"]
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | {cell('A_packed_to_bgr')} | "
                  f"{cell('B_to_nv12_then_cvt')} | {cell('C_nv12_to_bgr_ceiling')} | {r['A_rate_over_B_rate']:.3f} | {r['A_rate_over_C_rate']:.3f} | "
                  f"{r['spread']:.3f} | {r['A_bytes_per_s'] / 1e12:.2f} | {kk.get(wr, {}).get('A_p50_us', 0):.0f} us | "
                  f"{kk.get(wr, {}).get('B_p50_us', 0):.0f} us | {kk.get('color_kernel', {}).get('B_p50_us', 0):.0f} us |")
    behind = [(r["width"], r["format"], r["op"], round(r["A_rate_over_B_rate"], 3)) for r in rows if not r["A_ahead_of_B_by_more_than_the_spread"]]
    md += ["", "Rows in which the one-call form is NOT ahead of the two-call route by more than the spread: " + (str(behind) if behind else "none") + "."]
    (outdir / "r25_packed422_to_bgr_ab.md").write_text("\n".join(md) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
