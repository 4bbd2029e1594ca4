"""Four-channel BGRA images in, equalized packed 4:2:2 frames (YUY2 and UYVY) out in one call (mi_*_bgra_to_packed422_batch_dev)
against what a caller with 4 B/px surfaces had to write before it, in ONE process (boxes differ by several per cent, so the legs are
timed interleaved, call by call):
    (a)  the new form (4 + 2 + 2 + 2 = 10 B/px equalizeHist, 6 + 2 + 4 = 12 B/px CLAHE)
    (b)  the route a caller has today: torch img[..., :3] copied into a contiguous three-channel scratch batch (4 read + 3 written),
         then mi_*_bgr_to_packed422_batch_dev (9 / 11 B/px): about 16 / 18 B/px, one torch kernel and a scratch batch more
    (c)  mi_*_bgr_to_packed422_batch_dev alone on PRE-MADE three-channel images: a ceiling nobody with 4 B/px surfaces can use
    (a2) leg (a) a second time in the same rotation: the ratio of the two medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight images per call (rotating between two sets: far beyond the 256 MiB Infinity Cache);
equalizeHist and CLAHE 8x8 clip 2.0; YUY2 and UYVY out; MI_ORDER_BGR, MI_UV_COPY.  Low-contrast colour bytes (a 64-value band), the
fourth byte full range.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  (a), (b) and (c) agree byte for byte before anything is timed.
Stage 1 alone: the median of the MI_K_COLOR slot over 30 profiled calls, as TB/s on the 6 B/px it moves (4 read, 2 written, either op)
next to the three-channel stage 1 of leg (c) on its 5 B/px, in the same run.
Bar: (a) beats (b) in every row by more than the run's spread.  No figure is fixed in advance; (a) against (c) is recorded as a
finding, whatever it reads.
    python tools/bgra_to_packed422_ab.py [--out DIR] [--calls N]   -> DIR/r37_bgra_to_packed422_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_bgra_to_packed422_frames_dev) against leg (a) under the same protocol:
    (a)   the batch form, tight; (a2) the same a second time in the rotation: the spread
    (l)   ONE list call whose entries are the batch's own addresses: the list kernel and the 128-frame chunk alone
    (lp)  ONE list call on POOLS: every image and every frame its own allocation (tight rows), of sizes of their own so that no
          allocator lays them out at one stride
(l) and (lp) hold the bytes of (a) before anything is timed.  No bar: a row in which a list leg trails (a) by more than the spread is
reported as a finding.
    python tools/bgra_to_packed422_ab.py --list [--out DIR] [--calls N]   -> DIR/r38_bgra_to_packed422_frames_ab.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import ORDER_BGR, FMT_YUY2, FMT_UYVY, UV_COPY  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
FMTS = (("yuy2", FMT_YUY2), ("uyvy", FMT_UYVY))
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = {"equalize": 10.0, "clahe": 12.0}
OLD_BYTES_PER_PX = {"equalize": 16.0, "clahe": 18.0}
C_BYTES_PER_PX = {"equalize": 9.0, "clahe": 11.0}
LEGS = ("a_new", "b_slice_then_bgr", "c_bgr_premade", "a2_new_again")
LIST_LEGS = ("a_batch", "l_list_on_batch", "lp_list_on_pools", "a2_batch_again")
COUNTERS = ("bgra_packed422_vec", "bgra_packed422_bytes", "bgra_packed422_list_frames_vec", "bgra_packed422_list_frames_bytes")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def make_sets(w, h, n):
    """Two sets of n tight four-channel images: the colour bytes in a 64-value band, the fourth byte full range."""
    sets = []
    for k in range(2):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED3700 + w + k)
        x = torch.randint(0, 256, (n, h, w, 4), dtype=torch.uint8, device="cuda:0", generator=g)
        x[..., :3] = x[..., :3] // 4 + 64 + 16 * k
        sets.append(x)
    return sets


def timed(legs, names, args, stream):
    """Interleaved timing: {leg: {median_us, p10_us, p90_us}}; legs[name](k) runs the leg on set k."""
    times = {k: [] for k in names}
    for it in range(args.warmup + args.calls):
        order = names[it % len(names):] + names[: it % len(names)]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[name](it & 1)
            e1.record(stream)
            if it >= args.warmup:
                times[name].append((e0, e1))
        if it % 20 == 19:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    out = {}
    for name, ev in times.items():
        ms = [a.elapsed_time(b) for a, b in ev]
        out[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3}
    return out


def color_kernel_p50_us(ctx, leg):
    ctx.profile_read(reset=True)
    for it in range(30):
        leg(it & 1)
    torch.cuda.synchronize()
    return ctx.profile_read(reset=True)["color_kernel"]["p50_ms"] * 1e3


def stat_delta(ctx, before):
    return [ctx.get_stat(k) - a for k, a in zip(COUNTERS, before)]


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        sets = make_sets(w, h, n)
        out_a = torch.empty((n, h, 2 * w), dtype=torch.uint8, device="cuda:0")
        out_l = torch.empty_like(out_a)
        # a surface pool and a playout buffer pool: per frame a separately allocated buffer, the surfaces filled from the tight sets
        pool_out = [torch.zeros((2 * w * h + 256 * (f % 3),), dtype=torch.uint8, device="cuda:0") for f in range(n)]
        pools_in = [[torch.empty((4 * w * h + 256 * ((f + 1) % 3),), dtype=torch.uint8, device="cuda:0") for f in range(n)] for _ in range(2)]
        for k in range(2):
            for f in range(n):
                pools_in[k][f][: 4 * w * h].copy_(sets[k][f].reshape(-1))
        on_batch = [([sets[k][f].data_ptr() for f in range(n)], [out_l[f].data_ptr() for f in range(n)]) for k in range(2)]
        on_pools = [([pools_in[k][f].data_ptr() for f in range(n)], [pool_out[f].data_ptr() for f in range(n)]) for k in range(2)]
        for fname, fmt in FMTS:
            for op in OPS:
                eq = op == "equalize"

                def batch(k):
                    if eq:
                        ctx.equalize_hist_bgra_to_packed422_batch_dev(sets[k], out_a, w, h, n, ORDER_BGR, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgra_to_packed422_batch_dev(sets[k], out_a, w, h, n, ORDER_BGR, fmt, UV_COPY, *CLAHE, stream=s)

                def lst(entries, k):
                    ins, outs = entries[k]
                    if eq:
                        ctx.equalize_hist_bgra_to_packed422_frames(ins, outs, w, h, ORDER_BGR, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgra_to_packed422_frames(ins, outs, w, h, ORDER_BGR, fmt, UV_COPY, *CLAHE, stream=s)

                legs = {"a_batch": batch, "l_list_on_batch": lambda k: lst(on_batch, k), "lp_list_on_pools": lambda k: lst(on_pools, k),
                        "a2_batch_again": batch}
                names = list(LIST_LEGS)
                stat0 = [ctx.get_stat(k) for k in COUNTERS]
                for name in names:                                   # the legs agree before anything is timed
                    legs[name](0)
                torch.cuda.synchronize()
                assert stat_delta(ctx, stat0) == [2, 0, 2 * n, 0], ("a leg left the vector walk", stat_delta(ctx, stat0))
                assert torch.equal(out_l, out_a), ("(l) and (a) differ", w, h, fname, op)
                for f in range(n):
                    assert torch.equal(pool_out[f][: 2 * w * h], out_a[f].reshape(-1)), ("(lp) and (a) differ", f, w, h, fname, op)
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "out": fname, "order": "BGR", "calls": args.calls,
                       "chunk_frames": {"list": 128, "batch": 256}}
                res.update(timed(legs, names, args, stream))
                med = {k: res[k]["median_us"] for k in names}
                for k in names:
                    res[k]["frames_per_s"] = n / (med[k] * 1e-6)
                res["spread"] = abs(med["a_batch"] / med["a2_batch_again"] - 1.0)
                res["list_on_batch_rate_over_batch_rate"] = med["a_batch"] / med["l_list_on_batch"]
                res["list_on_pools_rate_over_batch_rate"] = med["a_batch"] / med["lp_list_on_pools"]
                rows.append(res)
                print(json.dumps(res), flush=True)
        del sets, pools_in, on_batch, on_pools, out_a, out_l, pool_out
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "copy", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r38_bgra_to_packed422_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGRA in, equalized packed 4:2:2 out: the list form against the batch form", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY; tight rows.  Rates are frames per second.  "
          "(a): mi_*_bgra_to_packed422_batch_dev on a tight batch.  (l): ONE mi_*_bgra_to_packed422_frames_dev call naming the batch's own "
          "addresses.  (lp): ONE list call on pools, every image and every frame its own allocation.  Spread: the two (a) legs of the "
          "same rotation against each other.", "",
          "| frames | op | out | (a) batch | (l) list on a batch | (lp) list on pools | l / a | lp / a | spread |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | {r['out']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LIST_LEGS[:3]) +
                  f" | {r['list_on_batch_rate_over_batch_rate']:.3f} | {r['list_on_pools_rate_over_batch_rate']:.3f} | {r['spread']:.3f} |")
    behind = [(r["width"], r["op"], r["out"], k, round(r[k], 3), round(r["spread"], 3)) for r in rows
              for k in ("list_on_batch_rate_over_batch_rate", "list_on_pools_rate_over_batch_rate") if r[k] < 1.0 - r["spread"]]
    md += ["", "Rows in which a list leg trails the batch form by more than the spread (width, op, out, ratio, value, spread): " +
           (str(behind) if behind else "none") + "."]
    (outdir / "r38_bgra_to_packed422_frames_ab.md").write_text("\n".join(md) + "\n")
    if behind:
        print("FINDING: a list leg trails the batch form by more than the spread in", behind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="the frame-list form against the batch form")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if args.list:
        return main_list(args)
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        sets = make_sets(w, h, n)
        premade = [x[..., :3].contiguous() for x in sets]                            # leg (c): three-channel images nobody with 4 B/px surfaces has
        scratch = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")      # leg (b): the three-channel scratch the size of the video
        out_a = torch.empty((n, h, 2 * w), dtype=torch.uint8, device="cuda:0")
        out_b, out_c = torch.empty_like(out_a), torch.empty_like(out_a)
        for fname, fmt in FMTS:
            for op in OPS:
                eq = op == "equalize"

                def new_form(k):
                    if eq:
                        ctx.equalize_hist_bgra_to_packed422_batch_dev(sets[k], out_a, w, h, n, ORDER_BGR, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgra_to_packed422_batch_dev(sets[k], out_a, w, h, n, ORDER_BGR, fmt, UV_COPY, *CLAHE, stream=s)

                def three(src, dst):
                    if eq:
                        ctx.equalize_hist_bgr_to_packed422_batch_dev(src, dst, w, h, n, ORDER_BGR, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgr_to_packed422_batch_dev(src, dst, w, h, n, ORDER_BGR, fmt, UV_COPY, *CLAHE, stream=s)

                def leg_b(k):
                    scratch.copy_(sets[k][..., :3])                  # the slice-and-copy a caller writes today
                    three(scratch, out_b)

                legs = {"a_new": new_form, "b_slice_then_bgr": leg_b, "c_bgr_premade": lambda k: three(premade[k], out_c),
                        "a2_new_again": new_form}
                names = list(LEGS)
                stat0 = [ctx.get_stat(k) for k in COUNTERS]
                for name in names:                                   # the legs agree before anything is timed
                    legs[name](0)
                torch.cuda.synchronize()
                assert stat_delta(ctx, stat0) == [2, 0, 0, 0], ("the new form left the vector walk", stat_delta(ctx, stat0))
                assert torch.equal(out_a, out_b), ("(a) and (b) differ", w, h, fname, op)
                assert torch.equal(out_a, out_c), ("(a) and (c) differ", w, h, fname, op)
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "out": fname, "order": "BGR", "calls": args.calls}
                res.update(timed(legs, names, args, stream))
                med = {k: res[k]["median_us"] for k in names}
                for k in names:
                    res[k]["frames_per_s"] = n / (med[k] * 1e-6)
                res["spread"] = abs(med["a_new"] / med["a2_new_again"] - 1.0)
                res["a_rate_over_b_rate"] = med["b_slice_then_bgr"] / med["a_new"]
                res["a_rate_over_c_rate"] = med["c_bgr_premade"] / med["a_new"]
                res["a_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (med["a_new"] * 1e-6)
                res["b_bytes_per_s"] = OLD_BYTES_PER_PX[op] * w * h * n / (med["b_slice_then_bgr"] * 1e-6)
                res["c_bytes_per_s"] = C_BYTES_PER_PX[op] * w * h * n / (med["c_bgr_premade"] * 1e-6)
                res["bar_a_beats_b_by_more_than_the_spread"] = bool(res["a_rate_over_b_rate"] > 1.0 + res["spread"])
                ctx.set_profiling(1)
                ka, kc = color_kernel_p50_us(ctx, new_form), color_kernel_p50_us(ctx, legs["c_bgr_premade"])
                ctx.set_profiling(0)
                res["kernels"] = {"a_color_kernel_p50_us": ka, "c_color_kernel_p50_us": kc,
                                  "a_stage1_bytes_per_s": 6.0 * w * h * n / (ka * 1e-6), "c_stage1_bytes_per_s": 5.0 * w * h * n / (kc * 1e-6)}
                res["kernels"]["a_over_c_stage1_bytes_per_s"] = res["kernels"]["a_stage1_bytes_per_s"] / res["kernels"]["c_stage1_bytes_per_s"]
                rows.append(res)
                print(json.dumps(res), flush=True)
        del sets, premade, scratch, out_a, out_b, out_c
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "copy", "warmup": args.warmup, "bar": "(a) beats (b) in every row by more than the run's spread"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r37_bgra_to_packed422_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGRA in, equalized packed 4:2:2 out: the one-pass form against the slice-and-copy route it replaces", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY; tight batches.  Rates are frames per second.  "
          "(a): mi_*_bgra_to_packed422_batch_dev.  (b): torch img[..., :3] copied into a contiguous scratch batch, then "
          "mi_*_bgr_to_packed422_batch_dev.  (c): mi_*_bgr_to_packed422_batch_dev alone on pre-made three-channel images: a ceiling, not "
          "a route.  Spread: the two (a) legs of the same rotation against each other.  Stage 1 TB/s: the MI_K_COLOR kernel alone "
          "(median of 30 profiled calls) on the 6 B/px it moves in (a) and the 5 B/px in (c).", "",
          "| frames | op | out | (a) new | (b) slice + BGR form | (c) BGR form, pre-made | a / b | a / c | spread | (a) stage 1 TB/s | (c) stage 1 TB/s |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | {r['out']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS[:3]) +
                  f" | {r['a_rate_over_b_rate']:.3f} | {r['a_rate_over_c_rate']:.3f} | {r['spread']:.3f} "
                  f"| {r['kernels']['a_stage1_bytes_per_s'] / 1e12:.2f} | {r['kernels']['c_stage1_bytes_per_s'] / 1e12:.2f} |")
    missed = [(r["width"], r["op"], r["out"], round(r["a_rate_over_b_rate"], 3), round(r["spread"], 3)) for r in rows
              if not r["bar_a_beats_b_by_more_than_the_spread"]]
    behind = [(r["width"], r["op"], r["out"], round(r["kernels"]["a_over_c_stage1_bytes_per_s"], 3), round(r["spread"], 3)) for r in rows
              if r["kernels"]["a_over_c_stage1_bytes_per_s"] < 1.0 - r["spread"]]
    md += ["", "Bar, (a) beats (b) by more than the spread: " + ("met in every row" if not missed else "MISSED in " + str(missed)) + ".",
           "Rows in which stage 1 moves fewer bytes per second than its three-channel sibling by more than the spread (width, op, out, "
           "ratio, spread): " + (str(behind) if behind else "none") + "."]
    (outdir / "r37_bgra_to_packed422_ab.md").write_text("\n".join(md) + "\n")
    if missed:
        print("BAR MISSED: the one-pass form does not beat the slice-and-copy route by more than the spread in", missed)


if __name__ == "__main__":
    main()
