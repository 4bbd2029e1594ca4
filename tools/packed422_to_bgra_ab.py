"""Packed 4:2:2 frames (YUY2 and UYVY) in, equalized four-channel BGRA out in one call (mi_*_packed422_to_bgra_batch_dev) against what
a caller who needs a four-byte-per-pixel surface had to write before it, in ONE process (boxes differ by several per cent, so the legs
are timed interleaved, call by call):
    (a)  the new form (the packed frame read twice, 4 B/px written: 8 B/px)
    (b)  the route a caller has today: mi_*_packed422_to_bgr_batch_dev into a three-channel scratch batch (7 B/px), then a torch widen
         to four channels with alpha 255 (torch.cat of the scratch and an alpha plane: 3 + 1 read, 4 written): about 14 - 15 B/px
    (c)  mi_*_packed422_to_bgr_batch_dev alone: a ceiling, not a route -- it writes 1 B/px less and is not what the caller needs
    (a2) leg (a) a second time in the same rotation: the ratio of the two medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight frames per call (rotating between two sets: far beyond the 256 MiB Infinity Cache);
equalizeHist and CLAHE 8x8 clip 2.0; YUY2 and UYVY in; MI_ORDER_BGR.  Low-contrast luma (a 64-value band), full-range chroma.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  (a) and (b) agree byte for byte, and (a)[..., :3] equals (c),
before anything is timed.
Bar: (a) beats (b) in every row by more than the run's spread.  No figure is fixed in advance; (a) against (c) is recorded as a
finding, whatever it reads.
    python tools/packed422_to_bgra_ab.py [--out DIR] [--calls N]   -> DIR/r35_packed422_to_bgra_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_packed422_to_bgra_frames_dev) against leg (a) under the same protocol:
    (a)   the batch form, tight; (a2) the same a second time in the rotation: the spread
    (l)   ONE list call whose entries are the batch's own addresses: the list kernels and the 128-frame chunk alone
    (lp)  ONE list call on POOLS: every frame and every image its own allocation (tight rows), of sizes of their own so that no
          allocator lays them out at one stride
(l) and (lp) hold the bytes of (a) before anything is timed.  No bar: a row in which a list leg trails (a) by more than the spread is
reported as a finding.
    python tools/packed422_to_bgra_ab.py --list [--out DIR] [--calls N]   -> DIR/r36_packed422_to_bgra_frames_ab.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import ORDER_BGR, FMT_YUY2, FMT_UYVY  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
FMTS = (("yuy2", FMT_YUY2), ("uyvy", FMT_UYVY))
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = 8.0
LEGS = ("a_new", "b_bgr_then_widen", "c_bgr_alone", "a2_new_again")
LIST_LEGS = ("a_batch", "l_list_on_batch", "lp_list_on_pools", "a2_batch_again")
COUNTERS = ("packed422_bgra_wide", "packed422_bgra_bytes", "packed422_bgra_list_frames_wide", "packed422_bgra_list_frames_bytes")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def make_sets(w, h, n, fmt):
    """Two sets of n tight packed frames: luma (byte 0 of a pixel for YUY2, byte 1 for UYVY) in a 64-value band, chroma full range."""
    sets = []
    for k in range(2):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED3500 + w + k)
        x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
        x[:, :, fmt - 2::2] = x[:, :, fmt - 2::2] // 4 + 64 + 16 * k
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


def stat_delta(ctx, before):
    return [ctx.get_stat(k) - a for k, a in zip(COUNTERS, before)]


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        out_a = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda:0")
        out_l = torch.empty_like(out_a)
        pool_out = [torch.zeros((4 * w * h + 256 * (f % 3),), dtype=torch.uint8, device="cuda:0") for f in range(n)]
        for fname, fmt in FMTS:
            sets = make_sets(w, h, n, fmt)
            # a capture device's buffer pool: per frame a separately allocated buffer, filled from the tight sets
            pools_in = [[torch.empty((2 * w * h + 256 * ((f + 1) % 3),), dtype=torch.uint8, device="cuda:0") for f in range(n)]
                        for _ in range(2)]
            for k in range(2):
                for f in range(n):
                    pools_in[k][f][: 2 * w * h].copy_(sets[k][f].reshape(-1))
            on_batch = [([sets[k][f].data_ptr() for f in range(n)], [out_l[f].data_ptr() for f in range(n)]) for k in range(2)]
            on_pools = [([pools_in[k][f].data_ptr() for f in range(n)], [pool_out[f].data_ptr() for f in range(n)]) for k in range(2)]
            for op in OPS:
                eq = op == "equalize"

                def batch(k):
                    if eq:
                        ctx.equalize_hist_packed422_to_bgra_batch_dev(sets[k], out_a, w, h, n, fmt, ORDER_BGR, stream=s)
                    else:
                        ctx.clahe_packed422_to_bgra_batch_dev(sets[k], out_a, w, h, n, fmt, ORDER_BGR, *CLAHE, stream=s)

                def lst(entries, k):
                    ins, outs = entries[k]
                    if eq:
                        ctx.equalize_hist_packed422_to_bgra_frames(ins, outs, w, h, fmt, ORDER_BGR, stream=s)
                    else:
                        ctx.clahe_packed422_to_bgra_frames(ins, outs, w, h, fmt, ORDER_BGR, *CLAHE, stream=s)

                legs = {"a_batch": batch, "l_list_on_batch": lambda k: lst(on_batch, k), "lp_list_on_pools": lambda k: lst(on_pools, k),
                        "a2_batch_again": batch}
                names = list(LIST_LEGS)
                stat0 = [ctx.get_stat(k) for k in COUNTERS]
                for name in names:                                   # the legs agree before anything is timed
                    legs[name](0)
                torch.cuda.synchronize()
                assert stat_delta(ctx, stat0) == [2, 0, 2 * n, 0], ("a leg left the wide store path", stat_delta(ctx, stat0))
                assert torch.equal(out_l, out_a), ("(l) and (a) differ", w, h, fname, op)
                for f in range(n):
                    assert torch.equal(pool_out[f][: 4 * w * h], out_a[f].reshape(-1)), ("(lp) and (a) differ", f, w, h, fname, op)
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "in": fname, "order": "BGR", "calls": args.calls,
                       "chunk_frames": {"list": 128, "batch": 65535}}
                res.update(timed(legs, names, args, stream))
                med = {k: res[k]["median_us"] for k in names}
                for k in names:
                    res[k]["frames_per_s"] = n / (med[k] * 1e-6)
                res["spread"] = abs(med["a_batch"] / med["a2_batch_again"] - 1.0)
                res["list_on_batch_rate_over_batch_rate"] = med["a_batch"] / med["l_list_on_batch"]
                res["list_on_pools_rate_over_batch_rate"] = med["a_batch"] / med["lp_list_on_pools"]
                rows.append(res)
                print(json.dumps(res), flush=True)
            del sets, pools_in, on_batch, on_pools
        del out_a, out_l, pool_out
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r36_packed422_to_bgra_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# Packed 4:2:2 in, equalized BGRA out: the list form against the batch form", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR; tight rows.  Rates are frames per second.  "
          "(a): mi_*_packed422_to_bgra_batch_dev on a tight batch.  (l): ONE mi_*_packed422_to_bgra_frames_dev call naming the batch's own "
          "addresses.  (lp): ONE list call on pools, every frame and every image its own allocation.  Spread: the two (a) legs of the "
          "same rotation against each other.", "",
          "| frames | op | in | (a) batch | (l) list on a batch | (lp) list on pools | l / a | lp / a | spread |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | {r['in']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LIST_LEGS[:3]) +
                  f" | {r['list_on_batch_rate_over_batch_rate']:.3f} | {r['list_on_pools_rate_over_batch_rate']:.3f} | {r['spread']:.3f} |")
    behind = [(r["width"], r["op"], r["in"], k, round(r[k], 3), round(r["spread"], 3)) for r in rows
              for k in ("list_on_batch_rate_over_batch_rate", "list_on_pools_rate_over_batch_rate") if r[k] < 1.0 - r["spread"]]
    md += ["", "Rows in which a list leg trails the batch form by more than the spread (width, op, in, ratio, value, spread): " +
           (str(behind) if behind else "none") + "."]
    (outdir / "r36_packed422_to_bgra_frames_ab.md").write_text("\n".join(md) + "\n")
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
        out_a = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda:0")
        out_b = torch.empty_like(out_a)
        scratch = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")      # leg (b): the three-channel scratch the size of the video
        out_c = torch.empty_like(scratch)
        alpha = torch.full((n, h, w, 1), 255, dtype=torch.uint8, device="cuda:0")
        for fname, fmt in FMTS:
            sets = make_sets(w, h, n, fmt)
            for op in OPS:
                eq = op == "equalize"

                def new_form(k):
                    if eq:
                        ctx.equalize_hist_packed422_to_bgra_batch_dev(sets[k], out_a, w, h, n, fmt, ORDER_BGR, stream=s)
                    else:
                        ctx.clahe_packed422_to_bgra_batch_dev(sets[k], out_a, w, h, n, fmt, ORDER_BGR, *CLAHE, stream=s)

                def three(k, dst):
                    if eq:
                        ctx.equalize_hist_packed422_to_bgr_batch_dev(sets[k], dst, w, h, n, fmt, ORDER_BGR, stream=s)
                    else:
                        ctx.clahe_packed422_to_bgr_batch_dev(sets[k], dst, w, h, n, fmt, ORDER_BGR, *CLAHE, stream=s)

                def leg_b(k):
                    three(k, scratch)
                    torch.cat((scratch, alpha), dim=3, out=out_b)    # the widen a caller writes today: alpha 255 behind every pixel

                legs = {"a_new": new_form, "b_bgr_then_widen": leg_b, "c_bgr_alone": lambda k: three(k, out_c), "a2_new_again": new_form}
                names = list(LEGS)
                stat0 = [ctx.get_stat(k) for k in COUNTERS]
                for name in names:                                   # the legs agree before anything is timed
                    legs[name](0)
                torch.cuda.synchronize()
                assert stat_delta(ctx, stat0) == [2, 0, 0, 0], ("the new form left the wide store path", stat_delta(ctx, stat0))
                assert torch.equal(out_a, out_b), ("(a) and (b) differ", w, h, fname, op)
                assert torch.equal(out_a[..., :3], out_c), ("(a)[..., :3] and (c) differ", w, h, fname, op)
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "in": fname, "order": "BGR", "calls": args.calls}
                res.update(timed(legs, names, args, stream))
                med = {k: res[k]["median_us"] for k in names}
                for k in names:
                    res[k]["frames_per_s"] = n / (med[k] * 1e-6)
                res["spread"] = abs(med["a_new"] / med["a2_new_again"] - 1.0)
                res["a_rate_over_b_rate"] = med["b_bgr_then_widen"] / med["a_new"]
                res["a_rate_over_c_rate"] = med["c_bgr_alone"] / med["a_new"]
                res["a_bytes_per_s"] = BYTES_PER_PX * w * h * n / (med["a_new"] * 1e-6)
                res["c_bytes_per_s"] = 7.0 * w * h * n / (med["c_bgr_alone"] * 1e-6)
                res["bar_a_beats_b_by_more_than_the_spread"] = bool(res["a_rate_over_b_rate"] > 1.0 + res["spread"])
                rows.append(res)
                print(json.dumps(res), flush=True)
            del sets
        del out_a, out_b, out_c, scratch, alpha
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "warmup": args.warmup, "bar": "(a) beats (b) in every row by more than the run's spread"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r35_packed422_to_bgra_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# Packed 4:2:2 in, equalized BGRA out: the one-call form against the decode-then-widen route it replaces", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR; tight batches.  Rates are frames per second.  "
          "(a): mi_*_packed422_to_bgra_batch_dev.  (b): mi_*_packed422_to_bgr_batch_dev into a scratch batch, then torch.cat with an alpha "
          "plane of 255 into the four-channel batch.  (c): mi_*_packed422_to_bgr_batch_dev alone: a ceiling, not a route (it writes 1 B/px "
          "less).  Spread: the two (a) legs of the same rotation against each other.  TB/s: the whole call on the 8 B/px (a) and 7 B/px (c) "
          "it moves.", "",
          "| frames | op | in | (a) new | (b) BGR form + widen | (c) BGR form alone | a / b | a / c | spread | (a) TB/s | (c) TB/s |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | {r['in']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS[:3]) +
                  f" | {r['a_rate_over_b_rate']:.3f} | {r['a_rate_over_c_rate']:.3f} | {r['spread']:.3f} "
                  f"| {r['a_bytes_per_s'] / 1e12:.2f} | {r['c_bytes_per_s'] / 1e12:.2f} |")
    missed = [(r["width"], r["op"], r["in"], round(r["a_rate_over_b_rate"], 3), round(r["spread"], 3)) for r in rows
              if not r["bar_a_beats_b_by_more_than_the_spread"]]
    md += ["", "Bar, (a) beats (b) by more than the spread: " + ("met in every row" if not missed else "MISSED in " + str(missed)) + "."]
    (outdir / "r35_packed422_to_bgra_ab.md").write_text("\n".join(md) + "\n")
    if missed:
        print("BAR MISSED: the one-call form does not beat the decode-then-widen route by more than the spread in", missed)


if __name__ == "__main__":
    main()
