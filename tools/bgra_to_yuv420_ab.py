"""Four-channel BGRA in, equalized 4:2:0 (I420 and NV12) out in one call (mi_*_bgra_to_yuv420_batch_dev) against what a caller with a
four-byte-per-pixel surface had to write before it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved,
call by call):
    (a)  the new form on the BGRA batch (equalizeHist 7.5 B/px, CLAHE 8.5)
    (b)  what a caller had before: torch `img[..., :3].contiguous()` into a scratch batch (4 B/px read, 3 written), then
         mi_*_bgr_to_yuv420_batch_dev on the scratch (6.5 / 7.5 B/px): 14.5 / 15.5 B/px
    (c)  mi_*_bgr_to_yuv420_batch_dev on three-channel images made beforehand: a ceiling, not a route -- nobody hands such a caller
         three-byte pixels
    (a2) leg (a) a second time in the same rotation: the ratio of the two medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight BGRA images per call (2 GiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; tight I420 and tight NV12 out; MI_ORDER_BGR, MI_UV_COPY.  Low-contrast pixels
(every colour channel in a 64-value band), the fourth byte full-range random.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  (a), (b) and (c) agree byte for byte before anything is timed.
Bar: (a) beats (b) in every row by more than the run's spread.  The byte counts (7.5 against 14.5, 8.5 against 15.5) are a reason to
expect 1.7 - 1.9 x, not a result.  After the timed legs each row runs 30 profiled calls of (a) and (c) and records the p50 time of the
conversion kernel (MI_K_COLOR) and its bytes per second on the 5.5 B/px (a) and 4.5 B/px (c) stage 1 moves: a finding, not a gate.
    python tools/bgra_to_yuv420_ab.py [--out DIR] [--calls N]   -> DIR/r31_bgra_to_yuv420_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_bgra_to_yuv420_frames_dev) against leg (a) under the same protocol:
    (a)   the batch form, tight; (a2) the same a second time in the rotation: the spread
    (l)   ONE list call whose entries are the addresses of a tight batch like (a)'s: the list kernels and the 64-frame chunk alone
    (lp)  ONE list call on POOLS: every image its own allocation and every plane its own allocation (tight rows), of sizes of their own
          so that no allocator lays them out at one stride
(l) and (lp) hold the bytes of (a) before anything is timed.  No bar: a row in which a list leg trails (a) by more than the spread is
reported as a finding.
    python tools/bgra_to_yuv420_ab.py --list [--out DIR] [--calls N]   -> DIR/r32_bgra_to_yuv420_frames_ab.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR, CHROMA_PLANAR, CHROMA_INTERLEAVED, Yuv420Planes, BgrYuv420FrameDev  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
FMTS = ("i420", "nv12")
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = {"equalize": 7.5, "clahe": 8.5}
OLD_BYTES_PER_PX = {"equalize": 14.5, "clahe": 15.5}
LEGS = ("a_new", "b_slice_then_bgr", "c_bgr_premade", "a2_new_again")
LIST_LEGS = ("a_batch", "l_list_on_batch", "lp_list_on_pools", "a2_batch_again")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def make_sets(w, h, n):
    """Two sets of n BGRA images: colour channels in a 64-value band (~60 populated luma bins), the fourth byte full range."""
    sets = []
    for k in range(2):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED3100 + w + k)
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


def planes_of(t, w, h, fmt):
    return Yuv420Planes.i420(t, w, h) if fmt == "i420" else Yuv420Planes.nv12(t, w, h)


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        ysz, q, frame = w * h, w * h // 4, w * h * 3 // 2
        sets = make_sets(w, h, n)
        pools_in = [[torch.empty((4 * ysz + 256 * (f % 3),), dtype=torch.uint8, device="cuda:0") for f in range(n)] for _ in range(2)]
        for k in range(2):
            for f in range(n):
                pools_in[k][f][: 4 * ysz].copy_(sets[k][f].reshape(-1))
        out_a = torch.empty((n, frame), dtype=torch.uint8, device="cuda:0")
        out_l = torch.empty_like(out_a)
        for fmt in FMTS:
            planar = fmt == "i420"
            chroma = CHROMA_PLANAR if planar else CHROMA_INTERLEAVED
            cp = w // 2 if planar else w
            # an encoder's frame pool: per frame separately allocated planes (Y, U, V or Y, UV)
            sizes = (ysz, q, q) if planar else (ysz, 2 * q)
            pool_out = [tuple(torch.zeros((sz + 256 * ((f + i) % 3),), dtype=torch.uint8, device="cuda:0") for i, sz in enumerate(sizes))
                        for f in range(n)]
            bl = out_l.data_ptr()

            def entry(i, y, c0, c1):
                return BgrYuv420FrameDev.of(i, y, c0, c1 if planar else None)
            on_batch = [(BgrYuv420FrameDev * n)(*[entry(sets[k][f].data_ptr(), bl + f * frame, bl + f * frame + ysz, bl + f * frame + ysz + q)
                                                   for f in range(n)]) for k in range(2)]
            on_pools = [(BgrYuv420FrameDev * n)(*[entry(pools_in[k][f].data_ptr(), pool_out[f][0].data_ptr(), pool_out[f][1].data_ptr(),
                                                        pool_out[f][2].data_ptr() if planar else None) for f in range(n)]) for k in range(2)]
            tight = planes_of(out_a, w, h, fmt)
            for op in OPS:
                eq = op == "equalize"

                def batch(k):
                    if eq:
                        ctx.equalize_hist_bgra_to_yuv420_batch_dev(sets[k], tight, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgra_to_yuv420_batch_dev(sets[k], tight, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

                def lst(entries, k):
                    a = (entries[k], w, h, 4 * w, w, cp, chroma, ORDER_BGR, UV_COPY)
                    if eq:
                        ctx.equalize_hist_bgra_to_yuv420_frames_dev(*a, stream=s)
                    else:
                        ctx.clahe_bgra_to_yuv420_frames_dev(*a, *CLAHE, stream=s)

                legs = {"a_batch": batch, "l_list_on_batch": lambda k: lst(on_batch, k), "lp_list_on_pools": lambda k: lst(on_pools, k),
                        "a2_batch_again": batch}
                names = list(LIST_LEGS)
                stats = ("bgra_yuv420_vec", "bgra_yuv420_list_frames_vec", "bgra_yuv420_bytes", "bgra_yuv420_list_frames_bytes")
                stat0 = [ctx.get_stat(k) for k in stats]
                for name in names:                                   # the legs agree before anything is timed
                    legs[name](0)
                torch.cuda.synchronize()
                assert [ctx.get_stat(k) - a for k, a in zip(stats, stat0)] == [2, 2 * n, 0, 0], "a leg left the 16 x 2 groups"
                assert torch.equal(out_l, out_a), ("(l) and (a) differ", w, h, fmt, op)
                for f in range(n):
                    got = torch.cat([p[:sz] for p, sz in zip(pool_out[f], sizes)])
                    assert torch.equal(got, out_a[f]), ("(lp) and (a) differ", f, w, h, fmt, op)
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "out": fmt, "order": "BGR", "uv_mode": "COPY",
                       "calls": args.calls, "chunk_frames": {"list": 64, "batch": 256}}
                res.update(timed(legs, names, args, stream))
                med = {k: res[k]["median_us"] for k in names}
                for k in names:
                    res[k]["frames_per_s"] = n / (med[k] * 1e-6)
                res["spread"] = abs(med["a_batch"] / med["a2_batch_again"] - 1.0)
                res["list_on_batch_rate_over_batch_rate"] = med["a_batch"] / med["l_list_on_batch"]
                res["list_on_pools_rate_over_batch_rate"] = med["a_batch"] / med["lp_list_on_pools"]
                rows.append(res)
                print(json.dumps(res), flush=True)
            del pool_out, on_batch, on_pools
        del sets, pools_in, out_a, out_l
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r32_bgra_to_yuv420_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGRA in, equalized 4:2:0 out: the list form against the batch form", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY; tight rows.  Rates are frames per second.  "
          "(a): mi_*_bgra_to_yuv420_batch_dev on a tight batch.  (l): ONE mi_*_bgra_to_yuv420_frames_dev call naming the frames of such a "
          "tight batch.  (lp): ONE list call on pools, every image and every plane its own allocation.  Spread: the two (a) legs of the "
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
    (outdir / "r32_bgra_to_yuv420_frames_ab.md").write_text("\n".join(md) + "\n")
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
        frame = w * h * 3 // 2
        sets = make_sets(w, h, n)
        premade = [x[..., :3].contiguous() for x in sets]           # leg (c): three-channel images nobody hands over
        scratch = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")      # leg (b): the scratch pool the size of the video
        out_a = torch.empty((n, frame), dtype=torch.uint8, device="cuda:0")
        out_b, out_c = torch.empty_like(out_a), torch.empty_like(out_a)
        for fmt in FMTS:
            pa, pb, pc = (planes_of(t, w, h, fmt) for t in (out_a, out_b, out_c))
            for op in OPS:
                eq = op == "equalize"

                def new_form(k):
                    if eq:
                        ctx.equalize_hist_bgra_to_yuv420_batch_dev(sets[k], pa, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgra_to_yuv420_batch_dev(sets[k], pa, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

                def three(x, dst):
                    if eq:
                        ctx.equalize_hist_bgr_to_yuv420_batch_dev(x, dst, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgr_to_yuv420_batch_dev(x, dst, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

                def leg_b(k):
                    scratch.copy_(sets[k][..., :3])                  # img[..., :3].contiguous() into the scratch pool
                    three(scratch, pb)

                legs = {"a_new": new_form, "b_slice_then_bgr": leg_b, "c_bgr_premade": lambda k: three(premade[k], pc), "a2_new_again": new_form}
                names = list(LEGS)
                vec0 = ctx.get_stat("bgra_yuv420_vec")
                for name in names:                                   # the legs agree before anything is timed
                    legs[name](0)
                torch.cuda.synchronize()
                assert ctx.get_stat("bgra_yuv420_vec") == vec0 + 2, "a leg of the new form left the 16 x 2 groups"
                assert torch.equal(out_a, out_b), ("(a) and (b) differ", w, h, fmt, op)
                assert torch.equal(out_a, out_c), ("(a) and (c) differ", w, h, fmt, op)
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "out": fmt, "order": "BGR", "uv_mode": "COPY",
                       "calls": args.calls}
                res.update(timed(legs, names, args, stream))
                med = {k: res[k]["median_us"] for k in names}
                for k in names:
                    res[k]["frames_per_s"] = n / (med[k] * 1e-6)
                res["spread"] = abs(med["a_new"] / med["a2_new_again"] - 1.0)
                res["a_rate_over_b_rate"] = med["b_slice_then_bgr"] / med["a_new"]
                res["a_rate_over_c_rate"] = med["c_bgr_premade"] / med["a_new"]
                res["a_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (med["a_new"] * 1e-6)
                res["b_bytes_per_s"] = OLD_BYTES_PER_PX[op] * w * h * n / (med["b_slice_then_bgr"] * 1e-6)
                res["bar_a_beats_b_by_more_than_the_spread"] = bool(res["a_rate_over_b_rate"] > 1.0 + res["spread"])
                ctx.set_profiling(1)
                ka, kc = color_kernel_p50_us(ctx, new_form), color_kernel_p50_us(ctx, legs["c_bgr_premade"])
                ctx.set_profiling(0)
                res["kernels"] = {"a_color_kernel_p50_us": ka, "c_color_kernel_p50_us": kc,
                                  "a_stage1_bytes_per_s": 5.5 * w * h * n / (ka * 1e-6), "c_stage1_bytes_per_s": 4.5 * w * h * n / (kc * 1e-6)}
                res["kernels"]["a_over_c_stage1_bytes_per_s"] = res["kernels"]["a_stage1_bytes_per_s"] / res["kernels"]["c_stage1_bytes_per_s"]
                rows.append(res)
                print(json.dumps(res), flush=True)
        del sets, premade, scratch, out_a, out_b, out_c
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bar": "(a) beats (b) in every row by more than the run's spread"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r31_bgra_to_yuv420_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGRA in, equalized 4:2:0 out: the one-call form against the slice-and-copy route it replaces", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY; tight batches.  Rates are frames per second.  "
          "(a): mi_*_bgra_to_yuv420_batch_dev.  (b): torch `img[..., :3]` copied into a scratch batch, then mi_*_bgr_to_yuv420_batch_dev.  "
          "(c): mi_*_bgr_to_yuv420_batch_dev on three-channel images made beforehand: a ceiling, not a route.  Spread: the two (a) legs of "
          "the same rotation against each other.  Stage 1: p50 of the conversion kernel (MI_K_COLOR) from 30 profiled calls, as TB/s on "
          "the 5.5 B/px (a) and 4.5 B/px (c) it moves.", "",
          "| frames | op | out | (a) new | (b) slice + BGR form | (c) BGR form, pre-made | a / b | a / c | spread | stage 1 (a) TB/s | stage 1 (c) TB/s |",
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
    (outdir / "r31_bgra_to_yuv420_ab.md").write_text("\n".join(md) + "\n")
    if missed:
        print("BAR MISSED: the one-call form does not beat the slice-and-copy route by more than the spread in", missed)
    if behind:
        print("FINDING: stage 1 falls behind its three-channel sibling's bytes per second in", behind)


if __name__ == "__main__":
    main()
