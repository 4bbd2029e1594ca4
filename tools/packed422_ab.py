"""Packed 4:2:2 frames (mi_*_packed422_batch_dev) against the only route the library offered before them, in ONE process (boxes
differ by several per cent, so the legs are timed interleaved, call by call):
    (A)  torch gathers the luma (x[..., off::2] into a plane), the planar mi_*_u8_batch_dev form, torch writes luma and chroma
         (copied, or 128) into the packed output
    (B)  the packed form on the same frames
    (C)  for orientation only: the planar form alone on the gathered plane (no gather / scatter timed)
64 x 3840x2160 and 256 x 1920x1080 frames per call (1 GiB of packed input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; MI_UV_COPY and MI_UV_FILL128; YUY2, plus one UYVY row.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  Out of place, inputs never change.
Bar: B faster than A in every row (B moves 6 B/px, A at least 9).  B / C is recorded without a bar.
After the timed legs each row runs 30 profiled calls of B and of C (fused 0) and records, per kernel role, bytes moved / p50 time as a
fraction of 8 TB/s for the packed kernel and its planar sibling.
    python tools/packed422_ab.py [--out DIR] [--calls N]   -> DIR/r10_packed422_ab.json and .txt (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, UV_FILL128, FMT_YUY2, FMT_UYVY  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
ROWS = [(op, uv, FMT_YUY2) for op in ("equalize", "clahe") for uv in (UV_COPY, UV_FILL128)] + [("clahe", UV_COPY, FMT_UYVY)]
PEAK = 8.0e12
# bytes per pixel each kernel role moves: (packed, planar)
ROLES = {"equalize": {"hist_partial_kernel": (2, 1), "lut_apply_kernel": (4, 2)},
         "clahe": {"tile_hist_kernel": (2, 1), "clahe_interp_kernel": (4, 2)}}


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def content(n, h, w, seed):
    """Low-contrast luma (D2-like: ~60 populated bins) and random chroma, generated on the device."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
    return x


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
        sets = []
        for k in range(2):
            x = content(n, h, w, 0x5EED0000 + w + k)
            for off in (0, 1):                                    # both byte lanes low-contrast, so either may be the luma
                lane = x[:, :, off::2]
                lane.copy_(lane // 4 + 64 + 16 * k)
            sets.append(x)
        out = torch.empty_like(sets[0])
        y = torch.empty((n, h, w), dtype=torch.uint8, device="cuda:0")
        yo = torch.empty_like(y)
        for op, uv, fmt in ROWS:
            off = fmt - 2

            def planar():
                if op == "equalize":
                    ctx.equalize_hist_batch_dev(y, yo, w, h, n, stream=s)
                else:
                    ctx.clahe_batch_dev(y, yo, w, h, n, 2.0, 8, 8, stream=s)

            def leg_a(x):
                y.copy_(x[:, :, off::2])
                planar()
                out[:, :, off::2].copy_(yo)
                if uv == UV_COPY:
                    out[:, :, 1 - off::2].copy_(x[:, :, 1 - off::2])
                else:
                    out[:, :, 1 - off::2].fill_(128)

            def leg_b(x):
                if op == "equalize":
                    ctx.equalize_hist_packed422_batch_dev(x, out, w, h, n, fmt, uv, stream=s)
                else:
                    ctx.clahe_packed422_batch_dev(x, out, w, h, n, fmt, uv, 2.0, 8, 8, stream=s)

            def leg_c(x):
                planar()

            legs = {"A_gather_planar_scatter": leg_a, "B_packed": leg_b, "C_planar_only": leg_c}
            names = list(legs)
            times = {k: [] for k in names}
            for it in range(args.warmup + args.calls):
                x = sets[it & 1]
                order = names[it % len(names):] + names[: it % len(names)]
                for name in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    legs[name](x)
                    e1.record(stream)
                    if it >= args.warmup:
                        times[name].append((e0, e1))
                if it % 20 == 19:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "uv": "copy" if uv == UV_COPY else "fill128",
                   "format": "YUY2" if fmt == FMT_YUY2 else "UYVY", "calls": args.calls}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            res["B_over_A"] = res["B_packed"]["median_us"] / res["A_gather_planar_scatter"]["median_us"]
            res["C_over_B_frame_rate_fraction"] = res["C_planar_only"]["median_us"] / res["B_packed"]["median_us"]
            # the library's own kernel times: packed kernels, then their planar siblings (three-kernel equalizeHist)
            px = float(w) * h * n
            ctx.set_profiling(1)
            frac = {}
            for leg, idx in ((leg_b, 0), (leg_c, 1)):
                ctx.set_option("fused", 0)
                ctx.profile_read(reset=True)
                for it in range(30):
                    leg(sets[it & 1])
                torch.cuda.synchronize()
                prof = ctx.profile_read(reset=True)
                ctx.set_option("fused", 1)
                for role, bpp in ROLES[op].items():
                    p50 = prof[role]["p50_ms"] * 1e-3
                    frac.setdefault(role, {})["packed" if idx == 0 else "planar"] = {
                        "p50_us": p50 * 1e6, "fraction_of_8TBps": bpp[idx] * px / p50 / PEAK if p50 > 0 else 0.0}
            ctx.set_profiling(0)
            res["kernels"] = frac
            rows.append(res)
            line = (f"{w}x{h} x{n:3d} {op:8s} {res['uv']:7s} {res['format']} " +
                    "  ".join(f"{k[0]} {res[k]['median_us']:8.1f} us [{res[k]['p10_us']:.1f} {res[k]['p90_us']:.1f}]" for k in names) +
                    f"  | B/A {res['B_over_A']:.3f}  B rate / C rate {res['C_over_B_frame_rate_fraction']:.3f}  | " +
                    "  ".join(f"{role} packed {v['packed']['fraction_of_8TBps']:.2f} planar {v['planar']['fraction_of_8TBps']:.2f}"
                              for role, v in frac.items()))
            print(line, flush=True)
            lines.append(line)
        del sets, out, y, yo
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": 2.0, "tiles": [8, 8]},
            "bar": "B_over_A < 1 in every row", "peak_bytes_per_s": PEAK}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r10_packed422_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (outdir / "r10_packed422_ab.txt").write_text(__doc__.split("\n    python")[0] + "\n\n" + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")
    ctx.close()
    bad = [r for r in rows if r["B_over_A"] >= 1.0]
    if bad:
        print("BAR MISSED: B is not faster than A in", [(r["width"], r["op"], r["uv"], r["format"]) for r in bad])
        sys.exit(1)


if __name__ == "__main__":
    main()
