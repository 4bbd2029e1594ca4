"""NV12 in, interleaved BGR out in the equalizing pass (mi_*_nv12_to_bgr_batch_dev) against the two calls a caller had before it, in ONE
process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (A)  the one-pass form: NV12 frames in, BGR images out (5.5 B/px: Y read twice, UV once, 3 B/px written)
    (B)  mi_*_nv12_batch_dev(MI_UV_COPY) into an NV12 batch, then mi_cvt_color_420_u8_batch_dev(MI_COLOR_YUV2BGR_NV12) (4 + 4.5 B/px)
    (A2) leg A a second time in the same rotation: the ratio of the two A medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight NV12 frames per call (760 MiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR.  Low-contrast luma, random chroma.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  A and B agree byte for byte before anything is timed.
Bar: at 64 x 4K, A is not slower than B beyond the spread (B time / A time >= 1 - spread); the 1080p rows are recorded.
After the timed legs each row runs 30 profiled calls of A and of B and records the p50 time of each kernel role.
    python tools/nv12_to_bgr_ab.py [--out DIR] [--calls N]   -> DIR/r15_nv12_to_bgr_ab.json and .txt (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR, COLOR_YUV2BGR_NV12  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
ROLES = ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel", "tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel",
         "equalize_fused_kernel", "fused_finish_kernel", "color_kernel")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


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
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED1500 + w + k)
            x = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0", generator=g)
            y = x[:, :h, :]
            y.copy_(y // 4 + 64 + 16 * k)                        # low-contrast luma (~60 populated bins), random chroma
            sets.append(x)
        mid = torch.empty_like(sets[0])
        bgr_a = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")
        bgr_b = torch.empty_like(bgr_a)
        for op in OPS:
            def leg_a(x):
                if op == "equalize":
                    ctx.equalize_hist_nv12_to_bgr_batch_dev(x, None, bgr_a, w, h, n, ORDER_BGR, stream=s)
                else:
                    ctx.clahe_nv12_to_bgr_batch_dev(x, None, bgr_a, w, h, n, ORDER_BGR, *CLAHE, stream=s)

            def leg_b(x):
                if op == "equalize":
                    ctx.equalize_hist_nv12_batch_dev(x, mid, w, h, n, UV_COPY, stream=s)
                else:
                    ctx.clahe_nv12_batch_dev(x, mid, w, h, n, UV_COPY, *CLAHE, stream=s)
                ctx.cvt_color_420_batch_dev(mid, bgr_b, w, h, n, COLOR_YUV2BGR_NV12, stream=s)

            legs = {"A_one_pass": leg_a, "B_two_calls": leg_b, "A2_one_pass_again": leg_a}
            names = list(legs)
            # the legs agree before anything is timed, and A took the one-pass kernels
            one0 = ctx.get_stat("nv12_bgr_onepass")
            leg_a(sets[0])
            leg_b(sets[0])
            torch.cuda.synchronize()
            assert torch.equal(bgr_a, bgr_b), ("A and B differ", w, h, op)
            assert ctx.get_stat("nv12_bgr_onepass") == one0 + 1, "leg A did not take the one-pass path"
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "calls": args.calls}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            a, a2, b = (res[k]["median_us"] for k in ("A_one_pass", "A2_one_pass_again", "B_two_calls"))
            res["spread"] = abs(a / a2 - 1.0)
            res["B_time_over_A_time"] = b / a
            res["A_bytes_per_s"] = 5.5 * w * h * n / (a * 1e-6)
            # the library's own kernel times, by role
            ctx.set_profiling(1)
            kern = {}
            for leg, tag in ((leg_a, "A"), (leg_b, "B")):
                ctx.profile_read(reset=True)
                for it in range(30):
                    leg(sets[it & 1])
                torch.cuda.synchronize()
                prof = ctx.profile_read(reset=True)
                for role in ROLES:
                    if prof[role]["launches"]:
                        kern.setdefault(role, {})[tag + "_p50_us"] = prof[role]["p50_ms"] * 1e3
            ctx.set_profiling(0)
            res["kernels"] = kern
            rows.append(res)
            line = (f"{w}x{h} x{n:3d} {op:8s} " +
                    "  ".join(f"{k.split('_')[0]} {res[k]['median_us']:8.1f} us [{res[k]['p10_us']:.1f} {res[k]['p90_us']:.1f}]" for k in names) +
                    f"  | B time / A time {res['B_time_over_A_time']:.3f}  spread {res['spread']:.3f}  A {res['A_bytes_per_s'] / 1e12:.2f} TB/s of 5.5 B/px  | " +
                    "  ".join(f"{role} A {v.get('A_p50_us', 0):.1f} B {v.get('B_p50_us', 0):.1f} us" for role, v in kern.items()))
            print(line, flush=True)
            lines.append(line)
        del sets, mid, bgr_a, bgr_b
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "bar": "B_time_over_A_time >= 1 - spread in the 64 x 3840x2160 rows"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r15_nv12_to_bgr_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (outdir / "r15_nv12_to_bgr_ab.txt").write_text(__doc__.split("\n    python")[0] + "\n\n" + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")
    bad = [(r["width"], r["op"]) for r in rows if r["width"] == 3840 and r["B_time_over_A_time"] < 1.0 - r["spread"]]
    if bad:
        print("BAR MISSED in", bad)
        sys.exit(1)


if __name__ == "__main__":
    main()
