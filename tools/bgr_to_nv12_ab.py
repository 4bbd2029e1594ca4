"""Interleaved BGR in, equalized NV12 out in one call (mi_*_bgr_to_nv12_batch_dev) against the composition a caller had to write before
it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (A)  the one-call form: BGR images in, tight NV12 frames out (equalizeHist 6.5 B/px: 3 read and 1.5 written by the conversion that
         counts the luma, 1 read and 1 written by the in-place map; CLAHE 7.5: 4.5, then the planar CLAHE in place on Y)
    (B)  mi_cvt_color_420_u8_batch_dev(MI_COLOR_BGR2YUV_I420) into a tight I420 batch, a torch interleave of its U and V planes into
         the chroma half of the same frames (torch.stack into a preallocated buffer, one copy back: the Y plane of an I420 frame
         already lies where an NV12 frame has it), then mi_*_nv12_batch_dev in place with MI_UV_COPY
    (A2) leg A a second time in the same rotation: the ratio of the two A medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight BGR images per call (1.5 GiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Low-contrast pixels (every channel in a 64-value band).
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  A and B agree byte for byte before anything is timed.
No bar: 6.5 B/px is a reason to expect A ahead of B, not a result.  A row in which A is slower than B by more than the spread is
reported as a finding.  After the timed legs each row runs 30 profiled calls of A and of B and records the p50 time of each kernel role.
    python tools/bgr_to_nv12_ab.py [--out DIR] [--calls N]   -> DIR/r17_bgr_to_nv12_ab.json and .md (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR, COLOR_BGR2YUV_I420  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = {"equalize": 6.5, "clahe": 7.5}
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
    rows = []
    for w, h, n in CASES:
        ysz, q = w * h, w * h // 4
        sets = []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED1700 + w + k)
            x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda:0", generator=g)
            x.copy_(x // 4 + 64 + 16 * k)                        # low contrast: ~60 populated luma bins
            sets.append(x)
        nv12_a = torch.empty((n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0")
        mid = torch.empty_like(nv12_a)                          # leg B: the I420 batch, turned into NV12 where it lies
        uv_tmp = torch.empty((n, q, 2), dtype=torch.uint8, device="cuda:0")
        for op in OPS:
            def leg_a(x):
                if op == "equalize":
                    ctx.equalize_hist_bgr_to_nv12_batch_dev(x, nv12_a, None, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                else:
                    ctx.clahe_bgr_to_nv12_batch_dev(x, nv12_a, None, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

            def leg_b(x):
                ctx.cvt_color_420_batch_dev(x, mid, w, h, n, COLOR_BGR2YUV_I420, stream=s)
                torch.stack((mid[:, ysz: ysz + q], mid[:, ysz + q:]), dim=2, out=uv_tmp)
                mid[:, ysz:].copy_(uv_tmp.view(n, 2 * q))
                if op == "equalize":
                    ctx.equalize_hist_nv12_batch_dev(mid, mid, w, h, n, UV_COPY, stream=s)
                else:
                    ctx.clahe_nv12_batch_dev(mid, mid, w, h, n, UV_COPY, *CLAHE, stream=s)

            legs = {"A_one_call": leg_a, "B_composition": leg_b, "A2_one_call_again": leg_a}
            names = list(legs)
            leg_a(sets[0])                                       # the legs agree before anything is timed
            leg_b(sets[0])
            torch.cuda.synchronize()
            assert torch.equal(nv12_a, mid), ("A and B differ", w, h, op)
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "uv_mode": "COPY", "calls": args.calls}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            a, a2, b = (res[k]["median_us"] for k in ("A_one_call", "A2_one_call_again", "B_composition"))
            res["spread"] = abs(a / a2 - 1.0)
            res["A_rate_over_B_rate"] = b / a
            res["A_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (a * 1e-6)
            # the library's own kernel times, by role (leg B's torch kernels are not the library's: they show in the leg's time only)
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
            print(json.dumps(res), flush=True)
        del sets, nv12_a, mid, uv_tmp
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r17_bgr_to_nv12_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGR in, equalized NV12 out: the one-call form against the composition it replaces", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Rates are frames per second.  A: "
          "mi_*_bgr_to_nv12_batch_dev.  B: mi_cvt_color_420_u8_batch_dev(BGR2YUV_I420), a torch interleave of U and V in the same "
          "frames, mi_*_nv12_batch_dev in place.  Spread: the two A legs of the same rotation against each other.", "",
          "| frames | op | A one call | B composition | A / B | spread | A bytes/s at its B/px | conversion kernel of A (p50) |",
          "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in ("A_one_call", "B_composition")) +
                  f" | {r['A_rate_over_B_rate']:.3f} | {r['spread']:.3f} | {r['A_bytes_per_s'] / 1e12:.2f} TB/s of {BYTES_PER_PX[r['op']]} "
                  f"| {r['kernels'].get('color_kernel', {}).get('A_p50_us', 0):.0f} us |")
    slow = [(r["width"], r["op"], round(r["A_rate_over_B_rate"], 3)) for r in rows if r["A_rate_over_B_rate"] < 1.0 - r["spread"]]
    md += ["", "Rows in which the one-call form is slower than the composition by more than the spread: " + (str(slow) if slow else "none") + "."]
    (outdir / "r17_bgr_to_nv12_ab.md").write_text("\n".join(md) + "\n")
    if slow:
        print("FINDING: the one-call form is slower than the composition in", slow)


if __name__ == "__main__":
    main()
