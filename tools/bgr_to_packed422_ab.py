"""Interleaved BGR in, equalized packed 4:2:2 (YUY2 / UYVY) out in one call (mi_*_bgr_to_packed422_batch_dev) against what a caller had
before it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (a)  the new form on a tight packed batch (equalizeHist 9 B/px, CLAHE 11)
    (b)  what a caller has without it: mi_*_bgr_to_nv12_batch_dev into a tight scratch NV12 batch (6.5 / 7.5 B/px), then a torch scatter
         of Y and of the row-repeated UV plane into packed frames (four strided copies: 3.5 B/px read, 2 written, the frame touched four
         times).  NOT the same pixels: NV12 has dropped every second chroma row, so B's odd-row chroma is the row above's, where (a)
         computes every row's own.  The luma and the even-row chroma agree byte for byte, which is checked before anything is timed.
    (c)  mi_*_packed422_batch_dev with MI_UV_COPY in place on an already packed batch: stage 2 alone plus its histogram launch -- a
         floor for (a), not a route (nothing has converted the images)
    (a2) leg (a) a second time in the same rotation: the ratio of the two medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight BGR images per call (1.5 GiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); YUY2 and UYVY; equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Low-contrast pixels (every channel in
a 64-value band).
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.
No bar: (a) moves fewer bytes than (b) in fewer launches, so (a) is expected ahead.  A row in which (a) is behind (b) by more than the
spread is reported as a finding.  After the timed legs each row runs 30 profiled calls of (a), of the library call of (b) and of (c) and
records every kernel's launches per call and p50 time, and the bytes per second of stage 1 (MI_K_COLOR: 5 B/px here, 4.5 B/px in
mi_*_bgr_to_nv12_batch_dev) from the same run.
    python tools/bgr_to_packed422_ab.py [--out DIR] [--calls N]   -> DIR/r27_bgr_to_packed422_ab.json and .md (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR, FMT_YUY2, FMT_UYVY  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
FMTS = (("YUY2", FMT_YUY2), ("UYVY", FMT_UYVY))
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = {"equalize": 9.0, "clahe": 11.0}
LEGS = ("a_new_form", "b_via_nv12_and_torch", "c_packed_in_place", "a2_new_form_again")


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
        ysz = w * h
        sets = []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2700 + w + k)
            x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda:0", generator=g)
            x.copy_(x // 4 + 64 + 16 * k)                        # low contrast: ~60 populated luma bins
            sets.append(x)
        out_a = torch.empty((n, h, w // 2, 4), dtype=torch.uint8, device="cuda:0")
        out_b = torch.empty_like(out_a)
        out_c = torch.empty_like(out_a)                          # leg (c): an already packed batch, mapped in place
        scratch = torch.empty((n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0")       # leg (b): the NV12 batch in between
        y_b = scratch[:, :ysz].view(n, h, w)
        uv_b = scratch[:, ysz:].view(n, h // 2, w // 2, 2)
        for fname, fmt in FMTS:
            y0, y1, ui, vi = (0, 2, 1, 3) if fmt == FMT_YUY2 else (1, 3, 0, 2)
            for op in OPS:
                eq = op == "equalize"

                def new_form(x):
                    if eq:
                        ctx.equalize_hist_bgr_to_packed422_batch_dev(x, out_a, w, h, n, ORDER_BGR, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgr_to_packed422_batch_dev(x, out_a, w, h, n, ORDER_BGR, fmt, UV_COPY, *CLAHE, stream=s)

                def to_nv12(x):
                    if eq:
                        ctx.equalize_hist_bgr_to_nv12_batch_dev(x, scratch, None, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgr_to_nv12_batch_dev(x, scratch, None, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

                def leg_b(x):
                    to_nv12(x)
                    out_b[..., y0] = y_b[:, :, 0::2]
                    out_b[..., y1] = y_b[:, :, 1::2]
                    ob = out_b.view(n, h // 2, 2, w // 2, 4)
                    ob[..., ui] = uv_b[:, :, None, :, 0]         # every UV row goes to two packed rows
                    ob[..., vi] = uv_b[:, :, None, :, 1]

                def leg_c(x):
                    if eq:
                        ctx.equalize_hist_packed422_batch_dev(out_c, out_c, w, h, n, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_packed422_batch_dev(out_c, out_c, w, h, n, fmt, UV_COPY, *CLAHE, stream=s)

                legs = {"a_new_form": new_form, "b_via_nv12_and_torch": leg_b, "c_packed_in_place": leg_c, "a2_new_form_again": new_form}
                names = list(LEGS)
                vec0 = ctx.get_stat("bgr_packed422_vec")
                new_form(sets[0])                                # what agrees between (a) and (b) agrees before anything is timed
                leg_b(sets[0])
                torch.cuda.synchronize()
                assert ctx.get_stat("bgr_packed422_vec") == vec0 + 1, "the new form left the 16-pixel groups"
                assert torch.equal(out_a[..., y0], out_b[..., y0]) and torch.equal(out_a[..., y1], out_b[..., y1]), ("luma of (a) and (b)", w, op)
                assert torch.equal(out_a[:, 0::2, :, ui], out_b[:, 0::2, :, ui]) and torch.equal(out_a[:, 0::2, :, vi], out_b[:, 0::2, :, vi]), \
                    ("even-row chroma of (a) and (b)", w, op)
                odd_differs = float((out_a[:, 1::2, :, ui] != out_b[:, 1::2, :, ui]).float().mean())
                out_c.copy_(out_a)
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
                res = {"width": w, "height": h, "frames_per_call": n, "format": fname, "op": op, "order": "BGR", "uv_mode": "COPY",
                       "calls": args.calls, "odd_row_u_bytes_of_b_that_differ_from_a": odd_differs}
                for name, ev in times.items():
                    ms = [a.elapsed_time(b) for a, b in ev]
                    res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                                 "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
                med = {k: res[k]["median_us"] for k in names}
                res["spread"] = abs(med["a_new_form"] / med["a2_new_form_again"] - 1.0)
                res["a_rate_over_b_rate"] = med["b_via_nv12_and_torch"] / med["a_new_form"]
                res["a_rate_over_c_rate"] = med["c_packed_in_place"] / med["a_new_form"]
                res["a_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (med["a_new_form"] * 1e-6)
                ctx.set_profiling(1)
                kern = {}
                for tag, fn in (("a_new_form", new_form), ("b_library_call", to_nv12), ("c_packed_in_place", leg_c)):
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        fn(sets[it & 1])
                    torch.cuda.synchronize()
                    kern[tag] = {k: {"launches_per_call": v["launches"] / 30, "p50_us": v["p50_ms"] * 1e3}
                                 for k, v in ctx.profile_read(reset=True).items() if v["launches"]}
                ctx.set_profiling(0)
                res["kernels"] = kern
                res["stage1_bytes_per_s"] = {"bgr_to_packed422": 5.0 * w * h * n / (kern["a_new_form"]["color_kernel"]["p50_us"] * 1e-6),
                                             "bgr_to_nv12": 4.5 * w * h * n / (kern["b_library_call"]["color_kernel"]["p50_us"] * 1e-6)}
                rows.append(res)
                print(json.dumps(res), flush=True)
        del sets, out_a, out_b, out_c, scratch, y_b, uv_b
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r27_bgr_to_packed422_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGR in, equalized packed 4:2:2 out: the one-call form against what a caller had", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Rates are frames per second.  (a): "
          "mi_*_bgr_to_packed422_batch_dev on a tight batch.  (b): mi_*_bgr_to_nv12_batch_dev into scratch + a torch scatter of Y and the "
          "row-repeated UV plane into packed frames; B's odd-row chroma DIFFERS from (a)'s (it is the row above's: NV12 has dropped every "
          "second chroma row), its luma and even-row chroma are (a)'s.  (c): mi_*_packed422_batch_dev in place on an already packed batch: "
          "stage 2 and its histogram launch alone, a floor and not a route.  Spread: the two (a) legs of the same rotation against each "
          "other.  Stage 1: bytes per second of the MI_K_COLOR launch (p50 of 30 profiled calls), 5 B/px here, 4.5 B/px in (b)'s call.", "",
          "| frames | format | op | (a) new form | (b) via NV12 + torch | (c) packed in place | a / b | a / c | spread | stage 1 GB/s: packed, NV12 |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS[:3]) +
                  f" | {r['a_rate_over_b_rate']:.3f} | {r['a_rate_over_c_rate']:.3f} | {r['spread']:.3f} "
                  f"| {r['stage1_bytes_per_s']['bgr_to_packed422'] / 1e9:.0f}, {r['stage1_bytes_per_s']['bgr_to_nv12'] / 1e9:.0f} |")
    md += ["", "| frames | format | op | leg | kernels: launches per call x p50 us |", "|---|---|---|---|---|"]
    for r in rows:
        for tag, kk in r["kernels"].items():
            md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | {tag} | " +
                      ", ".join(f"{k} {v['launches_per_call']:g} x {v['p50_us']:.0f}" for k, v in kk.items()) + " |")
    slow = [(r["width"], r["format"], r["op"], round(r["a_rate_over_b_rate"], 3), round(r["spread"], 3)) for r in rows
            if r["a_rate_over_b_rate"] < 1.0 - r["spread"]]
    md += ["", "Rows in which the new form is behind (b) by more than the spread (width, format, op, a / b, spread): " +
           (str(slow) if slow else "none") + "."]
    (outdir / "r27_bgr_to_packed422_ab.md").write_text("\n".join(md) + "\n")
    if slow:
        print("FINDING: the new form is behind the NV12 + torch route in", slow)


if __name__ == "__main__":
    main()
