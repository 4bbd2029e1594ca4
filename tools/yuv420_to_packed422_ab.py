"""4:2:0 (NV12 / I420) in, equalized packed 4:2:2 (YUY2 / UYVY) out in one call (mi_*_yuv420_to_packed422_batch_dev) against what a
caller had before it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (a)  the new form on a tight batch, NV12 input (equalizeHist 4.5 B/px, one-pass CLAHE 4.5)
    (ai) the new form on the same samples as I420 (U and V planes: two 8-byte chroma loads per lane and a zip instead of one 16-byte load)
    (b)  what a caller has without it: mi_*_yuv420_batch_dev NV12 -> NV12 into a tight scratch batch with MI_UV_COPY (4 B/px), then a
         torch scatter of Y and of the row-repeated UV plane into packed frames (four strided copies: 3.5 B/px read, 2 written, the
         frame touched four times).  The SAME bytes as (a), checked before anything is timed.
    (c)  mi_*_packed422_batch_dev with MI_UV_COPY in place on an already packed batch (5 B/px): a floor, not a route (nothing has
         packed the frames)
    (a2) leg (a) a second time in the same rotation: |a / a2 - 1| is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight frames per call (0.8 GiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); YUY2 and UYVY; equalizeHist and CLAHE 8x8 clip 2.0; MI_UV_COPY.  Low-contrast luma (a 64-value band), random chroma.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.
No bar: (a) moves fewer bytes than (b) in fewer launches, so (a) is expected ahead.  A row in which (a) is behind (b) by more than the
spread is reported as a finding.  After the timed legs each row runs 30 profiled calls of (a), (ai), the library call of (b) and (c) and
records every kernel's launches per call and p50 time, and the bytes per second of the new pixel-writing kernel (3.5 B/px: 1.5 read,
2 written) from the same run.
    python tools/yuv420_to_packed422_ab.py [--out DIR] [--calls N]   -> DIR/r29_yuv420_to_packed422_ab.json and .md (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, FMT_YUY2, FMT_UYVY, Yuv420Planes  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
FMTS = (("YUY2", FMT_YUY2), ("UYVY", FMT_UYVY))
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = {"equalize": 4.5, "clahe": 4.5}
WRITER = {"equalize": "lut_apply_kernel", "clahe": "clahe_interp_kernel"}
LEGS = ("a_new_form_nv12", "ai_new_form_i420", "b_via_nv12_and_torch", "c_packed_in_place", "a2_new_form_nv12_again")
STATS = ("yuv420_packed422_onepass", "yuv420_packed422_twopass", "yuv420_packed422_vec", "yuv420_packed422_bytes")


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
        nv12, i420 = [], []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2900 + w + k)
            x = torch.randint(0, 256, (n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0", generator=g)
            x[:, :ysz].copy_(x[:, :ysz] // 4 + 64 + 16 * k)     # low contrast: 64 populated luma bins; the chroma stays full range
            p = torch.empty_like(x)                              # the same samples as three planes
            p[:, :ysz].copy_(x[:, :ysz])
            uv = x[:, ysz:].view(n, ysz // 4, 2)
            p[:, ysz: ysz + ysz // 4].copy_(uv[:, :, 0])
            p[:, ysz + ysz // 4:].copy_(uv[:, :, 1])
            nv12.append(x)
            i420.append(p)
        out_a = torch.empty((n, h, w // 2, 4), dtype=torch.uint8, device="cuda:0")
        out_i = torch.empty_like(out_a)
        out_b = torch.empty_like(out_a)
        out_c = torch.empty_like(out_a)                          # leg (c): an already packed batch, mapped in place
        scratch = torch.empty((n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0")       # leg (b): the NV12 batch in between
        y_b = scratch[:, :ysz].view(n, h, w)
        uv_b = scratch[:, ysz:].view(n, h // 2, w // 2, 2)
        d_scratch = Yuv420Planes.nv12(scratch, w, h)
        for fname, fmt in FMTS:
            y0, y1, ui, vi = (0, 2, 1, 3) if fmt == FMT_YUY2 else (1, 3, 0, 2)
            for op in OPS:
                eq = op == "equalize"

                def new_form(planes, out):
                    if eq:
                        ctx.equalize_hist_yuv420_to_packed422_batch_dev(planes, out, w, h, n, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_yuv420_to_packed422_batch_dev(planes, out, w, h, n, fmt, UV_COPY, *CLAHE, stream=s)

                def leg_a(k):
                    new_form(Yuv420Planes.nv12(nv12[k], w, h), out_a)

                def leg_ai(k):
                    new_form(Yuv420Planes.i420(i420[k], w, h), out_i)

                def to_nv12(k):
                    if eq:
                        ctx.equalize_hist_yuv420_batch_dev(Yuv420Planes.nv12(nv12[k], w, h), d_scratch, w, h, n, UV_COPY, stream=s)
                    else:
                        ctx.clahe_yuv420_batch_dev(Yuv420Planes.nv12(nv12[k], w, h), d_scratch, w, h, n, UV_COPY, *CLAHE, stream=s)

                def leg_b(k):
                    to_nv12(k)
                    out_b[..., y0] = y_b[:, :, 0::2]
                    out_b[..., y1] = y_b[:, :, 1::2]
                    ob = out_b.view(n, h // 2, 2, w // 2, 4)
                    ob[..., ui] = uv_b[:, :, None, :, 0]         # every UV row goes to two packed rows
                    ob[..., vi] = uv_b[:, :, None, :, 1]

                def leg_c(k):
                    if eq:
                        ctx.equalize_hist_packed422_batch_dev(out_c, out_c, w, h, n, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_packed422_batch_dev(out_c, out_c, w, h, n, fmt, UV_COPY, *CLAHE, stream=s)

                legs = {"a_new_form_nv12": leg_a, "ai_new_form_i420": leg_ai, "b_via_nv12_and_torch": leg_b, "c_packed_in_place": leg_c,
                        "a2_new_form_nv12_again": leg_a}
                names = list(LEGS)
                before = [ctx.get_stat(k) for k in STATS]
                out_a.zero_()
                leg_a(0)                                         # (a), (ai) and (b) agree byte for byte before anything is timed
                leg_ai(0)
                leg_b(0)
                torch.cuda.synchronize()
                assert [ctx.get_stat(k) - b for k, b in zip(STATS, before)] == [2, 0, 2, 0], "the new form left the one-pass 16 x 2 groups"
                assert torch.equal(out_a, out_b), ("(a) and (b) differ", w, fname, op)
                assert torch.equal(out_a, out_i), ("NV12 and I420 input differ", w, fname, op)
                assert int(out_a.max()) > 0, "(a) wrote nothing"
                out_c.copy_(out_a)
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
                res = {"width": w, "height": h, "frames_per_call": n, "format": fname, "op": op, "uv_mode": "COPY", "calls": args.calls}
                for name, ev in times.items():
                    ms = [a.elapsed_time(b) for a, b in ev]
                    res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                                 "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
                med = {k: res[k]["median_us"] for k in names}
                res["spread"] = abs(med["a_new_form_nv12"] / med["a2_new_form_nv12_again"] - 1.0)
                res["a_rate_over_b_rate"] = med["b_via_nv12_and_torch"] / med["a_new_form_nv12"]
                res["ai_rate_over_b_rate"] = med["b_via_nv12_and_torch"] / med["ai_new_form_i420"]
                res["a_rate_over_c_rate"] = med["c_packed_in_place"] / med["a_new_form_nv12"]
                res["a_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (med["a_new_form_nv12"] * 1e-6)
                ctx.set_profiling(1)
                kern = {}
                for tag, fn in (("a_new_form_nv12", leg_a), ("ai_new_form_i420", leg_ai), ("b_library_call", to_nv12), ("c_packed_in_place", leg_c)):
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        fn(it & 1)
                    torch.cuda.synchronize()
                    kern[tag] = {k: {"launches_per_call": v["launches"] / 30, "p50_us": v["p50_ms"] * 1e3}
                                 for k, v in ctx.profile_read(reset=True).items() if v["launches"]}
                ctx.set_profiling(0)
                res["kernels"] = kern
                res["writer_bytes_per_s"] = {tag: 3.5 * w * h * n / (kern[tag][WRITER[op]]["p50_us"] * 1e-6)
                                             for tag in ("a_new_form_nv12", "ai_new_form_i420")}
                rows.append(res)
                print(json.dumps(res), flush=True)
        del nv12, i420, out_a, out_i, out_b, out_c, scratch, y_b, uv_b, d_scratch
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r29_yuv420_to_packed422_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# 4:2:0 in, equalized packed 4:2:2 out: the one-call form against what a caller had", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_UV_COPY.  Rates are frames per second.  (a): "
          "mi_*_yuv420_to_packed422_batch_dev on a tight NV12 batch; (ai): the same samples as I420.  (b): mi_*_yuv420_batch_dev NV12 -> "
          "NV12 into scratch + a torch scatter of Y and the row-repeated UV plane into packed frames: the same bytes as (a), checked "
          "before timing.  (c): mi_*_packed422_batch_dev in place on an already packed batch: a floor and not a route.  Spread: the two "
          "(a) legs of the same rotation against each other.  Writer: bytes per second of the new pixel-writing launch (MI_K_LUT_APPLY / "
          "MI_K_CLAHE_INTERP, p50 of 30 profiled calls) at 3.5 B/px.", "",
          "| frames | format | op | (a) NV12 in | (ai) I420 in | (b) via NV12 + torch | (c) packed in place | a / b | ai / b | a / c | spread | writer TB/s: NV12, I420 |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS[:4]) +
                  f" | {r['a_rate_over_b_rate']:.3f} | {r['ai_rate_over_b_rate']:.3f} | {r['a_rate_over_c_rate']:.3f} | {r['spread']:.3f} "
                  f"| {r['writer_bytes_per_s']['a_new_form_nv12'] / 1e12:.2f}, {r['writer_bytes_per_s']['ai_new_form_i420'] / 1e12:.2f} |")
    md += ["", "| frames | format | op | leg | kernels: launches per call x p50 us |", "|---|---|---|---|---|"]
    for r in rows:
        for tag, kk in r["kernels"].items():
            md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | {tag} | " +
                      ", ".join(f"{k} {v['launches_per_call']:g} x {v['p50_us']:.0f}" for k, v in kk.items()) + " |")
    slow = [(r["width"], r["format"], r["op"], round(r["a_rate_over_b_rate"], 3), round(r["spread"], 3)) for r in rows
            if r["a_rate_over_b_rate"] < 1.0 - r["spread"]]
    md += ["", "Rows in which the new form is behind (b) by more than the spread (width, format, op, a / b, spread): " +
           (str(slow) if slow else "none") + "."]
    (outdir / "r29_yuv420_to_packed422_ab.md").write_text("\n".join(md) + "\n")
    if slow:
        print("FINDING: the new form is behind the NV12 + torch route in", slow)


if __name__ == "__main__":
    main()
