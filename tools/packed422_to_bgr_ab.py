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
    python tools/packed422_to_bgr_ab.py [--out DIR] [--calls N]   -> DIR/r25_packed422_to_bgr_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_packed422_to_bgr_frames_dev) over a capture device's buffer pool and an image pool -- every packed
buffer and every image its own allocation, pitches align(2W, 256) and align(3W, 256) -- with the same cases and the same method:
    (A)  the list form, the entry point on a prebuilt address list
    (B)  mi_*_packed422_to_bgr_batch_dev on the same pixels at the same pitches in one allocation per side
    (C)  one n_frames = 1 batch call per frame, on the pools' own buffers
    (D)  repacking: every buffer copied into strided scratch, ONE batch call into strided scratch images, every image copied out
    (A2) the list form once more in the same rotation: |A / A2 - 1| is the run's own spread
A, B, C and D are compared byte for byte before anything is timed.  After the timed legs each row runs 30 profiled calls of A and of B
and records the launches and the p50 time of each kernel role.  Nothing is gated: the run records A / B, A / C and A / D beside the
spread and prints a finding when A trails B at 64 x 4K by more than 0.96 beyond the spread, or does not beat C or D.
    python tools/packed422_to_bgr_ab.py --list [--out DIR] [--calls N]   -> DIR/r26_packed422_to_bgr_frames_ab.json and .md"""
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


def align256(x):
    return (x + 255) // 256 * 256


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    L, hd = ctx._L, ctx._h
    roles = {"equalize": ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel"),
             "clahe": ("tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel")}
    rows, findings = [], []
    for w, h, n in CASES:
        ip, op_ = align256(2 * w), align256(3 * w)
        for fmt, fname in FMTS:
            off = fmt - 2
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2600 + w + fmt)
            x = torch.randint(0, 256, (n, h, ip), dtype=torch.uint8, device="cuda:0", generator=g)    # B's input: one allocation
            lane = x[:, :, off:2 * w:2]
            lane.copy_(lane // 4 + 64)                               # low-contrast luma (~60 populated bins), random chroma
            pool_in = [x[f].clone() for f in range(n)]               # the buffer pool: every frame its own allocation
            pool_a = [torch.zeros((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]   # the image pool of A
            pool_c = [torch.zeros((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
            pool_d = [torch.zeros((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
            out_b = torch.zeros((n, h, op_), dtype=torch.uint8, device="cuda:0")
            scratch_in, scratch_out = torch.empty_like(x), torch.zeros_like(out_b)
            table = (mi_lumaeq.Packed422BgrFrameDev * n)()
            for f in range(n):
                table[f] = mi_lumaeq.Packed422BgrFrameDev(pool_in[f].data_ptr(), pool_a[f].data_ptr())
            kw = dict(in_pitch=ip, in_frame=ip * h, out_pitch=op_, out_frame=op_ * h, stream=s)
            for op in ("equalize", "clahe"):
                def batch(d_in, d_out, nf):
                    if op == "equalize":
                        ctx.equalize_hist_packed422_to_bgr_batch_dev(d_in, d_out, w, h, nf, fmt, ORDER_BGR, **kw)
                    else:
                        ctx.clahe_packed422_to_bgr_batch_dev(d_in, d_out, w, h, nf, fmt, ORDER_BGR, *CLAHE, **kw)

                def leg_a():
                    if op == "equalize":
                        rc = L.mi_equalize_hist_packed422_to_bgr_frames_dev(hd, table, n, w, h, ip, op_, fmt, ORDER_BGR, s)
                    else:
                        rc = L.mi_clahe_packed422_to_bgr_frames_dev(hd, table, n, w, h, ip, op_, fmt, ORDER_BGR, *CLAHE, s)
                    assert rc == 0, rc

                def leg_b():
                    batch(x, out_b, n)

                def leg_c():
                    for f in range(n):
                        batch(pool_in[f], pool_c[f], 1)

                def leg_d():
                    for f in range(n):
                        scratch_in[f].copy_(pool_in[f], non_blocking=True)
                    batch(scratch_in, scratch_out, n)
                    for f in range(n):
                        pool_d[f].copy_(scratch_out[f], non_blocking=True)

                for leg in (leg_a, leg_b, leg_c, leg_d):
                    leg()
                torch.cuda.synchronize()
                for f in range(n):
                    for name, other in (("B", out_b[f]), ("C", pool_c[f]), ("D", pool_d[f])):
                        assert torch.equal(pool_a[f], other), ("A and " + name + " differ", w, h, fname, op, f)
                assert int(pool_a[0][:, : 3 * w].max()) > 0, "A wrote nothing"
                legs = {"A_list": leg_a, "B_batch": leg_b, "C_per_frame": leg_c, "D_repack": leg_d, "A2_list_again": leg_a}
                res = {"width": w, "height": h, "frames_per_call": n, "op": op, "format": fname, "order": "BGR", "calls": args.calls,
                       "in_pitch": ip, "out_pitch": op_}
                for name, r in timed(stream, legs, args.warmup, args.calls).items():
                    r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                    res[name] = r
                a, a2 = res["A_list"]["median_us"], res["A2_list_again"]["median_us"]
                res["spread"] = abs(a / a2 - 1.0)
                for k, leg in (("B", "B_batch"), ("C", "C_per_frame"), ("D", "D_repack")):
                    res["A_rate_over_%s_rate" % k] = res[leg]["median_us"] / a
                ctx.set_profiling(1)
                kern = {}
                for leg, tag in ((leg_a, "A"), (leg_b, "B")):
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        leg()
                    torch.cuda.synchronize()
                    prof = ctx.profile_read(reset=True)
                    for role in roles[op]:
                        if prof[role]["launches"]:
                            kern.setdefault(role, {})[tag + "_p50_us"] = prof[role]["p50_ms"] * 1e3
                            kern[role][tag + "_launches_per_call"] = prof[role]["launches"] / 30.0
                ctx.set_profiling(0)
                res["kernels"] = kern
                rows.append(res)
                if n == 64 and res["A_rate_over_B_rate"] < 0.96 - res["spread"]:
                    findings.append(f"{w}x{h} x{n} {fname} {op}: A / B = {res['A_rate_over_B_rate']:.3f} (spread {res['spread']:.3f})")
                for k in ("C", "D"):
                    if res["A_rate_over_%s_rate" % k] - 1.0 <= res["spread"]:
                        findings.append(f"{w}x{h} x{n} {fname} {op}: A does not beat {k}: {res['A_rate_over_%s_rate' % k]:.3f}")
                print(f"{w}x{h} x{n:3d} {fname} {op:8s} " +
                      "  ".join(f"{k.split('_')[0]} {res[k]['median_us']:8.1f} us" for k in legs) +
                      f"  | A/B {res['A_rate_over_B_rate']:.3f}  A/C {res['A_rate_over_C_rate']:.3f}  A/D {res['A_rate_over_D_rate']:.3f}"
                      f"  spread {res['spread']:.3f}  | " +
                      "  ".join(f"{role} A {v.get('A_p50_us', 0):.1f} x{v.get('A_launches_per_call', 0):.0f}"
                                f" B {v.get('B_p50_us', 0):.1f} x{v.get('B_launches_per_call', 0):.0f}" for role, v in kern.items()), flush=True)
            del x, lane, pool_in, pool_a, pool_c, pool_d, out_b, scratch_in, scratch_out
            torch.cuda.empty_cache()
    wide, byte = ctx.get_stat("packed422_bgr_list_frames_wide"), ctx.get_stat("packed422_bgr_list_frames_bytes")
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "list_frames_wide": wide, "list_frames_bytes": byte, "bars": "none: recorded, not gated", "findings": findings}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r26_packed422_to_bgr_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# Packed 4:2:2 in, BGR out on lists of device frames: the list form against the batch form and the two routes without it", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one "
          "process, medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR; every packed buffer and every image its own "
          "allocation at pitches align(2W, 256) / align(3W, 256).  Rates are frames per second.  (A): mi_*_packed422_to_bgr_frames_dev on "
          "a prebuilt address list.  (B): mi_*_packed422_to_bgr_batch_dev on the same pixels at the same pitches in one allocation per "
          "side.  (C): one n_frames = 1 batch call per frame.  (D): both pools repacked through strided scratch around one batch call.  "
          "Spread: |A / A2 - 1|, the two list legs of the same rotation.  Slots: p50 of one launch (launches per call) of the "
          "histogram and the pixel-writing kernel, list / batch.  "
          f"Frames by store path over the whole run: {wide} wide, {byte} bytes.", "",
          "| frames | format | op | (A) list | (B) batch | (C) per frame | (D) repack | A / B | A / C | A / D | spread | hist A / B | writer A / B |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(k):
            return f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)"

        def slot(role):
            v = r["kernels"].get(role, {})
            return (f"{v.get('A_p50_us', 0):.0f} us x{v.get('A_launches_per_call', 0):.0f} / "
                    f"{v.get('B_p50_us', 0):.0f} us x{v.get('B_launches_per_call', 0):.0f}")
        hist, wr = ("hist_partial_kernel", "lut_apply_kernel") if r["op"] == "equalize" else ("tile_hist_kernel", "clahe_interp_kernel")
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | {cell('A_list')} | {cell('B_batch')} | "
                  f"{cell('C_per_frame')} | {cell('D_repack')} | {r['A_rate_over_B_rate']:.3f} | {r['A_rate_over_C_rate']:.3f} | "
                  f"{r['A_rate_over_D_rate']:.3f} | {r['spread']:.3f} | {slot(hist)} | {slot(wr)} |")
    md += ["", "Findings: " + ("; ".join(findings) if findings else "none") + "."]
    (outdir / "r26_packed422_to_bgr_frames_ab.md").write_text("\n".join(md) + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="measure the frame-list form (mi_*_packed422_to_bgr_frames_dev)")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if args.list:
        return main_list(args)
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
