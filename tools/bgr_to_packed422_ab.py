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
    python tools/bgr_to_packed422_ab.py [--out DIR] [--calls N]   -> DIR/r27_bgr_to_packed422_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_bgr_to_packed422_frames_dev) with the same cases, pixels and method, tight pitches (3W, 2W):
    (A)  the list form on the addresses of a strided batch layout: base + f * frame stride, every address a multiple of 16
    (B)  mi_*_bgr_to_packed422_batch_dev on the same addresses -- the yardstick: its code and ISA are unchanged
    (P)  the list form on a pool: every image and every frame its own allocation, frame k a further 16 * (k % 16) bytes into its
         allocation (differently aligned, all on the 16-pixel groups)
    (C)  one n_frames = 1 batch call per frame on the addresses of (A)
    (A2) leg (A) once more in the same rotation: |A / A2 - 1| is the run's own spread
A, B, P and C are compared byte for byte before anything is timed.  After the timed legs each row runs 30 profiled calls of A and of B
and records the launches and the p50 time of each kernel role.  Nothing is gated: the run records A / B, P / B and A / C beside the
spread, and names the rows in which A / B lies outside 0.87 .. 1.05 (where the sibling list forms landed) by more than the spread.
    python tools/bgr_to_packed422_ab.py --list [--out DIR] [--calls N]   -> DIR/r28_bgr_to_packed422_frames_ab.json and .md"""
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


def timed(stream, legs, warmup, calls):
    """Every call of every leg between its own pair of events, the legs' order rotating every iteration."""
    names = list(legs)
    times = {k: [] for k in names}
    for it in range(warmup + calls):
        order = names[it % len(names):] + names[: it % len(names)]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[name](it & 1)
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


LIST_LEGS = ("A_list", "B_batch", "P_list_pool", "C_per_frame", "A2_list_again")
LIST_ROLES = {"equalize": ("color_kernel", "equalize_lut_kernel", "lut_apply_kernel"),
              "clahe": ("color_kernel", "tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel")}
SIBLINGS = (0.87, 1.05)                                         # A / B of the sibling list forms (profiles/r22 .. r26)


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    L, hd = ctx._L, ctx._h
    Entry = mi_lumaeq.BgrPacked422FrameDev
    rows, outside = [], []
    for w, h, n in CASES:
        ip, op_ = 3 * w, 2 * w
        in_bytes, out_bytes = ip * h, op_ * h
        sets = []                                                # two input sets a leg alternates between, as the batch run does
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2800 + w + k)
            x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda:0", generator=g)
            x.copy_(x // 4 + 64 + 16 * k)                        # low contrast: ~60 populated luma bins
            sets.append(x)
        out_a, out_b, out_c = (torch.zeros((n, h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(3))
        skew = [16 * (f % 16) for f in range(n)]                 # the pool: own allocations, differently aligned, all multiples of 16
        pool_in = [[torch.empty(in_bytes + 256, dtype=torch.uint8, device="cuda:0") for f in range(n)] for k in range(2)]
        pool_out = [torch.zeros(out_bytes + 256, dtype=torch.uint8, device="cuda:0") for f in range(n)]
        for k in range(2):
            for f in range(n):
                pool_in[k][f][skew[f]: skew[f] + in_bytes].copy_(sets[k][f].reshape(-1))

        def table(ins, outs):
            t = (Entry * n)()
            for f in range(n):
                t[f] = Entry(ins[f], outs[f])
            return t
        t_same = [table([sets[k].data_ptr() + f * in_bytes for f in range(n)], [out_a.data_ptr() + f * out_bytes for f in range(n)])
                  for k in range(2)]
        t_pool = [table([pool_in[k][f].data_ptr() + skew[f] for f in range(n)], [pool_out[f].data_ptr() + skew[f] for f in range(n)])
                  for k in range(2)]
        for fname, fmt in FMTS:
            for op in OPS:
                eq = op == "equalize"

                def list_call(t):
                    if eq:
                        rc = L.mi_equalize_hist_bgr_to_packed422_frames_dev(hd, t, n, w, h, ip, op_, ORDER_BGR, fmt, UV_COPY, s)
                    else:
                        rc = L.mi_clahe_bgr_to_packed422_frames_dev(hd, t, n, w, h, ip, op_, ORDER_BGR, fmt, UV_COPY, *CLAHE, s)
                    assert rc == 0, rc

                def batch(d_in, d_out, nf):
                    if eq:
                        ctx.equalize_hist_bgr_to_packed422_batch_dev(d_in, d_out, w, h, nf, ORDER_BGR, fmt, UV_COPY, stream=s)
                    else:
                        ctx.clahe_bgr_to_packed422_batch_dev(d_in, d_out, w, h, nf, ORDER_BGR, fmt, UV_COPY, *CLAHE, stream=s)

                def leg_a(k):
                    list_call(t_same[k])

                def leg_b(k):
                    batch(sets[k], out_b, n)

                def leg_p(k):
                    list_call(t_pool[k])

                def leg_c(k):
                    for f in range(n):
                        batch(sets[k][f], out_c[f], 1)

                vec0, byte0 = ctx.get_stat("bgr_packed422_list_frames_vec"), ctx.get_stat("bgr_packed422_list_frames_bytes")
                for leg in (leg_a, leg_b, leg_p, leg_c):
                    leg(0)
                torch.cuda.synchronize()
                assert (ctx.get_stat("bgr_packed422_list_frames_vec"), ctx.get_stat("bgr_packed422_list_frames_bytes")) == (vec0 + 2 * n, byte0), \
                    "a frame of a list left the 16-pixel groups"
                assert torch.equal(out_a, out_b) and torch.equal(out_a, out_c), ("A, B and C differ", w, fname, op)
                for f in range(n):
                    assert torch.equal(pool_out[f][skew[f]: skew[f] + out_bytes], out_a[f].reshape(-1)), ("A and P differ", w, fname, op, f)
                assert int(out_a.max()) > 0, "A wrote nothing"
                legs = {"A_list": leg_a, "B_batch": leg_b, "P_list_pool": leg_p, "C_per_frame": leg_c, "A2_list_again": leg_a}
                res = {"width": w, "height": h, "frames_per_call": n, "format": fname, "op": op, "order": "BGR", "uv_mode": "COPY",
                       "calls": args.calls, "in_pitch": ip, "out_pitch": op_}
                for name, r in timed(stream, legs, args.warmup, args.calls).items():
                    r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                    res[name] = r
                med = {k: res[k]["median_us"] for k in LIST_LEGS}
                res["spread"] = abs(med["A_list"] / med["A2_list_again"] - 1.0)
                res["A_rate_over_B_rate"] = med["B_batch"] / med["A_list"]
                res["P_rate_over_B_rate"] = med["B_batch"] / med["P_list_pool"]
                res["A_rate_over_C_rate"] = med["C_per_frame"] / med["A_list"]
                ctx.set_profiling(1)
                kern = {}
                for leg, tag in ((leg_a, "A"), (leg_b, "B")):
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        leg(it & 1)
                    torch.cuda.synchronize()
                    prof = ctx.profile_read(reset=True)
                    for role in LIST_ROLES[op]:
                        if prof[role]["launches"]:
                            kern.setdefault(role, {})[tag + "_p50_us"] = prof[role]["p50_ms"] * 1e3
                            kern[role][tag + "_launches_per_call"] = prof[role]["launches"] / 30.0
                ctx.set_profiling(0)
                res["kernels"] = kern
                rows.append(res)
                ab = res["A_rate_over_B_rate"]
                if ab < SIBLINGS[0] - res["spread"] or ab > SIBLINGS[1] + res["spread"]:
                    outside.append(f"{n} x {w}x{h} {fname} {op}: A / B = {ab:.3f} (spread {res['spread']:.3f})")
                print(json.dumps(res), flush=True)
        del sets, out_a, out_b, out_c, pool_in, pool_out, t_same, t_pool
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bars": "none: recorded, not gated",
            "list_frames_vec": ctx.get_stat("bgr_packed422_list_frames_vec"), "list_frames_bytes": ctx.get_stat("bgr_packed422_list_frames_bytes"),
            "a_over_b_outside_the_siblings_range": outside}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r28_bgr_to_packed422_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGR in, packed 4:2:2 out on lists of device frames: the list form against the batch form and per-frame calls", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY; tight pitches (3W, 2W).  Rates are frames per "
          "second.  (A): mi_*_bgr_to_packed422_frames_dev on the addresses of a strided batch layout.  (B): "
          "mi_*_bgr_to_packed422_batch_dev on the same addresses.  (P): the list form on a pool, every image and every frame its own "
          "allocation, frame k 16 * (k % 16) bytes into it.  (C): one n_frames = 1 batch call per frame.  Spread: |A / A2 - 1|, the two (A) "
          "legs of the same rotation.  Slots: p50 of one launch (launches per call), list / batch.  "
          f"Frames by walk over the whole run: {meta['list_frames_vec']} on 16-pixel groups, {meta['list_frames_bytes']} on macropixels.  "
          "The list form cuts a call into chunks of 128 frames, the batch form into chunks of 256: at 256 frames a call (A) and (P) run "
          "two launch sequences where (B) runs one.", "",
          "| frames | format | op | (A) list | (B) batch | (P) list, pool | (C) per frame | A / B | P / B | A / C | spread | stage 1 A / B | writer A / B |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(k):
            return f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)"

        def slot(role):
            v = r["kernels"].get(role, {})
            return (f"{v.get('A_p50_us', 0):.0f} us x{v.get('A_launches_per_call', 0):.0f} / "
                    f"{v.get('B_p50_us', 0):.0f} us x{v.get('B_launches_per_call', 0):.0f}")
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['format']} | {r['op']} | {cell('A_list')} | {cell('B_batch')} | "
                  f"{cell('P_list_pool')} | {cell('C_per_frame')} | {r['A_rate_over_B_rate']:.3f} | {r['P_rate_over_B_rate']:.3f} | "
                  f"{r['A_rate_over_C_rate']:.3f} | {r['spread']:.3f} | {slot('color_kernel')} | "
                  f"{slot('lut_apply_kernel' if r['op'] == 'equalize' else 'clahe_interp_kernel')} |")
    md += ["", f"Rows in which A / B lies outside {SIBLINGS[0]} .. {SIBLINGS[1]} by more than the spread: " +
           ("; ".join(outside) if outside else "none") + "."]
    (outdir / "r28_bgr_to_packed422_frames_ab.md").write_text("\n".join(md) + "\n")
    if outside:
        print("FINDING: A / B outside the range of the sibling list forms in", outside)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="measure the frame-list form (mi_*_bgr_to_packed422_frames_dev)")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if args.list:
        return main_list(args)
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
