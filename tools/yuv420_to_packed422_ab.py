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
    python tools/yuv420_to_packed422_ab.py [--out DIR] [--calls N]   -> DIR/r29_yuv420_to_packed422_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_yuv420_to_packed422_frames_dev) against the batch form, again in ONE process with the legs interleaved:
    (b)  mi_*_yuv420_to_packed422_batch_dev on a tight batch: the yardstick of this run, never an earlier figure
    (l)  the list form on the batch's own addresses (entry f = the batch's frame f: same memory, same pitches)
    (lp) the list form on a POOL: every Y, U, V (or UV) plane and every packed frame its own allocation, pitches align(row, 256)
    (p)  what a pool caller has without the list form: one n_frames = 1 batch call per frame of that pool
    (b2) leg (b) a second time in the same rotation: |b / b2 - 1| is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 (the list form runs one resp. four 64-frame launch sequences against the batch form's one); NV12 and
I420; YUY2; MI_UV_COPY; equalizeHist and CLAHE 8x8 clip 2.0.  (l), (lp) and (p) are checked byte for byte against (b) before anything is
timed.  No bar.  A row at 64 x 4K in which (l) is behind (b) by more than the spread is reported as a finding; per-kernel p50 times of
(b), (l) and (lp) from 30 profiled calls each are recorded next to every row to explain one.
    python tools/yuv420_to_packed422_ab.py --list [--out DIR] [--calls N]   -> DIR/r30_yuv420_to_packed422_frames_ab.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, FMT_YUY2, FMT_UYVY, CHROMA_INTERLEAVED, CHROMA_PLANAR, Yuv420Planes, Yuv420Packed422FrameDev  # noqa: E402

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


LIST_LEGS = ("b_batch", "l_list_same_addresses", "lp_list_pool", "p_batch_call_per_frame", "b2_batch_again")
LIST_STATS = ("yuv420_packed422_onepass", "yuv420_packed422_twopass", "yuv420_packed422_list_frames_vec", "yuv420_packed422_list_frames_bytes")


def align256(v):
    return (v + 255) & ~255


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    fmt = FMT_YUY2
    rows = []
    for w, h, n in CASES:
        ysz = w * h
        for layout in ("nv12", "i420"):
            planar = layout == "i420"
            chroma = CHROMA_PLANAR if planar else CHROMA_INTERLEAVED
            crow, cplanes = (w // 2, 2) if planar else (w, 1)
            yp, cp, op = align256(w), align256(crow), align256(2 * w)
            mk = Yuv420Planes.i420 if planar else Yuv420Planes.nv12
            batch, b_planes, b_entries, pools, p_entries, p_planes = [], [], [], [], [], []
            out_b = torch.empty((n, h, 2 * w), dtype=torch.uint8, device="cuda:0")
            out_l = torch.empty_like(out_b)
            out_p = [torch.empty((h, op), dtype=torch.uint8, device="cuda:0") for _ in range(n)]      # the pool's buffers, each its own
            for k in range(2):
                g = torch.Generator(device="cuda:0")
                g.manual_seed(0x5EED3000 + w + k)
                x = torch.randint(0, 256, (n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0", generator=g)
                x[:, :ysz].copy_(x[:, :ysz] // 4 + 64 + 16 * k)  # low contrast: 64 populated luma bins; the chroma stays full range
                batch.append(x)
                d = mk(x, w, h)
                b_planes.append(d)
                fs = d.frame_stride
                arr = (Yuv420Packed422FrameDev * n)()
                for f in range(n):
                    arr[f] = Yuv420Packed422FrameDev(d.y + f * fs, d.c0 + f * fs, d.c1 + f * fs if planar else None, out_l[f].data_ptr())
                b_entries.append(arr)
                # the pool: the same samples, every plane its own pitched allocation
                ys = [torch.empty((h, yp), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
                cs = [[torch.empty((h // 2, cp), dtype=torch.uint8, device="cuda:0") for _ in range(n)] for _ in range(cplanes)]
                for f in range(n):
                    ys[f][:, :w].copy_(x[f, :ysz].view(h, w))
                    for q in range(cplanes):
                        lo = ysz + q * (ysz // 4)
                        cs[q][f][:, :crow].copy_(x[f, lo: lo + (h // 2) * crow].view(h // 2, crow))
                pools.append((ys, cs))
                arr = (Yuv420Packed422FrameDev * n)()
                one = []
                for f in range(n):
                    c0, c1 = cs[0][f].data_ptr(), cs[1][f].data_ptr() if planar else None
                    arr[f] = Yuv420Packed422FrameDev(ys[f].data_ptr(), c0, c1, out_p[f].data_ptr())
                    one.append(Yuv420Planes(ys[f].data_ptr(), yp, c0, c1, cp, 0, chroma))
                p_entries.append(arr)
                p_planes.append(one)
            for opname in OPS:
                eq = opname == "equalize"

                def batch_call(planes, out, nf, **kw):
                    if eq:
                        ctx.equalize_hist_yuv420_to_packed422_batch_dev(planes, out, w, h, nf, fmt, UV_COPY, stream=s, **kw)
                    else:
                        ctx.clahe_yuv420_to_packed422_batch_dev(planes, out, w, h, nf, fmt, UV_COPY, *CLAHE, stream=s, **kw)

                def list_call(entries, y_pitch, c_pitch, out_pitch):
                    if eq:
                        ctx.equalize_hist_yuv420_to_packed422_frames_dev(entries, w, h, y_pitch, c_pitch, chroma, fmt, UV_COPY,
                                                                         out_pitch=out_pitch, stream=s)
                    else:
                        ctx.clahe_yuv420_to_packed422_frames_dev(entries, w, h, y_pitch, c_pitch, chroma, fmt, UV_COPY, *CLAHE,
                                                                 out_pitch=out_pitch, stream=s)

                def leg_b(k):
                    batch_call(b_planes[k], out_b, n)

                def leg_l(k):
                    list_call(b_entries[k], w, crow, 2 * w)

                def leg_lp(k):
                    list_call(p_entries[k], yp, cp, op)

                def leg_p(k):
                    for f in range(n):
                        batch_call(p_planes[k][f], out_p[f], 1, out_pitch=op, out_frame=op * h)

                legs = {"b_batch": leg_b, "l_list_same_addresses": leg_l, "lp_list_pool": leg_lp, "p_batch_call_per_frame": leg_p,
                        "b2_batch_again": leg_b}
                names = list(LIST_LEGS)
                # bytes against the batch form before anything is timed
                leg_b(0)
                before = [ctx.get_stat(k) for k in LIST_STATS]
                leg_l(0)
                leg_lp(0)
                torch.cuda.synchronize()
                assert [ctx.get_stat(k) - v for k, v in zip(LIST_STATS, before)] == [2, 0, 2 * n, 0], "the list form left the one-pass 16 x 2 groups"
                assert torch.equal(out_l, out_b), ("(l) and (b) differ", w, layout, opname)
                assert int(out_b.max()) > 0, "(b) wrote nothing"
                for f in range(n):
                    assert torch.equal(out_p[f][:, : 2 * w], out_b[f]), ("(lp) and (b) differ", w, layout, opname, f)
                    out_p[f].zero_()
                leg_p(0)
                torch.cuda.synchronize()
                for f in range(n):
                    assert torch.equal(out_p[f][:, : 2 * w], out_b[f]), ("(p) and (b) differ", w, layout, opname, f)
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
                res = {"width": w, "height": h, "frames_per_call": n, "layout": layout, "format": "YUY2", "op": opname, "uv_mode": "COPY",
                       "calls": args.calls, "pool_pitches": [yp, cp, op]}
                for name, ev in times.items():
                    ms = [a.elapsed_time(b) for a, b in ev]
                    res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                                 "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
                med = {k: res[k]["median_us"] for k in names}
                res["spread"] = abs(med["b_batch"] / med["b2_batch_again"] - 1.0)
                res["l_rate_over_b_rate"] = med["b_batch"] / med["l_list_same_addresses"]
                res["lp_rate_over_b_rate"] = med["b_batch"] / med["lp_list_pool"]
                res["lp_rate_over_p_rate"] = med["p_batch_call_per_frame"] / med["lp_list_pool"]
                ctx.set_profiling(1)
                kern = {}
                for tag, fn in (("b_batch", leg_b), ("l_list_same_addresses", leg_l), ("lp_list_pool", leg_lp)):
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        fn(it & 1)
                    torch.cuda.synchronize()
                    kern[tag] = {k: {"launches_per_call": v["launches"] / 30, "p50_us": v["p50_ms"] * 1e3}
                                 for k, v in ctx.profile_read(reset=True).items() if v["launches"]}
                ctx.set_profiling(0)
                res["kernels"] = kern
                rows.append(res)
                print(json.dumps(res), flush=True)
            del batch, b_planes, b_entries, pools, p_entries, p_planes, out_b, out_l, out_p
            torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "uv_mode": "COPY", "format": "YUY2", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r30_yuv420_to_packed422_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# 4:2:0 in, packed 4:2:2 out on lists of device frames: the list form against the batch form", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; YUY2; CLAHE 8x8 clip 2.0; MI_UV_COPY.  Rates are frames per second.  (b): "
          "mi_*_yuv420_to_packed422_batch_dev on a tight batch, the yardstick of the same run.  (l): mi_*_yuv420_to_packed422_frames_dev on "
          "the batch's own addresses.  (lp): the list form on a pool of separately allocated planes and buffers at pitches "
          "align(row, 256).  (p): one n_frames = 1 batch call per frame of that pool.  (l), (lp) and (p) are byte-equal to (b), checked "
          "before timing.  Spread: the two (b) legs of the same rotation against each other.  The list form runs one 64-frame launch "
          "sequence at 64 frames and four at 256, against the batch form's one.", "",
          "| frames | layout | op | (b) batch | (l) list, same addresses | (lp) list, pool | (p) batch call per frame | l / b | lp / b | lp / p | spread |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['layout']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LIST_LEGS[:4]) +
                  f" | {r['l_rate_over_b_rate']:.3f} | {r['lp_rate_over_b_rate']:.3f} | {r['lp_rate_over_p_rate']:.2f} | {r['spread']:.3f} |")
    md += ["", "| frames | layout | op | leg | kernels: launches per call x p50 us |", "|---|---|---|---|---|"]
    for r in rows:
        for tag, kk in r["kernels"].items():
            md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['layout']} | {r['op']} | {tag} | " +
                      ", ".join(f"{k} {v['launches_per_call']:g} x {v['p50_us']:.0f}" for k, v in kk.items()) + " |")
    slow = [(r["layout"], r["op"], round(r["l_rate_over_b_rate"], 3), round(r["spread"], 3)) for r in rows
            if r["frames_per_call"] == 64 and r["l_rate_over_b_rate"] < 1.0 - r["spread"]]
    md += ["", "Rows at 64 x 4K in which the list form on the batch's own addresses is behind the batch form by more than the spread "
           "(layout, op, l / b, spread): " + (str(slow) if slow else "none") + "."]
    (outdir / "r30_yuv420_to_packed422_frames_ab.md").write_text("\n".join(md) + "\n")
    if slow:
        print("FINDING: the list form is behind the batch form on the same addresses in", slow)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="the frame-list form against the batch form (r30)")
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
