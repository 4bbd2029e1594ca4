"""Packed 4:2:2 in, planar 4:2:0 out (mi_*_packed422_to_yuv420_batch_dev) against the route a caller had before it and against the NV12
form, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (P)  the new form: packed frames in, tight I420 frames out
    (a)  the route a caller had: mi_*_packed422_to_nv12_batch_dev with the Y plane written in place of the I420 frame's and the UV plane
         into scratch, then a torch de-interleave of the UV plane into the U and the V plane
    (b)  mi_*_packed422_to_nv12_batch_dev alone on the same input (tight NV12 frames: not what a software encoder takes)
64 x 3840x2160 and 256 x 1920x1080 frames per call (1 GiB of packed input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; YUY2 and UYVY; MI_UV_COPY.  Tight layouts on both sides.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times: the p10 .. p90 band of a leg is the run's own spread.  Inputs
never change.  Before anything is timed, P and (a) must have written identical bytes, and P's planes must be (b)'s de-interleaved.
Bar: P is faster than (a) in every row by more than the spread (P's p90 below (a)'s p10): it removes a launch sequence and 1 B/px of
traffic.  Finding, not a bar: P against (b) -- the ratio is recorded, and a row where P's p10 lies above (b)'s p90 is marked "behind".
    python tools/packed422_to_yuv420_ab.py [--out DIR] [--calls N]   -> DIR/r39_packed422_to_yuv420_ab.json and .md (default DIR: profiles)

Frame lists (mi_*_packed422_to_yuv420_frames_dev), with --list, same method, legs interleaved:
    (B)  the batch form on one tight allocation
    (L0) the list form on the batch's own addresses (every entry points into the same tight allocations)
    (L1) the list form over separately allocated buffers: every input its own allocation at pitch align(2W, 256), every Y plane at
         pitch align(W, 256), every U and every V plane at pitch align(W/2, 256) (a capture pool in, an encoder's frame pool out)
The list's bytes are the batch's, frame by frame, before anything is timed.  Recorded, not enforced.
    python tools/packed422_to_yuv420_ab.py --list   -> DIR/r40_packed422_to_yuv420_frames_ab.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, FMT_YUY2, FMT_UYVY  # noqa: E402
from mi_lumaeq.capi import Yuv420Planes, BgrYuv420FrameDev, CHROMA_PLANAR  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
ROWS = [(op, fmt) for op in ("equalize", "clahe") for fmt in (FMT_YUY2, FMT_UYVY)]
FMT_NAME = {FMT_YUY2: "YUY2", FMT_UYVY: "UYVY"}
CLAHE = (2.0, 8, 8)
UV = UV_COPY


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def align(x, a):
    return (x + a - 1) // a * a


def make_sets(w, h, n, fmt, seed, count=2):
    """`count` sets of n packed frames: low-contrast luma (~60 populated bins), random chroma"""
    sets = []
    for k in range(count):
        g = torch.Generator(device="cuda:0")
        g.manual_seed(seed + w + k)
        x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
        lane = x[:, :, fmt - 2::2]
        lane.copy_(lane // 4 + 64 + 16 * k)
        sets.append(x)
    return sets


def timed(stream, legs, sets, warmup, calls):
    """legs: name -> callable(x).  Interleaved, the order rotating every iteration; every call between its own pair of events."""
    names = list(legs)
    times = {k: [] for k in names}
    for it in range(warmup + calls):
        x = sets[it % len(sets)]
        order = names[it % len(names):] + names[: it % len(names)]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[name](x)
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


def table(head, rows):
    return "\n".join(["| " + " | ".join(head) + " |", "|" + "---|" * len(head)] + ["| " + " | ".join(r) + " |" for r in rows])


def cell(r):
    return f"{r['median_us']:.1f} [{r['p10_us']:.1f} .. {r['p90_us']:.1f}]"


def batch_forms(ctx, args):
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows, md = [], []
    for w, h, n in CASES:
        ysz, csz = w * h, (w // 2) * (h // 2)
        i420 = torch.empty((n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0")            # P's frames
        route = torch.empty_like(i420)                                                       # (a)'s frames
        scratch = torch.empty_like(i420)                                                     # (a)'s UV planes, at the frames' stride
        nv12 = torch.empty_like(i420)                                                        # (b)'s frames
        p_planes = Yuv420Planes.i420(i420, w, h)
        route_u = route[:, ysz: ysz + csz].view(n, h // 2, w // 2)
        route_v = route[:, ysz + csz:].view(n, h // 2, w // 2)
        scratch_uv = scratch[:, : 2 * csz].view(n, h // 2, w)
        for op, fmt in ROWS:
            sets = make_sets(w, h, n, fmt, 0x5EED3900)

            def leg_p(x):
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_yuv420_batch_dev(x, p_planes, w, h, n, fmt, UV, stream=s)
                else:
                    ctx.clahe_packed422_to_yuv420_batch_dev(x, p_planes, w, h, n, fmt, UV, *CLAHE, stream=s)

            def nv12_form(x, y, uv):
                kw = dict(y_pitch=w, uv_pitch=w, out_frame=ysz * 3 // 2, stream=s)
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_nv12_batch_dev(x, y, uv, w, h, n, fmt, UV, **kw)
                else:
                    ctx.clahe_packed422_to_nv12_batch_dev(x, y, uv, w, h, n, fmt, UV, *CLAHE, **kw)

            def leg_a(x):
                nv12_form(x, route, scratch)
                route_u.copy_(scratch_uv[:, :, 0::2])
                route_v.copy_(scratch_uv[:, :, 1::2])

            def leg_b(x):
                nv12_form(x, nv12, nv12.data_ptr() + ysz)

            # identical bytes before anything is timed
            for leg in (leg_p, leg_a, leg_b):
                leg(sets[0])
            torch.cuda.synchronize()
            assert torch.equal(i420, route), ("P and (a) differ", w, h, op, fmt)
            b_uv = nv12[:, ysz:].view(n, h // 2, w)
            assert torch.equal(i420[:, :ysz], nv12[:, :ysz]), ("P's Y is not (b)'s", w, h, op, fmt)
            assert torch.equal(i420[:, ysz: ysz + csz].view(n, h // 2, w // 2), b_uv[:, :, 0::2]), ("P's U is not (b)'s", w, h, op, fmt)
            assert torch.equal(i420[:, ysz + csz:].view(n, h // 2, w // 2), b_uv[:, :, 1::2]), ("P's V is not (b)'s", w, h, op, fmt)
            legs = {"P_planar": leg_p, "a_nv12_then_torch_deinterleave": leg_a, "b_nv12": leg_b}
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "format": FMT_NAME[fmt], "uv": "copy", "calls": args.calls}
            for name, r in timed(stream, legs, sets, args.warmup, args.calls).items():
                r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                res[name] = r
            P, A, B = res["P_planar"], res["a_nv12_then_torch_deinterleave"], res["b_nv12"]
            res["P_speed_over_a_speed"] = A["median_us"] / P["median_us"]
            res["P_speed_over_b_speed"] = B["median_us"] / P["median_us"]
            res["faster_than_a_by_more_than_the_spread"] = P["p90_us"] < A["p10_us"]
            res["behind_b_by_more_than_the_spread"] = P["p10_us"] > B["p90_us"]
            rows.append(res)
            md.append([f"{w}x{h} x{n}", op, FMT_NAME[fmt], cell(P), cell(A), cell(B), f"{res['P_speed_over_a_speed']:.3f}",
                       "yes" if res["faster_than_a_by_more_than_the_spread"] else "NO", f"{res['P_speed_over_b_speed']:.3f}",
                       "behind" if res["behind_b_by_more_than_the_spread"] else "within the spread or ahead"])
            print(" ".join(md[-1]), flush=True)
            del sets
        del i420, route, scratch, nv12
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "uv_mode": "copy",
            "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])}, "times": "microseconds per call: median [p10 .. p90]",
            "bar": "P's p90 below (a)'s p10 in every row; P against (b) is recorded, not enforced"}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r39_packed422_to_yuv420_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    head = ["frames", "op", "format", "P planar, us", "(a) NV12 + torch de-interleave, us", "(b) NV12 alone, us", "P speed / (a) speed",
            "faster than (a) by more than the spread", "P speed / (b) speed", "against (b)"]
    (outdir / "r39_packed422_to_yuv420_ab.md").write_text("```\n" + __doc__.split("\n    python")[0] + "\n```\n\n" + json.dumps(meta) + "\n\n"
                                                         + table(head, md) + "\n")
    return [(r["width"], r["op"], r["format"]) for r in rows if not r["faster_than_a_by_more_than_the_spread"]]


def frame_lists(ctx, args):
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows, md = [], []
    for w, h, n in CASES:
        ysz, csz = w * h, (w // 2) * (h // 2)
        out_b = torch.empty((n, ysz * 3 // 2), dtype=torch.uint8, device="cuda:0")
        out_l0 = torch.empty_like(out_b)
        ip, yp, cp = align(2 * w, 256), align(w, 256), align(w // 2, 256)
        ins = [torch.zeros(ip * h, dtype=torch.uint8, device="cuda:0").view(h, ip)[:, : 2 * w] for _ in range(n)]
        ys = [torch.zeros(yp * h, dtype=torch.uint8, device="cuda:0").view(h, yp)[:, :w] for _ in range(n)]
        us = [torch.zeros(cp * (h // 2), dtype=torch.uint8, device="cuda:0").view(h // 2, cp)[:, : w // 2] for _ in range(n)]
        vs = [torch.zeros(cp * (h // 2), dtype=torch.uint8, device="cuda:0").view(h // 2, cp)[:, : w // 2] for _ in range(n)]
        l1 = (BgrYuv420FrameDev * n)(*[BgrYuv420FrameDev.of(ins[k], ys[k], us[k], vs[k]) for k in range(n)])
        p_planes = Yuv420Planes.i420(out_b, w, h)
        for op, fmt in ROWS:
            d_in = make_sets(w, h, n, fmt, 0x5EED4000, count=1)[0]
            for k in range(n):
                ins[k].copy_(d_in[k])
            base = out_l0.data_ptr()
            fs = ysz * 3 // 2
            l0 = (BgrYuv420FrameDev * n)(*[BgrYuv420FrameDev(d_in.data_ptr() + k * 2 * ysz, base + k * fs, base + k * fs + ysz,
                                                             base + k * fs + ysz + csz) for k in range(n)])

            def batch(x):
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_yuv420_batch_dev(d_in, p_planes, w, h, n, fmt, UV, stream=s)
                else:
                    ctx.clahe_packed422_to_yuv420_batch_dev(d_in, p_planes, w, h, n, fmt, UV, *CLAHE, stream=s)

            def lst(arr, pitches):
                a = (arr, w, h, *pitches, CHROMA_PLANAR, fmt, UV)
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_yuv420_frames_dev(*a, stream=s)
                else:
                    ctx.clahe_packed422_to_yuv420_frames_dev(*a, *CLAHE, stream=s)

            legs = {"B_batch": batch, "L0_list_on_the_batch_addresses": lambda x: lst(l0, (2 * w, w, w // 2)),
                    "L1_list_on_separate_allocations": lambda x: lst(l1, (ip, yp, cp))}
            for leg in legs.values():
                leg(None)
            torch.cuda.synchronize()
            assert torch.equal(out_b, out_l0), ("L0 and the batch differ", w, h, op, fmt)
            for k in (0, n // 2, n - 1):
                f = out_b[k]
                assert (torch.equal(ys[k], f[:ysz].view(h, w)) and torch.equal(us[k], f[ysz: ysz + csz].view(h // 2, w // 2))
                        and torch.equal(vs[k], f[ysz + csz:].view(h // 2, w // 2))), ("L1 and the batch differ", w, h, op, fmt, k)
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "format": FMT_NAME[fmt], "uv": "copy", "calls": args.calls}
            for name, r in timed(stream, legs, [None], args.warmup, args.calls).items():
                r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                res[name] = r
            B = res["B_batch"]["median_us"]
            res["L0_speed_over_batch_speed"] = B / res["L0_list_on_the_batch_addresses"]["median_us"]
            res["L1_speed_over_batch_speed"] = B / res["L1_list_on_separate_allocations"]["median_us"]
            rows.append(res)
            md.append([f"{w}x{h} x{n}", op, FMT_NAME[fmt]] + [cell(res[k]) for k in legs] +
                      [f"{res['L0_speed_over_batch_speed']:.3f}", f"{res['L1_speed_over_batch_speed']:.3f}"])
            print(" ".join(md[-1]), flush=True)
            del d_in, l0
        del out_b, out_l0, ins, ys, us, vs, l1
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "uv_mode": "copy",
            "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])}, "times": "microseconds per call: median [p10 .. p90]",
            "separate_allocations": "input pitch align(2W, 256), Y pitch align(W, 256), chroma pitch align(W/2, 256)",
            "note": "recorded, not enforced"}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r40_packed422_to_yuv420_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    head = ["frames", "op", "format", "(B) batch, us", "(L0) list on the batch's addresses, us", "(L1) list on separate allocations, us",
            "L0 speed / batch speed", "L1 speed / batch speed"]
    (outdir / "r40_packed422_to_yuv420_frames_ab.md").write_text("```\nFrame lists" + __doc__.split("\nFrame lists")[1] + "\n```\n\n"
                                                                + json.dumps(meta) + "\n\n" + table(head, md) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="the frame-list rows (r40) instead of the batch-form rows (r39)")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if not torch.cuda.is_available():
        sys.exit("this tool measures on the GPU: no HIP device found")
    ctx = mi_lumaeq.Context(0)
    if args.list:
        frame_lists(ctx, args)
        ctx.close()
        return
    missed = batch_forms(ctx, args)
    ctx.close()
    if missed:
        print("BAR MISSED in", missed)
        sys.exit(1)


if __name__ == "__main__":
    main()
