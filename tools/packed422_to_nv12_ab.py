"""Packed 4:2:2 in, NV12 out (mi_*_packed422_to_nv12_batch_dev) against the packed form and against the route a caller had before it,
in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (A)  the new form: packed frames in, NV12 frames out
    (B)  mi_*_packed422_batch_dev out of place on the same input (a packed frame comes back: not what an encoder takes)
    (C)  B followed by a torch conversion of its output to NV12 with the same chroma rule (luma gathered into the Y plane, chroma rows
         2r and 2r+1 averaged with (a + b + 1) >> 1, or 128)
64 x 3840x2160 and 256 x 1920x1080 YUY2 frames per call (1 GiB of packed input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; MI_UV_COPY and MI_UV_FILL128.  Tight layouts on both sides.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  Inputs never change.
Bars: A reaches at least 0.95 x the frame rate of B in every row (A reads the same 4 B/px in two passes and writes 1.5 B/px against
B's 2; the margin is the +- 3 % box-to-box spread on both sides of the ratio), and A beats C in every row.
After the timed legs each row runs 30 profiled calls of A and of B and records the p50 time of each kernel role, so that a row that
misses the first bar names the stage that loses the time.
    python tools/packed422_to_nv12_ab.py [--out DIR] [--calls N]   -> DIR/r13_packed422_to_nv12_ab.json and .txt (default DIR: profiles)

Frame lists (mi_*_packed422_to_nv12_frames_dev), in the same run, same method, legs interleaved:
    (L)  the list form over separately allocated buffers: every input its own allocation at pitch align(2W, 256), every Y and every UV
         plane its own allocation at pitch align(W, 256) (a capture pool in, an encoder's surface pool out)
    (a)  mi_*_packed422_to_nv12_batch_dev on the same pixels in one tight allocation
    (b)  what a caller with pools had before the list form: a torch repack of every input buffer into a tight batch, the batch form,
         a copy of every Y and UV plane out to its surface
64 x 3840x2160 and 256 x 1920x1080 YUY2 frames per call, equalizeHist and CLAHE 8x8 clip 2.0, MI_UV_COPY; inputs never change.
Expectation (recorded, not enforced): L at least 0.95 x the frame rate of (a) at 4K, and clearly ahead of (b) in every row.
    -> DIR/r14_packed422_to_nv12_frames_ab.json and .txt      (--lists-only / --no-lists run one half)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, UV_FILL128, FMT_YUY2  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
ROWS = [(op, uv) for op in ("equalize", "clahe") for uv in (UV_COPY, UV_FILL128)]
ROLES = {"equalize": ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel"),
         "clahe": ("tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel")}


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def align(x, a):
    return (x + a - 1) // a * a


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


def frame_lists(ctx, args):
    """The list-form rows: -> r14_packed422_to_nv12_frames_ab.{json,txt}"""
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    fmt, uv, clahe = FMT_YUY2, UV_COPY, (2.0, 8, 8)
    rows, lines = [], []
    for w, h, n in CASES:
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED1400 + w + n)
        d_in = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
        lane = d_in[:, :, 0::2]
        lane.copy_(lane // 4 + 64)                               # low-contrast luma, random chroma
        nv12 = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")
        tmp_in, tmp_nv12 = torch.empty_like(d_in), torch.empty_like(nv12)
        ip, op_ = align(2 * w, 256), align(w, 256)
        ins = [torch.zeros(ip * h, dtype=torch.uint8, device="cuda:0").view(h, ip)[:, : 2 * w] for _ in range(n)]
        ys = [torch.zeros(op_ * h, dtype=torch.uint8, device="cuda:0").view(h, op_)[:, :w] for _ in range(n)]
        uvs = [torch.zeros(op_ * (h // 2), dtype=torch.uint8, device="cuda:0").view(h // 2, op_)[:, :w] for _ in range(n)]
        for k in range(n):
            ins[k].copy_(d_in[k])
        for op in ("equalize", "clahe"):
            def batch(a, b):
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_nv12_batch_dev(a, b, None, w, h, n, fmt, uv, stream=s)
                else:
                    ctx.clahe_packed422_to_nv12_batch_dev(a, b, None, w, h, n, fmt, uv, *clahe, stream=s)

            def frame_list():
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_nv12_frames(ins, ys, uvs, w, h, fmt, uv, stream=s)
                else:
                    ctx.clahe_packed422_to_nv12_frames(ins, ys, uvs, w, h, fmt, uv, *clahe, stream=s)

            def repack():
                for k in range(n):
                    tmp_in[k].copy_(ins[k])
                batch(tmp_in, tmp_nv12)
                for k in range(n):
                    ys[k].copy_(tmp_nv12[k, :h])
                    uvs[k].copy_(tmp_nv12[k, h:])

            # the list's output is the batch's, frame by frame, before anything is timed
            frame_list()
            batch(d_in, nv12)
            torch.cuda.synchronize()
            for k in (0, n // 2, n - 1):
                assert torch.equal(ys[k], nv12[k, :h]) and torch.equal(uvs[k], nv12[k, h:]), (w, h, n, op, k)
            legs = {"L_list": frame_list, "a_batch": lambda: batch(d_in, nv12), "b_repack_batch_copy_out": repack}
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "uv": "copy", "format": "YUY2", "calls": args.calls}
            for name, r in timed(stream, legs, args.warmup, args.calls).items():
                r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                res[name] = r
            L = res["L_list"]["median_us"]
            res["list_speed_over_batch_speed"] = res["a_batch"]["median_us"] / L
            res["repack_over_list"] = res["b_repack_batch_copy_out"]["median_us"] / L
            line = (f"{w}x{h} x{n:3d} {op:8s} " +
                    "  ".join(f"{k} {res[k]['median_us']:8.1f} us [{res[k]['p10_us']:.1f} {res[k]['p90_us']:.1f}]" for k in legs) +
                    f"  | list speed / batch speed {res['list_speed_over_batch_speed']:.3f}  repack / list {res['repack_over_list']:.2f}")
            rows.append(res)
            print(line, flush=True)
            lines.append(line)
        del d_in, nv12, tmp_in, tmp_nv12, ins, ys, uvs, legs
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "uv_mode": "copy", "format": "YUY2",
            "clahe": {"clip": clahe[0], "tiles": list(clahe[1:])}, "input_pitch": "align(2W, 256)", "output_pitches": "align(W, 256)",
            "expectation": "list speed / batch speed >= 0.95 at 4K; repack / list > 1 in every row (recorded, not enforced)"}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r14_packed422_to_nv12_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (outdir / "r14_packed422_to_nv12_frames_ab.txt").write_text("Frame lists" + __doc__.split("\nFrame lists")[1].split("\n    ->")[0] + "\n\n"
                                                               + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lists-only", action="store_true", help="only the frame-list rows (r14)")
    ap.add_argument("--no-lists", action="store_true", help="only the batch-form rows (r13)")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    ctx = mi_lumaeq.Context(0)
    if args.lists_only:
        frame_lists(ctx, args)
        ctx.close()
        return
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    fmt, off = FMT_YUY2, 0
    rows, lines = [], []
    for w, h, n in CASES:
        sets = []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED0000 + w + k)
            x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
            lane = x[:, :, off::2]
            lane.copy_(lane // 4 + 64 + 16 * k)                   # low-contrast luma (~60 populated bins), random chroma
            sets.append(x)
        packed = torch.empty_like(sets[0])
        nv12_a = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0")
        nv12_c = torch.empty_like(nv12_a)
        for op, uv in ROWS:
            def leg_a(x):
                if op == "equalize":
                    ctx.equalize_hist_packed422_to_nv12_batch_dev(x, nv12_a, None, w, h, n, fmt, uv, stream=s)
                else:
                    ctx.clahe_packed422_to_nv12_batch_dev(x, nv12_a, None, w, h, n, fmt, uv, 2.0, 8, 8, stream=s)

            def leg_b(x):
                if op == "equalize":
                    ctx.equalize_hist_packed422_batch_dev(x, packed, w, h, n, fmt, uv, stream=s)
                else:
                    ctx.clahe_packed422_batch_dev(x, packed, w, h, n, fmt, uv, 2.0, 8, 8, stream=s)

            def leg_c(x):
                leg_b(x)
                nv12_c[:, :h, :].copy_(packed[:, :, off::2])
                if uv == UV_COPY:
                    ch = packed[:, :, 1 - off::2]
                    nv12_c[:, h:, :].copy_((ch[:, 0::2, :].to(torch.int16) + ch[:, 1::2, :] + 1) >> 1)
                else:
                    nv12_c[:, h:, :].fill_(128)

            legs = {"A_packed_to_nv12": leg_a, "B_packed": leg_b, "C_packed_then_torch_nv12": leg_c}
            names = list(legs)
            # the three legs agree before anything is timed
            x = sets[0]
            leg_a(x)
            leg_c(x)
            torch.cuda.synchronize()
            assert torch.equal(nv12_a, nv12_c), ("A and C differ", w, h, op, uv)
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
                   "format": "YUY2", "calls": args.calls}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            res["A_rate_over_B_rate"] = res["B_packed"]["median_us"] / res["A_packed_to_nv12"]["median_us"]
            res["A_rate_over_C_rate"] = res["C_packed_then_torch_nv12"]["median_us"] / res["A_packed_to_nv12"]["median_us"]
            # the library's own kernel times, by role
            ctx.set_profiling(1)
            kern = {}
            for leg, tag in ((leg_a, "A"), (leg_b, "B")):
                ctx.profile_read(reset=True)
                for it in range(30):
                    leg(sets[it & 1])
                torch.cuda.synchronize()
                prof = ctx.profile_read(reset=True)
                for role in ROLES[op]:
                    if prof[role]["launches"]:
                        kern.setdefault(role, {})[tag + "_p50_us"] = prof[role]["p50_ms"] * 1e3
            ctx.set_profiling(0)
            res["kernels"] = kern
            rows.append(res)
            line = (f"{w}x{h} x{n:3d} {op:8s} {res['uv']:7s} " +
                    "  ".join(f"{k[0]} {res[k]['median_us']:8.1f} us [{res[k]['p10_us']:.1f} {res[k]['p90_us']:.1f}]" for k in names) +
                    f"  | A rate / B rate {res['A_rate_over_B_rate']:.3f}  A rate / C rate {res['A_rate_over_C_rate']:.3f}  | " +
                    "  ".join(f"{role} A {v.get('A_p50_us', 0):.1f} B {v.get('B_p50_us', 0):.1f} us" for role, v in kern.items()))
            print(line, flush=True)
            lines.append(line)
        del sets, packed, nv12_a, nv12_c
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": 2.0, "tiles": [8, 8]},
            "bars": "A_rate_over_B_rate >= 0.95 and A_rate_over_C_rate > 1 in every row"}
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r13_packed422_to_nv12_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (outdir / "r13_packed422_to_nv12_ab.txt").write_text(__doc__.split("\n    python")[0] + "\n\n" + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")
    if not args.no_lists:
        frame_lists(ctx, args)
    ctx.close()
    bad = [(r["width"], r["op"], r["uv"]) for r in rows if r["A_rate_over_B_rate"] < 0.95 or r["A_rate_over_C_rate"] <= 1.0]
    if bad:
        print("BAR MISSED in", bad)
        sys.exit(1)


if __name__ == "__main__":
    main()
