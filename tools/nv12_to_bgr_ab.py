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
    python tools/nv12_to_bgr_ab.py [--out DIR] [--calls N]   -> DIR/r15_nv12_to_bgr_ab.json and .txt (default DIR: profiles)

--list: the LIST form (mi_*_nv12_to_bgr_frames_dev) on a decoder's surface pool instead -- every Y plane, UV plane and image its own
allocation, pitches align(W, 256) and align(3 W, 256) -- against what such a caller had before it, same sizes, ops and method:
    (L)  the list form on the separate surfaces
    (A)  the batch form on the same pixels at the same pitches in one allocation: the frame rate the list form has to meet
    (S)  one batch call with n_frames = 1 per surface
    (R)  repack: every plane copied into a batch, the batch form, every image copied out to its own allocation
    (L2) leg L a second time in the same rotation: the ratio of the two L medians is the run-to-run spread of this very run
L, A, S and R agree byte for byte before anything is timed.  A ratio L frame rate / A frame rate below 0.95 is reported as a finding.
    python tools/nv12_to_bgr_ab.py --list [--out DIR] [--calls N]   -> DIR/r16_nv12_to_bgr_frames_ab.json and .md"""
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


def align(v, a):
    return (v + a - 1) // a * a


def list_leg(args):
    """The --list run: see the module docstring."""
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        yp, op_ = align(w, 256), align(3 * w, 256)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED1600 + w)
        # the batch: n frames of a pitched Y plane, a pitched UV plane behind it; low-contrast luma, random chroma
        batch = torch.randint(0, 256, (n, h * 3 // 2, yp), dtype=torch.uint8, device="cuda:0", generator=g)
        batch[:, :h, :].copy_(batch[:, :h, :] // 4 + 64)
        out_batch = torch.empty((n, h, op_), dtype=torch.uint8, device="cuda:0")
        # the pool: the same pixels, every plane and every image its own allocation
        ys = [batch[k, :h, :].clone() for k in range(n)]
        uvs = [batch[k, h:, :].clone() for k in range(n)]
        outs = [torch.empty((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        outs_s = [torch.empty((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        outs_r = [torch.empty((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        in_r = torch.empty_like(batch)
        fi, fo = yp * (h * 3 // 2), op_ * h
        arr = mi_lumaeq.capi._nv12_bgr_list(ys, uvs, outs, w, None, None, None, "nv12_to_bgr_ab")[0]
        for op in OPS:
            eq = op == "equalize"

            def batch_call(y, uv, out, nf):
                kw = dict(y_pitch=yp, uv_pitch=yp, in_frame=fi, out_pitch=op_, out_frame=fo, stream=s)
                if eq:
                    ctx.equalize_hist_nv12_to_bgr_batch_dev(y, uv, out, w, h, nf, ORDER_BGR, **kw)
                else:
                    ctx.clahe_nv12_to_bgr_batch_dev(y, uv, out, w, h, nf, ORDER_BGR, *CLAHE, **kw)

            def leg_l():
                # the entry point itself on the prebuilt address list, as a C caller with a pool has it: building 256 entries in
                # Python would cost as much host time as a fifth of the call
                if eq:
                    st = ctx._L.mi_equalize_hist_nv12_to_bgr_frames_dev(ctx._h, arr, n, w, h, yp, yp, op_, ORDER_BGR, s)
                else:
                    st = ctx._L.mi_clahe_nv12_to_bgr_frames_dev(ctx._h, arr, n, w, h, yp, yp, op_, ORDER_BGR, *CLAHE, s)
                assert st == 0, st

            def leg_a():
                batch_call(batch, batch.data_ptr() + yp * h, out_batch, n)

            def leg_s():
                for k in range(n):
                    batch_call(ys[k], uvs[k], outs_s[k], 1)

            def leg_r():
                for k in range(n):
                    in_r[k, :h, :].copy_(ys[k], non_blocking=True)
                    in_r[k, h:, :].copy_(uvs[k], non_blocking=True)
                batch_call(in_r, in_r.data_ptr() + yp * h, out_batch, n)
                for k in range(n):
                    outs_r[k].copy_(out_batch[k], non_blocking=True)

            legs = {"L_list": leg_l, "A_batch": leg_a, "S_single_frame_calls": leg_s, "R_repack": leg_r, "L2_list_again": leg_l}
            names = list(legs)
            one0 = ctx.get_stat("nv12_bgr_onepass")
            for f in (leg_l, leg_a, leg_s):
                f()
            torch.cuda.synchronize()
            assert ctx.get_stat("nv12_bgr_onepass") == one0 + 2 + n, "a leg did not take the one-pass path"
            for k in range(n):
                assert torch.equal(outs[k][:, : 3 * w], out_batch[k, :, : 3 * w]), ("L and A differ", w, h, op, k)
                assert torch.equal(outs[k][:, : 3 * w], outs_s[k][:, : 3 * w]), ("L and S differ", w, h, op, k)
            leg_r()
            torch.cuda.synchronize()
            for k in range(n):
                assert torch.equal(outs[k][:, : 3 * w], outs_r[k][:, : 3 * w]), ("L and R differ", w, h, op, k)
            times = {k: [] for k in names}
            for it in range(args.warmup + args.calls):
                order = names[it % len(names):] + names[: it % len(names)]
                for name in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    legs[name]()
                    e1.record(stream)
                    if it >= args.warmup:
                        times[name].append((e0, e1))
                if it % 10 == 9:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "calls": args.calls,
                   "y_pitch": yp, "uv_pitch": yp, "out_pitch": op_}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            l, l2 = res["L_list"]["median_us"], res["L2_list_again"]["median_us"]
            res["spread"] = abs(l / l2 - 1.0)
            for k in ("A_batch", "S_single_frame_calls", "R_repack"):
                res["L_rate_over_" + k.split("_")[0] + "_rate"] = res[k]["median_us"] / l
            rows.append(res)
            print(json.dumps(res), flush=True)
        del batch, out_batch, ys, uvs, outs, outs_s, outs_r, in_r
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "warmup": args.warmup,
            "figure_to_meet": "the batch form's frame rate on the same pixels in the same run: L_rate_over_A_rate >= 0.95"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r16_nv12_to_bgr_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# NV12 in, BGR out on a surface pool: list form against batch form, per-surface calls and repacking", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR.  Rates are frames per second.  L runs the entry "
          "point on a prebuilt address list; S and R are driven from Python, one binding call or three copies per surface, and their "
          "times contain that host work where the GPU waits for it.", "",
          "| frames | op | L list | A batch | S per-surface calls | R repack | L / A | L / S | L / R | spread |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in ("L_list", "A_batch", "S_single_frame_calls", "R_repack")) +
                  f" | {r['L_rate_over_A_rate']:.3f} | {r['L_rate_over_S_rate']:.2f} | {r['L_rate_over_R_rate']:.2f} | {r['spread']:.3f} |")
    (outdir / "r16_nv12_to_bgr_frames_ab.md").write_text("\n".join(md) + "\n")
    low = [(r["width"], r["op"], round(r["L_rate_over_A_rate"], 3)) for r in rows if r["L_rate_over_A_rate"] < 0.95]
    if low:
        print("FINDING: list form below 0.95 x the batch form in", low)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="the list form on separate surfaces (mi_*_nv12_to_bgr_frames_dev)")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if args.list:
        return list_leg(args)
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
