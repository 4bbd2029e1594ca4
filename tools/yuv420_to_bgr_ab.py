"""Planar 4:2:0 (I420) in, interleaved BGR out in the equalizing pass (mi_*_yuv420_to_bgr_batch_dev) against what a caller with I420 frames
had before it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (N)  the new form: I420 frames in, BGR images out (5.5 B/px: Y read twice, U and V once, 3 B/px written)
    (C)  the two-call composition: mi_*_yuv420_batch_dev(I420 -> NV12, MI_UV_COPY) into a preallocated tight NV12 batch, then
         mi_cvt_color_420_u8_batch_dev(MI_COLOR_YUV2BGR_NV12) (4 + 4.5 B/px)
    (B)  mi_*_nv12_to_bgr_batch_dev on the same pixels, U and V interleaved OUTSIDE the timed region: the same bytes moved with the same
         arithmetic, 16-byte chroma loads where N makes two 8-byte loads and a zip
    (N2) leg N a second time in the same rotation: the ratio of the two N medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight I420 frames per call (760 MiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR.  Low-contrast luma, random chroma.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  N, C and B agree byte for byte before anything is timed.
Bar: N is faster than C in every row by more than the run's spread (C time / N time > 1 + spread).  N / B (B time / N time) is recorded
with no bar; below 1 - 2 x spread at 64 x 4K it is reported as a finding, next to the per-slot kernel times of both legs.
After the timed legs each row runs 30 profiled calls of N and of B and records the p50 time of each kernel role.
    python tools/yuv420_to_bgr_ab.py [--out DIR] [--calls N]   -> DIR/r21_yuv420_to_bgr_ab.json and .txt (default DIR: profiles)

--list: the LIST form (mi_*_yuv420_to_bgr_frames_dev) on a software decoder's frame pool instead -- every Y, U and V plane and every image
its own allocation, pitches align(row, 256) (so the chroma pitch is a multiple of 8) -- against what such a caller had before it, same
sizes, ops and method, I420, MI_ORDER_BGR:
    (N)  the list form on the separate planes
    (B)  mi_*_yuv420_to_bgr_batch_dev on the same pixels at the same pitches in one allocation a side: the frame rate the list form has
         to meet
    (P)  one batch call with n_frames = 1 per frame
    (R)  repack: every plane copied into a batch, the batch form, every image copied out to its own allocation
    (I)  the list form again, its entries pointing INTO leg B's input allocation and into a second image allocation of leg B's shape:
         the same kernels as N on the addresses of B, which separates what the list costs from what the placement of a pool's
         allocations costs or gains
    (N2) leg N a second time in the same rotation: the ratio of the two N medians is the run-to-run spread of this very run
N, B, P, R and I agree byte for byte before anything is timed.
Bar: N is faster than P and than R in every row by more than twice the run's spread.  N / B is recorded with no bar; below
1 - 2 x spread at 64 x 4K it is reported as a finding, next to the per-slot kernel times of both legs (30 profiled calls each).
    python tools/yuv420_to_bgr_ab.py --list [--out DIR] [--calls N]   -> DIR/r22_yuv420_to_bgr_frames_ab.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR, COLOR_YUV2BGR_NV12, CHROMA_PLANAR, Yuv420Planes, Yuv420BgrFrameDev  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
ROLES = ("hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel", "tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel",
         "equalize_fused_kernel", "fused_finish_kernel", "color_kernel")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def interleave(x, w, h):
    """the NV12 batch of an I420 batch (n, H*3/2, W): the same Y rows, U and V zipped"""
    n = x.shape[0]
    flat = x.reshape(n, -1)
    ysz, csz = w * h, w * h // 4
    out = torch.empty_like(flat)
    out[:, :ysz] = flat[:, :ysz]
    out[:, ysz:] = torch.stack([flat[:, ysz: ysz + csz], flat[:, ysz + csz:]], dim=2).reshape(n, 2 * csz)
    return out.reshape(x.shape)


def align(v, a):
    return (v + a - 1) // a * a


def list_leg(args):
    """The --list run: see the module docstring."""
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        yp, cp, op_ = align(w, 256), align(w // 2, 256), align(3 * w, 256)
        ysz, csz = yp * h, cp * (h // 2)
        fi, fo = ysz + 2 * csz, op_ * h
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED2200 + w)
        # the batch: n frames of a pitched Y plane, a pitched U and a pitched V plane behind it; low-contrast luma, random chroma
        batch = torch.randint(0, 256, (n, fi), dtype=torch.uint8, device="cuda:0", generator=g)
        batch[:, :ysz].copy_(batch[:, :ysz] // 4 + 64)
        out_batch = torch.empty((n, h, op_), dtype=torch.uint8, device="cuda:0")
        # the pool: the same pixels, every plane and every image its own allocation
        ys = [batch[k, :ysz].clone() for k in range(n)]
        us = [batch[k, ysz: ysz + csz].clone() for k in range(n)]
        vs = [batch[k, ysz + csz:].clone() for k in range(n)]
        outs = [torch.empty((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        outs_p = [torch.empty((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        outs_r = [torch.empty((h, op_), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        in_r = torch.empty_like(batch)
        out_i = torch.empty_like(out_batch)
        b0, o0 = batch.data_ptr(), out_i.data_ptr()
        arr_i = (Yuv420BgrFrameDev * n)(*[Yuv420BgrFrameDev(b0 + k * fi, b0 + k * fi + ysz, b0 + k * fi + ysz + csz, o0 + k * fo) for k in range(n)])
        arr = (Yuv420BgrFrameDev * n)(*[Yuv420BgrFrameDev.of(ys[k], us[k], vs[k], outs[k]) for k in range(n)])

        def planes(base, stride):
            b = base if isinstance(base, int) else base.data_ptr()
            return Yuv420Planes(b, yp, b + ysz, b + ysz + csz, cp, stride, CHROMA_PLANAR)
        one = [Yuv420Planes(ys[k].data_ptr(), yp, us[k].data_ptr(), vs[k].data_ptr(), cp, 0, CHROMA_PLANAR) for k in range(n)]
        for op in OPS:
            eq = op == "equalize"

            def batch_call(a, out, nf):
                kw = dict(out_pitch=op_, out_frame=fo, stream=s)
                if eq:
                    ctx.equalize_hist_yuv420_to_bgr_batch_dev(a, out, w, h, nf, ORDER_BGR, **kw)
                else:
                    ctx.clahe_yuv420_to_bgr_batch_dev(a, out, w, h, nf, ORDER_BGR, *CLAHE, **kw)

            def leg_n(a=arr):
                # the entry point itself on the prebuilt address list, as a C caller with a pool has it
                if eq:
                    st = ctx._L.mi_equalize_hist_yuv420_to_bgr_frames_dev(ctx._h, a, n, w, h, yp, cp, CHROMA_PLANAR, op_, ORDER_BGR, s)
                else:
                    st = ctx._L.mi_clahe_yuv420_to_bgr_frames_dev(ctx._h, a, n, w, h, yp, cp, CHROMA_PLANAR, op_, ORDER_BGR, *CLAHE, s)
                assert st == 0, st

            def leg_i():
                leg_n(arr_i)

            def leg_b():
                batch_call(planes(batch, fi), out_batch, n)

            def leg_p():
                for k in range(n):
                    batch_call(one[k], outs_p[k], 1)

            def leg_r():
                for k in range(n):
                    in_r[k, :ysz].copy_(ys[k], non_blocking=True)
                    in_r[k, ysz: ysz + csz].copy_(us[k], non_blocking=True)
                    in_r[k, ysz + csz:].copy_(vs[k], non_blocking=True)
                batch_call(planes(in_r, fi), out_batch, n)
                for k in range(n):
                    outs_r[k].copy_(out_batch[k], non_blocking=True)

            legs = {"N_list": leg_n, "B_batch": leg_b, "P_per_frame_calls": leg_p, "R_repack": leg_r, "I_list_on_batch_addresses": leg_i,
                    "N2_list_again": leg_n}
            names = list(legs)
            stat0 = [ctx.get_stat(k) for k in ("yuv420_bgr_onepass", "yuv420_bgr_list_frames_vec", "yuv420_bgr_vec")]
            for f in (leg_n, leg_b, leg_p, leg_i):
                f()
            torch.cuda.synchronize()
            stat1 = [ctx.get_stat(k) for k in ("yuv420_bgr_onepass", "yuv420_bgr_list_frames_vec", "yuv420_bgr_vec")]
            assert [b - a for a, b in zip(stat0, stat1)] == [3 + n, 2 * n, 1 + n], "a leg did not take the one-pass path on 16 x 2 groups"
            assert torch.equal(out_i[:, :, : 3 * w], out_batch[:, :, : 3 * w]), ("I and B differ", w, h, op)
            for k in range(n):
                assert torch.equal(outs[k][:, : 3 * w], out_batch[k, :, : 3 * w]), ("N and B differ", w, h, op, k)
                assert torch.equal(outs[k][:, : 3 * w], outs_p[k][:, : 3 * w]), ("N and P differ", w, h, op, k)
            leg_r()
            torch.cuda.synchronize()
            for k in range(n):
                assert torch.equal(outs[k][:, : 3 * w], outs_r[k][:, : 3 * w]), ("N and R differ", w, h, op, k)
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "layout": "I420", "calls": args.calls,
                   "y_pitch": yp, "c_pitch": cp, "out_pitch": op_}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            t, t2 = res["N_list"]["median_us"], res["N2_list_again"]["median_us"]
            res["spread"] = abs(t / t2 - 1.0)
            for k in ("B_batch", "P_per_frame_calls", "R_repack"):
                res["N_rate_over_" + k.split("_")[0] + "_rate"] = res[k]["median_us"] / t
            res["I_rate_over_B_rate"] = res["B_batch"]["median_us"] / res["I_list_on_batch_addresses"]["median_us"]
            # the library's own kernel times, by role: where a shortfall against B would come from
            ctx.set_profiling(1)
            kern = {}
            for leg, tag in ((leg_n, "N"), (leg_b, "B")):
                ctx.profile_read(reset=True)
                for it in range(30):
                    leg()
                torch.cuda.synchronize()
                prof = ctx.profile_read(reset=True)
                for role in ROLES:
                    if prof[role]["launches"]:
                        kern.setdefault(role, {})[tag + "_p50_us"] = prof[role]["p50_ms"] * 1e3
                        kern[role][tag + "_launches_per_call"] = prof[role]["launches"] / 30
            ctx.set_profiling(0)
            res["kernels"] = kern
            rows.append(res)
            print(json.dumps(res), flush=True)
        del batch, out_batch, ys, us, vs, outs, outs_p, outs_r, in_r, out_i, arr, arr_i, one
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "layout": "I420", "warmup": args.warmup,
            "bar": "N_rate_over_P_rate > 1 + 2 x spread and N_rate_over_R_rate > 1 + 2 x spread in every row",
            "recorded": "N_rate_over_B_rate; a finding below 1 - 2 x spread at 64 x 3840x2160.  I_rate_over_B_rate: the list form on leg B's addresses"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r22_yuv420_to_bgr_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# Planar 4:2:0 in, BGR out on a frame pool: list form against batch form, per-frame calls and repacking", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; I420, CLAHE 8x8 clip 2.0, MI_ORDER_BGR; pitches align(row, 256).  Rates are frames per "
          "second.  N runs the entry point on a prebuilt address list; P and R are driven from Python, one binding call or four copies "
          "per frame, and their times contain that host work where the GPU waits for it.", "",
          "| frames | op | N list | B batch | P per-frame calls | R repack | I list on B's addresses | N / B | N / P | N / R | I / B | spread |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in ("N_list", "B_batch", "P_per_frame_calls", "R_repack", "I_list_on_batch_addresses")) +
                  f" | {r['N_rate_over_B_rate']:.3f} | {r['N_rate_over_P_rate']:.2f} | {r['N_rate_over_R_rate']:.2f} | {r['I_rate_over_B_rate']:.3f} | {r['spread']:.3f} |")
    md += ["", "Kernel p50 times by profiling slot, list form / batch form (us; launches per call in brackets):", ""]
    for r in rows:
        md.append(f"- {r['frames_per_call']} x {r['width']}x{r['height']} {r['op']}: " +
                  ", ".join(f"{role} {v.get('N_p50_us', 0):.1f} [{v.get('N_launches_per_call', 0):g}] / {v.get('B_p50_us', 0):.1f} [{v.get('B_launches_per_call', 0):g}]"
                            for role, v in r["kernels"].items()))
    (outdir / "r22_yuv420_to_bgr_frames_ab.md").write_text("\n".join(md) + "\n")
    low = [(r["width"], r["op"], round(r["N_rate_over_B_rate"], 3)) for r in rows
           if r["width"] == 3840 and r["N_rate_over_B_rate"] < 1.0 - 2.0 * r["spread"]]
    if low:
        print("FINDING: the list form is slower than the batch form beyond twice the spread in", low)
    bad = [(r["width"], r["op"]) for r in rows
           if min(r["N_rate_over_P_rate"], r["N_rate_over_R_rate"]) <= 1.0 + 2.0 * r["spread"]]
    if bad:
        print("BAR MISSED in", bad)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="the list form on separate planes (mi_*_yuv420_to_bgr_frames_dev)")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if args.list:
        return list_leg(args)
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows, lines = [], []
    for w, h, n in CASES:
        sets, inter = [], []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2100 + w + k)
            x = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device="cuda:0", generator=g)
            y = x[:, :h, :]
            y.copy_(y // 4 + 64 + 16 * k)                        # low-contrast luma (~60 populated bins), random chroma
            sets.append(x)
            inter.append(interleave(x, w, h))                    # leg B's input, made once, outside every timed region
        mid = torch.empty_like(sets[0])
        bgr_n = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")
        bgr_c, bgr_b = torch.empty_like(bgr_n), torch.empty_like(bgr_n)
        for op in OPS:
            def leg_n(k):
                a = Yuv420Planes.i420(sets[k], w, h)
                if op == "equalize":
                    ctx.equalize_hist_yuv420_to_bgr_batch_dev(a, bgr_n, w, h, n, ORDER_BGR, stream=s)
                else:
                    ctx.clahe_yuv420_to_bgr_batch_dev(a, bgr_n, w, h, n, ORDER_BGR, *CLAHE, stream=s)

            def leg_c(k):
                a, b = Yuv420Planes.i420(sets[k], w, h), Yuv420Planes.nv12(mid, w, h)
                if op == "equalize":
                    ctx.equalize_hist_yuv420_batch_dev(a, b, w, h, n, UV_COPY, stream=s)
                else:
                    ctx.clahe_yuv420_batch_dev(a, b, w, h, n, UV_COPY, *CLAHE, stream=s)
                ctx.cvt_color_420_batch_dev(mid, bgr_c, w, h, n, COLOR_YUV2BGR_NV12, stream=s)

            def leg_b(k):
                if op == "equalize":
                    ctx.equalize_hist_nv12_to_bgr_batch_dev(inter[k], None, bgr_b, w, h, n, ORDER_BGR, stream=s)
                else:
                    ctx.clahe_nv12_to_bgr_batch_dev(inter[k], None, bgr_b, w, h, n, ORDER_BGR, *CLAHE, stream=s)

            legs = {"N_new_form": leg_n, "C_two_calls": leg_c, "B_nv12_form": leg_b, "N2_new_form_again": leg_n}
            names = list(legs)
            # the legs agree before anything is timed, and N took the one-pass kernels on 16 x 2 pixel groups
            one0, vec0 = ctx.get_stat("yuv420_bgr_onepass"), ctx.get_stat("yuv420_bgr_vec")
            for f in (leg_n, leg_c, leg_b):
                f(0)
            torch.cuda.synchronize()
            assert torch.equal(bgr_n, bgr_c), ("N and C differ", w, h, op)
            assert torch.equal(bgr_n, bgr_b), ("N and B differ", w, h, op)
            assert (ctx.get_stat("yuv420_bgr_onepass"), ctx.get_stat("yuv420_bgr_vec")) == (one0 + 1, vec0 + 1), "leg N off the fast path"
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "calls": args.calls}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            tn, tn2, tc, tb = (res[k]["median_us"] for k in ("N_new_form", "N2_new_form_again", "C_two_calls", "B_nv12_form"))
            res["spread"] = abs(tn / tn2 - 1.0)
            res["C_time_over_N_time"] = tc / tn
            res["B_time_over_N_time"] = tb / tn                  # N / B as a rate: below 1, N is the slower of the two
            res["N_bytes_per_s"] = 5.5 * w * h * n / (tn * 1e-6)
            # the library's own kernel times, by role
            ctx.set_profiling(1)
            kern = {}
            for leg, tag in ((leg_n, "N"), (leg_b, "B")):
                ctx.profile_read(reset=True)
                for it in range(30):
                    leg(it & 1)
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
                    f"  | C time / N time {res['C_time_over_N_time']:.3f}  B time / N time {res['B_time_over_N_time']:.3f}  "
                    f"spread {res['spread']:.3f}  N {res['N_bytes_per_s'] / 1e12:.2f} TB/s of 5.5 B/px  | " +
                    "  ".join(f"{role} N {v.get('N_p50_us', 0):.1f} B {v.get('B_p50_us', 0):.1f} us" for role, v in kern.items()))
            print(line, flush=True)
            lines.append(line)
        del sets, inter, mid, bgr_n, bgr_c, bgr_b
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "warmup": args.warmup, "bar": "C_time_over_N_time > 1 + spread in every row",
            "recorded": "B_time_over_N_time; a finding below 1 - 2 x spread at 64 x 3840x2160"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r21_yuv420_to_bgr_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (outdir / "r21_yuv420_to_bgr_ab.txt").write_text(__doc__.split("\n    python")[0] + "\n\n" + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")
    low = [(r["width"], r["op"], round(r["B_time_over_N_time"], 3)) for r in rows
           if r["width"] == 3840 and r["B_time_over_N_time"] < 1.0 - 2.0 * r["spread"]]
    if low:
        print("FINDING: the new form is slower than the NV12 form beyond twice the spread in", low)
    bad = [(r["width"], r["op"]) for r in rows if r["C_time_over_N_time"] <= 1.0 + r["spread"]]
    if bad:
        print("BAR MISSED in", bad)
        sys.exit(1)


if __name__ == "__main__":
    main()
