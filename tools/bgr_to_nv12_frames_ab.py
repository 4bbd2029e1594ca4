"""Interleaved BGR in, NV12 out on an image pool and an encoder's surface pool: the LIST form (mi_*_bgr_to_nv12_frames_dev) against what
such a caller had before it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (L)  the list form: every image its own allocation, every NV12 surface (Y plane, UV plane behind it) its own allocation
    (A)  the batch form on the same pixels at the same pitches in one allocation each: the frame rate the list form has to meet
    (S)  one batch call with n_frames = 1 per surface
    (R)  repack: every image copied into a batch, the batch form, every surface copied out to its own allocation
    (L2) leg L a second time in the same rotation: the ratio of the two L medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 frames per call, pitches align(3 W, 256) for the images and align(W, 256) for both planes;
equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Low-contrast pixels.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  L, A, S and R agree byte for byte before anything is timed.
A ratio L frame rate / A frame rate below 0.90 at 64 x 3840x2160 is reported as a finding.
    python tools/bgr_to_nv12_frames_ab.py [--out DIR] [--calls N]   -> DIR/r18_bgr_to_nv12_frames_ab.json and .md (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
LEGS = ("L_list", "A_batch", "S_single_frame_calls", "R_repack")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def align(v, a):
    return (v + a - 1) // a * a


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
        ip, yp = align(3 * w, 256), align(w, 256)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0x5EED1800 + w)
        # the batch: n pitched images in one allocation, n pitched NV12 surfaces in another; low-contrast pixels
        in_batch = torch.randint(0, 256, (n, h, ip), dtype=torch.uint8, device="cuda:0", generator=g)
        in_batch.copy_(in_batch // 4 + 64)
        out_batch = torch.empty((n, h * 3 // 2, yp), dtype=torch.uint8, device="cuda:0")
        # the pools: the same pixels, every image and every surface its own allocation
        ins = [in_batch[k].clone() for k in range(n)]

        def surfaces():
            return [torch.empty((h * 3 // 2, yp), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        surf, surf_s, surf_r = surfaces(), surfaces(), surfaces()
        in_r = torch.empty_like(in_batch)
        fi, fo = ip * h, yp * (h * 3 // 2)
        arr = mi_lumaeq.capi._bgr_nv12_list(ins, surf, [t[h:] for t in surf], w, None, None, None, "bgr_to_nv12_frames_ab")[0]
        for op in OPS:
            eq = op == "equalize"

            def batch_call(src, dst, nf):
                kw = dict(in_pitch=ip, in_frame=fi, y_pitch=yp, uv_pitch=yp, out_frame=fo, stream=s)
                uv = dst.data_ptr() + yp * h
                if eq:
                    ctx.equalize_hist_bgr_to_nv12_batch_dev(src, dst, uv, w, h, nf, ORDER_BGR, UV_COPY, **kw)
                else:
                    ctx.clahe_bgr_to_nv12_batch_dev(src, dst, uv, w, h, nf, ORDER_BGR, UV_COPY, *CLAHE, **kw)

            def leg_l():
                # the entry point itself on the prebuilt address list, as a C caller with a pool has it: building 256 entries in
                # Python would cost as much host time as a fifth of the call
                if eq:
                    st = ctx._L.mi_equalize_hist_bgr_to_nv12_frames_dev(ctx._h, arr, n, w, h, ip, yp, yp, ORDER_BGR, UV_COPY, s)
                else:
                    st = ctx._L.mi_clahe_bgr_to_nv12_frames_dev(ctx._h, arr, n, w, h, ip, yp, yp, ORDER_BGR, UV_COPY, *CLAHE, s)
                assert st == 0, st

            def leg_a():
                batch_call(in_batch, out_batch, n)

            def leg_s():
                for k in range(n):
                    batch_call(ins[k], surf_s[k], 1)

            def leg_r():
                for k in range(n):
                    in_r[k].copy_(ins[k], non_blocking=True)
                batch_call(in_r, out_batch, n)
                for k in range(n):
                    surf_r[k].copy_(out_batch[k], non_blocking=True)

            legs = {"L_list": leg_l, "A_batch": leg_a, "S_single_frame_calls": leg_s, "R_repack": leg_r, "L2_list_again": leg_l}
            names = list(legs)
            # the legs agree before anything is timed (the W bytes of every row; the pitch padding is never written)
            for t in surf + surf_s + surf_r + [out_batch]:
                t.zero_()
            for f in (leg_l, leg_a, leg_s):
                f()
            torch.cuda.synchronize()
            for k in range(n):
                assert torch.equal(surf[k][:, :w], out_batch[k, :, :w]), ("L and A differ", w, h, op, k)
                assert torch.equal(surf[k][:, :w], surf_s[k][:, :w]), ("L and S differ", w, h, op, k)
            assert int(surf[0][:h, :w].max()) > int(surf[0][:h, :w].min()), "the legs wrote nothing"
            leg_r()
            torch.cuda.synchronize()
            for k in range(n):
                assert torch.equal(surf[k][:, :w], surf_r[k][:, :w]), ("L and R differ", w, h, op, k)
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "uv_mode": "MI_UV_COPY", "calls": args.calls,
                   "in_pitch": ip, "y_pitch": yp, "uv_pitch": yp}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            l, l2 = res["L_list"]["median_us"], res["L2_list_again"]["median_us"]
            res["spread"] = abs(l / l2 - 1.0)
            for k in LEGS[1:]:
                res["L_rate_over_" + k.split("_")[0] + "_rate"] = res[k]["median_us"] / l
            rows.append(res)
            print(json.dumps(res), flush=True)
        del in_batch, out_batch, ins, surf, surf_s, surf_r, in_r, arr
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "MI_UV_COPY", "warmup": args.warmup,
            "figure_to_meet": "the batch form's frame rate on the same pixels in the same run: L_rate_over_A_rate >= 0.90 at 64 x 3840x2160"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r18_bgr_to_nv12_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGR in, NV12 out on an image pool and a surface pool: list form against batch form, per-surface calls and repacking", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY; pitches align(3 W, 256) / align(W, 256).  "
          "Rates are frames per second.  L runs the entry point on a prebuilt address list; S and R are driven from Python, one binding "
          "call or two copies per surface, and their times contain that host work where the GPU waits for it.", "",
          "| frames | op | L list | A batch | S per-surface calls | R repack | L / A | L / S | L / R | spread |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS) +
                  f" | {r['L_rate_over_A_rate']:.3f} | {r['L_rate_over_S_rate']:.2f} | {r['L_rate_over_R_rate']:.2f} | {r['spread']:.3f} |")
    (outdir / "r18_bgr_to_nv12_frames_ab.md").write_text("\n".join(md) + "\n")
    low = [(r["width"], r["op"], round(r["L_rate_over_A_rate"], 3)) for r in rows if r["width"] == 3840 and r["L_rate_over_A_rate"] < 0.90]
    if low:
        print("FINDING: list form below 0.90 x the batch form in", low)


if __name__ == "__main__":
    main()
