"""Planar 4:2:0 (I420) <-> NV12 with the luma equalized in one call (mi_*_yuv420_batch_dev) against what a caller had before it, in ONE
process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (A)  the one-call form: tight I420 frames in, tight NV12 frames out (i420_to_nv12), or the other way round (nv12_to_i420)
    (B)  mi_*_u8_batch_dev on the Y planes of the same frames (frame strides W*H*3/2 on both sides), and the chroma outside the library:
         i420_to_nv12: torch.stack of the U and V planes into a preallocated buffer and one copy into the destination's UV plane;
         nv12_to_i420: two strided torch copies of the even and the odd bytes of the UV plane into the destination's U and V plane
    (A2) leg A a second time in the same rotation: the ratio of the two A medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight frames per call (rotating between two input sets: far beyond the 256 MiB Infinity Cache);
equalizeHist and CLAHE 8x8 clip 2.0; MI_UV_COPY.  Low-contrast luma (a 64-value band), full-range chroma.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  A and B agree byte for byte before anything is timed.
The chroma kernel's own rate: with profiling on, the p50 time of the launches charged to MI_K_LUT_APPLY during 30 CLAHE calls of A (for
CLAHE that slot holds the chroma launch alone), as bytes read + written per launch over that time; beside it uv_frames_kernel copying
the UV planes of the same frames (mi_clahe_nv12_frames_dev with a 63 x 1 grid, whose chroma is a launch of its own in the same slot, 64
frames a launch) in the same run.
No bar: nothing here has been measured before.  A row in which A is slower than B by more than the spread is reported as a finding.
    python tools/yuv420_ab.py [--out DIR] [--calls N]   -> DIR/r19_yuv420_ab.json and .txt (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, Yuv420Planes  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
DIRECTIONS = ("i420_to_nv12", "nv12_to_i420")
CLAHE = (2.0, 8, 8)


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
        ysz, q, frame = w * h, w * h // 4, w * h * 3 // 2
        sets = {d: [] for d in DIRECTIONS}
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED1900 + w + k)
            x = torch.randint(0, 256, (n, frame), dtype=torch.uint8, device="cuda:0", generator=g)
            x[:, :ysz].copy_(x[:, :ysz] // 4 + 64 + 16 * k)          # low-contrast luma: ~60 populated bins
            sets["i420_to_nv12"].append(x)                           # read as I420 by one direction ...
            sets["nv12_to_i420"].append(x.clone())                   # ... and as NV12 by the other: the bytes need no meaning
        out_a = torch.empty((n, frame), dtype=torch.uint8, device="cuda:0")
        out_b = torch.empty_like(out_a)
        uv_tmp = torch.empty((n, q, 2), dtype=torch.uint8, device="cuda:0")
        for direction in DIRECTIONS:
            to_nv12 = direction == "i420_to_nv12"
            mk_in, mk_out = (Yuv420Planes.i420, Yuv420Planes.nv12) if to_nv12 else (Yuv420Planes.nv12, Yuv420Planes.i420)
            for op in OPS:
                def leg_a(x):
                    a, b = mk_in(x, w, h), mk_out(out_a, w, h)
                    if op == "equalize":
                        ctx.equalize_hist_yuv420_batch_dev(a, b, w, h, n, UV_COPY, stream=s)
                    else:
                        ctx.clahe_yuv420_batch_dev(a, b, w, h, n, UV_COPY, *CLAHE, stream=s)

                def leg_b(x):
                    if op == "equalize":
                        ctx.equalize_hist_batch_dev(x, out_b, w, h, n, src_frame=frame, dst_frame=frame, stream=s)
                    else:
                        ctx.clahe_batch_dev(x, out_b, w, h, n, *CLAHE, src_frame=frame, dst_frame=frame, stream=s)
                    if to_nv12:
                        torch.stack((x[:, ysz: ysz + q], x[:, ysz + q:]), dim=2, out=uv_tmp)
                        out_b[:, ysz:].copy_(uv_tmp.view(n, 2 * q))
                    else:
                        uv = x[:, ysz:].view(n, q, 2)
                        out_b[:, ysz: ysz + q].copy_(uv[:, :, 0])
                        out_b[:, ysz + q:].copy_(uv[:, :, 1])

                legs = {"A_one_call": leg_a, "B_planar_plus_torch": leg_b, "A2_one_call_again": leg_a}
                names = list(legs)
                x0 = sets[direction][0]
                leg_a(x0)                                            # the legs agree before anything is timed
                leg_b(x0)
                torch.cuda.synchronize()
                assert torch.equal(out_a, out_b), ("A and B differ", w, h, direction, op)
                times = {k: [] for k in names}
                for it in range(args.warmup + args.calls):
                    x = sets[direction][it & 1]
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
                res = {"width": w, "height": h, "frames_per_call": n, "direction": direction, "op": op, "uv_mode": "COPY", "calls": args.calls}
                for name, ev in times.items():
                    ms = [a.elapsed_time(b) for a, b in ev]
                    res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                                 "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
                a, a2, b = (res[k]["median_us"] for k in ("A_one_call", "A2_one_call_again", "B_planar_plus_torch"))
                res["spread"] = abs(a / a2 - 1.0)
                res["A_rate_over_B_rate"] = b / a
                if op == "clahe":                                    # the chroma launch is alone in its profiling slot
                    ctx.set_profiling(1)
                    ctx.profile_read(reset=True)
                    for it in range(30):
                        leg_a(sets[direction][it & 1])
                    torch.cuda.synchronize()
                    p = ctx.profile_read(reset=True)["lut_apply_kernel"]
                    launch_frames = min(n, 256)
                    res["chroma_kernel"] = {"launches": p["launches"], "p50_us": p["p50_ms"] * 1e3, "frames_per_launch": launch_frames,
                                            "bytes_per_s": 2 * (ysz // 2) * launch_frames / (p["p50_ms"] * 1e-3)}
                    ins = [(x0[k, :ysz].view(h, w), x0[k, ysz:].view(h // 2, w)) for k in range(n)]
                    outs = [(out_b[k, :ysz].view(h, w), out_b[k, ysz:].view(h // 2, w)) for k in range(n)]
                    ctx.profile_read(reset=True)
                    for it in range(3):
                        ctx.clahe_nv12_frames(ins, outs, w, h, UV_COPY, 2.0, 63, 1, stream=s)
                    torch.cuda.synchronize()
                    p = ctx.profile_read(reset=True)["lut_apply_kernel"]
                    res["uv_frames_kernel"] = {"launches": p["launches"], "p50_us": p["p50_ms"] * 1e3, "frames_per_launch": 64,
                                               "bytes_per_s": 2 * (ysz // 2) * 64 / (p["p50_ms"] * 1e-3)}
                    ctx.set_profiling(0)
                rows.append(res)
                print(json.dumps(res), flush=True)
        del sets, out_a, out_b, uv_tmp
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r19_yuv420_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    txt = ["I420 <-> NV12 with the luma equalized: the one-call form against the planar form plus a torch interleave / deinterleave", "",
           f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process,",
           "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_UV_COPY.  Rates are frames per second.  A: mi_*_yuv420_batch_dev.",
           "B: mi_*_u8_batch_dev on the Y planes, the chroma moved by torch.  Spread: the two A legs of the same rotation against each other.",
           "Chroma kernel: p50 of its launches, bytes read + written per launch over that time; uv_frames_kernel: the same planes copied.", "",
           "frames | direction | op | A one call | B planar + torch | A / B | spread | chroma kernel | uv_frames_kernel"]
    for r in rows:
        ck, uk = r.get("chroma_kernel"), r.get("uv_frames_kernel")
        txt.append(f"{r['frames_per_call']} x {r['width']}x{r['height']} | {r['direction']} | {r['op']} | " +
                   " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in ("A_one_call", "B_planar_plus_torch")) +
                   f" | {r['A_rate_over_B_rate']:.3f} | {r['spread']:.3f} | " +
                   (f"{ck['bytes_per_s'] / 1e12:.2f} TB/s ({ck['p50_us']:.0f} us x {ck['frames_per_launch']} frames)" if ck else "-") + " | " +
                   (f"{uk['bytes_per_s'] / 1e12:.2f} TB/s ({uk['p50_us']:.0f} us x {uk['frames_per_launch']} frames)" if uk else "-"))
    slow = [(r["width"], r["direction"], r["op"], round(r["A_rate_over_B_rate"], 3)) for r in rows if r["A_rate_over_B_rate"] < 1.0 - r["spread"]]
    txt += ["", "Rows in which the one-call form is slower than the planar form plus torch by more than the spread: " + (str(slow) if slow else "none") + "."]
    (outdir / "r19_yuv420_ab.txt").write_text("\n".join(txt) + "\n")
    if slow:
        print("FINDING: the one-call form is slower than the planar form plus torch in", slow)


if __name__ == "__main__":
    main()
