"""Planar 4:2:0 (I420) <-> NV12 with the luma equalized on a decoder's frame pool and an encoder's surface pool: the LIST form
(mi_*_yuv420_frames_dev) against what such a caller had before it, in ONE process (boxes differ by several per cent, so the legs are
timed interleaved, call by call):
    (L)  the list form: every plane of every frame its own allocation
    (A)  the batch form (mi_*_yuv420_batch_dev) on the same pixels at the same pitches in one allocation a side
    (S)  one batch call with n_frames = 1 per frame, on the pools' own planes
    (R)  repack: every input plane copied into a batch, the batch form, every output plane copied out to its own allocation
    (L2) leg L a second time in the same rotation: the ratio of the two L medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 frames per call, every pitch align(row, 256); I420 -> NV12 and NV12 -> I420 under MI_UV_COPY;
equalizeHist and CLAHE 8x8 clip 2.0.  Low-contrast pixels.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  L, A, S and R agree byte for byte before anything is timed.
After the timed calls, ten profiled calls of L and of A give the per-kernel time of one call (the library's own per-launch timing).
No ratio is fixed in advance; the list form has to beat S and R by more than the spread, and a row in which it does not is reported.
    python tools/yuv420_frames_ab.py [--out DIR] [--calls N]   -> DIR/r20_yuv420_frames_ab.json and .md (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, CHROMA_INTERLEAVED, CHROMA_PLANAR, Yuv420FrameDev, Yuv420Planes  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
DIRECTIONS = [("i420", "nv12"), ("nv12", "i420")]
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
LEGS = ("L_list", "A_batch", "S_single_frame_calls", "R_repack")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def align(v, a):
    return (v + a - 1) // a * a


class Side:
    """n frames of one layout: as a batch (one allocation, constant frame stride) or as a pool (every plane its own allocation).
    planes[k] = the frame's plane tensors (rows x pitch): [Y, UV] or [Y, U, V]; rows_of / row_of: their heights and row bytes."""

    def __init__(self, fmt, w, h, n, pool, like=None):
        self.fmt, self.n = fmt, n
        planar = fmt == "i420"
        self.chroma = CHROMA_PLANAR if planar else CHROMA_INTERLEAVED
        self.y_pitch, self.c_pitch = align(w, 256), align(w // 2 if planar else w, 256)
        self.rows_of = [h] + [h // 2] * (2 if planar else 1)
        self.row_of = [w] + [w // 2 if planar else w] * (2 if planar else 1)
        pitches = [self.y_pitch] + [self.c_pitch] * (len(self.rows_of) - 1)
        sizes = [r * p for r, p in zip(self.rows_of, pitches)]
        self.frame_stride = sum(sizes)
        if pool:
            self.planes = [[torch.empty((r, p), dtype=torch.uint8, device="cuda:0") if like is None else like.planes[k][i].clone()
                            for i, (r, p) in enumerate(zip(self.rows_of, pitches))] for k in range(n)]
        else:
            self.flat = torch.empty((n, self.frame_stride), dtype=torch.uint8, device="cuda:0")
            offs = [sum(sizes[:i]) for i in range(len(sizes))]
            self.planes = [[self.flat[k, o: o + sz].view(r, p) for o, sz, r, p in zip(offs, sizes, self.rows_of, pitches)] for k in range(n)]

    def desc(self, k=0):
        p = self.planes[k]
        return Yuv420Planes(p[0].data_ptr(), self.y_pitch, p[1].data_ptr(), p[2].data_ptr() if len(p) == 3 else None, self.c_pitch,
                            self.frame_stride, self.chroma)

    def zero(self):
        for f in self.planes:
            for p in f:
                p.zero_()

    def same_pixels(self, other):
        """the W (or W/2) bytes of every row; the pitch padding is never written"""
        return all(torch.equal(a[:, :rw], b[:, :rw]) for fa, fb in zip(self.planes, other.planes) for a, b, rw in zip(fa, fb, self.row_of))


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
        for fin, fout in DIRECTIONS:
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2000 + w)
            in_batch = Side(fin, w, h, n, pool=False)
            in_batch.flat.copy_(torch.randint(0, 256, in_batch.flat.shape, dtype=torch.uint8, device="cuda:0", generator=g) // 4 + 64)
            in_pool = Side(fin, w, h, n, pool=True, like=in_batch)                  # the same pixels, every plane its own allocation
            in_r = Side(fin, w, h, n, pool=False)
            out_batch = Side(fout, w, h, n, pool=False)
            out_l, out_s, out_r = (Side(fout, w, h, n, pool=True) for _ in range(3))
            arr = (Yuv420FrameDev * n)(*[Yuv420FrameDev.of(*(in_pool.planes[k] + [None] * (3 - len(in_pool.planes[k]))),
                                                           *(out_l.planes[k] + [None] * (3 - len(out_l.planes[k])))) for k in range(n)])
            shape = (w, h, in_pool.y_pitch, in_pool.c_pitch, in_pool.chroma, out_l.y_pitch, out_l.c_pitch, out_l.chroma, UV_COPY)
            d_in, d_out = in_batch.desc(), out_batch.desc()
            d_in_r = in_r.desc()
            d_s = [(in_pool.desc(k), out_s.desc(k)) for k in range(n)]
            for op in OPS:
                eq = op == "equalize"

                def batch_call(a, b, nf):
                    if eq:
                        ctx.equalize_hist_yuv420_batch_dev(a, b, w, h, nf, UV_COPY, stream=s)
                    else:
                        ctx.clahe_yuv420_batch_dev(a, b, w, h, nf, UV_COPY, *CLAHE, stream=s)

                def leg_l():
                    # the entry point itself on the prebuilt address list, as a C caller with a pool has it
                    if eq:
                        st = ctx._L.mi_equalize_hist_yuv420_frames_dev(ctx._h, arr, n, *shape, s)
                    else:
                        st = ctx._L.mi_clahe_yuv420_frames_dev(ctx._h, arr, n, *shape, *CLAHE, s)
                    assert st == 0, st

                def leg_a():
                    batch_call(d_in, d_out, n)

                def leg_s():
                    for a, b in d_s:
                        batch_call(a, b, 1)

                def leg_r():
                    for k in range(n):
                        for dst, src in zip(in_r.planes[k], in_pool.planes[k]):
                            dst.copy_(src, non_blocking=True)
                    batch_call(d_in_r, d_out, n)
                    for k in range(n):
                        for dst, src in zip(out_r.planes[k], out_batch.planes[k]):
                            dst.copy_(src, non_blocking=True)

                legs = {"L_list": leg_l, "A_batch": leg_a, "S_single_frame_calls": leg_s, "R_repack": leg_r, "L2_list_again": leg_l}
                names = list(legs)
                # the legs agree before anything is timed
                for sd in (out_l, out_s, out_r, out_batch):
                    sd.zero()
                for f in (leg_l, leg_a, leg_s):
                    f()
                torch.cuda.synchronize()
                assert out_l.same_pixels(out_batch), ("L and A differ", w, h, fin, fout, op)
                assert out_l.same_pixels(out_s), ("L and S differ", w, h, fin, fout, op)
                y0 = out_l.planes[0][0][:, :w]
                assert int(y0.max()) > int(y0.min()), "the legs wrote nothing"
                leg_r()
                torch.cuda.synchronize()
                assert out_l.same_pixels(out_r), ("L and R differ", w, h, fin, fout, op)
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
                res = {"width": w, "height": h, "frames_per_call": n, "direction": f"{fin}->{fout}", "op": op, "uv_mode": "MI_UV_COPY",
                       "calls": args.calls, "y_pitch": in_pool.y_pitch, "c_in_pitch": in_pool.c_pitch, "c_out_pitch": out_l.c_pitch}
                for name, ev in times.items():
                    ms = [a.elapsed_time(b) for a, b in ev]
                    res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                                 "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
                l, l2 = res["L_list"]["median_us"], res["L2_list_again"]["median_us"]
                res["spread"] = abs(l / l2 - 1.0)
                for k in LEGS[1:]:
                    res["L_rate_over_" + k.split("_")[0] + "_rate"] = res[k]["median_us"] / l
                # per-kernel time of one call of L and of A: ten profiled calls each
                ctx.set_profiling(1)
                for name, f in (("L_list", leg_l), ("A_batch", leg_a)):
                    ctx.profile_read(reset=True)
                    for _ in range(10):
                        f()
                    torch.cuda.synchronize()
                    prof = {k: v for k, v in ctx.profile_read(reset=True).items() if v["launches"]}
                    res[name]["kernel_us_per_call"] = {k: round(v["total_ms"] * 100.0, 1) for k, v in prof.items()}
                    res[name]["launches_per_call"] = {k: v["launches"] // 10 for k, v in prof.items()}
                ctx.set_profiling(0)
                rows.append(res)
                print(json.dumps(res), flush=True)
            del in_batch, in_pool, in_r, out_batch, out_l, out_s, out_r, arr, d_s
            torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "uv_mode": "MI_UV_COPY", "warmup": args.warmup,
            "figure_to_meet": "L_rate_over_S_rate and L_rate_over_R_rate above 1 + spread in every row; L_rate_over_A_rate is reported"}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r20_yuv420_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# Planar 4:2:0 <-> NV12 on a frame pool and a surface pool: list form against batch form, per-frame calls and repacking", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_UV_COPY; every pitch align(row, 256).  Rates are frames per second.  "
          "L runs the entry point on a prebuilt address list; S and R are driven from Python, one binding call or five copies per frame, "
          "and their times contain that host work where the GPU waits for it.", "",
          "| frames | direction | op | L list | A batch | S per-frame calls | R repack | L / A | L / S | L / R | spread |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['direction']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS) +
                  f" | {r['L_rate_over_A_rate']:.3f} | {r['L_rate_over_S_rate']:.2f} | {r['L_rate_over_R_rate']:.2f} | {r['spread']:.3f} |")
    md += ["", "Per-kernel time of one call (us, ten profiled calls): list form / batch form.", "",
           "| frames | direction | op | L kernels | A kernels |", "|---|---|---|---|---|"]
    for r in rows:
        def fmt(d):
            return ", ".join(f"{k} {v:.0f}" for k, v in d.items())
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['direction']} | {r['op']} | "
                  f"{fmt(r['L_list']['kernel_us_per_call'])} | {fmt(r['A_batch']['kernel_us_per_call'])} |")
    (outdir / "r20_yuv420_frames_ab.md").write_text("\n".join(md) + "\n")
    lost = [(r["frames_per_call"], r["width"], r["direction"], r["op"], k) for r in rows for k in ("S", "R")
            if r[f"L_rate_over_{k}_rate"] <= 1.0 + r["spread"]]
    if lost:
        print("FINDING: the list form does not beat the leg by more than the spread in", lost)


if __name__ == "__main__":
    main()
