"""Packed 4:2:2 frame lists (mi_*_packed422_frames_dev) against the batch form and against the two routes a caller with a capture
device's buffer pool had before them, in ONE process (boxes differ by several per cent, so every leg is timed interleaved, call by
call):
    (L)  the frame list over separately allocated pitched buffers (pitch align(2W, 256) bytes, every buffer its own allocation)
    (a)  mi_*_packed422_batch_dev on the same pixels in one tight allocation (frame stride 2*W*H bytes)
    (b)  one mi_*_packed422_batch_dev call with n_frames = 1 per buffer
    (c)  a torch repack of every buffer into a tight batch, the batch call, a copy back into the output buffers
64 x 3840x2160 and 256 x 1920x1080 YUY2 frames per call, equalizeHist and CLAHE 8x8 clip 2.0, MI_UV_COPY, out of place, inputs never
change.  Content: low-contrast luma, random chroma.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.
Expectation: L about 1.0 x (a) at 64 x 4K, and ahead of (b) and (c) in every row.
--list-only times (L) and (a) alone on the 256 x 1080p case and writes <label>.json only: the table-size leg (run it once per
library build, MI_LUMAEQ_LIB naming the build with the other MI_PACKED422_FRAMES_PER_LAUNCH, alternating in one job; (a) does not
depend on the table and gives each run its own yardstick).
    python tools/packed422_frames_ab.py [--out DIR] [--calls N] [--list-only --label NAME]
        -> DIR/r12_packed422_frames_ab.json and .txt (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, FMT_YUY2  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ["equalize", "clahe"]
CLAHE = (2.0, 8, 8)


def align(x, a):
    return (x + a - 1) // a * a


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def tight_batch(w, h, n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    x = torch.randint(0, 256, (n, h, 2 * w), dtype=torch.uint8, device="cuda:0", generator=g)
    lane = x[:, :, 0::2]
    lane.copy_(lane // 4 + 64)
    return x


class Buffers:
    """n separately allocated pitched buffers; .frames are their H x 2W views."""

    def __init__(self, batch, w, h, fill=True):
        self.pitch = align(2 * w, 256)
        self.bufs = [torch.zeros(self.pitch * h, dtype=torch.uint8, device="cuda:0") for _ in range(batch.shape[0])]
        self.frames = [b.view(h, self.pitch)[:, : 2 * w] for b in self.bufs]
        if fill:
            for k, f in enumerate(self.frames):
                f.copy_(batch[k])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list-only", action="store_true")
    ap.add_argument("--label", default="list_only")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows, lines = [], []
    for w, h, n in CASES:
        if args.list_only and n != 256:
            continue
        d_in = tight_batch(w, h, n, 0x5EED0000 + w + n)
        d_out = torch.empty_like(d_in)
        src, dst = Buffers(d_in, w, h), Buffers(d_in, w, h, fill=False)
        if not args.list_only:
            tmp_in, tmp_out = torch.empty_like(d_in), torch.empty_like(d_in)
        for op in OPS:
            def batch(a, b, k=n, **kw):
                if op == "equalize":
                    ctx.equalize_hist_packed422_batch_dev(a, b, w, h, k, FMT_YUY2, UV_COPY, stream=s, **kw)
                else:
                    ctx.clahe_packed422_batch_dev(a, b, w, h, k, FMT_YUY2, UV_COPY, *CLAHE, stream=s, **kw)

            def frame_list():
                if op == "equalize":
                    ctx.equalize_hist_packed422_frames(src.frames, dst.frames, w, h, FMT_YUY2, UV_COPY, stream=s)
                else:
                    ctx.clahe_packed422_frames(src.frames, dst.frames, w, h, FMT_YUY2, UV_COPY, *CLAHE, stream=s)

            def per_frame():
                for k in range(n):
                    batch(src.frames[k], dst.frames[k], 1, in_pitch=src.pitch, out_pitch=dst.pitch)

            def repack():
                for k in range(n):
                    tmp_in[k].copy_(src.frames[k])
                batch(tmp_in, tmp_out)
                for k in range(n):
                    dst.frames[k].copy_(tmp_out[k])

            legs = {"L_list": frame_list, "a_batch": lambda: batch(d_in, d_out)}
            if not args.list_only:
                legs["b_one_call_per_frame"] = per_frame
                legs["c_repack_batch_copyback"] = repack
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "uv": "copy", "format": "YUY2", "calls": args.calls}
            for name, r in timed(stream, legs, args.warmup, args.calls).items():
                r["frames_per_s"] = n / (r["median_us"] * 1e-6)
                res[name] = r
            L = res["L_list"]["median_us"]
            res["list_speed_over_batch_speed"] = res["a_batch"]["median_us"] / L
            line = f"{w}x{h} x{n:3d} {op:8s} " + "  ".join(f"{k} {res[k]['median_us']:8.1f} us [{res[k]['p10_us']:.1f} {res[k]['p90_us']:.1f}]" for k in legs)
            line += f"  | list speed / batch speed {res['list_speed_over_batch_speed']:.3f}"
            if not args.list_only:
                res["b_over_list"] = res["b_one_call_per_frame"]["median_us"] / L
                res["c_over_list"] = res["c_repack_batch_copyback"]["median_us"] / L
                line += f"  per-frame calls / list {res['b_over_list']:.2f}  repack / list {res['c_over_list']:.2f}"
            # the list's output is the batch's, frame by frame (a timing tool that compares nothing proves nothing)
            dst.bufs[0].zero_()
            dst.bufs[n - 1].zero_()
            frame_list()
            batch(d_in, d_out)
            torch.cuda.synchronize()
            for k in (0, n - 1):
                assert torch.equal(dst.frames[k], d_out[k]), (w, h, n, op, k)
            rows.append(res)
            print(line, flush=True)
            lines.append(line)
        del d_in, d_out, src, dst, legs
        if not args.list_only:
            del tmp_in, tmp_out
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "library_path": str(mi_lumaeq.lib_path().name),
            "uv_mode": "copy", "format": "YUY2", "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])}, "buffer_pitch": "align(2W, 256)",
            "expectation": "list about 1.0 x batch at 64 x 4K; per-frame calls / list > 1 and repack / list > 1 in every row"}
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    if args.list_only:
        (out / f"{args.label}.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    else:
        (out / "r12_packed422_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
        (out / "r12_packed422_frames_ab.txt").write_text(__doc__.split("\n--list-only")[0] + "\n\n" + json.dumps(meta) + "\n"
                                                         + "\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
