"""NV12 frame lists (mi_*_nv12_frames_dev) against the existing contiguous batch forms and against what a caller with separate
surfaces does today, in ONE process (boxes differ by several per cent, so every variant is timed interleaved, call by call):
    (a)  mi_*_nv12_batch_dev on one contiguous batch (equalize: fused 0 and fused 1)
    (b)  the frame list over those same contiguous frames
    (c)  the frame list over separately allocated pitched surfaces (pitch align(W, 256), vertical stride align(H, 64))
    (d)  today's workaround for (c): a torch repack of every surface into a contiguous batch, the batch call, a copy back
64 x 3840x2160 and 256 x 1920x1080 frames per call, D2 content, MI_UV_COPY; equalizeHist and CLAHE 8x8 clip 2.0.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per variant, the variants'
order rotating every iteration; median and p10 / p90 of the per-call times.  Out of place, inputs never change.
Bar: (c) within 10 % of (a) on the same kernels (CLAHE; equalize with fused 0), and clearly faster than (d).
    python tools/nv12_frames_ab.py [--out DIR] [--calls N]   -> DIR/r08_nv12_frames_ab.json and .txt (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import synth, UV_COPY  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]


def align(x, a):
    return (x + a - 1) // a * a


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


class Surfaces:
    """n separately allocated pitched NV12 surfaces holding the frames of `batch` (n x 1.5WH)."""

    def __init__(self, batch, w, h, fill=True):
        self.pitch, self.vstride = align(w, 256), align(h, 64)
        n, p = batch.shape[0], self.pitch
        self.bufs = [torch.zeros(p * self.vstride + p * (h // 2), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
        self.y = [b[: p * h].view(h, p)[:, :w] for b in self.bufs]
        self.uv = [b[p * self.vstride: p * self.vstride + p * (h // 2)].view(h // 2, p)[:, :w] for b in self.bufs]
        if fill:
            for k in range(n):
                self.y[k].copy_(batch[k, : w * h].view(h, w))
                self.uv[k].copy_(batch[k, w * h:].view(h // 2, w))

    def planes(self):
        return list(zip(self.y, self.uv))


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
    rows, lines = [], []
    for w, h, n in CASES:
        fb = w * h * 3 // 2
        d_in = synth.nv12_batch_torch(w, h, n, "D2", "cuda:0", seed=0x5EED0000 + w)
        d_out = torch.empty_like(d_in)
        tmp_in, tmp_out = torch.empty_like(d_in), torch.empty_like(d_in)
        src, dst = Surfaces(d_in, w, h), Surfaces(d_in, w, h, fill=False)
        base, obase = d_in.data_ptr(), d_out.data_ptr()
        tight_in = [(base + k * fb, base + k * fb + w * h) for k in range(n)]
        tight_out = [(obase + k * fb, obase + k * fb + w * h) for k in range(n)]
        for op in ("equalize", "clahe"):
            def batch(a, b):
                if op == "equalize":
                    ctx.equalize_hist_nv12_batch_dev(a, b, w, h, n, UV_COPY, stream=s)
                else:
                    ctx.clahe_nv12_batch_dev(a, b, w, h, n, UV_COPY, 2.0, 8, 8, stream=s)

            def frames(ins, outs):
                if op == "equalize":
                    ctx.equalize_hist_nv12_frames(ins, outs, w, h, UV_COPY, stream=s)
                else:
                    ctx.clahe_nv12_frames(ins, outs, w, h, UV_COPY, 2.0, 8, 8, stream=s)

            def repack():
                for k in range(n):
                    tmp_in[k, : w * h].view(h, w).copy_(src.y[k])
                    tmp_in[k, w * h:].view(h // 2, w).copy_(src.uv[k])
                batch(tmp_in, tmp_out)
                for k in range(n):
                    dst.y[k].copy_(tmp_out[k, : w * h].view(h, w))
                    dst.uv[k].copy_(tmp_out[k, w * h:].view(h // 2, w))

            variants = {}
            if op == "equalize":
                variants["a_batch_fused0"] = (0, lambda: batch(d_in, d_out))
                variants["a_batch_fused1"] = (1, lambda: batch(d_in, d_out))
            else:
                variants["a_batch"] = (1, lambda: batch(d_in, d_out))
            variants["b_list_contiguous"] = (1, lambda: frames(tight_in, tight_out))
            variants["c_list_surfaces"] = (1, lambda: frames(src.planes(), dst.planes()))
            variants["d_repack_batch_copyback"] = (1, repack)
            names = list(variants)
            times = {k: [] for k in names}
            for it in range(args.warmup + args.calls):
                order = names[it % len(names):] + names[: it % len(names)]
                for name in order:
                    fused, fn = variants[name]
                    ctx.set_option("fused", fused)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    if it >= args.warmup:
                        times[name].append((e0, e1))
                if it % 20 == 19:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            ctx.set_option("fused", 1)
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "uv": "copy", "calls": args.calls}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            a_same = res["a_batch_fused0"] if op == "equalize" else res["a_batch"]
            res["c_over_a_same_kernels"] = res["c_list_surfaces"]["median_us"] / a_same["median_us"]
            res["d_over_c"] = res["d_repack_batch_copyback"]["median_us"] / res["c_list_surfaces"]["median_us"]
            if op == "equalize":
                res["c_over_a_fused"] = res["c_list_surfaces"]["median_us"] / res["a_batch_fused1"]["median_us"]
            rows.append(res)
            line = f"{w}x{h} x{n:3d} {op:8s} " + "  ".join(f"{k} {res[k]['median_us']:8.1f} us" for k in names)
            line += f"  | c/a(same kernels) {res['c_over_a_same_kernels']:.3f}  d/c {res['d_over_c']:.2f}"
            if op == "equalize":
                line += f"  c/a(fused) {res['c_over_a_fused']:.3f}"
            print(line, flush=True)
            lines.append(line)
        del d_in, d_out, tmp_in, tmp_out, src, dst
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "uv_mode": "copy", "content": "D2",
            "clahe": {"clip": 2.0, "tiles": [8, 8]}, "surface": {"pitch": "align(W, 256)", "vstride": "align(H, 64)"},
            "targets": {"c_over_a_same_kernels_max": 1.10, "d_over_c_min": 1.0}}
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r08_nv12_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (out / "r08_nv12_frames_ab.txt").write_text(__doc__.split("\n    python")[0] + "\n\n" + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
