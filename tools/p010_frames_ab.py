"""P010 frame lists (mi_clahe_p010_frames_dev) against the tight batch form and against what a caller with separate surfaces does
today, in ONE process (boxes differ by several per cent, so every variant is timed interleaved, call by call):
    (a)  mi_clahe_p010_batch_dev on one tight batch (frame pitch 3*W*H bytes)
    (c)  the frame list over separately allocated pitched surfaces holding the same pixels (pitch align(2W, 256) bytes, vertical
         stride align(H, 64), the UV plane at pitch * vstride)
    (d)  today's workaround for (c): a torch repack of every surface into a tight batch, the batch call, a copy back
4K P010 at 16 and 64 frames per call; 12-bit and 14-bit content at 4K x 16; 256 x 1920x1080 P010.  Content: uniform samples of the
bit depth (10 and 12 bits in the high bits of the word, as P010 / P012 store them; 14 bits in the low bits), MI_UV_COPY, CLAHE 8x8
clip 2.0, out of place, inputs never change.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per variant, the variants'
order rotating every iteration; median and p10 / p90 of the per-call times.
Target: (c) >= 0.90x the speed of (a) at 4K 10-bit, and faster than (d).
--batch-only times (a) alone on the 10-bit cases (the no-regression leg: run this file from a parent's tree and from this one,
alternating, in one job) and writes <label>.json only.
    python tools/p010_frames_ab.py [--out DIR] [--calls N] [--batch-only --label NAME]
        -> DIR/r09_p010_frames_ab.json and .txt (default DIR: profiles)"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY  # noqa: E402

# (width, height, frames per call, content)
CASES = [(3840, 2160, 16, "10-bit"), (3840, 2160, 64, "10-bit"), (3840, 2160, 16, "12-bit"), (3840, 2160, 16, "14-bit"),
         (1920, 1080, 256, "10-bit")]
CONTENT = {"10-bit": (10, 6), "12-bit": (12, 4), "14-bit": (14, 0)}     # bits, shift into the word
CLAHE = (2.0, 8, 8)


def align(x, a):
    return (x + a - 1) // a * a


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def tight_batch(w, h, n, content, seed):
    """n P010 frames (n x 3WH bytes as int16 samples) on the device: luma uniform over the content's bit depth, chroma 10-bit."""
    bits, shift = CONTENT[content]
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    b = torch.empty((n, 3 * h // 2, w), dtype=torch.int32, device="cuda:0")
    b[:, :h] = torch.randint(0, 1 << bits, (n, h, w), generator=g, device="cuda:0", dtype=torch.int32) << shift
    b[:, h:] = torch.randint(0, 1 << 10, (n, h // 2, w), generator=g, device="cuda:0", dtype=torch.int32) << 6
    return (b - ((b >> 15) << 16)).to(torch.int16)                   # the same 16 bits, as the int16 tensors the binding takes


class Surfaces:
    """n separately allocated pitched P010 surfaces holding the frames of `batch` (n x 3H/2 x W int16 samples)."""

    def __init__(self, batch, w, h, fill=True):
        self.pitch, self.vstride = align(2 * w, 256), align(h, 64)
        n, ps = batch.shape[0], self.pitch // 2
        self.bufs = [torch.zeros(ps * self.vstride + ps * (h // 2), dtype=torch.int16, device="cuda:0") for _ in range(n)]
        self.y = [b[: ps * h].view(h, ps)[:, :w] for b in self.bufs]
        self.uv = [b[ps * self.vstride: ps * self.vstride + ps * (h // 2)].view(h // 2, ps)[:, :w] for b in self.bufs]
        if fill:
            for k in range(n):
                self.y[k].copy_(batch[k, :h])
                self.uv[k].copy_(batch[k, h:])

    def planes(self):
        return list(zip(self.y, self.uv))


def timed(stream, variants, warmup, calls):
    names = list(variants)
    times = {k: [] for k in names}
    for it in range(warmup + calls):
        order = names[it % len(names):] + names[: it % len(names)]
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            variants[name]()
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
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--label", default="batch_only")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows, lines = [], []
    for w, h, n, content in CASES:
        if args.batch_only and content != "10-bit":
            continue
        d_in = tight_batch(w, h, n, content, 0x5EED0000 + w + n)
        d_out = torch.empty_like(d_in)

        def batch(a, b):
            ctx.clahe_p010_batch_dev(a, b, w, h, n, UV_COPY, *CLAHE, stream=s)

        variants = {"a_batch": lambda: batch(d_in, d_out)}
        if not args.batch_only:
            tmp_in, tmp_out = torch.empty_like(d_in), torch.empty_like(d_in)
            src, dst = Surfaces(d_in, w, h), Surfaces(d_in, w, h, fill=False)

            def repack():
                for k in range(n):
                    tmp_in[k, :h].copy_(src.y[k])
                    tmp_in[k, h:].copy_(src.uv[k])
                batch(tmp_in, tmp_out)
                for k in range(n):
                    dst.y[k].copy_(tmp_out[k, :h])
                    dst.uv[k].copy_(tmp_out[k, h:])

            variants["c_list_surfaces"] = lambda: ctx.clahe_p010_frames(src.planes(), dst.planes(), w, h, UV_COPY, *CLAHE, stream=s)
            variants["d_repack_batch_copyback"] = repack
        res = {"width": w, "height": h, "frames_per_call": n, "content": content, "uv": "copy", "calls": args.calls}
        for name, r in timed(stream, variants, args.warmup, args.calls).items():
            r["frames_per_s"] = n / (r["median_us"] * 1e-6)
            res[name] = r
        line = f"{w}x{h} x{n:3d} {content:6s} " + "  ".join(f"{k} {res[k]['median_us']:8.1f} us" for k in variants)
        if not args.batch_only:
            res["a_over_c_speed"] = res["a_batch"]["median_us"] / res["c_list_surfaces"]["median_us"]
            res["d_over_c"] = res["d_repack_batch_copyback"]["median_us"] / res["c_list_surfaces"]["median_us"]
            line += f"  | list speed / batch speed {res['a_over_c_speed']:.3f}  repack / list {res['d_over_c']:.2f}"
            # the list's output is the batch's, frame by frame (a timing tool that compares nothing proves nothing)
            for k in (0, n - 1):
                assert torch.equal(dst.y[k], d_out[k, :h]) and torch.equal(dst.uv[k], d_out[k, h:]), (w, h, n, content, k)
        rows.append(res)
        print(line, flush=True)
        lines.append(line)
        del d_in, d_out, variants
        if not args.batch_only:
            del tmp_in, tmp_out, src, dst
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "uv_mode": "copy",
            "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])}, "surface": {"pitch": "align(2W, 256)", "vstride": "align(H, 64)"},
            "targets": {"list_speed_over_batch_speed_min_4k_10bit": 0.90, "repack_over_list_min": 1.0}}
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    if args.batch_only:
        (out / f"{args.label}.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    else:
        (out / "r09_p010_frames_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
        (out / "r09_p010_frames_ab.txt").write_text(__doc__.split("\n--batch-only")[0] + "\n\n" + json.dumps(meta) + "\n"
                                                    + "\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
