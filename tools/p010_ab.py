"""P010 CLAHE: mi_clahe_p010_batch_dev against the composition a user would otherwise write, in ONE process (boxes differ by
several per cent, so both sides are timed interleaved, call by call):
    composition = mi_clahe_u16_batch_dev on the Y view (pitch 2W, frame stride 3WH) + a torch copy (or 0x8000 fill) of the chroma half
4K, 16 frames per call, 10-bit << 6 and 12-bit << 4 content, MI_UV_FILL128 and MI_UV_COPY, out of place and in place.
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per side; calls rotate over
64 distinct frames (4 batches of 16: 1.6 GB of input, far beyond the 256 MiB Infinity Cache); median and p10 / p90 of the per-call
times.  In place, each call's batch is first restored from a pristine copy OUTSIDE the events (CLAHE's output is full 16-bit, and
feeding it back would measure the wide-content path).  The chroma kernel alone: the library's own profiler (MI_K_LUT_APPLY is the
chroma kernel's slot, the 16-bit path never uses it), in a separate pass, reported in TB/s on its bytes (copy: 2*W*H per frame
read + written, fill: W*H written).
    python tools/p010_ab.py [--out DIR] [--calls N]      -> DIR/r07_p010_ab.json and DIR/r07_p010_ab.txt (default DIR: profiles)"""
import argparse
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_FILL128, UV_COPY  # noqa: E402

W, H, N, BATCHES = 3840, 2160, 16, 4
HBM_TBS = 8.0


def make_batches(bits, shift, seed):
    """BATCHES device batches of N P010 frames (uint8 view, N x 3WH), luma `bits` wide << shift, chroma 10-bit << 6."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    out = []
    for _ in range(BATCHES):
        y = torch.randint(0, 1 << bits, (N, H * W), dtype=torch.int32, device="cuda:0", generator=g) << shift
        uv = torch.randint(0, 1 << 10, (N, H * W // 2), dtype=torch.int32, device="cuda:0", generator=g) << 6
        s = torch.cat([y, uv], dim=1)
        b = torch.stack([(s & 0xFF).to(torch.uint8), (s >> 8).to(torch.uint8)], dim=-1).reshape(N, 3 * W * H)
        out.append(b.contiguous())
        del y, uv, s
    return out


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
    ybytes, fbytes = 2 * W * H, 3 * W * H
    L = ctx._L
    rows, lines = [], []

    def ours(d_in, d_out, uv):
        ctx.clahe_p010_batch_dev(d_in, d_out, W, H, N, uv, 2.0, 8, 8, stream=s)

    def composition(d_in, d_out, uv):
        ctx._chk(L.mi_clahe_u16_batch_dev(ctx._h, d_in.data_ptr(), 2 * W, fbytes, d_out.data_ptr(), 2 * W, fbytes, W, H, N, 2.0, 8, 8, s),
                 "mi_clahe_u16_batch_dev")
        if uv == UV_FILL128:
            d_out[:, ybytes:].view(torch.int16).fill_(-32768)          # 0x8000 in every chroma sample
        elif d_out.data_ptr() != d_in.data_ptr():
            d_out[:, ybytes:].copy_(d_in[:, ybytes:])

    for name, bits, shift in (("10-bit << 6", 10, 6), ("12-bit << 4", 12, 4)):
        src = make_batches(bits, shift, 1234 + bits)
        outs = [torch.empty_like(b) for b in src]
        work = [b.clone() for b in src]                                  # in place: restored from src before every call
        for uv in (UV_FILL128, UV_COPY):
            for inplace in (False, True):
                times = {"p010": [], "composition": []}
                fns = {"p010": ours, "composition": composition}
                for it in range(args.warmup + args.calls):
                    k = it % BATCHES
                    for side in ("p010", "composition") if it % 2 == 0 else ("composition", "p010"):
                        if inplace:
                            work[k].copy_(src[k])
                            d_in = d_out = work[k]
                        else:
                            d_in, d_out = src[k], outs[k]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        fns[side](d_in, d_out, uv)
                        e1.record(stream)
                        if it >= args.warmup:
                            times[side].append((e0, e1))
                torch.cuda.synchronize()
                res = {"content": name, "uv": "fill" if uv == UV_FILL128 else "copy", "placement": "in place" if inplace else "out of place",
                       "frames_per_call": N, "calls": args.calls}
                for side, ev in times.items():
                    ms = [a.elapsed_time(b) for a, b in ev]
                    res[side] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                                 "frames_per_s": N / (pct(ms, 0.5) * 1e-3)}
                res["ratio"] = res["p010"]["frames_per_s"] / res["composition"]["frames_per_s"]
                # the chroma kernel on its own: the library's profiler, a separate pass (events on every launch cost a little)
                if not (inplace and uv == UV_COPY):
                    ctx.set_profiling(1)
                    ctx.profile_read(reset=True)
                    for it in range(args.calls):
                        k = it % BATCHES
                        if inplace:
                            work[k].copy_(src[k])
                        ours(work[k] if inplace else src[k], work[k] if inplace else outs[k], uv)
                    torch.cuda.synchronize()
                    prof = ctx.profile_read(reset=True)["lut_apply_kernel"]
                    ctx.set_profiling(0)
                    moved = N * W * H * (2 if uv == UV_COPY else 1)
                    res["chroma_kernel"] = {"median_us": prof["p50_ms"] * 1e3, "p10_us": prof["p10_ms"] * 1e3, "p90_us": prof["p90_ms"] * 1e3,
                                            "launches": prof["launches"], "bytes": moved, "tb_per_s": moved / (prof["p50_ms"] * 1e-3) / 1e12}
                    res["chroma_kernel"]["frac_of_8tbs"] = res["chroma_kernel"]["tb_per_s"] / HBM_TBS
                else:
                    res["chroma_kernel"] = None                          # in-place copy: nothing moves, no launch
                rows.append(res)
                ck = res["chroma_kernel"]
                line = (f"{name:12s} {res['uv']:4s} {res['placement']:12s}  p010 {res['p010']['frames_per_s']:8.0f} fr/s "
                        f"(median {res['p010']['median_us']:6.1f} us, p10 {res['p010']['p10_us']:6.1f}, p90 {res['p010']['p90_us']:6.1f})  "
                        f"composition {res['composition']['frames_per_s']:8.0f} fr/s (median {res['composition']['median_us']:6.1f} us)  "
                        f"ratio {res['ratio']:.3f}  "
                        + (f"chroma kernel {ck['median_us']:5.1f} us = {ck['tb_per_s']:.2f} TB/s ({ck['frac_of_8tbs']:.2f} of 8)" if ck else "chroma: no launch"))
                print(line, flush=True)
                lines.append(line)
        del src, outs, work
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "width": W, "height": H,
            "distinct_frames": N * BATCHES, "working_set_bytes": N * BATCHES * fbytes, "clip": 2.0, "tiles": [8, 8],
            "targets": {"ratio_min": 0.95, "chroma_frac_of_8tbs_min": 0.60}}
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r07_p010_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    (out / "r07_p010_ab.txt").write_text(__doc__.split("\n    python")[0] + "\n\n" + json.dumps(meta) + "\n" + "\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
