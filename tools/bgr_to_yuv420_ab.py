"""Interleaved BGR in, equalized planar 4:2:0 (I420) out in one call (mi_*_bgr_to_yuv420_batch_dev) against what a caller had to write
before it, in ONE process (boxes differ by several per cent, so the legs are timed interleaved, call by call):
    (a)  the new form on a tight I420 batch (equalizeHist 6.5 B/px, CLAHE 7.5)
    (b)  the two calls that served a tight batch before: mi_cvt_color_420_u8_batch_dev(MI_COLOR_BGR2YUV_I420) into the batch, then
         mi_*_u8_batch_dev in place on its Y rows
    (c)  the new form on pitched, separately offset planes in one allocation (every pitch align(row, 256))
    (d)  what a caller needed for (c) before: mi_*_bgr_to_nv12_batch_dev into a tight scratch NV12 batch, then
         mi_*_yuv420_batch_dev(NV12 -> I420, MI_UV_COPY) into the pitched planes.  (The second call maps the luma once more, so the leg
         stands for the bytes moved and the launches made; its output is not compared.)
    (e)  mi_*_bgr_to_nv12_batch_dev on the same pixels into a tight NV12 batch: the planar-store against interleaved-store ratio, with
         the conversion kernel's own time from the profile
    (a2) leg (a) a second time in the same rotation: the ratio of the two medians is the run-to-run spread of this very run
64 x 3840x2160 and 256 x 1920x1080 tight BGR images per call (1.5 GiB of input, rotating between two such sets: far beyond the 256 MiB
Infinity Cache); equalizeHist and CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Low-contrast pixels (every channel in a 64-value band).
Method: every call bracketed by its own pair of HIP events on the stream; 20 warm-up and 200 timed calls per leg, the legs' order
rotating every iteration; median and p10 / p90 of the per-call times.  (a) and (b) agree byte for byte, and the planes of (c) are the
planes of (a), before anything is timed.
No bar: the byte counts predict parity between (a) and (b), not a gain.  A row in which the new form is slower than what it replaces by
more than the spread is reported as a finding.  After the timed legs each row runs 30 profiled calls of (a), (c) and (e) and records
the p50 time of the conversion kernel.
    python tools/bgr_to_yuv420_ab.py [--out DIR] [--calls N]   -> DIR/r23_bgr_to_yuv420_ab.json and .md (default DIR: profiles)

--list: the frame-list form (mi_*_bgr_to_yuv420_frames_dev) on POOLS -- every image its own allocation, every output frame three
separately allocated planes at pitches align(row, 256), what a renderer and a software encoder hand over -- against the routes such a
caller had before it, under the same protocol (same cases, pixels, ops, warm-up, timed calls, rotation and per-call HIP events):
    (l)  ONE list call on the pools
    (a)  one mi_*_bgr_to_yuv420_batch_dev call per frame with n_frames = 1, on the same pools
    (b)  repacking: every image copied into a strided scratch batch, ONE batch call into strided scratch planes at the same pitches,
         every plane copied out into the pool (device-to-device copies on the same stream: 4 per frame)
    (c)  the batch form on a tight batch of the same frames: the ceiling; (c2) the same a second time in the rotation: the spread
    (l2) ONE list call whose entries are the addresses of (c)'s tight batches: the list kernels and the 64-frame chunk alone, without
         the pools' placement and pitches
The three pools of (l), (a) and (b) hold the planes of (c) before anything is timed.  Legs (a) and (b) make n and 4n + 1 calls from
Python per timed call, so their times include what the interpreter adds to each; a C caller pays less per call, not fewer calls.
No bar.  A row in which the list form is slower than (a) or (b), or trails (c) by more than the spread, is reported as a finding.
After the timed legs each row runs 30 profiled calls of (l), (l2) and (c) and records every kernel's launches per call and p50 time.
    python tools/bgr_to_yuv420_ab.py --list [--out DIR] [--calls N]   -> DIR/r24_bgr_to_yuv420_ab_list.json and .md"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))
import mi_lumaeq  # noqa: E402
from mi_lumaeq import UV_COPY, ORDER_BGR, COLOR_BGR2YUV_I420, CHROMA_PLANAR, Yuv420Planes, BgrYuv420FrameDev  # noqa: E402

CASES = [(3840, 2160, 64), (1920, 1080, 256)]
OPS = ("equalize", "clahe")
CLAHE = (2.0, 8, 8)
BYTES_PER_PX = {"equalize": 6.5, "clahe": 7.5}
LEGS = ("a_tight", "b_two_calls", "c_pitched", "d_via_nv12", "e_nv12_out", "a2_tight_again")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def align(n, a):
    return (n + a - 1) // a * a


LIST_LEGS = ("l_list", "a_per_frame", "b_repack", "c_batch_tight", "c2_batch_tight_again", "l2_list_on_batch")


def main_list(args):
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        ysz, q, frame = w * h, w * h // 4, w * h * 3 // 2
        yp, cp = align(w, 256), align(w // 2, 256)
        u_off = yp * h + 256
        v_off = u_off + cp * (h // 2) + 256
        fstride = v_off + cp * (h // 2) + 256
        sets, pools_in = [], []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2300 + w + k)
            x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda:0", generator=g)
            x.copy_(x // 4 + 64 + 16 * k)                        # low contrast: ~60 populated luma bins
            sets.append(x)
            # the image pool: every image its own allocation, of a size of its own so that no allocator lays them out at one stride
            pool = [torch.empty((3 * ysz + 256 * (f % 3),), dtype=torch.uint8, device="cuda:0") for f in range(n)]
            for f in range(n):
                pool[f][: 3 * ysz].copy_(x[f].reshape(-1))
            pools_in.append(pool)

        def surfaces():
            """an encoder's frame pool: per frame three separately allocated planes"""
            return [(torch.zeros((yp * h,), dtype=torch.uint8, device="cuda:0"), torch.zeros((cp * (h // 2),), dtype=torch.uint8, device="cuda:0"),
                     torch.zeros((cp * (h // 2),), dtype=torch.uint8, device="cuda:0")) for _ in range(n)]
        out_l, out_a, out_b = surfaces(), surfaces(), surfaces()
        i420_c = torch.empty((n, frame), dtype=torch.uint8, device="cuda:0")
        scratch_in = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")                   # leg (b): the strided batch in
        scratch_out = torch.zeros((n * fstride,), dtype=torch.uint8, device="cuda:0")                # leg (b): the strided planes out
        sb = scratch_out.data_ptr()
        scratch_planes = Yuv420Planes(sb, yp, sb + u_off, sb + v_off, cp, fstride, CHROMA_PLANAR)
        scratch_views = [(scratch_out[f * fstride: f * fstride + yp * h], scratch_out[f * fstride + u_off: f * fstride + u_off + cp * (h // 2)],
                          scratch_out[f * fstride + v_off: f * fstride + v_off + cp * (h // 2)]) for f in range(n)]
        entries = [(BgrYuv420FrameDev * n)(*[BgrYuv420FrameDev(pools_in[k][f].data_ptr(), *(p.data_ptr() for p in out_l[f])) for f in range(n)])
                   for k in range(2)]
        planes_a = [Yuv420Planes(y.data_ptr(), yp, u.data_ptr(), v.data_ptr(), cp, 0, CHROMA_PLANAR) for y, u, v in out_a]
        tight = Yuv420Planes.i420(i420_c, w, h)
        i420_l2 = torch.empty_like(i420_c)                      # leg (l2): a tight batch of its own, named frame by frame
        b2 = i420_l2.data_ptr()
        entries2 = [(BgrYuv420FrameDev * n)(*[BgrYuv420FrameDev(sets[k][f].data_ptr(), b2 + f * frame, b2 + f * frame + ysz,
                                                                b2 + f * frame + ysz + q) for f in range(n)]) for k in range(2)]
        for op in OPS:
            eq = op == "equalize"

            def batch(x, dst, nf, **kw):
                if eq:
                    ctx.equalize_hist_bgr_to_yuv420_batch_dev(x, dst, w, h, nf, ORDER_BGR, UV_COPY, stream=s, **kw)
                else:
                    ctx.clahe_bgr_to_yuv420_batch_dev(x, dst, w, h, nf, ORDER_BGR, UV_COPY, *CLAHE, stream=s, **kw)

            def leg_l(k, on_batch=False):
                a = (entries2[k], w, h, 3 * w, w, w // 2) if on_batch else (entries[k], w, h, 3 * w, yp, cp)
                a += (CHROMA_PLANAR, ORDER_BGR, UV_COPY)
                if eq:
                    ctx.equalize_hist_bgr_to_yuv420_frames_dev(*a, stream=s)
                else:
                    ctx.clahe_bgr_to_yuv420_frames_dev(*a, *CLAHE, stream=s)

            def leg_a(k):
                for f in range(n):
                    batch(pools_in[k][f].data_ptr(), planes_a[f], 1, in_frame=0)

            def leg_b(k):
                for f in range(n):
                    scratch_in[f].view(-1).copy_(pools_in[k][f][: 3 * ysz], non_blocking=True)
                batch(scratch_in, scratch_planes, n)
                for f in range(n):
                    for dst, src in zip(out_b[f], scratch_views[f]):
                        dst.copy_(src, non_blocking=True)

            legs = {"l_list": leg_l, "a_per_frame": leg_a, "b_repack": leg_b, "c_batch_tight": lambda k: batch(sets[k], tight, n),
                    "c2_batch_tight_again": lambda k: batch(sets[k], tight, n), "l2_list_on_batch": lambda k: leg_l(k, True)}
            names = list(LIST_LEGS)
            stat0 = [ctx.get_stat(k) for k in ("bgr_yuv420_list_frames_vec", "bgr_yuv420_list_frames_bytes", "bgr_yuv420_bytes")]
            for name in names:                                   # the legs agree before anything is timed
                legs[name](0)
            torch.cuda.synchronize()
            stat1 = [ctx.get_stat(k) for k in ("bgr_yuv420_list_frames_vec", "bgr_yuv420_list_frames_bytes", "bgr_yuv420_bytes")]
            assert [b - a for a, b in zip(stat0, stat1)] == [2 * n, 0, 0], "a leg left the 16 x 2 groups"
            assert torch.equal(i420_l2, i420_c), ("(l2) and (c) differ", w, h, op)
            for tag, pool in (("l", out_l), ("a", out_a), ("b", out_b)):
                for f in range(n):
                    y, u, v = pool[f]
                    assert torch.equal(y.view(h, yp)[:, :w].reshape(-1), i420_c[f, :ysz]), ("Y of (%s)" % tag, f, w, h, op)
                    assert torch.equal(u.view(h // 2, cp)[:, : w // 2].reshape(-1), i420_c[f, ysz: ysz + q]), ("U of (%s)" % tag, f, w, h, op)
                    assert torch.equal(v.view(h // 2, cp)[:, : w // 2].reshape(-1), i420_c[f, ysz + q:]), ("V of (%s)" % tag, f, w, h, op)
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "uv_mode": "COPY", "calls": args.calls,
                   "pitches": {"in": 3 * w, "y": yp, "c": cp}, "chunk_frames": {"list": 64, "batch": 256}}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            med = {k: res[k]["median_us"] for k in names}
            res["spread"] = abs(med["c_batch_tight"] / med["c2_batch_tight_again"] - 1.0)
            res["list_rate_over_per_frame_rate"] = med["a_per_frame"] / med["l_list"]
            res["list_rate_over_repack_rate"] = med["b_repack"] / med["l_list"]
            res["list_rate_over_batch_rate"] = med["c_batch_tight"] / med["l_list"]
            res["list_on_batch_rate_over_batch_rate"] = med["c_batch_tight"] / med["l2_list_on_batch"]
            res["list_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (med["l_list"] * 1e-6)
            ctx.set_profiling(1)
            kern = {}
            for tag in ("l_list", "l2_list_on_batch", "c_batch_tight"):
                ctx.profile_read(reset=True)
                for it in range(30):
                    legs[tag](it & 1)
                torch.cuda.synchronize()
                kern[tag] = {k: {"launches_per_call": v["launches"] / 30, "p50_us": v["p50_ms"] * 1e3}
                             for k, v in ctx.profile_read(reset=True).items() if v["launches"]}
            ctx.set_profiling(0)
            res["kernels"] = kern
            rows.append(res)
            print(json.dumps(res), flush=True)
        del sets, pools_in, out_l, out_a, out_b, i420_c, i420_l2, scratch_in, scratch_out, scratch_views, entries, entries2, planes_a
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r24_bgr_to_yuv420_ab_list.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGR in, equalized planar 4:2:0 out on pools: the list form against the routes it replaces", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Rates are frames per second.  Every image "
          "is its own allocation (tight rows), every output frame three separately allocated planes at pitches align(row, 256).  (l): ONE "
          "mi_*_bgr_to_yuv420_frames_dev call.  (a): one mi_*_bgr_to_yuv420_batch_dev call per frame, n_frames = 1.  (b): every image "
          "copied into a strided scratch batch, one batch call into strided scratch planes, every plane copied out.  (c): the batch form "
          "on a tight batch of the same frames.  (l2): one list call naming the frames of such a tight batch.  Spread: the two (c) legs "
          "of the same rotation against each other.  (a) and (b) are driven from Python: their times include the interpreter's share of "
          "n and 4n + 1 calls.  Kernels: launches per call x p50 of a launch, from 30 profiled calls after the timed legs.", "",
          "| frames | op | (l) list | (a) per frame | (b) repack | (c) batch, tight | (l2) list on a tight batch | l / a | l / b | l / c | l2 / c | spread |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LIST_LEGS[:4] + LIST_LEGS[5:]) +
                  f" | {r['list_rate_over_per_frame_rate']:.3f} | {r['list_rate_over_repack_rate']:.3f} "
                  f"| {r['list_rate_over_batch_rate']:.3f} | {r['list_on_batch_rate_over_batch_rate']:.3f} | {r['spread']:.3f} |")
    md += ["", "| frames | op | leg | kernels: launches per call x p50 us |", "|---|---|---|---|"]
    for r in rows:
        for tag, kk in r["kernels"].items():
            md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | {tag} | " +
                      ", ".join(f"{k} {v['launches_per_call']:g} x {v['p50_us']:.0f}" for k, v in kk.items()) + " |")
    slow = [(r["width"], r["op"], k, round(r[k], 3)) for r in rows for k in ("list_rate_over_per_frame_rate", "list_rate_over_repack_rate")
            if r[k] < 1.0]
    behind = [(r["width"], r["op"], round(r["list_rate_over_batch_rate"], 3), round(r["spread"], 3)) for r in rows
              if r["list_rate_over_batch_rate"] < 1.0 - r["spread"]]
    md += ["", "Rows in which the list form is slower than a route it replaces: " + (str(slow) if slow else "none") + ".",
           "Rows in which the list form trails the tight batch form by more than the spread (width, op, l / c, spread): " +
           (str(behind) if behind else "none") + "."]
    (outdir / "r24_bgr_to_yuv420_ab_list.md").write_text("\n".join(md) + "\n")
    if slow:
        print("FINDING: the list form is slower than a route it replaces in", slow)
    if behind:
        print("FINDING: the list form trails the tight batch form by more than the spread in", behind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--list", action="store_true", help="the frame-list form on pools against the routes it replaces")
    args = ap.parse_args()
    assert args.calls >= 200 and args.warmup >= 20, "the method wants >= 20 warm-up and >= 200 timed calls"
    if args.list:
        return main_list(args)
    ctx = mi_lumaeq.Context(0)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    rows = []
    for w, h, n in CASES:
        ysz, q, frame = w * h, w * h // 4, w * h * 3 // 2
        sets = []
        for k in range(2):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(0x5EED2300 + w + k)
            x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda:0", generator=g)
            x.copy_(x // 4 + 64 + 16 * k)                        # low contrast: ~60 populated luma bins
            sets.append(x)
        i420_a = torch.empty((n, frame), dtype=torch.uint8, device="cuda:0")
        i420_b = torch.empty_like(i420_a)
        nv12_e = torch.empty_like(i420_a)
        scratch = torch.empty_like(i420_a)                      # leg (d): the NV12 batch in between
        yp, cp = align(w, 256), align(w // 2, 256)
        u_off = yp * h + 256
        v_off = u_off + cp * (h // 2) + 256
        fstride = v_off + cp * (h // 2) + 256
        pitched = [torch.zeros((n * fstride,), dtype=torch.uint8, device="cuda:0") for _ in range(2)]       # legs (c) and (d)

        def planes_of(t):
            b = t.data_ptr()
            return Yuv420Planes(b, yp, b + u_off, b + v_off, cp, fstride, CHROMA_PLANAR)
        tight, p_c, p_d, nv12_in = Yuv420Planes.i420(i420_a, w, h), planes_of(pitched[0]), planes_of(pitched[1]), Yuv420Planes.nv12(scratch, w, h)
        for op in OPS:
            eq = op == "equalize"

            def new_form(x, dst):
                if eq:
                    ctx.equalize_hist_bgr_to_yuv420_batch_dev(x, dst, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                else:
                    ctx.clahe_bgr_to_yuv420_batch_dev(x, dst, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

            def leg_b(x):
                ctx.cvt_color_420_batch_dev(x, i420_b, w, h, n, COLOR_BGR2YUV_I420, stream=s)
                if eq:
                    ctx.equalize_hist_batch_dev(i420_b, i420_b, w, h, n, src_frame=frame, dst_frame=frame, stream=s)
                else:
                    ctx.clahe_batch_dev(i420_b, i420_b, w, h, n, *CLAHE, src_frame=frame, dst_frame=frame, stream=s)

            def to_nv12(x, dst):
                if eq:
                    ctx.equalize_hist_bgr_to_nv12_batch_dev(x, dst, None, w, h, n, ORDER_BGR, UV_COPY, stream=s)
                else:
                    ctx.clahe_bgr_to_nv12_batch_dev(x, dst, None, w, h, n, ORDER_BGR, UV_COPY, *CLAHE, stream=s)

            def leg_d(x):
                to_nv12(x, scratch)
                if eq:
                    ctx.equalize_hist_yuv420_batch_dev(nv12_in, p_d, w, h, n, UV_COPY, stream=s)
                else:
                    ctx.clahe_yuv420_batch_dev(nv12_in, p_d, w, h, n, UV_COPY, *CLAHE, stream=s)

            legs = {"a_tight": lambda x: new_form(x, tight), "b_two_calls": leg_b, "c_pitched": lambda x: new_form(x, p_c),
                    "d_via_nv12": leg_d, "e_nv12_out": lambda x: to_nv12(x, nv12_e), "a2_tight_again": lambda x: new_form(x, tight)}
            names = list(LEGS)
            vec0 = ctx.get_stat("bgr_yuv420_vec")
            for name in names:                                   # the legs agree before anything is timed
                legs[name](sets[0])
            torch.cuda.synchronize()
            assert ctx.get_stat("bgr_yuv420_vec") == vec0 + 3, "a leg of the new form left the 16 x 2 groups"
            assert torch.equal(i420_a, i420_b), ("(a) and (b) differ", w, h, op)
            pc = pitched[0].view(n, fstride)
            assert torch.equal(pc[:, : yp * h].view(n, h, yp)[:, :, :w].reshape(n, ysz), i420_a[:, :ysz]), ("Y of (c)", w, h, op)
            for off, lo in ((u_off, ysz), (v_off, ysz + q)):
                got = pc[:, off: off + cp * (h // 2)].view(n, h // 2, cp)[:, :, : w // 2].reshape(n, q)
                assert torch.equal(got, i420_a[:, lo: lo + q]), ("chroma of (c)", w, h, op)
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
            res = {"width": w, "height": h, "frames_per_call": n, "op": op, "order": "BGR", "uv_mode": "COPY", "calls": args.calls,
                   "pitches": {"y": yp, "c": cp, "frame_stride": fstride}}
            for name, ev in times.items():
                ms = [a.elapsed_time(b) for a, b in ev]
                res[name] = {"median_us": pct(ms, 0.5) * 1e3, "p10_us": pct(ms, 0.1) * 1e3, "p90_us": pct(ms, 0.9) * 1e3,
                             "frames_per_s": n / (pct(ms, 0.5) * 1e-3)}
            med = {k: res[k]["median_us"] for k in names}
            res["spread"] = abs(med["a_tight"] / med["a2_tight_again"] - 1.0)
            res["a_rate_over_b_rate"] = med["b_two_calls"] / med["a_tight"]
            res["c_rate_over_d_rate"] = med["d_via_nv12"] / med["c_pitched"]
            res["a_rate_over_e_rate"] = med["e_nv12_out"] / med["a_tight"]
            res["a_bytes_per_s"] = BYTES_PER_PX[op] * w * h * n / (med["a_tight"] * 1e-6)
            ctx.set_profiling(1)
            kern = {}
            for tag in ("a_tight", "c_pitched", "e_nv12_out"):
                ctx.profile_read(reset=True)
                for it in range(30):
                    legs[tag](sets[it & 1])
                torch.cuda.synchronize()
                kern[tag + "_color_kernel_p50_us"] = ctx.profile_read(reset=True)["color_kernel"]["p50_ms"] * 1e3
            ctx.set_profiling(0)
            kern["planar_store_over_interleaved_store"] = kern["a_tight_color_kernel_p50_us"] / kern["e_nv12_out_color_kernel_p50_us"]
            res["kernels"] = kern
            rows.append(res)
            print(json.dumps(res), flush=True)
        del sets, i420_a, i420_b, nv12_e, scratch, pitched
        torch.cuda.empty_cache()
    meta = {"device": torch.cuda.get_device_name(0), "library": mi_lumaeq.version(), "clahe": {"clip": CLAHE[0], "tiles": list(CLAHE[1:])},
            "order": "BGR", "uv_mode": "COPY", "warmup": args.warmup, "bar": None}
    ctx.close()
    outdir = Path(args.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "r23_bgr_to_yuv420_ab.json").write_text(json.dumps({"meta": meta, "rows": rows}, indent=1) + "\n")
    md = ["# BGR in, equalized planar 4:2:0 out: the one-call form against what it replaces", "",
          f"{meta['device']}, {meta['library']}; {args.warmup} warm-up and {args.calls} timed calls per leg, legs interleaved in one process, "
          "medians of per-call HIP event times; CLAHE 8x8 clip 2.0; MI_ORDER_BGR, MI_UV_COPY.  Rates are frames per second.  (a): "
          "mi_*_bgr_to_yuv420_batch_dev on tight I420.  (b): mi_cvt_color_420_u8_batch_dev(BGR2YUV_I420) + mi_*_u8_batch_dev in place.  "
          "(c): the new form on planes at pitches align(row, 256).  (d): mi_*_bgr_to_nv12_batch_dev into scratch + "
          "mi_*_yuv420_batch_dev(NV12 -> I420) into those planes.  (e): mi_*_bgr_to_nv12_batch_dev, tight.  Spread: the two (a) legs of "
          "the same rotation against each other.  Kernel: p50 of the conversion kernel (MI_K_COLOR) of (a) over that of (e).", "",
          "| frames | op | (a) tight | (b) two calls | (c) pitched | (d) via NV12 | (e) NV12 out | a / b | c / d | a / e | spread | kernel a / e |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['frames_per_call']} x {r['width']}x{r['height']} | {r['op']} | " +
                  " | ".join(f"{r[k]['frames_per_s']:.0f} ({r[k]['median_us']:.0f} us)" for k in LEGS[:5]) +
                  f" | {r['a_rate_over_b_rate']:.3f} | {r['c_rate_over_d_rate']:.3f} | {r['a_rate_over_e_rate']:.3f} | {r['spread']:.3f} "
                  f"| {r['kernels']['planar_store_over_interleaved_store']:.3f} |")
    slow = [(r["width"], r["op"], k, round(r[k], 3)) for r in rows for k in ("a_rate_over_b_rate", "c_rate_over_d_rate")
            if r[k] < 1.0 - r["spread"]]
    md += ["", "Rows in which the one-call form is slower than what it replaces by more than the spread: " + (str(slow) if slow else "none") + "."]
    (outdir / "r23_bgr_to_yuv420_ab.md").write_text("\n".join(md) + "\n")
    if slow:
        print("FINDING: the one-call form is slower than what it replaces in", slow)


if __name__ == "__main__":
    main()
