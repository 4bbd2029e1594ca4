"""A/B of a fused-kernel option in one process (interleaved rounds).

    python tools/fused_ab.py <option> [modes e.g. 0,1]            wall time per call, option values alternating
    python tools/fused_ab.py --policy-matrix [--out FILE.json] [--sweep-top N]
        every cache policy of equalize_fused_kernel<20, POL> (option fused_cache_policy = 100 + POL) on four shapes, then the
        best few against the plain policy over frame counts (where does the streaming policy start to pay?).  Needs the
        library with the whole matrix: `make -C opencv-opencl_amd/csrc ab`, MI_LUMAEQ_LIB=opencv-opencl_amd/lib/libmi_lumaeq_ab.so.
        ONE context (a second fused context on the device would shrink the co-residency allowance), the policies alternating
        in rounds of 20 launches, 10 rounds = 200 launches per leg; kernel time from the events around each dispatch
        (set_profiling(2)); the figure of a leg is the median of its rounds' medians.
"""
import json, sys, time, torch
sys.path.insert(0, "opencv-opencl_amd/python"); sys.path.insert(0, ".")
import mi_lumaeq
from mi_lumaeq import synth

SEL = ("plain", "nt", "sc1")


def pol_code(y_ld, y_st, uv_st, uv_ld):
    return y_ld | (y_st << 1) | (uv_st << 3) | (uv_ld << 5)


def pol_name(p):
    return f"Yld={SEL[p & 1]} Yst={SEL[(p >> 1) & 3]} UVst={SEL[(p >> 3) & 3]} UVld={SEL[(p >> 5) & 1]}"


def time_policies(ctx, w, h, B, uv, pols, rounds=10, per_round=20):
    """{pol: median over rounds of the fused kernel's p50 (us)}; pols are POL codes, run as option value 100 + POL."""
    d_in = synth.nv12_batch_torch(w, h, B, "D2", "cuda", seed=1)
    d_out = torch.empty_like(d_in)
    res = {p: [] for p in pols}
    fused = True
    for p in pols:                                   # warm-up: scratch sized, every code object loaded
        ctx.set_option("fused_cache_policy", 100 + p)
        for _ in range(2): ctx.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, B, uv)
    ctx.synchronize()
    ctx.set_profiling(2)
    ctx.profile_read(True)
    for rnd in range(rounds):
        order = pols if rnd % 2 == 0 else pols[::-1]
        for p in order:
            ctx.set_option("fused_cache_policy", 100 + p)
            for _ in range(per_round): ctx.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, B, uv)
            ctx.synchronize()
            k = ctx.profile_read(True)["equalize_fused_kernel"]
            if k["launches"] != per_round: fused = False
            else: res[p].append(k["p50_ms"] * 1e3)
    ctx.set_profiling(0)
    del d_in, d_out
    if not fused: return None
    return {p: sorted(v)[len(v) // 2] for p, v in res.items()}


def policy_matrix(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    top_n = int(argv[argv.index("--sweep-top") + 1]) if "--sweep-top" in argv else 3
    ctx = mi_lumaeq.Context(0)
    record = {"matrix": [], "sweep": []}
    # UV loads exist for the copy only: the fill shapes walk 18 policies, the copy shape all 36
    fill_pols = [pol_code(a, b, c, 0) for a in range(2) for b in range(3) for c in range(3)]
    copy_pols = [pol_code(a, b, c, d) for a in range(2) for b in range(3) for c in range(3) for d in range(2)]
    shapes = (("64x4K fill", 3840, 2160, 64, 0, fill_pols), ("64x4K copy", 3840, 2160, 64, 1, copy_pols),
              ("256x1080p fill", 1920, 1080, 256, 0, fill_pols), ("16x4K fill", 3840, 2160, 16, 0, fill_pols))
    best = None
    for name, w, h, B, uv, pols in shapes:
        r = time_policies(ctx, w, h, B, uv, pols)
        print(f"== {name}: fused kernel us (median of 10 round medians, 20 launches a round), ratio to plain", flush=True)
        for p in sorted(pols, key=lambda p: r[p]):
            print(f"  POL {p:2d}  {pol_name(p):44s} {r[p]:8.2f}  {r[p] / r[0]:6.4f}")
        record["matrix"].append({"shape": name, "us": {str(p): r[p] for p in pols}})
        if best is None:
            best = sorted(pols, key=lambda p: r[p])[:top_n]
    # the sweep: plain against the best of the headline shape (and their UV-load-nt twins for nothing: fill only)
    cand = [0] + [p for p in best if p != 0]
    for w, h, counts in ((3840, 2160, (8, 12, 16, 24, 32, 64)), (1920, 1080, (32, 64, 128, 256))):
        for B in counts:
            r = time_policies(ctx, w, h, B, 0, cand)
            mb = B * w * h * 2.5 / 2**20
            if r is None:
                print(f"sweep {w}x{h} B={B:3d} ({mb:7.1f} MiB touched): not on the fused path", flush=True)
                record["sweep"].append({"w": w, "h": h, "B": B, "MiB": mb, "us": None})
                continue
            print(f"sweep {w}x{h} B={B:3d} ({mb:7.1f} MiB touched): " + "  ".join(f"POL {p}: {r[p]:7.2f} ({r[p] / r[0]:.4f})" for p in cand), flush=True)
            record["sweep"].append({"w": w, "h": h, "B": B, "MiB": mb, "us": {str(p): r[p] for p in cand}})
    if out_path:
        with open(out_path, "w") as f: json.dump(record, f, indent=1)


def option_ab(argv):
    opt = argv[1] if len(argv) > 1 else "fused_acquire"
    MODES = [int(x) for x in argv[2].split(",")] if len(argv) > 2 else [0, 1]
    a = mi_lumaeq.Context(0)
    for (w, h, B, uv) in ((3840, 2160, 64, 0), (3840, 2160, 64, 1), (3840, 2160, 8, 0), (1920, 1080, 256, 0), (3840, 2160, 1, 0)):
        d_in = synth.nv12_batch_torch(w, h, B, "D2", "cuda", seed=1)
        d_out = torch.empty_like(d_in)
        res = {m: [] for m in MODES}
        for rnd in range(9):
            for mode in MODES:
                a.set_option(opt, mode)
                for _ in range(2): a.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, B, uv)
                a.synchronize()
                t0 = time.perf_counter()
                for _ in range(20): a.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, B, uv)
                a.synchronize()
                res[mode].append((time.perf_counter() - t0) / 20 * 1e6)
        for mode in MODES:
            r = sorted(res[mode]); print(f"{w}x{h} B={B} uv={uv} {opt}={mode}: median {r[len(r)//2]:7.1f} us  min {r[0]:7.1f}  -> {B/(r[len(r)//2]*1e-6):9.0f} frames/s")


if __name__ == "__main__":
    if "--policy-matrix" in sys.argv: policy_matrix(sys.argv)
    else: option_ab(sys.argv)
