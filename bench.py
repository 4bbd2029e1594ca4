#!/usr/bin/env python3
"""bench.py -- frames/s of the NV12 luma equalizeHist hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
        N = 1: runs in this process.  N > 1 with WORLD_SIZE unset: this process starts N fresh children -- one per GPU, with
        RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set -- BEFORE it makes any GPU call itself, relays
        rank 0's JSON line and exits with the worst child's code (it never re-executes a process that has touched the GPU).
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
        the same ranks started by torchrun (WORLD_SIZE set: no self-launch).

One "step" = one pass of the hot path (mi_equalize_hist_nv12_batch_dev: histogram -> CDF/LUT ->
LUT apply + UV fill) over one batch of `--batch` synthetic 3840x2160 NV12 frames that are already
resident in HBM (BASELINE.json configs[1], batched so the working set exceeds the 256 MiB
Infinity Cache).  Every GPU processes its own replica batch (frame k -> GPU k mod N), no data-path
collective (weak scaling); value = frames all ranks processed / max-over-ranks time.  Each rank first
binds itself to the CPUs of its GPU's NUMA node (mi_thread_bind_near_device; --no-numa-bind to skip).

A plain run sets up, warms up, times the K steps and prints the JSON line; beside the headline it carries
  roofline     -- the dominant kernel's algorithmic bytes per launch (for the fused single-read kernel: the whole
                  path's 3.5 W H per frame) / its average launch duration (HIP events stamped by the dispatches
                  themselves on the launch stream inside the timed region; for N > 1 averaged over the ranks,
                  with the slowest and fastest rank beside it) against the 8 TB/s HBM peak.
--full adds everything else, after the timed region:
  parity_spot_check -- first, middle and last frame of the last step against the CPU oracle;
  nv12_1080p   -- the same protocol on 1920x1080 frames;
  stream_4k60_512_all_gpus (N > 1 or --force-dist), opencv_cross_check (where cv2 exists), extras (N = 1) -- secondary figures;
  cpu_baseline -- the CPU oracle (a port of OpenCV 4.4's arithmetic, see oracle/) timed on this
                  host's cores on a bounded sample of the same workload (rank 0, after the other ranks have left).
The oracle is used here only for that leg and for the parity spot check.
--dump-outputs DIR writes what the last timed step computed (rank 0's batch) as .npy files: see dump_outputs().
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "opencv-opencl_amd" / "python"))
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_MEASURED_COPY_GBS = 6290.0  # same guide: float4 copy ceiling
DEADLINE_DEFAULT_S = 480.0      # launcher deadline; a torchrun rank's own watchdog fires RANK_WATCHDOG_SLACK_S later: 510 s < the driver's 600 s
RANK_WATCHDOG_SLACK_S = 30.0
DUMP_SAMPLE = 1 << 23           # output bytes --dump-outputs writes as float32: 32 MiB of the 64 MB a dump may take
DUMP_SEED = 0x5EED0D


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the parity spot check, the 1920x1080 leg, the stream / OpenCV / extras "
                         "figures and the CPU baseline (a plain run does only the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float, at most 64 MB; see dump_outputs)")
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--dist", default="D2", help="Y distribution D1..D5 (mi_lumaeq.synth)")
    ap.add_argument("--uv", default="fill128", choices=["fill128", "copy"])
    ap.add_argument("--op", default="equalize", choices=["equalize", "clahe"])
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the cpu_baseline leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true")
    ap.add_argument("--no-second-resolution", action="store_true", help="skip the 1920x1080 leg that follows the 4K timed region")
    ap.add_argument("--graph-extras", action="store_true", help="also time single-frame launches replayed from a captured HIP graph")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (=RCCL) for real multi-GPU runs; gloo only to rehearse the N>1 path on a 1-GPU box")
    ap.add_argument("--all-ranks-on-device", type=int, default=None,
                    help="rehearsal only: every rank uses this GPU index instead of LOCAL_RANK")
    ap.add_argument("--no-numa-bind", action="store_true", help="do not bind each rank to the CPUs of its GPU's NUMA node")
    ap.add_argument("--force-dist", action="store_true",
                    help="bring the process group up even with ONE rank (RANK=0, WORLD_SIZE=1 on 127.0.0.1 when the environment sets "
                         "none): init_process_group on the chosen backend, every all_reduce / barrier of the N>1 path on that backend's "
                         "tensors, the all-ranks stream leg, destroy_process_group -- the statements an N-GPU run executes, on one GPU")
    ap.add_argument("--deadline-s", type=float, default=DEADLINE_DEFAULT_S,
                    help="whole-job deadline: the launcher ends its children by PID, says which phase each rank was in and exits 124; "
                         "a rank started by torchrun ends itself 30 s later (0 = none).  The default keeps both inside the 600 s the "
                         "driver gives a bench run, so a stuck job names its ranks' phases before it is killed from outside")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


# ---- heartbeats ------------------------------------------------------------------------------------------------------
# Every rank says on stderr which phase it is entering; the launcher keeps each rank's last phase, so a job that stops making
# progress is reported as "rank r was in phase p" instead of ending in silence (round 3's four-rank rehearsal left an empty record).
_T0 = time.monotonic()
_PHASE = {"name": "start", "rank": int(os.environ.get("RANK", "0"))}
HB_TAG = "[bench hb]"


def hb(phase):
    _PHASE["name"] = phase
    print(f"{HB_TAG} rank={_PHASE['rank']} phase={phase} t=+{time.monotonic() - _T0:.1f}s", file=sys.stderr, flush=True)


def arm_rank_watchdog(deadline_s):
    """A rank that outlives the deadline (+30 s, so that a launcher acts first and can report every rank) says where it was and
    leaves with 124.  os._exit: the main thread may sit in a collective or in a HIP call that never returns."""
    if not deadline_s or deadline_s <= 0:
        return None
    import threading

    def fire():
        print(f"{HB_TAG} rank={_PHASE['rank']} DEADLINE of {deadline_s:.0f} s passed in phase={_PHASE['name']}: leaving with 124",
              file=sys.stderr, flush=True)
        os._exit(124)
    t = threading.Timer(deadline_s + RANK_WATCHDOG_SLACK_S, fire)
    t.daemon = True
    t.start()
    return t


# ---- self-launch for N > 1 -----------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_children(n, argv, child_cmd=None, grace_s=30.0, env_extra=None, deadline_s=DEADLINE_DEFAULT_S):
    """Start n fresh processes of this script, one per GPU (RANK / LOCAL_RANK = 0..n-1, WORLD_SIZE = n, rendezvous on 127.0.0.1),
    relay rank 0's JSON line(s) to stdout and everything else to stderr, return the worst exit code.  The calling process must
    not have touched the GPU: nothing here does, and nothing is exec'd in place -- the children are ordinary child processes.
    When a rank dies, the others get `grace_s` seconds to notice (they may sit in a collective with it) and are then ended, by
    their own PIDs.  When the job as a whole outlives `deadline_s`, every child still running is ended the same way, the phase
    each rank last announced (hb()) is printed and 124 is returned.  `child_cmd` replaces `python bench.py` (the CPU tests pass stubs)."""
    import subprocess
    import threading
    port = _free_port()
    cmd = list(child_cmd) if child_cmd else [sys.executable, str(Path(__file__).resolve())]
    procs, pumps, rank0_lines = [], [], []
    phase = {r: "not started" for r in range(n)}

    def pump_out(rank, stream):
        for line in stream:
            if rank == 0 and line.lstrip().startswith("{"):
                rank0_lines.append(line)
                sys.stdout.write(line)
                sys.stdout.flush()
            else:
                sys.stderr.write(f"[rank {rank}] {line}")
                sys.stderr.flush()

    def pump_err(rank, stream):
        for line in stream:
            if line.startswith(HB_TAG):
                bits = dict(kv.split("=", 1) for kv in line[len(HB_TAG):].split() if "=" in kv)
                if "phase" in bits:
                    phase[rank] = f"{bits['phase']} (since {bits.get('t', '?')})"
            sys.stderr.write(line if line.startswith(HB_TAG) else f"[rank {rank}] {line}")
            sys.stderr.flush()

    t_start = time.monotonic()
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # RCCL on this pool: dmabuf IPC only
        if env_extra:
            env.update(env_extra)
        p = subprocess.Popen(cmd + list(argv), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)
        phase[r] = "started"
        for fn, stream in ((pump_out, p.stdout), (pump_err, p.stderr)):
            t = threading.Thread(target=fn, args=(r, stream), daemon=True)
            t.start()
            pumps.append(t)
        procs.append(p)

    def end_children():
        for p in procs:
            if p.poll() is None:
                p.terminate()                                      # by PID: never by pattern
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()

    deadline, own_failure, timed_out = None, 0, False
    while any(p.poll() is None for p in procs):
        if deadline is None and any(p.poll() not in (None, 0) for p in procs):
            deadline = time.monotonic() + grace_s                 # a rank failed: the rest may be waiting for it forever
            own_failure = next(p.poll() for p in procs if p.poll() not in (None, 0))     # ... and ITS code is the job's, not the
                                                                  # SIGTERM the launcher hands the others afterwards
        if deadline is not None and time.monotonic() > deadline:
            end_children()
            break
        if deadline_s and deadline_s > 0 and time.monotonic() - t_start > deadline_s:
            timed_out = True
            running = [r for r, p in enumerate(procs) if p.poll() is None]
            print(f"bench.py launcher: DEADLINE of {deadline_s:.0f} s passed; ranks still running: {running}", file=sys.stderr)
            for r in range(n):
                print(f"bench.py launcher:   rank {r}: {'running' if r in running else f'exited {procs[r].poll()}'}, last phase: {phase[r]}",
                      file=sys.stderr)
            sys.stderr.flush()
            end_children()
            break
        time.sleep(0.05)
    for t in pumps:
        t.join(timeout=10)
    codes = [p.wait() for p in procs]
    if timed_out:
        return 124
    worst = own_failure
    for c in codes:
        if c != 0 and worst == 0:
            worst = c
    if worst != 0:
        for r in range(n):
            print(f"bench.py launcher:   rank {r}: exit code {codes[r]}, last phase: {phase[r]}", file=sys.stderr)
    if worst == 0 and not rank0_lines:
        print("bench.py launcher: rank 0 printed no JSON line", file=sys.stderr)
        worst = 1
    if worst < 0:
        worst = 128 - worst                                        # killed by a signal: shell convention
    return worst


def cpu_baseline(args, w, h):
    """CPU oracle (kind 'port') on a bounded sample: whole NV12 frames, same op, all host threads."""
    import numpy as np
    import oracle
    from mi_lumaeq import synth
    nfr = 6
    frames = [synth.nv12_frame(w, h, args.dist, 1000 + k) for k in range(nfr)]
    uv_mode = 1 if args.uv == "copy" else 0
    op = 1 if args.op == "clahe" else 0
    # thread count: the GPU box shows 256 logical CPUs but grants a ~16-core share; oversubscribing
    # OpenMP is slower than 1 thread, so take the best of a short sweep (each ~0.5 s)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    best_t, best_rate = 1, 0.0
    swept = sorted({c for c in (1, 4, 8, 16, 32, 64) if c <= avail})
    for cand in swept:
        oracle.set_threads(cand)
        oracle.nv12_frame(frames[0], w, h, uv_mode=uv_mode, op=op)
        n0, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 0.5:
            oracle.nv12_frame(frames[n0 % nfr], w, h, uv_mode=uv_mode, op=op)
            n0 += 1
        rate = n0 / (time.perf_counter() - t0)
        if rate > best_rate:
            best_t, best_rate = cand, rate
    threads = oracle.set_threads(best_t)
    done, t0 = 0, time.perf_counter()
    while True:
        oracle.nv12_frame(frames[done % nfr], w, h, uv_mode=uv_mode, op=op)
        done += 1
        el = time.perf_counter() - t0
        if el >= args.cpu_seconds or done >= 100000:
            break
    multi = done / el
    # single-thread figure on a shorter sample
    oracle.set_threads(1)
    oracle.nv12_frame(frames[0], w, h, uv_mode=uv_mode, op=op)
    d1, t1 = 0, time.perf_counter()
    while time.perf_counter() - t1 < min(4.0, args.cpu_seconds / 3) and d1 < 500:
        oracle.nv12_frame(frames[d1 % nfr], w, h, uv_mode=uv_mode, op=op)
        d1 += 1
    single = d1 / (time.perf_counter() - t1)
    oracle.set_threads(threads)
    # BASELINE.json configs[0]: one 1920x1080 frame, CPU reference path (OpenCVequalHist.cpp) -- same oracle, same threads
    f1080 = [synth.nv12_frame(1920, 1080, args.dist, 2000 + k) for k in range(4)]
    oracle.nv12_frame(f1080[0], 1920, 1080, uv_mode=uv_mode, op=op)
    d2, t2 = 0, time.perf_counter()
    while time.perf_counter() - t2 < 1.5:
        oracle.nv12_frame(f1080[d2 % 4], 1920, 1080, uv_mode=uv_mode, op=op)
        d2 += 1
    fps1080 = d2 / (time.perf_counter() - t2)
    cpu_model = "unknown CPU"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    # `cores` is the number of OpenMP THREADS the figure was measured with -- the best of the sweep above -- not a count of physical
    # cores: the box's affinity mask is far wider than the CPU share it grants, and the sample string says all three numbers
    port = {"value": round(multi, 2), "unit": "frames/s", "cores": threads, "kind": "port", "cpu": cpu_model,
            "sample": f"{done} x {w}x{h} NV12 frames ({args.dist}, {args.op}, uv={args.uv}) in {el:.1f} s, "
                      f"OpenMP row/tile-striped CPU restatement of OpenCV 4.4 (oracle/lumaeq_oracle.c); "
                      f"{threads} OpenMP threads = best of a sweep over {swept} threads, affinity mask {avail} CPUs, "
                      f"host has {os.cpu_count()} logical CPUs",
            "threads_swept": swept, "affinity_cpus": avail,
            "value_1thread": round(single, 2), "value_1080p": round(fps1080, 2)}
    # Where a real OpenCV is importable the baseline is the REFERENCE itself -- cv::equalizeHist / CLAHE::apply on the Y plane and the
    # NV12 rebuild around it, as OpenCVequalHist.cpp:140-162 / clahevideo.cpp:178-201 do it (1frameMeasure.cpp:43-47 times the same
    # call) -- kind "reference"; the port's figures stay beside it.  Never on this pool (no cv2): kind "port".
    ref = reference_cpu_baseline(frames, f1080, w, h, uv_mode, op, min(6.0, max(1.0, args.cpu_seconds / 2)))
    if ref is None:
        return port
    ref.update({"cpu": cpu_model, "port": {k: port[k] for k in ("value", "cores", "value_1thread", "value_1080p", "sample")}})
    return ref


def reference_cpu_baseline(frames, f1080, w, h, uv_mode, op, seconds):
    """cv2 (the real OpenCV) on the same NV12 frames: frames/s with OpenCV's own thread count and with one thread; None without cv2."""
    try:
        import cv2
    except Exception:
        return None
    import numpy as np
    clahe = cv2.createCLAHE(2.0, (8, 8)) if op else None

    def one(frame, cw, ch, out):
        y = frame[: cw * ch].reshape(ch, cw)
        out[: cw * ch] = (clahe.apply(y) if op else cv2.equalizeHist(y)).reshape(-1)
        if uv_mode:
            out[cw * ch:] = frame[cw * ch:]
        else:
            out[cw * ch:] = 128

    def rate(fs, cw, ch, secs):
        out = np.empty_like(fs[0])
        one(fs[0], cw, ch, out)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < secs:
            one(fs[n % len(fs)], cw, ch, out)
            n += 1
        return n / (time.perf_counter() - t0), n
    try:
        default_threads = cv2.getNumThreads()
        multi, n = rate(frames, w, h, seconds)
        fps1080, _ = rate(f1080, 1920, 1080, 1.0)
        cv2.setNumThreads(1)
        single, _ = rate(frames, w, h, min(3.0, seconds / 2))
        cv2.setNumThreads(default_threads)
    except Exception as e:               # a broken cv2 build must not take the bench line down: the port stands
        print(f"[bench] reference_cpu_baseline failed: {e!r}", file=sys.stderr, flush=True)
        return None
    return {"value": round(multi, 2), "unit": "frames/s", "cores": int(default_threads), "kind": "reference",
            "sample": f"{n} x {w}x{h} NV12 frames in {seconds:.1f} s through cv2 {cv2.__version__} "
                      f"({'createCLAHE(2.0, (8, 8)).apply' if op else 'equalizeHist'} on the Y plane + UV {'copy' if uv_mode else '= 128'}), "
                      f"OpenCV's own thread count ({default_threads})",
            "value_1thread": round(single, 2), "value_1080p": round(fps1080, 2)}


def device_for_collectives(torch, backend, local_rank):
    return torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")


def dump_outputs(d_out, out_dir):
    """What a caller of the timed path receives -- the output batch of the last step, n_frames x NV12 frame bytes -- written to
    `out_dir` so that two builds can be compared output for output (the bench's inputs are seeded: the same arguments give the same
    frames).  The batch is larger than a dump may be (64 x 4K frames = 796 MB), so:
      frames_out_sample.npy  float32 [min(DUMP_SAMPLE, bytes)]  the output bytes at fixed positions, one in each of DUMP_SAMPLE equal
                             strata of the flattened batch, drawn by a generator seeded with DUMP_SEED (the whole batch when smaller);
      frames_out_hist.npy    float64 [n_frames, 256]            every output frame's byte histogram, so that every pixel is counted.
    Returns the paths written."""
    import numpy as np
    import torch
    from mi_lumaeq import xfer
    flat = d_out.reshape(-1)
    n = flat.numel()
    if n <= DUMP_SAMPLE:
        idx = torch.arange(n, device=flat.device)
    else:
        stride = n // DUMP_SAMPLE
        g = torch.Generator(device=flat.device)
        g.manual_seed(DUMP_SEED)
        idx = (torch.arange(DUMP_SAMPLE, device=flat.device) * stride +
               torch.randint(0, stride, (DUMP_SAMPLE,), device=flat.device, generator=g))
    sample = xfer.to_host(flat[idx]).astype(np.float32)
    hist = torch.stack([torch.bincount(d_out[k].reshape(-1).to(torch.int32), minlength=256) for k in range(d_out.shape[0])])
    hist = xfer.to_host(hist).astype(np.float64)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = [out_dir / "frames_out_sample.npy", out_dir / "frames_out_hist.npy"]
    np.save(paths[0], sample)
    np.save(paths[1], hist)
    return paths


def opencv_cross_check(ctx, w, h, dist_name):
    """the oracle is a restatement (parity unpinned).  Wherever a real OpenCV is importable, compare the GPU path with cv2
    itself and say so in the JSON line; None when there is no cv2 (this image has none).  The bench's own resolution AND 1920x1080
    (BASELINE config 1), equalizeHist and CLAHE 8x8 clip 2.0 in whichever of the two arithmetic modes this cv2 build computes, and
    config 5 in both readings: Y equalize + UV passthrough (what ColoropenCVCwqualHist.cpp does) and, literally,
    NV12 -> BGR -> equalizeHist on B, G, R -> NV12.  The C++ front end's own pin is tests/test_opencv_pin.py."""
    try:
        import cv2
    except Exception:
        return None
    import numpy as np
    import mi_lumaeq
    from mi_lumaeq import synth
    res = {"version": cv2.__version__, "shapes": {}}
    try:
        for (cw, ch) in sorted({(w, h), (1920, 1080)}):
            frame = synth.nv12_frame(cw, ch, dist_name, 4242)
            y = frame[: cw * ch].reshape(ch, cw)
            r = {"equalizeHist_bit_exact": bool(np.array_equal(ctx.equalize_hist(y), cv2.equalizeHist(y)))}
            want = cv2.createCLAHE(2.0, (8, 8)).apply(y)
            r["clahe_2.0_8x8_bit_exact"] = bool(np.array_equal(ctx.clahe(y, 2.0, 8, 8), want))          # x86-64 baseline arithmetic
            ctx.set_option("clahe_fp_contract", 1)                                                      # GCC FMA contraction (aarch64 builds)
            r["clahe_2.0_8x8_bit_exact_fp_contract"] = bool(np.array_equal(ctx.clahe(y, 2.0, 8, 8), want))
            ctx.set_option("clahe_fp_contract", 0)
            # config 5 as the named file does it: Y equalized, UV passed through
            out = ctx.equalize_hist_nv12(frame, cw, ch, mi_lumaeq.UV_COPY)
            want5 = frame.copy()
            want5[: cw * ch] = cv2.equalizeHist(y).reshape(-1)
            r["config5_y_equalize_uv_passthrough_bit_exact"] = bool(np.array_equal(out, want5))
            # config 5 read literally: cvtColor(YUV2BGR_NV12) -> split -> equalizeHist x 3 -> merge -> cvtColor(BGR2YUV_I420) -> interleave U, V
            bgr = cv2.cvtColor(frame.reshape(ch * 3 // 2, cw), cv2.COLOR_YUV2BGR_NV12)
            bgr = cv2.merge([cv2.equalizeHist(p) for p in cv2.split(bgr)])
            i420 = cv2.cvtColor(bgr, cv2.COLOR_BGR2YUV_I420).reshape(-1)
            lit = np.empty_like(frame)
            lit[: cw * ch] = i420[: cw * ch]
            lit[cw * ch:: 2] = i420[cw * ch: cw * ch * 5 // 4]
            lit[cw * ch + 1:: 2] = i420[cw * ch * 5 // 4:]
            r["config5_literal_bgr_channels_bit_exact"] = bool(np.array_equal(ctx.nv12_bgr_equalize(frame, cw, ch), lit))
            res["shapes"][f"{cw}x{ch}"] = r
        first = res["shapes"][f"{w}x{h}"]                            # (the round-2 keys, for whoever reads them)
        res.update({k: first[k] for k in ("equalizeHist_bit_exact", "clahe_2.0_8x8_bit_exact", "clahe_2.0_8x8_bit_exact_fp_contract")})
    except Exception as e:                 # a broken cv2 build must not take the bench line down
        res["error"] = repr(e)
    return res


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher.  Nothing above has touched the GPU (no torch import yet).
        sys.exit(launch_children(args.gpus, sys.argv[1:], deadline_s=args.deadline_s))
    arm_rank_watchdog(args.deadline_s)
    # stdout carries ONE JSON line and nothing else.  Native libraries write to file descriptor 1 behind Python's back (RCCL prints a
    # five-line version banner there when the first communicator comes up -- seen in round 5's first one-rank RCCL run), so from here on
    # fd 1 IS stderr, and the line goes out through a private duplicate of the real stdout.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    hb("import")
    import torch
    import torch.distributed as dist
    import mi_lumaeq
    from mi_lumaeq import synth, shard, xfer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.all_ranks_on_device is not None:
        local_rank = args.all_ranks_on_device
    _PHASE["rank"] = rank
    # --force-dist: a one-rank world on the real backend.  Decided here, before the first GPU call; the rendezvous is given to
    # torch.distributed through the environment of THIS process (nothing is re-executed).
    use_dist = world > 1 or args.force_dist
    if args.force_dist and "MASTER_PORT" not in os.environ:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local_rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # what launch_children gives its ranks
    if use_dist:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs HIP devices (no CPU fallback)")
        hb(f"dist_init({args.dist_backend})")
        torch.cuda.set_device(local_rank)
        # No silent substitution: if RCCL was asked for and does not come up with every rank, the run fails.  (gloo is only
        # ever used when asked for by name, to rehearse the N>1 path on a one-GPU box.)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
        backend_used = dist.get_backend()
        # every rank contributes 1 through the backend itself: the sum is the number of ranks the backend really connects
        one = torch.ones(1, device=device_for_collectives(torch, backend_used, local_rank))
        dist.all_reduce(one)
        world_seen = int(one.item())
        if backend_used != args.dist_backend or world_seen != world:
            raise SystemExit(f"dist backend check failed: asked {args.dist_backend} x {world}, got {backend_used} x {world_seen}")
    else:
        backend_used, world_seen = None, 1
    dgroup = dist if use_dist else None                              # what the reductions below go through
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    w, h, B = args.width, args.height, args.batch
    ysz = w * h
    fbytes = ysz + ysz // 2
    uv_mode = mi_lumaeq.UV_COPY if args.uv == "copy" else mi_lumaeq.UV_FILL128
    # placement before the context exists: its pinned buffers and helper thread then live next to this rank's GPU
    placement = {"node": None, "cpus": 0, "why": "NUMA binding off (--no-numa-bind)"}
    if not args.no_numa_bind:
        try:
            placement = mi_lumaeq.bind_thread_near_device(local_rank)
        except mi_lumaeq.MiError as e:
            placement = {"node": None, "cpus": 0, "why": f"not bound: {e}"}
    hb("context")
    ctx = mi_lumaeq.Context(local_rank)

    # this rank's shard: global frame indices k with k mod world == rank (no collective on the data path); the synthetic batch is
    # seeded by the first of them, so every rank works on different frames of the same distribution
    my_frames = shard.frames_for_rank(B * world, rank, world)
    if len(my_frames) != B:
        raise SystemExit(f"sharding error: rank {rank} got {len(my_frames)} frames for a batch of {B}")
    d_in = synth.nv12_batch_torch(w, h, B, args.dist, device, seed=0x5EED0000 + my_frames[0])
    d_out = torch.empty_like(d_in)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        if args.op == "equalize":
            ctx.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, B, uv_mode, stream=stream)
        else:
            ctx.clahe_nv12_batch_dev(d_in, d_out, w, h, B, uv_mode, 2.0, 8, 8, stream=stream)

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    hb("warmup")
    for _ in range(args.warmup):
        step()
    barrier()
    hb("timed")
    ctx.profile_read(reset=True)
    # HIP events stamped by the kernel dispatches themselves (hipExtLaunchKernelGGL start / stop events), on the launch stream
    ctx.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    ctx.set_profiling(False)
    hb("verdict")
    # The library's own verdict on the timed launches, on EVERY rank: synchronize() raises if the fused path met a frame it
    # could not repair, and a launch that had to be repaired on the device (correct output, but slower) is disclosed.
    run_ok, run_err = True, ""
    try:
        ctx.synchronize(stream)
        fused_fallbacks = ctx.get_stat("fused_fallbacks")
    except mi_lumaeq.MiError as e:
        run_ok, run_err, fused_fallbacks = False, str(e), -1
    prof = ctx.profile_read(reset=True)
    elapsed = shard.max_over_ranks(elapsed, dgroup)

    # parity spot check of the measured configuration (rank 0; first, middle and last frame of the last step) -- checker only
    parity = None
    if rank == 0 and run_ok and args.full:
        import numpy as np
        import oracle
        parity = True
        for k in sorted({0, B // 2, B - 1}):
            got = xfer.to_host(d_out[k])
            want = oracle.nv12_frame(xfer.to_host(d_in[k]), w, h, uv_mode=uv_mode, op=1 if args.op == "clahe" else 0,
                                     clip_limit=2.0, tiles_x=8, tiles_y=8)
            parity = parity and bool(np.array_equal(got, want))
    # one verdict for the whole job, shared BEFORE anybody exits, so no rank is left blocked in a barrier
    ok_local = 1.0 if (run_ok and parity is not False) else 0.0
    ok_all = -shard.max_over_ranks(-ok_local, dgroup)
    if ok_all < 1.0:
        if use_dist:
            dist.destroy_process_group()
        raise SystemExit("REFUSING TO REPORT: " + (run_err or ("PARITY FAILURE: GPU output differs from the oracle" if parity is False
                                                                 else "another rank failed its run or parity check")))
    if rank == 0 and args.dump_outputs:
        hb("dump_outputs")
        dump_outputs(d_out, args.dump_outputs)

    # The north star asks for 1920x1080 next to 3840x2160 at every GPU count: the same protocol (barriers on both sides, max over
    # ranks) on 4x as many frames of a quarter of the size, so that it is reported by the 1/2/4/8 runs as well.  Not the headline.
    second = None
    if args.full and (w, h) == (3840, 2160) and not args.no_second_resolution:
        hw, hh, hb2 = 1920, 1080, 4 * B
        hb("second_resolution")
        del d_in, d_out
        e_in = synth.nv12_batch_torch(hw, hh, hb2, args.dist, device, seed=0x5EED1080 + rank)
        e_out = torch.empty_like(e_in)

        def step2():
            if args.op == "equalize":
                ctx.equalize_hist_nv12_batch_dev(e_in, e_out, hw, hh, hb2, uv_mode, stream=stream)
            else:
                ctx.clahe_nv12_batch_dev(e_in, e_out, hw, hh, hb2, uv_mode, 2.0, 8, 8, stream=stream)
        for _ in range(max(3, args.warmup // 2)):
            step2()
        barrier()
        steps2 = max(10, args.steps // 2)
        t0 = time.perf_counter()
        for _ in range(steps2):
            step2()
        barrier()
        el2 = shard.max_over_ranks(time.perf_counter() - t0, dgroup)
        second = {"workload": f"{hb2} x {hw}x{hh} NV12 frames per GPU per step, same op", "value": round(hb2 * world * steps2 / el2, 1), "unit": "frames/s",
                  "steps": steps2, "ms_per_step": round(el2 / steps2 * 1e3, 4),
                  "whole_path_frac_of_8TBs": round((3 * hw * hh + (hw * hh // 2) * (2 if args.uv == "copy" else 1)) * hb2 * steps2 / el2 / 1e9 / HBM_PEAK_GBS, 4)}        # per GPU
        del e_in, e_out

    # BASELINE.json configs[3] as written -- 512 4K frames at 60 fps, frame-per-GPU across the node: with N > 1 every rank streams 512
    # host frames through an mi_pipe on its own GPU, all ranks at the same time (they share the host's memory bandwidth and PCIe root
    # complexes, which is what this figure is about); reduced over the ranks below.  IN THIS PROCESS: the round-3 form started one
    # nv12_stream child per rank, which doubles the processes on the GPUs (four ranks rehearsed on one GPU = 8 GPU processes, more than
    # a gpurun box allows -- docs/experiments.md R4.1).  Every rank takes part in the reductions whatever happened to its own leg.
    stream_all = None
    if args.full and use_dist and not args.no_extras and (w, h) == (3840, 2160):
        barrier()
        hb("stream_all_ranks")
        try:
            mine = stream_in_process(torch, mi_lumaeq, synth, local_rank, w, h, check_with_oracle=(rank == 0))
        except Exception as e:                   # a failed leg must not leave the other ranks in a collective
            mine = {"error": repr(e)}
            print(f"[bench] rank {rank}: stream leg failed: {e!r}", file=sys.stderr, flush=True)
        ok = 1.0 if ("p99_ms" in mine and mine.get("errors", 1) == 0 and mine.get("parity", True) is not False) else 0.0
        red = lambda v, op: shard.reduce_over_ranks(float(v), dist, op)
        stream_all = {"what": "every rank: 512 4K NV12 frames paced at 60 fps through an mi_pipe on its own GPU (pinned frame ring, in-process), "
                              "all ranks at once (host -> host, PCIe inclusive); then the same pipe unpaced",
                      "ranks_ok": int(red(ok, "sum")),
                      "p50_ms_max": red(mine.get("p50_ms", -1.0), "max"), "p99_ms_max": red(mine.get("p99_ms", -1.0), "max"),
                      "max_ms_max": red(mine.get("max_ms", -1.0), "max"), "late_total": int(red(mine.get("late", 0), "sum")),
                      "errors_total": int(red(mine.get("errors", 0), "sum")),
                      "unpaced_frames_per_s_total": round(red(mine.get("unpaced_frames_per_s", 0.0), "sum"), 1),
                      "parity_rank0": mine.get("parity")}
    # ---- kernel timing of THIS rank, then the figures every rank contributes to (before anybody leaves) ----------------
    # Algorithmic bytes per frame (SURVEY.md 8d / DESIGN.md): equalizeHist on Y = 3*W*H (histogram read +
    # apply read + apply write); + UV fill W*H/2 (write) or UV copy 2*(W*H/2).  The fused kernel performs
    # the WHOLE path in one launch, so its algorithmic bytes are the whole-path figure; its HBM traffic is
    # lower (the Y plane is read once and kept in registers) -- see `traffic` (PMC) and `moved_bytes_per_launch`.
    uv_bytes = (ysz // 2) * (2 if args.uv == "copy" else 1)
    per_kernel_alg = {"hist_partial_kernel": ysz * B, "lut_apply_kernel": (2 * ysz + uv_bytes) * B,
                      "equalize_fused_kernel": (3 * ysz + uv_bytes) * B,
                      "tile_hist_kernel": ysz * B, "clahe_interp_kernel": (2 * ysz + uv_bytes) * B}
    kinfo = {}
    for name, p in prof.items():
        if p["launches"]:
            avg_ms = p["total_ms"] / p["launches"]
            e = {"avg_ms": round(avg_ms, 5), "launches": p["launches"], "p10_ms": round(p["p10_ms"], 5), "p50_ms": round(p["p50_ms"], 5),
                 "p90_ms": round(p["p90_ms"], 5)}
            if name in per_kernel_alg:
                e["alg_GBs"] = round(per_kernel_alg[name] / (avg_ms * 1e-3) / 1e9, 1)
            kinfo[name] = e
    cands = sorted(k for k in kinfo if k in per_kernel_alg)
    dom = max(cands, key=lambda k: kinfo[k]["avg_ms"] * kinfo[k]["launches"]) if cands else None
    # the dominant kernel's average launch time on every rank: mean, fastest and slowest GPU (the same kernel dominates everywhere:
    # all ranks run the same configuration; a rank without timings contributes a negative value and voids the mean)
    hb("reduce")
    dom_ms_mine = kinfo[dom]["avg_ms"] if dom else -1.0
    dom_ms_sum = shard.reduce_over_ranks(dom_ms_mine, dgroup, "sum")
    dom_ms_max = shard.reduce_over_ranks(dom_ms_mine, dgroup, "max")
    dom_ms_min = -shard.reduce_over_ranks(-dom_ms_mine, dgroup, "max")
    fallbacks_all = int(shard.reduce_over_ranks(float(max(fused_fallbacks, 0)), dgroup, "sum"))
    ranks_bound = int(shard.reduce_over_ranks(1.0 if placement.get("cpus", 0) > 0 else 0.0, dgroup, "sum"))
    if use_dist:
        dist.barrier()                           # every reduction is done: the ranks leave together, rank 0 goes on alone
        dist.destroy_process_group()
    if rank != 0:
        hb("done")
        return

    total_frames = B * world * args.steps
    fps = total_frames / elapsed
    ms_step = elapsed / args.steps * 1e3

    # `traffic` is NOT measured by this run: PMC counters need rocprofv3 (separate --pmc passes, tools/collect_profiles.sh).
    # It is the committed per-launch figure of the same kernel / workload, and `traffic_source` says where it came from.
    traffic, traffic_source = None, None
    tfile = ROOT / "profiles" / "traffic.json"
    if tfile.exists() and dom:
        try:
            ent = json.loads(tfile.read_text()).get(f"{dom}:{args.op}:{w}x{h}x{B}:{args.uv}")
            if isinstance(ent, dict):
                traffic, traffic_source = ent.get("bytes"), ent.get("source")
            elif ent is not None:
                traffic, traffic_source = ent, "profiles/traffic.json (round 1 PMC passes)"
        except Exception:
            traffic = None
    roofline = None
    if dom and dom_ms_min > 0:
        alg_bytes = per_kernel_alg[dom]                              # per launch = per GPU: every rank launches on its own batch
        avg_ms_all = dom_ms_sum / world                              # mean over the ranks of each rank's average launch duration
        achieved = alg_bytes / (avg_ms_all * 1e-3) / 1e9
        roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                    "alg_bytes_per_launch": alg_bytes, "avg_launch_ms": round(avg_ms_all, 5),
                    "avg_launch_ms_fastest_rank": round(dom_ms_min, 5), "avg_launch_ms_slowest_rank": round(dom_ms_max, 5),
                    "frac_slowest_rank": round(alg_bytes / (dom_ms_max * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "ranks": world, "per": "GPU (each rank's own launches; mean over ranks)",
                    "launch_ms_p10_p50_p90_rank0": [kinfo[dom]["p10_ms"], kinfo[dom]["p50_ms"], kinfo[dom]["p90_ms"]]}
        # ONE CLOCK (round 6).  `frac` uses HIP events stamped by the dispatches; the committed profiles use rocprofv3's kernel trace.
        # profiles/clock.json holds, for this kernel and workload, ONE run in which the same 50 launches were timed by both
        # (tools/one_clock.sh): `avg_launch_ms_rocprof` / `frac_rocprof` are that run's rocprofv3 figures (another box, like `traffic`), and
        # `frac_this_run_on_rocprof_clock` rescales THIS run's launches by the ratio of the two clocks on those same launches -- so
        # a reader never has to choose a clock, or a box.
        cfile = ROOT / "profiles" / "clock.json"
        if cfile.exists():
            try:
                ent = json.loads(cfile.read_text()).get(f"{dom}:{args.op}:{w}x{h}x{B}:{args.uv}")
                if ent:
                    ratio = ent["avg_launch_ms_rocprof"] / ent["avg_launch_ms_hip_events_same_launches"]
                    roofline["avg_launch_ms_rocprof"] = ent["avg_launch_ms_rocprof"]
                    roofline["frac_rocprof"] = round(alg_bytes / (ent["avg_launch_ms_rocprof"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                    roofline["rocprof_over_hip_events_same_launches"] = round(ratio, 4)
                    roofline["frac_this_run_on_rocprof_clock"] = round(alg_bytes / (avg_ms_all * ratio * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                    roofline["clock_source"] = ent["source"]
            except Exception:
                pass
        # the same launch priced on the bytes that MOVE: the fused kernel reads Y once (2*W*H + UV per frame), every other
        # kernel moves its algorithmic bytes.  frac_moved_bytes is against the 8 TB/s peak, and the second figure against the
        # 6.29 TB/s a plain copy kernel reaches on this chip (MI355X_MICROARCH.md).
        moved = (2 * ysz + uv_bytes) * B if dom == "equalize_fused_kernel" else alg_bytes
        moved_GBs = moved / (avg_ms_all * 1e-3) / 1e9
        roofline["moved_bytes_per_launch"] = moved
        roofline["moved_GBs"] = round(moved_GBs, 1)
        roofline["frac_moved_bytes"] = round(moved_GBs / HBM_PEAK_GBS, 4)
        roofline["frac_moved_bytes_of_measured_copy_ceiling"] = round(moved_GBs / HBM_MEASURED_COPY_GBS, 4)

    out = {
        "metric": "frames/sec, 3840x2160 NV12 Y equalizeHist" if (args.op == "equalize" and (w, h) == (3840, 2160))
                  else f"frames/sec, {w}x{h} NV12 Y {args.op}",
        "value": round(fps, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_step, 4), "ms_per_frame": round(elapsed / total_frames * 1e3 * world, 6),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"{B} x {w}x{h} NV12 frames per GPU per step, Y {args.op}"
                               f"{'' if args.op == 'equalize' else ' 8x8 clip 2.0'} + UV {args.uv}, device-resident "
                               f"(BASELINE.json configs[1] batched), Y distribution {args.dist}",
                   "path": "fused single-read kernel" if "equalize_fused_kernel" in kinfo else "staged kernels",
                   "frames_per_gpu_per_step": B, "width": w, "height": h, "uv": args.uv, "op": args.op,
                   "sharding": f"one replica batch per GPU (frame k -> GPU k mod {world}), no data-path collective",
                   "numa": {"rank0": placement.get("why"), "ranks_bound": ranks_bound, "ranks": world}},
        "parity_spot_check": parity,
        "fused_fallbacks_in_run": fallbacks_all,
        "dist_backend_used": backend_used, "world_seen_by_backend": world_seen,
        "whole_path_alg_GBs": round((3 * ysz + uv_bytes) * fps / 1e9, 1),
        "nv12_1080p": second,
        "roofline": roofline,
        "kernels_rank0": kinfo,
    }

    # secondary figures must never cost the headline its JSON line
    def guarded(fn, *a):
        try:
            return fn(*a)
        except Exception as e:
            print(f"[bench] {fn.__name__} failed: {e!r}", file=sys.stderr, flush=True)
            return {"error": repr(e)}
    if stream_all is not None:
        out["stream_4k60_512_all_gpus"] = stream_all
    if args.full and world == 1:
        out["opencv_cross_check"] = guarded(opencv_cross_check, ctx, w, h, args.dist)
    if args.full and world == 1 and not use_dist and not args.no_extras:     # (--force-dist behaves like a rank of an N>1 job: no N=1 extras)
        hb("extras")
        out["extras"] = guarded(extras, ctx, args, torch, mi_lumaeq, synth)
    if args.full and not args.no_cpu_baseline:
        hb("cpu_baseline")                                   # N > 1 as well: rank 0 alone by now, the other ranks have exited
        out["cpu_baseline"] = guarded(cpu_baseline, args, w, h)
    line = (json.dumps(out) + "\n").encode()
    while line:
        line = line[os.write(json_fd, line):]
    os.close(json_fd)
    hb("done")


def stream_in_process(torch, mi_lumaeq, synth, device, w, h, frames=512, fps=60, unpaced_frames=1500, check_with_oracle=False, ring=8, depth=0):
    """BASELINE.json configs[3] inside THIS process: `frames` WxH NV12 host frames released at `fps` through an mi_pipe on `device`
    (a context of its own; pinned frame ring, the way a recycled buffer pool is registered once), latency = release -> delivered;
    then the same pipe unpaced with its depth kept in flight.  The N > 1 ranks use this instead of an nv12_stream child each, so a
    job never has more GPU processes than ranks."""
    import numpy as np
    fb = w * h * 3 // 2
    # the ring is ordinary memory registered ONCE with the library (mi_host_register), the way nv12_stream registers its ring and a
    # pipeline would register a recycled buffer pool: registered ranges are recognised without asking the runtime about every frame
    ins = [np.empty(fb, np.uint8) for _ in range(ring)]
    outs = [np.zeros(fb, np.uint8) for _ in range(ring)]
    base = [synth.nv12_frame(w, h, "D2", 4000 + k) for k in range(2)]
    for k in range(ring):
        ins[k][:] = base[k % 2]
    res = {"frames": frames, "fps": fps, "errors": 0}
    registered = []
    ctx2 = mi_lumaeq.Context(device)
    try:
        for a in ins + outs:
            mi_lumaeq.host_register(a)
            registered.append(a)
        with mi_lumaeq.Pipe(ctx2, w, h, op=mi_lumaeq.OP_EQUALIZE, uv_mode=mi_lumaeq.UV_FILL128, depth=depth) as pipe:
            depth = pipe.depth                                  # 0 asked for the library's default for this frame size
            res["driver"] = f"in-process mi_pipe (python), depth {depth}, registered ring of {ring}"
            for k in range(4):                                  # warm: staging verdicts, queues
                pipe.submit(ins[k % ring], outs[k % ring], k)
                pipe.wait()
            lat, period = [], 1.0 / fps
            t0 = time.perf_counter() + 0.002
            for k in range(frames):
                release = t0 + k * period
                while True:                                     # sleep most of the way, spin the last half millisecond
                    left = release - time.perf_counter()
                    if left <= 0:
                        break
                    if left > 0.0007:
                        time.sleep(left - 0.0005)
                try:
                    pipe.submit(ins[k % ring], outs[k % ring], k)
                    pipe.wait()
                    lat.append((time.perf_counter() - release) * 1e3)
                except mi_lumaeq.MiError:
                    res["errors"] += 1
            if lat:
                lat.sort()
                budget = 1000.0 / fps
                res.update(p50_ms=round(lat[len(lat) // 2], 3), p90_ms=round(lat[len(lat) * 9 // 10], 3),
                           p99_ms=round(lat[min(len(lat) - 1, len(lat) * 99 // 100)], 3), max_ms=round(lat[-1], 3),
                           late=sum(1 for v in lat if v > budget))
            if check_with_oracle:                               # checker only: the last delivered frame of this rank against the oracle
                import oracle
                k = (frames - 1) % ring
                res["parity"] = bool(np.array_equal(outs[k], oracle.nv12_frame(ins[k], w, h, uv_mode=0, op=0)))
            # unpaced: the C entry points directly with the ring's addresses taken once -- the binding's per-call argument checks and
            # `ndarray.ctypes` objects cost ~25 us of a 185 us frame, and this figure is about the pipe, not about Python
            import ctypes
            L, hp = ctx2._L, pipe._h
            in_ptr, out_ptr = [a.ctypes.data for a in ins], [a.ctypes.data for a in outs]
            tag, ptr = ctypes.c_uint64(0), ctypes.c_void_p()
            tag_ref, ptr_ref = ctypes.byref(tag), ctypes.byref(ptr)
            sub = done = 0
            t0 = time.perf_counter()
            while done < unpaced_frames:
                while sub < unpaced_frames and sub - done < depth:
                    if L.mi_pipe_submit(hp, in_ptr[sub % ring], out_ptr[sub % ring], sub) != 0:
                        res["errors"] += 1
                    sub += 1
                if L.mi_pipe_wait(hp, tag_ref, ptr_ref) != 0:
                    res["errors"] += 1
                    if res["errors"] > 8:
                        break
                done += 1
            if done:
                res["unpaced_frames_per_s"] = round(done / (time.perf_counter() - t0), 1)
    finally:
        ctx2.close()                                            # (the pipe is gone by now: nothing is pending on the ring)
        for a in registered:
            try:
                mi_lumaeq.host_unregister(a)
            except mi_lumaeq.MiError as e:
                print(f"[bench] stream ring: {e}", file=sys.stderr, flush=True)
    return res


def stream_config4(w, h, device=None):
    """BASELINE.json configs[3] on this GPU: 512 WxH NV12 frames released at 60 fps through ONE worker of the C++ frame pool
    (host frame in -> host frame out, PCIe inclusive; opencv-opencl_amd/cxx/examples/nv12_stream.cpp, the reference's worker
    pipeline OpenCVequalHist.cpp:102-196 minus the codecs), plus the same pipeline unpaced.  Never the headline value.
    `device`: the child process is shown only that GPU (HIP_VISIBLE_DEVICES), so its one worker lands on it -- how each rank of an
    N-GPU run streams on its own GPU."""
    import re
    import subprocess
    exe = ROOT / "opencv-opencl_amd" / "lib" / "nv12_stream"
    if not exe.exists():
        return {"error": "nv12_stream not built (python -c 'import __graft_entry__ as g; g.build()')"}
    env = None
    if device is not None:
        env = dict(os.environ)
        seen = [x for x in env.get("HIP_VISIBLE_DEVICES", "").split(",") if x.strip() != ""]
        env["HIP_VISIBLE_DEVICES"] = seen[device] if device < len(seen) else str(device)
    base = [str(exe), "--width", str(w), "--height", str(h), "--workers", "1", "--op", "equalize", "--uv", "fill128"]
    r = subprocess.run(base + ["--frames", "512", "--paced", "--fps", "60"], capture_output=True, text=True, timeout=180, env=env)
    res = {"frames": 512, "fps": 60, "workers": 1, "returncode": r.returncode,
           "what": "host NV12 frame in -> host NV12 frame out (PCIe inclusive), one pool worker driving an mi_pipe, registered frame ring"}
    m = re.search(r"p50=([0-9.]+) p90=([0-9.]+) p99=([0-9.]+) max=([0-9.]+); frames over the [0-9.]+ ms frame budget: (\d+)", r.stdout)
    if m:
        res.update(p50_ms=float(m.group(1)), p90_ms=float(m.group(2)), p99_ms=float(m.group(3)), max_ms=float(m.group(4)), late=int(m.group(5)))
    m = re.search(r"errors=(\d+)", r.stdout)
    if m:
        res["errors"] = int(m.group(1))
    res["placement"] = re.findall(r"^placement: (.*)$", r.stdout, flags=re.M)      # where the streamer's threads and frame ring live
    u = subprocess.run(base + ["--frames", "2000"], capture_output=True, text=True, timeout=180, env=env)
    m = re.search(r"= ([0-9.]+) frames/s", u.stdout)
    if m:
        res["unpaced_frames_per_s"] = float(m.group(1))
    return res


def extras(ctx, args, torch, mi_lumaeq, synth):
    """Secondary figures outside the timed region (N=1 only): single-frame latency, device-resident and
    through the host cv::Mat boundary (PCIe-inclusive; never the headline value), and CLAHE."""
    import numpy as np
    from mi_lumaeq import xfer
    w, h = args.width, args.height
    res = {}
    # the north star also asks for the stand-alone LUT-apply kernel's roofline: run the three-kernel path briefly
    if args.op == "equalize":
        Bq = args.batch
        q_in = synth.nv12_batch_torch(w, h, Bq, args.dist, "cuda", seed=3)
        q_out = torch.empty_like(q_in)
        uvm = mi_lumaeq.UV_COPY if args.uv == "copy" else mi_lumaeq.UV_FILL128
        ctx.set_option("fused", 0)
        for _ in range(3):
            ctx.equalize_hist_nv12_batch_dev(q_in, q_out, w, h, Bq, uvm)
        ctx.synchronize()
        ctx.profile_read(reset=True)
        ctx.set_profiling(True)
        for _ in range(20):
            ctx.equalize_hist_nv12_batch_dev(q_in, q_out, w, h, Bq, uvm)
        ctx.set_profiling(False)
        pr = ctx.profile_read(reset=True)
        ctx.set_option("fused", 1)
        ysz = w * h
        uvb = (ysz // 2) * (2 if args.uv == "copy" else 1)
        ap = pr["lut_apply_kernel"]; hp = pr["hist_partial_kernel"]
        if ap["launches"]:
            a_ms = ap["total_ms"] / ap["launches"]; h_ms = hp["total_ms"] / hp["launches"]
            res["three_kernel_path"] = {
                "lut_apply_kernel": {"avg_ms": round(a_ms, 5), "alg_GBs": round((2 * ysz + uvb) * Bq / (a_ms * 1e-3) / 1e9, 1),
                                     "frac_of_8TBs": round((2 * ysz + uvb) * Bq / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                "hist_partial_kernel": {"avg_ms": round(h_ms, 5), "alg_GBs": round(ysz * Bq / (h_ms * 1e-3) / 1e9, 1)}}
            # ... and the histogram stage on its own (mi_hist_u8_batch_dev in a loop): inside the three-kernel sequence it runs behind the
            # previous call's 0.8 GB write drain, which is charged to whoever runs next; alone it shows what the kernel itself does
            d_hist = torch.empty((Bq, 256), dtype=torch.int32, device="cuda")
            fs = w * h * 3 // 2
            for _ in range(3):
                ctx.hist_batch_dev(q_in, w, h, Bq, d_hist, src_frame=fs)
            ctx.synchronize()
            ctx.profile_read(reset=True)
            ctx.set_profiling(True)
            for _ in range(20):
                ctx.hist_batch_dev(q_in, w, h, Bq, d_hist, src_frame=fs)
            ctx.set_profiling(False)
            pr2 = ctx.profile_read(reset=True)["hist_partial_kernel"]
            if pr2["launches"]:
                i_ms = pr2["total_ms"] / pr2["launches"]
                res["three_kernel_path"]["hist_partial_kernel_alone"] = {"avg_ms": round(i_ms, 5), "alg_GBs": round(ysz * Bq / (i_ms * 1e-3) / 1e9, 1),
                                                                         "frac_of_8TBs": round(ysz * Bq / (i_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            del d_hist
        del q_in, q_out
    # north star: throughput on 1920x1080 as well as 3840x2160 (same path, 256-frame batches = the same bytes per step)
    if (w, h) == (3840, 2160) and args.op == "equalize":
        hw, hh, hb = 1920, 1080, 4 * args.batch
        hd_in = synth.nv12_batch_torch(hw, hh, hb, args.dist, "cuda", seed=17)
        hd_out = torch.empty_like(hd_in)
        uvm = mi_lumaeq.UV_COPY if args.uv == "copy" else mi_lumaeq.UV_FILL128
        sm = torch.cuda.current_stream().cuda_stream
        for _ in range(3):
            ctx.equalize_hist_nv12_batch_dev(hd_in, hd_out, hw, hh, hb, uvm, stream=sm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            ctx.equalize_hist_nv12_batch_dev(hd_in, hd_out, hw, hh, hb, uvm, stream=sm)
        torch.cuda.synchronize()
        res["nv12_1080p_equalize_frames_per_s"] = round(50 * hb / (time.perf_counter() - t0), 1)
        # every Y distribution reported separately (D1 uniform, D2 natural low-contrast, D3 constant -- the
        # shortcut path and worst-case atomic contention, D4 two-valued checkerboard, D5 ramp), same batch shape as the
        # headline; and BASELINE config 5's real behaviour (UV passthrough) next to the UV=128 headline
        by_dist = {}
        for dname in synth.DISTS:
            dd_in = synth.nv12_batch_torch(w, h, args.batch, dname, "cuda", seed=23)
            dd_out = torch.empty_like(dd_in)
            for _ in range(3):
                ctx.equalize_hist_nv12_batch_dev(dd_in, dd_out, w, h, args.batch, mi_lumaeq.UV_FILL128, stream=sm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30):
                ctx.equalize_hist_nv12_batch_dev(dd_in, dd_out, w, h, args.batch, mi_lumaeq.UV_FILL128, stream=sm)
            torch.cuda.synchronize()
            by_dist[dname] = round(30 * args.batch / (time.perf_counter() - t0), 1)
            if dname == args.dist:
                # the Y planes alone (cv::equalizeHist and nothing else: no NV12 rebuild), same frames, in place in the NV12 batch layout
                fs = w * h * 3 // 2
                for _ in range(3):
                    ctx.equalize_hist_batch_dev(dd_in, dd_out, w, h, args.batch, src_frame=fs, dst_frame=fs, stream=sm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(30):
                    ctx.equalize_hist_batch_dev(dd_in, dd_out, w, h, args.batch, src_frame=fs, dst_frame=fs, stream=sm)
                torch.cuda.synchronize()
                res["y_plane_only_equalize_frames_per_s"] = round(30 * args.batch / (time.perf_counter() - t0), 1)
                for _ in range(3):
                    ctx.equalize_hist_nv12_batch_dev(dd_in, dd_out, w, h, args.batch, mi_lumaeq.UV_COPY, stream=sm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(30):
                    ctx.equalize_hist_nv12_batch_dev(dd_in, dd_out, w, h, args.batch, mi_lumaeq.UV_COPY, stream=sm)
                torch.cuda.synchronize()
                res["uv_copy_equalize_frames_per_s"] = round(30 * args.batch / (time.perf_counter() - t0), 1)
            del dd_in, dd_out
        res["equalize_frames_per_s_by_distribution"] = by_dist
        del hd_in, hd_out
    if (w, h) == (3840, 2160) and args.op == "equalize":
        try:
            res["stream_4k60_512"] = stream_config4(w, h)
        except Exception as e:                                   # a secondary figure never costs the line
            res["stream_4k60_512"] = {"error": repr(e)}
    frame = synth.nv12_batch_torch(w, h, 1, args.dist, "cuda", seed=99)
    outb = torch.empty_like(frame)
    stream = torch.cuda.current_stream().cuda_stream

    def timeit(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def median_ms(fn, n):
        """synchronous calls: per-call wall time, median (one descheduled call must not move a latency figure)"""
        for _ in range(3):
            fn()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]

    res["single_frame_dev_equalize_ms"] = round(timeit(
        lambda: ctx.equalize_hist_nv12_batch_dev(frame, outb, w, h, 1, mi_lumaeq.UV_FILL128, stream=stream), 200), 4)
    res["single_frame_dev_clahe8x8_ms"] = round(timeit(
        lambda: ctx.clahe_nv12_batch_dev(frame, outb, w, h, 1, mi_lumaeq.UV_FILL128, 2.0, 8, 8, stream=stream), 200), 4)
    # the launch-bound case replayed from a captured HIP graph (all per-launch state of the fused path lives in device memory, so a
    # captured call replays as it is): one graph launch instead of 2 (equalize + finish) / 2-3 (CLAHE) kernel launches per frame
    gctx = None
    try:
        if not args.graph_extras:
            raise StopIteration
        gctx = mi_lumaeq.Context(torch.cuda.current_device())   # its own context: scratch seen by a capture is never freed again
        for name, fn in (("equalize", lambda st: gctx.equalize_hist_nv12_batch_dev(frame, outb, w, h, 1, mi_lumaeq.UV_FILL128, stream=st)),
                         ("clahe8x8", lambda st: gctx.clahe_nv12_batch_dev(frame, outb, w, h, 1, mi_lumaeq.UV_FILL128, 2.0, 8, 8, stream=st))):
            fn(stream)                                         # size the scratch eagerly: allocations are not capturable
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn(torch.cuda.current_stream().cuda_stream)
            res[f"single_frame_dev_{name}_graph_replay_ms"] = round(timeit(g.replay, 200), 4)
            del g
        torch.cuda.synchronize()
    except StopIteration:
        pass
    except Exception as e:                                   # never let an optional figure take the bench line down
        res["graph_replay_error"] = repr(e)
    finally:
        if gctx is not None:
            torch.cuda.synchronize()
            gctx.close()
    y = xfer.to_host(frame[0, : w * h]).reshape(h, w)
    dst = np.empty_like(y)
    res["host_mat_equalize_ms_pcie_inclusive"] = round(median_ms(lambda: ctx.equalize_hist(y, dst), 40), 3)
    res["host_mat_clahe8x8_ms_pcie_inclusive"] = round(median_ms(lambda: ctx.clahe(y, 2.0, 8, 8, dst), 40), 3)
    # the two figures above are for ordinary (unpinned) Mats, which the library packs through its own pinned staging; planes in
    # memory the caller pinned (a registered frame pool) are DMA'd as they are
    py, pd = torch.from_numpy(y.copy()).pin_memory(), torch.empty((h, w), dtype=torch.uint8).pin_memory()
    pyn, pdn = py.numpy(), pd.numpy()
    res["host_mat_equalize_ms_pcie_inclusive_pinned_mats"] = round(median_ms(lambda: ctx.equalize_hist(pyn, pdn), 40), 3)
    del py, pd
    B = args.batch
    d_in = synth.nv12_batch_torch(w, h, B, args.dist, "cuda", seed=5)
    d_out = torch.empty_like(d_in)
    for _ in range(10):                                           # steady state like the headline loop: clocks and caches settled
        ctx.clahe_nv12_batch_dev(d_in, d_out, w, h, B, mi_lumaeq.UV_FILL128, 2.0, 8, 8, stream=stream)
    ms = timeit(lambda: ctx.clahe_nv12_batch_dev(d_in, d_out, w, h, B, mi_lumaeq.UV_FILL128, 2.0, 8, 8, stream=stream), 100)
    res["clahe8x8_batch_frames_per_s"] = round(B / (ms * 1e-3), 1)
    # the tile-histogram (+ clip + LUT) pass on its own: inside the CLAHE sequence it runs behind the interpolation's 0.8 GB write drain
    d_luts = torch.empty((B, 64, 256), dtype=torch.uint8, device="cuda")
    fs = w * h * 3 // 2
    for _ in range(3):
        ctx.clahe_tile_luts_batch_dev(d_in, w, h, B, 2.0, 8, 8, d_luts, src_frame=fs, stream=stream)
    torch.cuda.synchronize()
    ctx.profile_read(reset=True)
    ctx.set_profiling(True)
    for _ in range(20):
        ctx.clahe_tile_luts_batch_dev(d_in, w, h, B, 2.0, 8, 8, d_luts, src_frame=fs, stream=stream)
    ctx.set_profiling(False)
    torch.cuda.synchronize()
    th = ctx.profile_read(reset=True)["tile_hist_kernel"]
    if th["launches"]:
        t_ms = th["total_ms"] / th["launches"]
        res["clahe_tile_hist_kernel_alone"] = {"avg_ms": round(t_ms, 5), "alg_GBs": round(w * h * B / (t_ms * 1e-3) / 1e9, 1),
                                               "frac_of_8TBs": round(w * h * B / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    del d_luts
    res["clahe8x8_batch_whole_path_frac_of_8TBs"] = round((3 * w * h + w * h // 2) * B / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    del d_in, d_out
    # BASELINE.json configs[4] taken literally (parity unpinned): BGR -> YUV -> equalize Y -> BGR on
    # 3-channel 4K images (the sequence of singlecolor.cpp:39-66); the file that config names,
    # ColoropenCVCwqualHist.cpp, actually does Y-only + UV passthrough = `--uv copy` of the main metric.
    Bc = 16
    bgr = torch.randint(0, 256, (Bc, h, w, 3), dtype=torch.uint8, device="cuda")
    bgr_out = torch.empty_like(bgr)
    ms = timeit(lambda: ctx.bgr_luma_op_batch_dev(bgr, bgr_out, w, h, Bc, mi_lumaeq.OP_EQUALIZE, stream=stream), 10)
    res["bgr_yuv_equalize_bgr_frames_per_s"] = round(Bc / (ms * 1e-3), 1)
    ms = timeit(lambda: ctx.bgr_luma_op_batch_dev(bgr, bgr_out, w, h, Bc, mi_lumaeq.OP_CLAHE, 2.0, 8, 8, stream=stream), 10)
    res["bgr_yuv_clahe8x8_bgr_frames_per_s"] = round(Bc / (ms * 1e-3), 1)      # clahe1frame.cpp:83-102 as one call
    ms = timeit(lambda: ctx.cvt_color_batch_dev(bgr, bgr_out, w, h, Bc, mi_lumaeq.COLOR_BGR2YUV, stream=stream), 10)
    res["cvtcolor_bgr2yuv_GBs"] = round(2 * 3 * w * h * Bc / (ms * 1e-3) / 1e9, 1)
    del bgr, bgr_out
    # ... and the NV12 form of the same wording: NV12 -> BGR -> equalizeHist on B, G and R -> NV12 (two passes, 4.5 B/px)
    Bn = 32
    nv = synth.nv12_batch_torch(w, h, Bn, args.dist, "cuda", seed=7)
    nv_out = torch.empty_like(nv)
    ms = timeit(lambda: ctx.nv12_bgr_equalize_batch_dev(nv, nv_out, w, h, Bn, stream=stream), 10)
    res["nv12_bgr_channels_equalize_frames_per_s"] = round(Bn / (ms * 1e-3), 1)
    res["nv12_bgr_channels_equalize_GBs"] = round(4.5 * w * h * Bn / (ms * 1e-3) / 1e9, 1)
    del nv, nv_out
    # a photo-like scene instead of noise (mi_lumaeq.synth.photo_like: piecewise-smooth gradients, flat and saturated regions, tiled
    # to 4K with a different window per frame): hot histogram bins, smooth neighbourhoods (LDS broadcasts in the CLAHE gather)
    yp = synth.photo_like(1919, 1079, 20261004)
    Bp = args.batch                                           # the headline's batch size, so that only the content differs
    reps = (-(-(h + 13 * Bp) // yp.shape[0]), -(-(w + 29 * Bp) // yp.shape[1]))
    big = np.tile(yp, reps)
    fr = np.empty((Bp, w * h * 3 // 2), np.uint8)
    for k in range(Bp):                                        # every frame a different window of the tiling
        fr[k, : w * h] = big[13 * k: 13 * k + h, 29 * k: 29 * k + w].reshape(-1)
        fr[k, w * h:] = 128
    d_in = xfer.to_device(fr)
    d_out = torch.empty_like(d_in)
    ms = timeit(lambda: ctx.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, Bp, mi_lumaeq.UV_FILL128, stream=stream), 20)
    res["photo_like_equalize_frames_per_s"] = round(Bp / (ms * 1e-3), 1)
    ms = timeit(lambda: ctx.clahe_nv12_batch_dev(d_in, d_out, w, h, Bp, mi_lumaeq.UV_FILL128, 2.0, 8, 8, stream=stream), 10)
    res["photo_like_clahe8x8_frames_per_s"] = round(Bp / (ms * 1e-3), 1)
    del d_in, d_out
    # equalizeHist on a strided ROI (generic path: row by row, unaligned starts) and 16-bit CLAHE
    Br = 16
    pitch = w + 64
    big = torch.randint(0, 256, (Br, h + 8, pitch), dtype=torch.uint8, device="cuda")
    big_out = torch.zeros_like(big)
    off = 3 * pitch + 21                                           # ROI origin (row 3, column 21): unaligned
    ms = timeit(lambda: ctx.equalize_hist_batch_dev(big.data_ptr() + off, big_out.data_ptr() + off, w, h, Br, src_step=pitch,
                                                    src_frame=(h + 8) * pitch, dst_step=pitch, dst_frame=(h + 8) * pitch, stream=stream), 10)
    res["strided_roi_equalize_frames_per_s"] = round(Br / (ms * 1e-3), 1)
    # 12-bit content (what 16-bit video carries: the range fits the LDS pair tables) and full-range 16-bit content (L2 gathers)
    # ... and 10-bit samples in the HIGH bits of the word, as P010 video stores them: full 16-bit span, 1024 populated values
    # Wider content is on the record too (round 6): 14-bit sensors (thermal / medical: four windows of 4096 values), a 12-bit frame
    # with ONE hot pixel at 65535 (its tile loses the 12-bit bet, the rectangles around it see the whole 16-bit range), and content
    # that fills the 16-bit range, at the 16 frames per call the other rows use (the 4-per-call key is kept for continuity).
    for name, hi, nb, shift, hot in (("clahe16_8x8_12bit_frames_per_s", 4096, 16, 0, False), ("clahe16_8x8_12bit_32_per_call_frames_per_s", 4096, 32, 0, False),
                                     ("clahe16_8x8_p010_10bit_msb_frames_per_s", 1024, 16, 6, False),
                                     ("clahe16_8x8_14bit_frames_per_s", 16384, 16, 0, False),
                                     ("clahe16_8x8_12bit_one_hot_pixel_frames_per_s", 4096, 16, 0, True),
                                     ("clahe16_8x8_fullrange_16_per_call_frames_per_s", 65536, 16, 0, False),
                                     ("clahe16_8x8_fullrange_frames_per_s", 65536, 4, 0, False)):
        s16 = (torch.randint(0, hi, (nb, h, w), dtype=torch.int32, device="cuda") << shift).to(torch.int16)     # bit pattern of the ushort
        if hot:
            s16[:, 1000, 2000] = -1                                # 65535
        o16 = torch.empty_like(s16)
        ms = timeit(lambda: ctx.clahe16_batch_dev(s16, o16, w, h, nb, 2.0, 8, 8, stream=stream), 5)
        res[name] = round(nb / (ms * 1e-3), 1)
        del s16, o16
    return res


if __name__ == "__main__":
    main()
