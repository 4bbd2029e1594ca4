"""CPU checks of bench.py's contract: it refuses to run without a GPU (no fallback), and the cpu_baseline leg
returns the fields the driver reads."""
import argparse
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def test_bench_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stderr + r.stdout)
    assert not r.stdout.strip().startswith("{")                  # no number is reported


def test_cpu_baseline_fields():
    import bench
    args = argparse.Namespace(dist="D2", uv="fill128", op="equalize", cpu_seconds=1.0)
    cb = bench.cpu_baseline(args, 640, 360)
    assert set(["value", "unit", "cores", "kind", "sample"]) <= set(cb)
    assert cb["unit"] == "frames/s" and cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    assert "640x360" in cb["sample"]


def test_cpu_baseline_turns_to_kind_reference_where_cv2_exists(monkeypatch):
    """Where a real OpenCV is importable the CPU baseline is the reference itself (cv2.equalizeHist / CLAHE on the Y plane + the NV12
    rebuild, OpenCVequalHist.cpp:140-162), kind "reference", with the port's figures beside it.  No cv2 on this pool: the plumbing
    runs here against a STAND-IN module named cv2 whose two functions are the oracle's -- it times nothing real and pins nothing."""
    import types
    import numpy as np
    import bench
    import oracle
    fake = types.ModuleType("cv2")
    fake.__version__ = "stand-in (oracle)"
    threads = {"n": 7}
    fake.getNumThreads = lambda: threads["n"]
    fake.setNumThreads = lambda n: threads.__setitem__("n", n)
    fake.equalizeHist = lambda a: oracle.equalize_hist(np.ascontiguousarray(a))

    class _Clahe:
        def apply(self, a): return oracle.clahe(np.ascontiguousarray(a), 2.0, 8, 8)
    fake.createCLAHE = lambda clip, tiles: _Clahe()
    monkeypatch.setitem(sys.modules, "cv2", fake)
    for op in ("equalize", "clahe"):
        args = argparse.Namespace(dist="D2", uv="copy", op=op, cpu_seconds=1.0)
        cb = bench.cpu_baseline(args, 640, 360)
        assert cb["kind"] == "reference" and cb["unit"] == "frames/s" and cb["value"] > 0 and cb["cores"] == 7
        assert "cv2 stand-in (oracle)" in cb["sample"] and "640x360" in cb["sample"]
        assert cb["value_1thread"] > 0 and cb["value_1080p"] > 0 and threads["n"] == 7          # thread count restored
        assert cb["port"]["value"] > 0 and cb["port"]["cores"] >= 1 and "restatement" in cb["port"]["sample"]


_STUB = r'''
import json, os, sys, time
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert os.environ["LOCAL_RANK"] == os.environ["RANK"] and os.environ["MASTER_ADDR"] == "127.0.0.1" and int(os.environ["MASTER_PORT"]) > 0
mode = sys.argv[1]
print(f"hello from rank {rank} of {world}: argv={sys.argv[1:]}", flush=True)
if mode == "ok":
    time.sleep(0.2 * (world - rank))                      # rank 0 finishes last, like the real bench
    if rank == 0:
        print(json.dumps({"metric": "stub", "n_gpus": world, "port": int(os.environ["MASTER_PORT"])}), flush=True)
elif mode == "rank1_fails":
    if rank == 1:
        sys.exit(7)
    time.sleep(600)                                       # "blocked in a collective with the dead rank"
elif mode == "no_line":
    pass
elif mode == "rank2_hangs":                               # every rank announces its phases; rank 2 never leaves "stream_all_ranks"
    print(f"[bench hb] rank={rank} phase=timed t=+0.1s", file=sys.stderr, flush=True)
    if rank == 2:
        print(f"[bench hb] rank={rank} phase=stream_all_ranks t=+0.2s", file=sys.stderr, flush=True)
        time.sleep(600)
    print(f"[bench hb] rank={rank} phase=done t=+0.3s", file=sys.stderr, flush=True)
'''


def test_self_launcher_starts_one_fresh_child_per_gpu(tmp_path, capfd):
    """`python bench.py --gpus N` with WORLD_SIZE unset becomes a launcher (bench.launch_children): N children with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, rank 0's JSON line relayed to stdout, everything else to stderr, the worst
    exit code returned, and ranks left waiting for a dead one are ended after the grace period.  Stub children: no GPU here."""
    import json
    import time
    import bench
    stub = tmp_path / "stub_child.py"
    stub.write_text(_STUB)
    cmd = [sys.executable, str(stub)]
    rc = bench.launch_children(3, ["ok", "--steps", "5"], child_cmd=cmd)
    out, err = capfd.readouterr()
    assert rc == 0
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 3
    for r in range(3):
        assert f"[rank {r}] hello from rank {r} of 3: argv=['ok', '--steps', '5']" in err
    t0 = time.monotonic()
    rc = bench.launch_children(2, ["rank1_fails"], child_cmd=cmd, grace_s=1.0)
    assert rc == 7 and time.monotonic() - t0 < 30                # rank 0 did not keep the launcher for its 600 s
    capfd.readouterr()
    assert bench.launch_children(2, ["no_line"], child_cmd=cmd) == 1     # all ranks fine but no result: still a failure


_STUB8 = r'''
import json, os, sys
rank = int(os.environ["RANK"])
rec = {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                       "HSA_ENABLE_IPC_MODE_LEGACY")}
rec["pid"], rec["ppid"], rec["argv"] = os.getpid(), os.getppid(), sys.argv[1:]
with open(os.path.join(os.environ["STUB_OUT"], f"rank{rank}.{os.getpid()}.json"), "w") as f:
    json.dump(rec, f)
print(f"[bench hb] rank={rank} phase=done t=+0.0s", file=sys.stderr, flush=True)
if rank == 0:
    print(json.dumps({"metric": "stub", "n_gpus": int(os.environ["WORLD_SIZE"])}), flush=True)
'''


def test_self_launcher_with_eight_gpus_one_child_per_rank(tmp_path, capfd, monkeypatch):
    """The shape of the driver's 8-GPU node (the reference's 1..8 workers: OpenCVequalHist.cpp:274, :397-402), with stub children: exactly
    one child per rank, LOCAL_RANK 0..7 = RANK (rank r takes GPU r), WORLD_SIZE 8, one rendezvous on 127.0.0.1 shared by all,
    HSA_ENABLE_IPC_MODE_LEGACY=0 in EVERY child's environment whether or not the launcher's own environment has it (RCCL's peers on this
    pool speak dmabuf IPC only) -- and a value the caller set on purpose is not overwritten -- the caller's arguments handed on unchanged,
    and the deadline a plain `python bench.py --gpus 8` runs under: 480 s, inside the driver's 600."""
    import json
    import os
    import bench
    stub = tmp_path / "stub8.py"
    stub.write_text(_STUB8)
    for legacy_in_parent, want in ((None, "0"), ("0", "0"), ("1", "1")):
        out_dir = tmp_path / f"out_{legacy_in_parent}"
        out_dir.mkdir()
        monkeypatch.setenv("STUB_OUT", str(out_dir))
        if legacy_in_parent is None:
            monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
        else:
            monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", legacy_in_parent)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
            monkeypatch.delenv(k, raising=False)
        rc = bench.launch_children(8, ["--gpus", "8", "--steps", "20", "--warmup", "5"], child_cmd=[sys.executable, str(stub)])
        out, err = capfd.readouterr()
        assert rc == 0, err[-2000:]
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 8            # rank 0's line, once
        recs = [json.loads(f.read_text()) for f in sorted(out_dir.iterdir())]
        assert len(recs) == 8                                                     # one child per rank: no rank twice, none missing
        assert sorted(int(r["RANK"]) for r in recs) == list(range(8))
        assert len({r["pid"] for r in recs}) == 8 and {r["ppid"] for r in recs} == {os.getpid()}      # fresh processes of THIS launcher
        assert len({r["MASTER_PORT"] for r in recs}) == 1 and int(recs[0]["MASTER_PORT"]) > 0
        for r in recs:
            assert r["LOCAL_RANK"] == r["RANK"] and r["WORLD_SIZE"] == "8" and r["LOCAL_WORLD_SIZE"] == "8"
            assert r["MASTER_ADDR"] == "127.0.0.1"
            assert r["HSA_ENABLE_IPC_MODE_LEGACY"] == want, (legacy_in_parent, r)
            assert r["argv"] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
        for rank in range(8):
            assert f"[bench hb] rank={rank} phase=done" in err
    # what a plain `python bench.py --gpus 8` hands launch_children: the parsed default deadline (480 s) -- and that is also the default
    # of launch_children itself, for callers that pass none
    args = bench.parse_args(["--gpus", "8"])
    assert args.gpus == 8 and args.deadline_s == 480.0 == bench.DEADLINE_DEFAULT_S == bench.launch_children.__defaults__[-1]


def test_launcher_deadline_reports_each_ranks_phase(tmp_path, capfd):
    """A job that stops making progress must not end in silence (round 3's four-rank rehearsal left an empty record): at the
    deadline the launcher ends the children by PID, says which phase each rank last announced, and returns 124."""
    import time
    import bench
    stub = tmp_path / "stub_child.py"
    stub.write_text(_STUB)
    t0 = time.monotonic()
    rc = bench.launch_children(4, ["rank2_hangs"], child_cmd=[sys.executable, str(stub)], deadline_s=3.0)
    assert rc == 124 and time.monotonic() - t0 < 40
    _, err = capfd.readouterr()
    assert "DEADLINE of 3 s passed; ranks still running: [2]" in err
    assert "rank 2: running, last phase: stream_all_ranks" in err
    for r in (0, 1, 3):
        assert f"rank {r}: exited 0, last phase: done" in err
    assert "[bench hb] rank=2 phase=stream_all_ranks" in err           # heartbeats are relayed as they come


def test_rank_watchdog_leaves_with_124():
    """A rank started by torchrun has no launcher above it: its own watchdog ends it (deadline + 30 s), naming the
    phase it was in."""
    # (the 30 s slack after the deadline is shortened to one second by substituting the Timer the watchdog builds)
    code = ("import sys, time, threading; sys.argv=['bench.py']; import bench; bench._PHASE['name']='timed'; "
            "real = threading.Timer; threading.Timer = lambda s, f: real(1.0, f); "
            "bench.arm_rank_watchdog(5.0); time.sleep(60)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert r.returncode == 124, (r.returncode, r.stderr[-500:])
    assert "DEADLINE of 5 s passed in phase=timed" in r.stderr


def test_plain_invocation_with_gpus_n_launches_instead_of_exiting(tmp_path):
    """The round-2 bench exited with "launch with torch.distributed.run" here.  Without a GPU the children fail loudly (no CPU fallback),
    and the launcher passes their failure on -- but they WERE started, each with its own rank."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by test_bench_two_ranks_contract_on_gpu")
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--dist-backend", "gloo"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0
    assert "no CPU fallback" in r.stderr or "needs HIP devices" in r.stderr, r.stderr[-2000:]
    assert "torch.distributed.run" not in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_bench_two_ranks_contract_on_gpu():
    """N > 1 from a plain invocation: two ranks rehearsed on ONE GPU over gloo (asked for by name; the real thing is RCCL on 2+ GPUs,
    which only the driver's 8-GPU node can run).  The line must carry what a SCALE line is graded on: n_gpus, whole-job value,
    roofline with the per-rank spread, cpu_baseline, the sharding wording, the backend that really connected the ranks."""
    import json
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--all-ranks-on-device", "0",
                        "--steps", "5", "--warmup", "2", "--full", "--no-extras", "--cpu-seconds", "1.5", "--batch", "32"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["scaling"] == "weak" and d["unit"] == "frames/s"
    assert d["dist_backend_used"] == "gloo" and d["world_seen_by_backend"] == 2
    assert abs(d["value"] - 2 * 32 * 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 0.01          # whole job: both ranks' frames
    assert "one replica batch per GPU" in d["config"]["sharding"] and "no data-path collective" in d["config"]["sharding"]
    assert d["config"]["numa"]["ranks"] == 2
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["ranks"] == 2 and rf["kernel"] in ("equalize_fused_kernel", "lut_apply_kernel")
    assert 0 < rf["avg_launch_ms_fastest_rank"] <= rf["avg_launch_ms"] <= rf["avg_launch_ms_slowest_rank"]
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1
    assert d["parity_spot_check"] is True and isinstance(d["fused_fallbacks_in_run"], int)


@pytest.mark.gpu
def test_bench_two_ranks_under_torchrun_as_the_driver_launches_it():
    """The driver does not use bench.py's own launcher for N > 1: it runs `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` (WORLD_SIZE set: every process is a rank).  Rehearsed here in exactly
    that form with two ranks on the one GPU over gloo: torchrun's stdout must carry rank 0's JSON line and NOTHING else from any rank
    (a rank writes the line through a private duplicate of fd 1 and points fd 1 at stderr), and the line must say two ranks."""
    import json
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--all-ranks-on-device", "0",
                        "--steps", "5", "--warmup", "2", "--full", "--cpu-seconds", "1.5", "--batch", "16"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out_lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(out_lines) == 1 and out_lines[0].startswith("{"), r.stdout[:1500]
    d = json.loads(out_lines[0])
    assert d["n_gpus"] == 2 and d["dist_backend_used"] == "gloo" and d["world_seen_by_backend"] == 2 and d["parity_spot_check"] is True
    assert abs(d["value"] - 2 * 16 * 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 0.01
    assert d["stream_4k60_512_all_gpus"]["ranks_ok"] == 2 and d["roofline"]["ranks"] == 2 and d["cpu_baseline"]["value"] > 0
    for rank in (0, 1):
        assert f"[bench hb] rank={rank} phase=done" in r.stderr


@pytest.mark.gpu
def test_bench_four_ranks_contract_on_gpu():
    """Four ranks rehearsed on ONE GPU over gloo, extras ON so that the all-ranks stream leg and its reductions run -- the code that
    only exists for world > 1 and that the driver's 4- and 8-GPU runs execute.  The job must end by itself with one line, every rank
    must have announced its phases, and no rank may start a further GPU process (a gpurun box allows six)."""
    import json
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4", "--dist-backend", "gloo", "--all-ranks-on-device", "0",
                        "--steps", "5", "--warmup", "2", "--full", "--cpu-seconds", "1.5", "--batch", "16", "--deadline-s", "600"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["steps"] == 5 and d["scaling"] == "weak"
    assert d["dist_backend_used"] == "gloo" and d["world_seen_by_backend"] == 4
    assert abs(d["value"] - 4 * 16 * 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 0.01
    assert d["roofline"]["ranks"] == 4 and d["config"]["numa"]["ranks"] == 4 and d["parity_spot_check"] is True
    sa = d["stream_4k60_512_all_gpus"]
    assert sa["ranks_ok"] == 4 and sa["errors_total"] == 0 and sa["parity_rank0"] is True, sa
    assert sa["p50_ms_max"] > 0 and sa["unpaced_frames_per_s_total"] > 0
    assert d["nv12_1080p"]["value"] > 0 and d["cpu_baseline"]["value"] > 0
    for rank in range(4):
        for phase in ("context", "timed", "stream_all_ranks", "reduce", "done"):
            assert f"[bench hb] rank={rank} phase={phase}" in r.stderr, (rank, phase)
    assert "nv12_stream" not in r.stderr


def test_deadlines_fit_inside_the_drivers_limit():
    """The driver ends a bench run after 600 s.  The launcher's deadline and a torchrun rank's own watchdog (deadline + slack) must
    both fire before that, or a stuck N-rank job is killed from outside without a single "rank r was in phase p" line."""
    import bench
    assert bench.parse_args([]).deadline_s == bench.DEADLINE_DEFAULT_S <= 480.0
    assert bench.DEADLINE_DEFAULT_S + bench.RANK_WATCHDOG_SLACK_S < 600.0 - 60.0
    assert bench.launch_children.__defaults__[-1] == bench.DEADLINE_DEFAULT_S


def test_plain_run_options():
    """A plain run does the headline only: --full (off by default) adds the other legs; --steps is the number of timed steps and must
    be at least one; --dump-outputs takes a directory."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "some/dir"])
    assert a.full is True and a.dump_outputs == "some/dir"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_sample_and_histograms(tmp_path, monkeypatch):
    """bench.dump_outputs on a CPU tensor: float files only, the whole batch when it fits the sample, otherwise one value from each
    stratum at seeded positions (the same on every call), and every frame's byte histogram; 64 x 4K NV12 frames stay under 64 MB."""
    import numpy as np
    import torch
    import bench
    fb = 3840 * 2160 * 3 // 2
    assert 4 * bench.DUMP_SAMPLE + 8 * 256 * 64 < 64e6 and bench.DUMP_SAMPLE < 64 * fb
    g = torch.Generator().manual_seed(1)
    out = torch.randint(0, 256, (3, 6000), dtype=torch.uint8, generator=g)
    flat = out.reshape(-1).numpy()
    p1 = bench.dump_outputs(out, tmp_path / "a")
    sample, hist = (np.load(p) for p in p1)
    assert sample.dtype == np.float32 and hist.dtype == np.float64
    assert np.array_equal(sample, flat.astype(np.float32))
    assert hist.shape == (3, 256) and np.array_equal(hist, np.stack([np.bincount(r, minlength=256) for r in out.numpy()]))
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    pa = bench.dump_outputs(out, tmp_path / "b")
    pb = bench.dump_outputs(out, tmp_path / "c")
    sa, sb = np.load(pa[0]), np.load(pb[0])
    assert sa.shape == (1000,) and np.array_equal(sa, sb)
    stride = flat.size // 1000
    for k in (0, 499, 999):                                   # value k comes from stratum k
        assert sa[k] in flat[k * stride:(k + 1) * stride].astype(np.float32)


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """`python bench.py --steps K --warmup W` without --full: the headline line with exactly K timed steps and nothing from the other
    legs; --dump-outputs writes the last step's output as float .npy files under 64 MB, the same in two runs with the same arguments."""
    import json
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and r.stdout.strip() == lines[0].strip(), r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["metric"] == "frames/sec, 3840x2160 NV12 Y equalizeHist" and line["unit"] == "frames/s" and line["dtype"] == "u8"
        assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 1
        assert abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 0.01
        assert line["parity_spot_check"] is None and line["nv12_1080p"] is None and line["fused_fallbacks_in_run"] == 0
        for key in ("cpu_baseline", "extras", "opencv_cross_check", "stream_4k60_512_all_gpus"):
            assert key not in line, key
        for phase in ("second_resolution", "extras", "cpu_baseline"):
            assert f"phase={phase}" not in r.stderr, phase
        files = sorted(d.iterdir())
        assert [f.name for f in files] == ["frames_out_hist.npy", "frames_out_sample.npy"]
        assert sum(f.stat().st_size for f in files) <= 64e6
        arrs = {f.name: np.load(f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        hist = arrs["frames_out_hist.npy"]
        assert hist.shape == (8, 256) and (hist.sum(axis=1) == 3840 * 2160 * 3 // 2).all()
        assert (hist[:, 128] >= 3840 * 2160 // 2).all()                   # UV = 128 (the default --uv fill128)
        dumps.append(arrs)
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name


@pytest.mark.gpu
def test_bench_nccl_world1_contract_on_gpu():
    """The RCCL branch on ONE GPU: `--force-dist` brings up a one-rank process group on the real backend, so init_process_group("nccl",
    device_id=...), the world_seen all-reduce, every shard.reduce_over_ranks / max_over_ranks on a CUDA tensor, barrier() on RCCL, the
    all-ranks stream leg beside a live communicator and destroy_process_group() execute exactly as on the driver's 8-GPU node
    (the reference's 1..8 workers, OpenCVequalHist.cpp:274, :397-402).  The headline must not move because of it."""
    import json
    env = {k: v for k, v in __import__("os").environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    common = ["--steps", "20", "--warmup", "5", "--cpu-seconds", "1.5"]
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--force-dist", "--full"] + common, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert r.stdout.strip() == lines[0].strip(), r.stdout[:600]      # nothing but the line: RCCL's version banner (fd 1) must land on stderr
    assert d["dist_backend_used"] == "nccl" and d["world_seen_by_backend"] == 1 and d["n_gpus"] == 1
    assert d["parity_spot_check"] is True and d["fused_fallbacks_in_run"] == 0 and d["roofline"]["ranks"] == 1
    sa = d["stream_4k60_512_all_gpus"]                               # the leg that only runs beside a process group
    assert sa["ranks_ok"] == 1 and sa["errors_total"] == 0 and sa["parity_rank0"] is True and sa["unpaced_frames_per_s_total"] > 0, sa
    assert "extras" not in d                                         # behaves like a rank of an N > 1 job
    for phase in ("dist_init(nccl)", "timed", "stream_all_ranks", "reduce", "done"):
        assert f"[bench hb] rank=0 phase={phase}" in r.stderr, phase
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--no-extras"] + common, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    plain = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert plain["dist_backend_used"] is None
    assert abs(d["value"] - plain["value"]) / plain["value"] < 0.03, (d["value"], plain["value"])


@pytest.mark.gpu
def test_bench_line_contract_on_gpu():
    """`python bench.py` prints ONE JSON line with the fields the driver reads, the roofline and cpu_baseline objects, and the
    truthfulness fields of round 2 (traffic source, moved-bytes fraction, backend, fallbacks)."""
    import json
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "5", "--warmup", "2", "--full", "--no-extras", "--cpu-seconds", "1.5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert r.stdout.strip() == lines[0].strip(), r.stdout[:600]      # stdout is the line and nothing else
    assert d["metric"] == "frames/sec, 3840x2160 NV12 Y equalizeHist" and d["unit"] == "frames/s"
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "u8" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 60 and abs(d["value"] - 64 * 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 0.01
    assert d["parity_spot_check"] is True and d["fused_fallbacks_in_run"] == 0
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and rf["kernel"] == "equalize_fused_kernel"
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.3 < rf["frac"] < 1.0
    assert rf["traffic"] and "profiles/" in rf["traffic_source"] and 0.2 < rf["frac_moved_bytes"] < rf["frac"]
    assert abs(rf["achieved"] - rf["alg_bytes_per_launch"] / (rf["avg_launch_ms"] * 1e-3) / 1e9) / rf["achieved"] < 1e-3
    # one clock: the committed rocprofv3 figure of the same kernel and workload, and this run's launches on that clock
    assert 0.1 < rf["avg_launch_ms_rocprof"] < 1.0 and "profiles/" in rf["clock_source"]
    assert abs(rf["frac_rocprof"] - rf["alg_bytes_per_launch"] / (rf["avg_launch_ms_rocprof"] * 1e-3) / 1e9 / rf["peak"]) < 1e-3
    assert 0.9 < rf["rocprof_over_hip_events_same_launches"] < 1.1
    assert abs(rf["frac_this_run_on_rocprof_clock"] - rf["frac"] / rf["rocprof_over_hip_events_same_launches"]) < 2e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "frames/s" and cb["cores"] >= 1 and cb["value"] > 0 and "3840x2160" in cb["sample"]
    assert d["nv12_1080p"]["value"] > d["value"]                       # four times fewer pixels per frame
    assert d["dist_backend_used"] is None and d["world_seen_by_backend"] == 1
    assert rf["ranks"] == 1 and rf["avg_launch_ms_fastest_rank"] == rf["avg_launch_ms_slowest_rank"] == rf["avg_launch_ms"]
    assert "one replica batch per GPU" in d["config"]["sharding"] and d["config"]["numa"]["ranks"] == 1
