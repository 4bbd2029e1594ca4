"""Cache policy of the fused equalizeHist kernel (option "fused_cache_policy": 0 = chosen from the bytes a launch loads and
stores, 1 = plain, 2 = streaming): whichever instantiation runs, the bytes are the oracle's -- out of place and in place, UV fill
and UV copy, on both sides of the size threshold, through the repair path and from a replayed graph.  Statistic
"fused_last_policy" reads back which instantiation the last launch used."""
import numpy as np
import pytest

import mi_lumaeq
import oracle
from mi_lumaeq import synth, xfer

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MI_ERR_BAD_ARG = 1
POLICIES = [0, 1, 2]                                    # automatic, and every forced policy the library ships
# 4K with enough frames for the fused path (more than two_kernel_max_frames = 8); 1080p (more than 16 frames), whose Y plane is
# 25.3 slices of 80 KiB: the last slice is short
SHAPES = [(3840, 2160, 10), (1920, 1080, 17)]

dev = xfer.to_device
host = xfer.to_host
_cache = {}


def batch(w, h, n, seed=4100):
    key = (w, h, n, seed)
    if key not in _cache:
        frames = np.stack([synth.nv12_frame(w, h, synth.DISTS[k % 5], seed + k) for k in range(n)])
        _cache[key] = (frames, {uv: [oracle.nv12_frame(frames[k], w, h, uv_mode=uv, op=0) for k in range(n)] for uv in (0, 1)})
    return _cache[key]


def policy_codes(c):
    """(plain, streaming): what "fused_last_policy" reads after a launch under the forced policies 1 and 2"""
    w, h, n = 640, 368, 3
    d_in = synth.nv12_batch_torch(w, h, n, "D2", "cuda:0", seed=3)
    d_out = torch.zeros_like(d_in)
    codes = []
    c.set_option("two_kernel_max_frames", 0)
    for forced in (1, 2):
        c.set_option("fused_cache_policy", forced)
        c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, 0)
        c.synchronize()
        codes.append(c.get_stat("fused_last_policy"))
    c.set_option("two_kernel_max_frames", 8)
    c.set_option("fused_cache_policy", 0)
    return tuple(codes)


@pytest.mark.parametrize("uv", [0, 1], ids=["uv_fill", "uv_copy"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("policy", POLICIES, ids=["auto", "plain", "streaming"])
@pytest.mark.parametrize("shape", SHAPES, ids=["4k_x10", "1080p_x17"])
def test_bytes_equal_oracle_under_every_policy(shape, policy, in_place, uv):
    w, h, n = shape
    frames, want = batch(w, h, n)
    c = mi_lumaeq.Context(0)
    try:
        plain, stream = policy_codes(c)
        assert plain == 0 and stream != plain
        c.set_option("fused_cache_policy", policy)
        c.set_profiling(1)
        d_in = dev(frames)
        d_out = d_in if in_place else torch.zeros_like(d_in)
        c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, uv)
        c.synchronize()
        prof = c.profile_read()
        assert prof["equalize_fused_kernel"]["launches"] == 1 and prof["fused_finish_kernel"]["launches"] == 1   # the path under test ran
        out = host(d_out)
        for k in range(n):
            assert np.array_equal(out[k], want[uv][k]), (shape, policy, in_place, uv, k)
        got = c.get_stat("fused_last_policy")
        if policy:
            assert got == (plain if policy == 1 else stream)
        else:
            assert got in (plain, stream)
        assert c.get_stat("fused_fallbacks") == 0 and c.get_stat("fused_hard_errors") == 0
    finally:
        c.close()


@pytest.mark.parametrize("uv", [0, 1], ids=["uv_fill", "uv_copy"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_automatic_choice_on_both_sides_of_the_threshold(in_place, uv):
    """The automatic choice goes by the bytes the launch loads and stores (Y in + Y out + UV out, + UV in when copied): one frame
    count below "fused_stream_min_bytes" runs the plain instantiation, the next one above it the streaming one, both the oracle's bytes."""
    w, h = 3840, 2160
    c = mi_lumaeq.Context(0)
    try:
        plain, stream = policy_codes(c)
        thr = c.get_stat("fused_stream_min_bytes")
        ysz = w * h
        moved = ysz // 2 if not uv else (0 if in_place else ysz)       # an in-place copy moves no UV byte
        per_frame = 2 * ysz + moved
        n_above = -(-thr // per_frame)                                    # first frame count whose launch reaches the threshold
        n_below = n_above - 1
        assert 9 <= n_below and n_above <= 96, (thr, per_frame)           # both launches take the fused path and fit the device
        frames, want = batch(w, h, n_above, seed=5200)
        for n, expect in ((n_below, plain), (n_above, stream)):
            d_in = dev(frames[:n])
            d_out = d_in if in_place else torch.zeros_like(d_in)
            c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, uv)
            c.synchronize()
            assert c.get_stat("fused_last_policy") == expect, (n, thr, per_frame)
            out = host(d_out)
            for k in range(n):
                assert np.array_equal(out[k], want[uv][k]), (n, in_place, uv, k)
            del d_in, d_out
    finally:
        c.close()


def hooks_ctx(policy):
    c = mi_lumaeq.Context(0, lib=mi_lumaeq.test_lib())
    c.set_option("two_kernel_max_frames", 0)
    c.set_option("fused_cache_policy", policy)
    return c


@pytest.mark.parametrize("mode", [1, 2, 3], ids=["lost_producer", "partial_frame", "bad_checksum"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("uv", [0, 1], ids=["uv_fill", "uv_copy"])
def test_injected_failures_are_repaired_under_the_streaming_policy(mode, in_place, uv):
    """The three injected hand-off failures with the streaming instantiation forced: the finish kernel (default policy, after a kernel
    boundary) sees the stamps and the slices the fused kernel did write, whatever policy wrote them, and produces the oracle's bytes."""
    w, h, n = 1920, 1080, 3
    frames, want = batch(w, h, n, seed=700)
    c = hooks_ctx(2)
    try:
        d_in = dev(frames)
        d_out = d_in if in_place else torch.zeros_like(d_in)
        c.set_option("fused_fault_inject", mode)
        c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, uv, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = host(d_out)
        for k in range(n):
            assert np.array_equal(out[k], want[uv][k]), (mode, in_place, uv, k)
        c.synchronize()
        assert c.get_stat("fused_fallbacks") == 1 and c.get_stat("fused_frames_repaired") >= 1 and c.get_stat("fused_hard_errors") == 0
        assert c.get_stat("fused_last_policy") != 0
        c.set_option("fused_fault_inject", 0)                            # the next launch is a normal one
        d_in2 = dev(frames); d_out2 = torch.zeros_like(d_in2)
        c.equalize_hist_nv12_batch_dev(d_in2, d_out2, w, h, n, 1 - uv)
        c.synchronize()
        out = host(d_out2)
        for k in range(n):
            assert np.array_equal(out[k], want[1 - uv][k]), k
        assert c.get_stat("fused_fallbacks") == 1
    finally:
        c.close()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_microsecond_wait_bound_under_the_streaming_policy(in_place):
    """Waits bounded to a few microseconds expire wherever the timing of a launch puts them; the repair must still end in the oracle's
    bytes with the streaming instantiation forced, in place included."""
    w, h, n = 1920, 1080, 6
    frames, want = batch(w, h, n, seed=1500)
    c = hooks_ctx(2)
    try:
        c.set_option("fused_demote_after", 0)
        for us in (1, 4, 16, 40):
            c.set_option("fused_timeout_us", us)
            for rep in range(4):
                uv = rep & 1
                d_in = dev(frames)
                d_out = d_in if in_place else torch.zeros_like(d_in)
                c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, uv)
                c.synchronize()
                out = host(d_out)
                for k in range(n):
                    assert np.array_equal(out[k], want[uv][k]), (us, rep, k)
            assert c.get_stat("fused_hard_errors") == 0
        assert c.get_stat("fused_fallbacks") > 0                         # the repair path was exercised
        assert c.get_stat("fused_last_policy") != 0
    finally:
        c.close()


@pytest.mark.parametrize("policy", POLICIES, ids=["auto", "plain", "streaming"])
def test_captured_and_replayed_launch(policy):
    w, h, n = 1920, 1080, 6
    c = mi_lumaeq.Context(0)
    try:
        c.set_option("two_kernel_max_frames", 0)
        c.set_option("fused_cache_policy", policy)
        d_in = synth.nv12_batch_torch(w, h, n, "D2", "cuda:0", seed=11)
        d_out = torch.zeros_like(d_in)
        c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, 1)            # sizes the scratch: allocations cannot be captured
        c.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, n, 1, stream=torch.cuda.current_stream().cuda_stream)
        for rep in range(2):
            d_in.copy_(synth.nv12_batch_torch(w, h, n, synth.DISTS[rep], "cuda:0", seed=100 + rep))
            d_out.zero_()
            g.replay()
            torch.cuda.synchronize()
            src, out = host(d_in), host(d_out)
            for k in range(n):
                assert np.array_equal(out[k], oracle.nv12_frame(src[k], w, h, uv_mode=1, op=0)), (policy, rep, k)
    finally:
        c.close()


def test_unknown_policy_is_refused():
    c = mi_lumaeq.Context(0)
    try:
        for bad in (-1, 3, 99, 100, 143, 1 << 20):
            with pytest.raises(mi_lumaeq.MiError) as e:
                c.set_option("fused_cache_policy", bad)
            assert e.value.status == MI_ERR_BAD_ARG, bad
        for good in (0, 1, 2, 0):
            c.set_option("fused_cache_policy", good)
    finally:
        c.close()
