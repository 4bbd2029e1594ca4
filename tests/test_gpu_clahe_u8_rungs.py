"""8-bit CLAHE on every branch of its launch plan, at small shapes (run with -m gpu on an MI355X).

launch_tile_luts and launch_interp (csrc/host/clahe.inc.hpp) choose among a dozen kernels and kernel modes by tile size, batch size and
CU count.  tests/clahe_u8_rungs.py holds one small shape per branch (the rung table, its content, the plan restated in Python) and
tests/test_clahe_u8_rungs.py shows on the CPU that every rung reaches its branch on 256 CUs and that its content lets the oracle see the
interpolation weights and the arithmetic mode.  Here every rung runs through three device forms:

    planar batch   clahe_batch_dev on strided_layouts Sides (pitched, guarded; pairings U-A16 and A16-U, in place on two rungs)
    NV12 batch     clahe_nv12_batch_dev on tight frames in a sentinel-filled allocation, 64 guard bytes at both ends, both UV modes
    NV12 list      clahe_nv12_frames, every plane in an allocation of its own at its own offset and a padded pitch, both UV modes,
                   Y in place on two rungs

and every call is checked three ways, all exact: the whole of every output allocation is sentinel plus the expected planes (Y is
oracle.clahe in the call's arithmetic mode, UV the fill or the copy), the whole of every input allocation is unchanged, and the
profiler counted one tile_hist_kernel launch, tile_lut_kernel iff the restated S > 1, one clahe_interp_kernel launch, a separate UV
launch (slot lut_apply_kernel) iff the rung is `global` and the form has chroma, and nothing else.

K, the tiles a tile_hist_multi*_kernel workgroup walks, is never compared against the library: it cannot be observed.  Before a multi*
rung calls, K is computed with hist_plan from the device's CU count and must be the table's value for 256 CUs; on any other part the
rung FAILS and names the CU count (a skipped rung is an untested kernel).  A 64-frame list is exactly one kFramesPerLaunch chunk, so the
list form of those rungs is one tile_hist_multi_frames_kernel launch.

Left out: the second round of the four-load loop inside tile_hist_multi_kernel needs tiles of 2048 and more 16-byte slots and enough
of them to fill the chip with K > 1 -- a batch of hundreds of MB.  tile_hist_kernel's second and third rounds are the `loads` rung."""
import functools

import numpy as np
import pytest
import torch

import mi_lumaeq
import oracle
import strided_layouts as L
import clahe_u8_rungs as R
from clahe_u8_rungs import RUNGS
from mi_lumaeq import UV_COPY, UV_FILL128
from mi_lumaeq.capi import KERNEL_NAMES

pytestmark = pytest.mark.gpu
SENT = L.SENTINEL
GUARD = 64
OFFS = (4, 9, 12, 1, 16)                                           # where a list's plane starts in its allocation


@pytest.fixture(scope="module")
def c():
    with mi_lumaeq.Context(0) as ctx:
        ctx.set_profiling(1)
        ctx.profile_read(reset=True)
        yield ctx
        ctx.set_profiling(0)


@pytest.fixture(scope="module")
def cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module", autouse=True)
def release_device_cache():
    """The module's many small batches leave nothing cached in torch's allocator for the modules that run after it."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- content and expected planes, computed once --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def y_in(name, h, k):
    r = RUNGS[name]
    f = R.frame(r.w, h, k, r.n)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def y_ref(name, h, k, clip, contract):
    r = RUNGS[name]
    old = oracle.set_fp_contract(bool(contract))
    try:
        out = oracle.clahe(y_in(name, h, k), clip, r.tx, r.ty)
    finally:
        oracle.set_fp_contract(old)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def uv_in(name, h, k):
    r = RUNGS[name]
    uv = np.random.default_rng(7000 + k).integers(0, 256, (h // 2, r.w), dtype=np.uint8)
    uv.setflags(write=False)
    return uv


def uv_ref(uv, uv_mode):
    return np.full_like(uv, 128) if uv_mode == UV_FILL128 else uv


# ---- options and launch counts -------------------------------------------------------------------------------------------------
class options:
    """Context options set for one call, all of the plan's options back at their defaults afterwards."""

    def __init__(self, c, opts):
        self.c, self.opts = c, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.c.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in R.DEFAULTS.items():
            self.c.set_option(k, v)


def want_launches(r, h, opts, cu, chroma):
    hist, interp = R.plans(r, h, cu, opts)
    want = dict.fromkeys(KERNEL_NAMES, 0)
    want.update(tile_hist_kernel=1, tile_lut_kernel=int(hist.S > 1), clahe_interp_kernel=1,
                lut_apply_kernel=int(interp.kind == "global" and chroma))
    return want


def check_plan(r, h, opts, cu):
    """What can be said before the call: K of a multi* rung is the 256-CU table's, or the rung fails naming the part."""
    if r.multi:
        k = R.plans(r, h, cu, opts)[0].K
        want = R.K256[r.name]                                       # multi2 keeps K = 2 without the XCD map, too
        assert k == want, f"rung {r.name} needs K = {want} tiles per workgroup (a 256-CU part); this device has {cu} CUs and gives K = {k}"


def run_call(c, cu, r, h, opts, chroma, call, why):
    """One library call between two profile reads; returns after the synchronize, the launch counts checked."""
    check_plan(r, h, opts, cu)
    with options(c, opts):
        c.profile_read(reset=True)
        call()
        torch.cuda.synchronize()
        prof = c.profile_read(reset=True)
    got = {k: v["launches"] for k, v in prof.items()}
    assert got == want_launches(r, h, opts, cu, chroma), (why, got)


# ---- sentinel-filled allocations (the Layout of the 4:2:2 ladder, for any number of frames) ---------------------------------------
class Planes:
    """Device allocations filled with a sentinel and the planes placed in them, each as (allocation, byte offset, pitch)."""

    def __init__(self):
        self.bufs = []

    def plane(self, rows, row_bytes, pitch, off):
        b = torch.full((off + (rows - 1) * pitch + row_bytes + GUARD,), SENT, dtype=torch.uint8, device="cuda:0")
        assert b.data_ptr() % 16 == 0
        self.bufs.append(b)
        return (len(self.bufs) - 1, off, pitch)

    def ptr(self, at):
        return self.bufs[at[0]].data_ptr() + at[1]

    def image(self, painted):
        imgs = [np.full(b.numel(), SENT, np.uint8) for b in self.bufs]
        for (bi, off, pitch), px in painted:
            rows, wb = px.shape
            np.lib.stride_tricks.as_strided(imgs[bi][off:], (rows, wb), (pitch, 1))[:] = px
        return np.concatenate(imgs)

    def upload(self, painted):
        img = torch.from_numpy(self.image(painted)).to("cuda:0")
        o = 0
        for b in self.bufs:
            b.copy_(img[o: o + b.numel()])
            o += b.numel()

    def host(self):
        return torch.cat(self.bufs).cpu().numpy()

    def assert_reads(self, painted, why):
        got, want = self.host(), self.image(painted)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (why, "bytes that differ:", int(bad.size), "first at", bad[:6].tolist(),
                               "got", got[bad[:6]].tolist(), "want", want[bad[:6]].tolist())


# ---- the three forms -----------------------------------------------------------------------------------------------------------
def planar_form(c, cu, r):
    h, n = r.h, r.n
    pairings = ["U-A16", "A16-U"] + (["inplace-U"] if r.inplace else [])
    frames = [y_in(r.name, h, k) for k in range(n)]
    for opts, clip in r.variants():
        contract = opts.get("clahe_fp_contract", 0)
        want = [y_ref(r.name, h, k, clip, contract) for k in range(n)]
        for pairing in pairings:
            why = (r.name, "planar", pairing, opts, clip)
            src, dst = L.make_pair(pairing, h, r.w, n)
            src.upload(frames)
            if dst is not src:
                dst.upload(None)
            assert src.buf.data_ptr() % 16 == 0 and dst.buf.data_ptr() % 16 == 0
            run_call(c, cu, r, h, opts, False,
                     lambda: c.clahe_batch_dev(src.ptr, dst.ptr, r.w, h, n, clip, r.tx, r.ty, src_step=src.pitch, src_frame=src.frame_stride,
                                               dst_step=dst.pitch, dst_frame=dst.frame_stride, stream=stream()), why)
            if dst is src:
                L.assert_sides(src, src.image(want), why)
            else:
                L.assert_sides([src, dst], [src.image(frames), dst.image(want)], why)


def nv12_batch_form(c, cu, r):
    h, n, w = r.h_nv12, r.n, r.w
    fb = w * h * 3 // 2
    lay = Planes()
    src, dst = lay.plane(n, fb, fb, GUARD), lay.plane(n, fb, fb, GUARD)     # a batch is n "rows" of one tight frame each
    if r.name == "float":
        assert (GUARD + fb) % 16 == 4                                       # the second frame starts 4 bytes past a 16-byte boundary
    ins = np.stack([np.concatenate([y_in(r.name, h, k).reshape(-1), uv_in(r.name, h, k).reshape(-1)]) for k in range(n)])
    for opts, clip in r.variants():
        contract = opts.get("clahe_fp_contract", 0)
        for uv_mode in (UV_FILL128, UV_COPY):
            why = (r.name, "nv12 batch", uv_mode, opts, clip)
            want = np.stack([np.concatenate([y_ref(r.name, h, k, clip, contract).reshape(-1), uv_ref(uv_in(r.name, h, k), uv_mode).reshape(-1)])
                             for k in range(n)])
            lay.upload([(src, ins)])                                        # also resets the output to the sentinel
            run_call(c, cu, r, h, opts, True,
                     lambda: c.clahe_nv12_batch_dev(lay.ptr(src), lay.ptr(dst), w, h, n, uv_mode, clip, r.tx, r.ty, stream=stream()), why)
            lay.assert_reads([(src, ins), (dst, want)], why)


def nv12_list_form(c, cu, r):
    h, n, w = r.h_nv12, r.n, r.w
    for y_in_place in ([False, True] if r.inplace else [False]):
        lay = Planes()
        yi_pitch, ui_pitch, uo_pitch = w + 5, w + 9, w + 3
        yo_pitch = yi_pitch if y_in_place else w + 20
        yi = [lay.plane(h, w, yi_pitch, OFFS[k % 5]) for k in range(n)]
        ui = [lay.plane(h // 2, w, ui_pitch, OFFS[(k + 1) % 5]) for k in range(n)]
        yo = yi if y_in_place else [lay.plane(h, w, yo_pitch, OFFS[(k + 2) % 5]) for k in range(n)]
        uo = [lay.plane(h // 2, w, uo_pitch, OFFS[(k + 3) % 5]) for k in range(n)]
        ins = [(yi[k], y_in(r.name, h, k)) for k in range(n)] + [(ui[k], uv_in(r.name, h, k)) for k in range(n)]
        inputs = [(lay.ptr(yi[k]), lay.ptr(ui[k])) for k in range(n)]
        outputs = [(lay.ptr(yo[k]), lay.ptr(uo[k])) for k in range(n)]
        for opts, clip in r.variants():
            contract = opts.get("clahe_fp_contract", 0)
            for uv_mode in (UV_FILL128, UV_COPY):
                why = (r.name, "nv12 list", "Y in place" if y_in_place else "out of place", uv_mode, opts, clip)
                lay.upload(ins)
                run_call(c, cu, r, h, opts, True,
                         lambda: c.clahe_nv12_frames(inputs, outputs, w, h, uv_mode, clip, r.tx, r.ty, y_in_pitch=yi_pitch, uv_in_pitch=ui_pitch,
                                                     y_out_pitch=yo_pitch, uv_out_pitch=uo_pitch, stream=stream()), why)
                outs = [(yo[k], y_ref(r.name, h, k, clip, contract)) for k in range(n)]
                outs += [(uo[k], uv_ref(uv_in(r.name, h, k), uv_mode)) for k in range(n)]
                lay.assert_reads(ins + outs, why)                            # later entries paint over earlier ones: Y in place


FORMS = {"planar": planar_form, "nv12_batch": nv12_batch_form, "nv12_list": nv12_list_form}


def cases():
    out = []
    for r in RUNGS.values():
        for form in FORMS:
            if form != "planar" and r.h_nv12 is None:               # split-pad: an odd height, planar only
                continue
            if form == "nv12_batch" and r.multi:                    # the multi* rungs: planar batch and NV12 list
                continue
            out.append(pytest.param(r.name, form, id=f"{r.name}-{form}"))
    return out


@pytest.mark.parametrize("name,form", cases())
def test_rung(c, cu, name, form):
    FORMS[form](c, cu, RUNGS[name])

