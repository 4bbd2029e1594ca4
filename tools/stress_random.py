"""Bounded random differential run, HIP vs oracle, aimed at the code paths a fixed test list visits only at a few points: ROI pitches
(multiples of 16 and not) with random origins, wide CLAHE grids at sizes where the per-segment float tables apply, large batches of small
tiles (several tiles per histogram workgroup), 16-bit CLAHE at random value ranges, the 4:2:0 codes at random aligned / unaligned sizes, NV12 in / BGR out
at random pitched layouts (aligned and not) and tile grids on both sides of its one-pass conditions, as a batch and as a frame list
(random order, every image at its own offset), and the same pixels from planar chroma (I420 / YV12 in, BGR out) at chroma layouts that are
multiples of 8 or of 1, as a batch and as a frame list against the batch form's bytes, and the way back on a frame list (those images in,
I420 / YV12 planes out at that layout, every frame at an offset of its own) against the oracle, and packed 4:2:2 in (YUY2 / UYVY), BGR
out on a frame list (every buffer and every image an allocation of its own, images at any byte offset) against the oracle and the batch form,
and BGR / RGB in, packed 4:2:2 out (every row with the chroma of its own left pixels) at random pitched layouts, aligned and not, odd heights
included, against the oracle on the row-doubled image (tests/bgr_packed422_ref.py), as a batch and as a frame list (every image and every
frame an allocation of its own at an offset of its own: 16-pixel groups and macropixels in one launch), and 4:2:0 in (NV12 / I420 / YV12),
packed 4:2:2 out (mi_*_yuv420_to_packed422_batch_dev: every chroma row under two output rows) at random pitched layouts on both sides
of its vector and one-pass conditions, against the oracle's luma and the input's own chroma, and the same on a frame list
(mi_*_yuv420_to_packed422_frames_dev: every plane and every packed frame an allocation of its own at a skew of its own, both layouts, both
formats, both UV modes, 16 x 2 groups and 2 x 2 blocks in one launch, the four list counters asserted).
    python tools/stress_random.py [seconds] [seed] [option=value ...]        prints a line every ~15 s, exits non-zero on the first mismatch"""
import sys, time
sys.path.insert(0, "opencv-opencl_amd/python"); sys.path.insert(0, ".")
import numpy as np, torch
import mi_lumaeq, oracle
from mi_lumaeq import xfer
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
ctx = mi_lumaeq.Context(0)
for kv in sys.argv[3:]:                                          # name=value options for the whole run, e.g. clahe16_wide=2 (mid kernel always launched)
    k_, v_ = kv.split("="); ctx.set_option(k_, int(v_)); print("option", k_, "=", v_, flush=True)
t0 = last = time.time(); n = {"roi": 0, "grid": 0, "small": 0, "c16": 0, "420": 0, "nv12": 0, "nv12bgr": 0, "yuv420bgr": 0, "yuv420bgrlist": 0, "bgryuv420list": 0, "p422bgrlist": 0, "bgrp422": 0, "bgrp422list": 0, "yuv420p422": 0, "yuv420p422list": 0}
def dev(a): return xfer.to_device(np.ascontiguousarray(a))
def fail(what, *info):
    print("MISMATCH", what, info, flush=True); sys.exit(1)
while time.time() - t0 < budget:
    k = int(rng.integers(0, 12))
    if k == 0:      # ROI batch on the device: random pitches, origins, sizes
        w, h, nf = int(rng.integers(1, 700)), int(rng.integers(1, 90)), int(rng.integers(1, 6))
        sp = w + int(rng.integers(0, 40)); sp += (16 - sp % 16) % 16 if rng.integers(0, 2) else 0
        dp = w + int(rng.integers(0, 40)); dp += (16 - dp % 16) % 16 if rng.integers(0, 2) else 0
        src = rng.integers(0, int(rng.integers(2, 257)), (nf, h + 4, sp), dtype=np.uint8)
        sx, dx = int(rng.integers(0, sp - w + 1)), int(rng.integers(0, dp - w + 1))
        d_src, d_dst = dev(src), torch.zeros((nf, h + 4, dp), dtype=torch.uint8, device="cuda")
        ctx.equalize_hist_batch_dev(d_src.data_ptr() + 2 * sp + sx, d_dst.data_ptr() + dp + dx, w, h, nf, src_step=sp, src_frame=(h + 4) * sp,
                                    dst_step=dp, dst_frame=(h + 4) * dp)
        ctx.synchronize(); out = xfer.to_host(d_dst)
        for f in range(nf):
            if not np.array_equal(out[f, 1:1 + h, dx:dx + w], oracle.equalize_hist(src[f, 2:2 + h, sx:sx + w])): fail("roi", w, h, nf, sp, dp, sx, dx, f)
        if out[:, 0].sum() or out[:, 1 + h:].sum(): fail("roi wrote outside", w, h, sp, dp)
        n["roi"] += 1
    elif k == 1:    # wide grids
        w, h = int(rng.integers(200, 2400)), int(rng.integers(20, 200))
        tx, ty = int(rng.integers(15, 64)), int(rng.integers(1, 9)); clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if not np.array_equal(ctx.clahe(y, clip, tx, ty), oracle.clahe(y, clip, tx, ty)): fail("grid", w, h, tx, ty, clip)
        n["grid"] += 1
    elif k == 2:    # many small tiles in a large batch
        tw, th = int(rng.integers(2, 12)) * 8, int(rng.integers(4, 40)); tx, ty = int(rng.choice([4, 8, 8, 16])), int(rng.integers(2, 9))
        w, h = tw * tx - int(rng.integers(0, 2)) * int(rng.integers(0, tx)), th * ty
        nf = int(rng.integers(2100, 2600)) // max(1, tx * ty // 2) + 1
        ys = rng.integers(0, 256, (min(nf, 9), h, w), dtype=np.uint8)
        batch = np.ascontiguousarray(ys[np.arange(nf) % ys.shape[0]])
        d_in = dev(batch); d_out = torch.zeros_like(d_in)
        ctx.clahe_batch_dev(d_in, d_out, w, h, nf, 2.0, tx, ty); ctx.synchronize(); out = xfer.to_host(d_out)
        want = [oracle.clahe(ys[i], 2.0, tx, ty) for i in range(ys.shape[0])]
        for f in range(nf):
            if not np.array_equal(out[f], want[f % ys.shape[0]]): fail("small tiles", w, h, tx, ty, nf, f)
        n["small"] += 1
    elif k == 3:    # 16-bit CLAHE, random ranges
        w, h = int(rng.integers(4, 80)) * 8, int(rng.integers(4, 60)) * 4
        lo = int(rng.integers(0, 65000)); hi = min(65536, lo + int(rng.choice([1, 50, 1000, 4096, 4097, 8192, 8193, 20000, 65536])))
        y = rng.integers(lo, hi, (h, w), dtype=np.uint16)
        if rng.integers(0, 3) == 0: y[: h // 2] = lo
        sh = 0
        if rng.integers(0, 2) == 0:                                   # samples in the high bits of the word (P010 / P016): every value a multiple of 1 << sh
            sh = int(rng.integers(1, 9)); bits = int(rng.integers(1, 17 - sh))
            y = (rng.integers(0, 1 << bits, (h, w), dtype=np.uint32) << sh).astype(np.uint16)
            r = int(rng.integers(0, 4))
            if r == 0: y[: h // 3] = 0                                  # a black bar: tiles with a larger shift than the frame's
            elif r == 1: y[int(rng.integers(0, h)), int(rng.integers(0, w))] |= 1 << int(rng.integers(0, sh))   # one value voids (or lowers) the shift
        want16 = oracle.clahe16(y, 2.0, 4, 4)
        if not np.array_equal(ctx.clahe16(y, 2.0, 4, 4), want16): fail("c16", w, h, lo, hi, sh)
        if rng.integers(0, 3) == 0:                                   # the same frame three times in a device batch, out of place and in place
            d16 = dev(np.stack([y, y, y]).view(np.int16)); o16 = torch.zeros_like(d16)
            ctx.clahe16_batch_dev(d16, o16, w, h, 3, 2.0, 4, 4); ctx.synchronize()
            if not all(np.array_equal(xfer.to_host(o16)[f].view(np.uint16), want16) for f in range(3)): fail("c16 batch", w, h, lo, hi, sh)
            ctx.clahe16_batch_dev(d16, d16, w, h, 3, 2.0, 4, 4); ctx.synchronize()
            if not all(np.array_equal(xfer.to_host(d16)[f].view(np.uint16), want16) for f in range(3)): fail("c16 in place", w, h, lo, hi, sh)
        n["c16"] += 1
    elif k == 5:    # NV12 batches of random even sizes through the fused kernel (or the three-kernel path where it does not apply), both ops
        w, h, nf = int(rng.integers(1, 400)) * 2, int(rng.integers(1, 200)) * 2, int(rng.integers(1, 9))
        uv = int(rng.integers(0, 2)); op = int(rng.integers(0, 2))
        fr = rng.integers(0, int(rng.integers(2, 257)), (nf, w * h * 3 // 2), dtype=np.uint8)
        d_in = dev(fr); inplace = bool(rng.integers(0, 2)); d_out = d_in if inplace else torch.zeros_like(d_in)
        if op == 0: ctx.equalize_hist_nv12_batch_dev(d_in, d_out, w, h, nf, uv)
        else: ctx.clahe_nv12_batch_dev(d_in, d_out, w, h, nf, uv, 2.0, 4, 4)
        ctx.synchronize(); out = xfer.to_host(d_out)
        for f in range(nf):
            if not np.array_equal(out[f], oracle.nv12_frame(fr[f], w, h, uv_mode=uv, op=op, clip_limit=2.0, tiles_x=4, tiles_y=4)): fail("nv12", w, h, nf, uv, op, inplace, f)
        n["nv12"] += 1
    elif k == 6:    # NV12 in, BGR / RGB out: pitched layouts, aligned (16-byte accesses, CLAHE in one pass where the grid allows) or not, both ops
        w, h, nf = int(rng.integers(1, 40)) * (16 if rng.integers(0, 2) else 2), int(rng.integers(1, 60)) * 2, int(rng.integers(1, 5))
        op, order = int(rng.integers(0, 2)), int(rng.integers(0, 2)); tx, ty = int(rng.integers(1, 17)), int(rng.integers(1, 6))
        clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        if op == 1 and w % 16 == 0 and rng.integers(0, 4): w, h = 16 * tx * int(rng.integers(1, 4)), 2 * ty * int(rng.integers(1, 12))
        al = 16 if rng.integers(0, 4) else 1                           # every pitch, gap and offset a multiple of `al`
        def pad(v): return (v + al - 1) // al * al + al * int(rng.integers(0, 40 // al + 1))
        yp, up, opi = pad(w), pad(w), pad(3 * w); off, gap, fgap, ooff, ofgap = (pad(0) for _ in range(5))
        uv_off = yp * h + gap; fi = uv_off + up * (h // 2) + fgap; fo = opi * h + ofgap
        fr = rng.integers(0, 256, (nf, w * h * 3 // 2), dtype=np.uint8)
        img = np.full(off + fi * nf + 64, 0x5A, np.uint8)
        for f in range(nf):
            o = off + f * fi
            img[o: o + yp * h].reshape(h, yp)[:, :w] = fr[f, : w * h].reshape(h, w)
            img[o + uv_off: o + uv_off + up * (h // 2)].reshape(h // 2, up)[:, :w] = fr[f, w * h:].reshape(h // 2, w)
        d_in = dev(img); d_out = torch.full((ooff + fo * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        a = (d_in.data_ptr() + off, d_in.data_ptr() + off + uv_off, d_out.data_ptr() + ooff, w, h, nf, order)
        kw = dict(y_pitch=yp, uv_pitch=up, in_frame=fi, out_pitch=opi, out_frame=fo)
        if op == 0: ctx.equalize_hist_nv12_to_bgr_batch_dev(*a, **kw)
        else: ctx.clahe_nv12_to_bgr_batch_dev(*a, clip, tx, ty, **kw)
        ctx.synchronize(); out = xfer.to_host(d_out); want = np.full(out.size, 0x5A, np.uint8); imgs = []
        for f in range(nf):
            bgr = oracle.nv12_to_bgr(oracle.nv12_frame(fr[f], w, h, uv_mode=1, op=op, clip_limit=clip, tiles_x=tx, tiles_y=ty), w, h)
            imgs.append((bgr if order == 0 else bgr[:, :, ::-1]).reshape(h, 3 * w))
            want[ooff + f * fo: ooff + f * fo + opi * h].reshape(h, opi)[:, : 3 * w] = imgs[f]
        if not np.array_equal(out, want): fail("nv12bgr", w, h, nf, op, order, clip, tx, ty, al, yp, up, opi, off, gap, fgap, ooff, ofgap, np.flatnonzero(out != want)[:8])
        # the list form on the same planes: the frames in a random order, every image at an offset of its own (one in three a random
        # number of bytes past where the batch would put it: that frame alone takes the byte path; CLAHE then takes the fallback)
        perm = [int(v) for v in rng.permutation(nf)]; jit = [int(rng.integers(0, 16)) if rng.integers(0, 3) == 0 else 0 for _ in range(nf)]
        d_out2 = torch.full((ooff + (fo + 16) * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda"); want = np.full(d_out2.numel(), 0x5A, np.uint8)
        oo = [ooff + f * (fo + 16) + jit[f] for f in range(nf)]
        la = ([d_in.data_ptr() + off + f * fi for f in perm], [d_in.data_ptr() + off + uv_off + f * fi for f in perm],
              [d_out2.data_ptr() + oo[f] for f in perm], w, h, order)
        lkw = dict(y_pitch=yp, uv_pitch=up, out_pitch=opi)
        if op == 0: ctx.equalize_hist_nv12_to_bgr_frames(*la, **lkw)
        else: ctx.clahe_nv12_to_bgr_frames(*la, clip, tx, ty, **lkw)
        ctx.synchronize(); out = xfer.to_host(d_out2)
        for f in range(nf): want[oo[f]: oo[f] + opi * h].reshape(h, opi)[:, : 3 * w] = imgs[f]
        if not np.array_equal(out, want): fail("nv12bgr list", w, h, nf, op, order, clip, tx, ty, al, yp, up, opi, off, gap, fgap, ooff, perm, jit, np.flatnonzero(out != want)[:8])
        if not np.array_equal(xfer.to_host(d_in), img): fail("nv12bgr wrote its input", w, h, nf, op)
        n["nv12bgr"] += 1
        # the same pixels from planar chroma (I420, or YV12: the two planes at exchanged addresses) into the same output layout: chroma
        # pitches, gaps and offsets multiples of 8 where the NV12 layout had 16 (the 16 x 2 groups still apply), or of 1
        ca = 8 if al == 16 else 1
        def cpad(v): return (v + ca - 1) // ca * ca + ca * int(rng.integers(0, 40 // ca + 1))
        cp, g0, g1 = cpad(w // 2), cpad(0), cpad(0); csz = cp * (h // 2); yv12 = bool(rng.integers(0, 2))
        a_off = yp * h + g0; b_off = a_off + csz + g1; pfi = b_off + csz; pfi += (-pfi) % al + al * int(rng.integers(0, 3))
        pimg = np.full(off + pfi * nf + 64, 0x5A, np.uint8)
        u_off, v_off = (b_off, a_off) if yv12 else (a_off, b_off)
        for f in range(nf):
            o = off + f * pfi; uvr = fr[f, w * h:].reshape(h // 2, w)
            pimg[o: o + yp * h].reshape(h, yp)[:, :w] = fr[f, : w * h].reshape(h, w)
            pimg[o + u_off: o + u_off + csz].reshape(h // 2, cp)[:, : w // 2] = uvr[:, 0::2]
            pimg[o + v_off: o + v_off + csz].reshape(h // 2, cp)[:, : w // 2] = uvr[:, 1::2]
        d_pin = dev(pimg); d_out3 = torch.full((ooff + fo * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda"); b = d_pin.data_ptr() + off
        pl = mi_lumaeq.Yuv420Planes(b, yp, b + u_off, b + v_off, cp, pfi, mi_lumaeq.CHROMA_PLANAR)
        pa = (pl, d_out3.data_ptr() + ooff, w, h, nf, order); pkw = dict(out_pitch=opi, out_frame=fo)
        if op == 0: ctx.equalize_hist_yuv420_to_bgr_batch_dev(*pa, **pkw)
        else: ctx.clahe_yuv420_to_bgr_batch_dev(*pa, clip, tx, ty, **pkw)
        ctx.synchronize()
        if not torch.equal(d_out3, d_out): fail("yuv420bgr", w, h, nf, op, order, clip, tx, ty, al, yp, cp, g0, g1, pfi, yv12, opi, off, ooff)
        if not np.array_equal(xfer.to_host(d_pin), pimg): fail("yuv420bgr wrote its input", w, h, nf, op)
        n["yuv420bgr"] += 1
        # the planar list form on the same planes, against the batch form's bytes: the frames in another random order, every image at
        # an offset of its own (one in three some bytes past a 16-byte boundary: that frame alone takes the byte walk and CLAHE the
        # fallback), U and V exchanged between c0 and c1 by the layout alone
        perm = [int(v) for v in rng.permutation(nf)]; jit = [int(rng.integers(0, 16)) if rng.integers(0, 3) == 0 else 0 for _ in range(nf)]
        oo = [ooff + f * (fo + 16) + jit[f] for f in range(nf)]
        d_out4 = torch.full((ooff + (fo + 16) * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda"); want = np.full(d_out4.numel(), 0x5A, np.uint8)
        ents = [mi_lumaeq.Yuv420BgrFrameDev(b + f * pfi, b + u_off + f * pfi, b + v_off + f * pfi, d_out4.data_ptr() + oo[f]) for f in perm]
        fa = (ents, w, h, yp, cp, mi_lumaeq.CHROMA_PLANAR, order); fkw = dict(out_pitch=opi)
        if op == 0: ctx.equalize_hist_yuv420_to_bgr_frames_dev(*fa, **fkw)
        else: ctx.clahe_yuv420_to_bgr_frames_dev(*fa, clip, tx, ty, **fkw)
        ctx.synchronize(); out = xfer.to_host(d_out4); bat = xfer.to_host(d_out3)
        for f in range(nf): want[oo[f]: oo[f] + opi * h].reshape(h, opi)[:, : 3 * w] = bat[ooff + f * fo: ooff + f * fo + opi * h].reshape(h, opi)[:, : 3 * w]
        if not np.array_equal(out, want): fail("yuv420bgr list", w, h, nf, op, order, clip, tx, ty, al, yp, cp, g0, g1, pfi, yv12, opi, off, ooff, perm, jit, np.flatnonzero(out != want)[:8])
        if not np.array_equal(xfer.to_host(d_pin), pimg): fail("yuv420bgr list wrote its input", w, h, nf, op)
        n["yuv420bgrlist"] += 1
        # the way back on a list: those images, where the list call above left them, in; planar 4:2:0 frames out at the planar layout
        # above (U and V exchanged between c0 and c1 by the layout alone), the frames in another random order, one in three some bytes
        # past where its neighbours lie (that frame alone takes the byte walk), against the oracle
        perm = [int(v) for v in rng.permutation(nf)]; jy = [int(rng.integers(0, 16)) if rng.integers(0, 3) == 0 else 0 for _ in range(nf)]
        uvm = int(rng.integers(0, 2)); po = [off + f * (pfi + 16) + jy[f] for f in range(nf)]
        d_out5 = torch.full((off + (pfi + 16) * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda"); want = np.full(d_out5.numel(), 0x5A, np.uint8)
        for f in range(nf):
            px = imgs[f].reshape(h, w, 3); px = px if order == 0 else px[:, :, ::-1]
            eqf = oracle.nv12_frame(oracle.bgr_to_nv12(np.ascontiguousarray(px)), w, h, uv_mode=uvm, op=op, clip_limit=clip, tiles_x=tx, tiles_y=ty)
            uvr = eqf[w * h:].reshape(h // 2, w)
            want[po[f]: po[f] + yp * h].reshape(h, yp)[:, :w] = eqf[: w * h].reshape(h, w)
            want[po[f] + u_off: po[f] + u_off + csz].reshape(h // 2, cp)[:, : w // 2] = uvr[:, 0::2]
            want[po[f] + v_off: po[f] + v_off + csz].reshape(h // 2, cp)[:, : w // 2] = uvr[:, 1::2]
        b5 = d_out5.data_ptr()
        ents = [mi_lumaeq.BgrYuv420FrameDev(d_out4.data_ptr() + oo[f], b5 + po[f], b5 + po[f] + u_off, b5 + po[f] + v_off) for f in perm]
        ba = (ents, w, h, opi, yp, cp, mi_lumaeq.CHROMA_PLANAR, order, uvm)
        if op == 0: ctx.equalize_hist_bgr_to_yuv420_frames_dev(*ba)
        else: ctx.clahe_bgr_to_yuv420_frames_dev(*ba, clip, tx, ty)
        ctx.synchronize(); got = xfer.to_host(d_out5)
        if not np.array_equal(got, want): fail("bgryuv420 list", w, h, nf, op, order, uvm, clip, tx, ty, al, opi, yp, cp, g0, g1, pfi, yv12, off, perm, jy, np.flatnonzero(got != want)[:8])
        if not np.array_equal(xfer.to_host(d_out4), out): fail("bgryuv420 list wrote its input", w, h, nf, op)
        n["bgryuv420list"] += 1
    elif k == 7:    # packed 4:2:2 in, BGR / RGB out on a frame list: every row its own chroma, every image at its own byte offset (wide and byte stores in one launch)
        w, h, nf = int(rng.integers(1, 120)) * 2, int(rng.integers(1, 70)), int(rng.integers(1, 7))
        op, order, fmt = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(2, 4)); off = fmt - 2
        tx, ty = int(rng.choice([1, 3, 8, 16, 64])), int(rng.integers(1, 6)); clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        ipi = 2 * w + 4 * int(rng.integers(0, 10)); opi = 3 * w + (4 - 3 * w % 4) % 4 + 4 * int(rng.integers(0, 4)) if rng.integers(0, 3) else 3 * w + int(rng.integers(0, 9))
        fr = rng.integers(0, 256, (nf, h, ipi), dtype=np.uint8)
        ioff = [4 * int(rng.integers(0, 4)) for _ in range(nf)]; ooff = [int(rng.integers(0, 16)) if rng.integers(0, 2) else 4 * int(rng.integers(0, 4)) for _ in range(nf)]
        imgs_in = [np.full(ioff[f] + ipi * h + 32, 0x5A, np.uint8) for f in range(nf)]
        for f in range(nf): imgs_in[f][ioff[f]: ioff[f] + ipi * h] = fr[f].reshape(-1)
        d_ins = [dev(a) for a in imgs_in]; d_outs = [torch.full((ooff[f] + opi * h + 32,), 0x5A, dtype=torch.uint8, device="cuda") for f in range(nf)]
        la = ([d_ins[f].data_ptr() + ioff[f] for f in range(nf)], [d_outs[f].data_ptr() + ooff[f] for f in range(nf)], w, h, fmt, order)
        d_bat = torch.full((nf, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda"); ba = (dev(fr), d_bat, w, h, nf, fmt, order); bkw = dict(in_pitch=ipi)
        try:
            if op == 0: ctx.equalize_hist_packed422_to_bgr_frames(*la, in_pitch=ipi, out_pitch=opi); ctx.equalize_hist_packed422_to_bgr_batch_dev(*ba, **bkw)
            else: ctx.clahe_packed422_to_bgr_frames(*la, clip, tx, ty, in_pitch=ipi, out_pitch=opi); ctx.clahe_packed422_to_bgr_batch_dev(*ba, clip, tx, ty, **bkw)
        except mi_lumaeq.MiError as e:
            if e.status != 2: fail("p422bgr list status", w, h, nf, op, tx, ty, e.status)
            continue                                                   # a tile grid the planar forms refuse
        ctx.synchronize(); bat = xfer.to_host(d_bat)
        for f in range(nf):
            y = np.ascontiguousarray(fr[f, :, off:2 * w:2]); uvr = np.ascontiguousarray(fr[f, :, 1 - off:2 * w:2])
            ym = oracle.equalize_hist(y) if op == 0 else oracle.clahe(y, clip, tx, ty)
            bgr = oracle.nv12_to_bgr(np.concatenate([np.repeat(ym, 2, axis=0).reshape(-1), uvr.reshape(-1)]), w, 2 * h)[0::2]   # row r decoded with chroma row r
            bgr = np.ascontiguousarray(bgr if order == 0 else bgr[:, :, ::-1])
            want = np.full(d_outs[f].numel(), 0x5A, np.uint8); want[ooff[f]: ooff[f] + opi * h].reshape(h, opi)[:, : 3 * w] = bgr.reshape(h, 3 * w)
            got = xfer.to_host(d_outs[f])
            if not np.array_equal(got, want): fail("p422bgr list", w, h, nf, op, order, fmt, clip, tx, ty, ipi, opi, ioff, ooff, f, np.flatnonzero(got != want)[:8])
            if not np.array_equal(bat[f], bgr): fail("p422bgr batch", w, h, nf, op, order, fmt, clip, tx, ty, f)
            if not np.array_equal(xfer.to_host(d_ins[f]), imgs_in[f]): fail("p422bgr list wrote its input", w, h, nf, op, f)
        n["p422bgrlist"] += 1
    elif k == 8:    # BGR / RGB in, packed 4:2:2 out: pitched layouts, aligned (16-pixel groups) or not (macropixels), any height, both ops
        w, h, nf = int(rng.integers(1, 40)) * (16 if rng.integers(0, 2) else 2), int(rng.integers(1, 70)), int(rng.integers(1, 6))
        op, order, fmt, uvm = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(2, 4)), int(rng.integers(0, 2))
        tx, ty = int(rng.choice([1, 3, 8, 16, 64])), int(rng.integers(1, 6)); clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        al = 16 if rng.integers(0, 4) else 1; oal = max(al, 4)         # the output terms are multiples of 4 whatever the input's are
        def pad(v, a): return (v + a - 1) // a * a + a * int(rng.integers(0, 40 // a + 1))
        ipi, opi = pad(3 * w, al), pad(2 * w, oal); ioff, ifgap, ooff, ofgap = pad(0, al), pad(0, al), pad(0, oal), pad(0, oal)
        fi, fo = ipi * h + ifgap, opi * h + ofgap
        px = rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
        img = np.full(ioff + fi * nf + 64, 0x5A, np.uint8)
        for f in range(nf): img[ioff + f * fi: ioff + f * fi + ipi * h].reshape(h, ipi)[:, : 3 * w] = px[f].reshape(h, 3 * w)
        d_in = dev(img); d_out = torch.full((ooff + fo * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        a = (d_in.data_ptr() + ioff, d_out.data_ptr() + ooff, w, h, nf, order, fmt, uvm); kw = dict(in_pitch=ipi, in_frame=fi, out_pitch=opi, out_frame=fo)
        try:
            if op == 0: ctx.equalize_hist_bgr_to_packed422_batch_dev(*a, **kw)
            else: ctx.clahe_bgr_to_packed422_batch_dev(*a, clip, tx, ty, **kw)
        except mi_lumaeq.MiError as e:
            if e.status != 2: fail("bgrp422 status", w, h, nf, op, tx, ty, e.status)
            continue                                                   # a tile grid the planar forms refuse
        ctx.synchronize(); out = xfer.to_host(d_out); want = np.full(out.size, 0x5A, np.uint8)
        for f in range(nf):
            bgr = px[f] if order == 0 else px[f][:, :, ::-1]
            nv = oracle.bgr_to_nv12(np.ascontiguousarray(np.repeat(bgr, 2, axis=0)))      # Y row 2r: row r's luma; UV row r: its left-pixel U V U V ...
            y = np.ascontiguousarray(nv[: 2 * h * w].reshape(2 * h, w)[0::2]); uvr = nv[2 * h * w:].reshape(h, w)
            fr = np.empty((h, 2 * w), np.uint8); fr[:, fmt - 2::2] = oracle.equalize_hist(y) if op == 0 else oracle.clahe(y, clip, tx, ty)
            fr[:, 3 - fmt::2] = uvr if uvm == 1 else 128
            want[ooff + f * fo: ooff + f * fo + opi * h].reshape(h, opi)[:, : 2 * w] = fr
        if not np.array_equal(out, want): fail("bgrp422", w, h, nf, op, order, fmt, uvm, clip, tx, ty, al, ipi, opi, ioff, ifgap, ooff, ofgap, np.flatnonzero(out != want)[:8])
        if not np.array_equal(xfer.to_host(d_in), img): fail("bgrp422 wrote its input", w, h, nf, op)
        n["bgrp422"] += 1
    elif k == 9:    # the same on a frame list: every image and every frame its own allocation; each frame on the groups or the macropixels by its own addresses
        w, h, nf = int(rng.integers(1, 40)) * (16 if rng.integers(0, 2) else 2), int(rng.integers(1, 70)), int(rng.integers(1, 7))
        op, order, fmt, uvm = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(2, 4)), int(rng.integers(0, 2))
        tx, ty = int(rng.choice([1, 3, 8, 16, 64])), int(rng.integers(1, 6)); clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        al = 16 if rng.integers(0, 4) else 1; oal = max(al, 4)         # the pitches: multiples of 16 three times in four
        def pad(v, a): return (v + a - 1) // a * a + a * int(rng.integers(0, 40 // a + 1))
        ipi, opi = pad(3 * w, al), pad(2 * w, oal)
        ioff = [16 * int(rng.integers(0, 4)) if rng.integers(0, 2) else int(rng.integers(0, 32)) for _ in range(nf)]      # any address
        ooff = [16 * int(rng.integers(0, 4)) if rng.integers(0, 2) else 4 * int(rng.integers(0, 8)) for _ in range(nf)]   # multiples of 4
        px = rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
        imgs = [np.full(ioff[f] + ipi * h + 32, 0x5A, np.uint8) for f in range(nf)]
        for f in range(nf): imgs[f][ioff[f]: ioff[f] + ipi * h].reshape(h, ipi)[:, : 3 * w] = px[f].reshape(h, 3 * w)
        d_ins = [dev(a) for a in imgs]; d_outs = [torch.full((ooff[f] + opi * h + 32,), 0x5A, dtype=torch.uint8, device="cuda") for f in range(nf)]
        perm = [int(v) for v in rng.permutation(nf)]                     # the list order is not the allocation order
        la = ([d_ins[f].data_ptr() + ioff[f] for f in perm], [d_outs[f].data_ptr() + ooff[f] for f in perm], w, h, order, fmt, uvm)
        nvec = sum(1 for f in range(nf) if w % 16 == 0 and ipi % 16 == 0 and opi % 16 == 0 and ioff[f] % 16 == 0 and ooff[f] % 16 == 0)
        st0 = (ctx.get_stat("bgr_packed422_list_frames_vec"), ctx.get_stat("bgr_packed422_list_frames_bytes"))
        try:
            if op == 0: ctx.equalize_hist_bgr_to_packed422_frames(*la, in_pitch=ipi, out_pitch=opi)
            else: ctx.clahe_bgr_to_packed422_frames(*la, clip, tx, ty, in_pitch=ipi, out_pitch=opi)
        except mi_lumaeq.MiError as e:
            if e.status != 2: fail("bgrp422 list status", w, h, nf, op, tx, ty, e.status)
            continue                                                   # a tile grid the planar forms refuse
        ctx.synchronize()
        if (ctx.get_stat("bgr_packed422_list_frames_vec") - st0[0], ctx.get_stat("bgr_packed422_list_frames_bytes") - st0[1]) != (nvec, nf - nvec):
            fail("bgrp422 list counters", w, h, nf, ipi, opi, ioff, ooff, nvec)
        for f in range(nf):
            bgr = px[f] if order == 0 else px[f][:, :, ::-1]
            nv = oracle.bgr_to_nv12(np.ascontiguousarray(np.repeat(bgr, 2, axis=0)))      # Y row 2r: row r's luma; UV row r: its left-pixel U V U V ...
            y = np.ascontiguousarray(nv[: 2 * h * w].reshape(2 * h, w)[0::2]); uvr = nv[2 * h * w:].reshape(h, w)
            fr = np.empty((h, 2 * w), np.uint8); fr[:, fmt - 2::2] = oracle.equalize_hist(y) if op == 0 else oracle.clahe(y, clip, tx, ty)
            fr[:, 3 - fmt::2] = uvr if uvm == 1 else 128
            want = np.full(d_outs[f].numel(), 0x5A, np.uint8); want[ooff[f]: ooff[f] + opi * h].reshape(h, opi)[:, : 2 * w] = fr
            got = xfer.to_host(d_outs[f])
            if not np.array_equal(got, want): fail("bgrp422 list", w, h, nf, op, order, fmt, uvm, clip, tx, ty, ipi, opi, ioff, ooff, perm, f, np.flatnonzero(got != want)[:8])
            if not np.array_equal(xfer.to_host(d_ins[f]), imgs[f]): fail("bgrp422 list wrote its input", w, h, nf, op, f)
        n["bgrp422list"] += 1
    elif k == 10:   # 4:2:0 in (NV12 / I420 / YV12), packed 4:2:2 out: pitched layouts, aligned (16 x 2 groups, CLAHE in one pass where the grid allows) or not, both ops
        w, h, nf = int(rng.integers(1, 40)) * (16 if rng.integers(0, 2) else 2), int(rng.integers(1, 40)) * 2, int(rng.integers(1, 6))
        op, sfmt, fmt, uvm = int(rng.integers(0, 2)), str(rng.choice(["nv12", "i420", "yv12"])), int(rng.integers(2, 4)), int(rng.integers(0, 2))
        tx, ty = int(rng.choice([1, 2, 4, 8, 3, 16])), int(rng.integers(1, 6)); clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        planar = sfmt != "nv12"; cw = w // 2 if planar else w
        al = 16 if rng.integers(0, 4) else 1; cal = (8 if planar and al == 16 and rng.integers(0, 2) else al); oal = max(al, 4)
        def pad(v, a): return (v + a - 1) // a * a + a * int(rng.integers(0, 40 // a + 1))
        ypi, cpi, opi = pad(w, al), pad(cw, cal), pad(2 * w, oal)
        yoff = pad(0, al); a_off = pad(yoff + ypi * h, cal); b_off = pad(a_off + cpi * (h // 2), cal) if planar else a_off
        fi = pad(b_off + cpi * (h // 2), al); ooff, fo = pad(0, oal), pad(opi * h, oal)
        u_off, v_off = (a_off, b_off) if sfmt != "yv12" else (b_off, a_off)
        Y = rng.integers(0, int(rng.integers(2, 257)), (nf, h, w), dtype=np.uint8); U, V = (rng.integers(0, 256, (nf, h // 2, w // 2), dtype=np.uint8) for _ in range(2))
        img = np.full(fi * nf + 64, 0x5A, np.uint8)
        for f in range(nf):
            b = f * fi
            img[b + yoff: b + yoff + ypi * h].reshape(h, ypi)[:, :w] = Y[f]
            if planar:
                img[b + u_off: b + u_off + cpi * (h // 2)].reshape(h // 2, cpi)[:, :cw] = U[f]; img[b + v_off: b + v_off + cpi * (h // 2)].reshape(h // 2, cpi)[:, :cw] = V[f]
            else:
                r = img[b + a_off: b + a_off + cpi * (h // 2)].reshape(h // 2, cpi); r[:, 0:w:2] = U[f]; r[:, 1:w:2] = V[f]
        d_in = dev(img); d_out = torch.full((ooff + fo * nf + 64,), 0x5A, dtype=torch.uint8, device="cuda"); base = d_in.data_ptr()
        pl = mi_lumaeq.Yuv420Planes(base + yoff, ypi, base + u_off if uvm else None, base + v_off if uvm and planar else None, cpi if uvm else 0, fi,
                                    mi_lumaeq.CHROMA_PLANAR if planar else mi_lumaeq.CHROMA_INTERLEAVED)
        terms = [yoff, ypi, fi, ooff, opi, fo]; cterms = ([u_off, cpi] + ([v_off] if planar else [])) if uvm else []
        vec = w % 16 == 0 and all(t % 16 == 0 for t in terms) and all(t % (8 if planar else 16) == 0 for t in cterms)
        one = op == 0 or (vec and w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= 15)
        names = ("yuv420_packed422_onepass", "yuv420_packed422_twopass", "yuv420_packed422_vec", "yuv420_packed422_bytes"); st0 = [ctx.get_stat(s) for s in names]
        a = (pl, d_out.data_ptr() + ooff, w, h, nf, fmt, uvm); kw = dict(out_pitch=opi, out_frame=fo)
        try:
            if op == 0: ctx.equalize_hist_yuv420_to_packed422_batch_dev(*a, **kw)
            else: ctx.clahe_yuv420_to_packed422_batch_dev(*a, clip, tx, ty, **kw)
        except mi_lumaeq.MiError as e:
            if e.status != 2: fail("yuv420p422 status", w, h, nf, op, tx, ty, e.status)
            continue                                                   # a tile grid the planar forms refuse
        ctx.synchronize(); out = xfer.to_host(d_out); want = np.full(out.size, 0x5A, np.uint8)
        if [ctx.get_stat(s) - v for s, v in zip(names, st0)] != [int(one), int(not one), int(vec), int(not vec)]:
            fail("yuv420p422 counters", w, h, nf, op, sfmt, uvm, tx, ty, terms, cterms, vec, one)
        for f in range(nf):
            fr = np.empty((h, 2 * w), np.uint8); fr[:, fmt - 2::2] = oracle.equalize_hist(Y[f]) if op == 0 else oracle.clahe(Y[f], clip, tx, ty)
            uvr = np.empty((h // 2, w), np.uint8); uvr[:, 0::2] = U[f]; uvr[:, 1::2] = V[f]
            fr[:, 3 - fmt::2] = np.repeat(uvr, 2, axis=0) if uvm == 1 else 128          # chroma row r under output rows 2r and 2r + 1
            want[ooff + f * fo: ooff + f * fo + opi * h].reshape(h, opi)[:, : 2 * w] = fr
        if not np.array_equal(out, want): fail("yuv420p422", w, h, nf, op, sfmt, fmt, uvm, clip, tx, ty, terms, cterms, np.flatnonzero(out != want)[:8])
        if not np.array_equal(xfer.to_host(d_in), img): fail("yuv420p422 wrote its input", w, h, nf, op)
        n["yuv420p422"] += 1
    elif k == 11:   # the same on a frame list: every plane and every frame its own allocation at its own skew; each frame on the groups or the blocks by its own addresses
        w, h, nf = int(rng.integers(1, 40)) * (16 if rng.integers(0, 2) else 2), int(rng.integers(1, 40)) * 2, int(rng.integers(1, 7))
        op, sfmt, fmt, uvm = int(rng.integers(0, 2)), str(rng.choice(["nv12", "i420"])), int(rng.integers(2, 4)), int(rng.integers(0, 2))      # a pool has no YV12 of its own: c0 is U
        tx, ty = int(rng.choice([1, 2, 4, 8, 3, 16])), int(rng.integers(1, 6)); clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
        planar = sfmt != "nv12"; cw = w // 2 if planar else w; cm = 8 if planar else 16
        al = 16 if rng.integers(0, 4) else 1; cal = (8 if planar and al == 16 and rng.integers(0, 2) else al); oal = max(al, 4)
        def pad(v, a): return (v + a - 1) // a * a + a * int(rng.integers(0, 40 // a + 1))
        ypi, cpi, opi = pad(w, al), pad(cw, cal), pad(2 * w, oal)
        def skew(m): return m * int(rng.integers(0, 4)) if rng.integers(0, 4) else int(rng.integers(0, 32))      # a multiple of the rule's, three times in four
        yoff, uoff, voff = [skew(16) for _ in range(nf)], [skew(cm) for _ in range(nf)], [skew(cm) for _ in range(nf)]
        ooff = [16 * int(rng.integers(0, 4)) if rng.integers(0, 4) else 4 * int(rng.integers(0, 8)) for _ in range(nf)]   # multiples of 4
        Y = rng.integers(0, int(rng.integers(2, 257)), (nf, h, w), dtype=np.uint8); U, V = (rng.integers(0, 256, (nf, h // 2, w // 2), dtype=np.uint8) for _ in range(2))
        def plane(off, pitch, rows, data):
            a = np.full(off + pitch * rows + 32, 0x5A, np.uint8); a[off: off + pitch * rows].reshape(rows, pitch)[:, : data.shape[1]] = data; return a
        def uvrow(f):
            r = np.empty((h // 2, w), np.uint8); r[:, 0::2] = U[f]; r[:, 1::2] = V[f]; return r
        hy = [plane(yoff[f], ypi, h, Y[f]) for f in range(nf)]
        hu = [plane(uoff[f], cpi, h // 2, U[f] if planar else uvrow(f)) for f in range(nf)]
        hv = [plane(voff[f], cpi, h // 2, V[f]) for f in range(nf)] if planar else []
        dy, du, dv = [dev(a) for a in hy], [dev(a) for a in hu], [dev(a) for a in hv]
        d_outs = [torch.full((ooff[f] + opi * h + 32,), 0x5A, dtype=torch.uint8, device="cuda") for f in range(nf)]
        perm = [int(v) for v in rng.permutation(nf)]                     # the list order is not the allocation order
        junk = uvm == 0 and bool(rng.integers(0, 2))                     # MI_UV_FILL128: null chroma addresses, or the real ones (ignored either way)
        ents = [mi_lumaeq.Yuv420Packed422FrameDev(dy[f].data_ptr() + yoff[f], None if junk else du[f].data_ptr() + uoff[f],
                                                  None if junk or not planar else dv[f].data_ptr() + voff[f], d_outs[f].data_ptr() + ooff[f]) for f in perm]
        shape = w % 16 == 0 and ypi % 16 == 0 and opi % 16 == 0 and (not uvm or cpi % cm == 0)
        def cok(f): return not uvm or (uoff[f] % cm == 0 and (not planar or voff[f] % cm == 0))
        one = op == 0 or (shape and w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= 15 and all(yoff[f] % 16 == 0 and ooff[f] % 16 == 0 and cok(f) for f in range(nf)))
        nvec = sum(1 for f in range(nf) if shape and (yoff[f] % 16 == 0 or not one) and ooff[f] % 16 == 0 and cok(f))      # two-pass: the luma comes from aligned scratch
        names = ("yuv420_packed422_onepass", "yuv420_packed422_twopass", "yuv420_packed422_list_frames_vec", "yuv420_packed422_list_frames_bytes",
                 "yuv420_packed422_vec", "yuv420_packed422_bytes"); st0 = [ctx.get_stat(s) for s in names]
        a = (ents, w, h, ypi, cpi if not junk else 0, mi_lumaeq.CHROMA_PLANAR if planar else mi_lumaeq.CHROMA_INTERLEAVED, fmt, uvm)
        try:
            if op == 0: ctx.equalize_hist_yuv420_to_packed422_frames_dev(*a, out_pitch=opi)
            else: ctx.clahe_yuv420_to_packed422_frames_dev(*a, clip, tx, ty, out_pitch=opi)
        except mi_lumaeq.MiError as e:
            if e.status != 2: fail("yuv420_to_packed422_frames status", w, h, nf, op, tx, ty, e.status)
            continue                                                   # a tile grid the planar forms refuse
        ctx.synchronize()
        if [ctx.get_stat(s) - v for s, v in zip(names, st0)] != [int(one), int(not one), nvec, nf - nvec, 0, 0]:
            fail("yuv420_to_packed422_frames counters", w, h, nf, op, sfmt, uvm, tx, ty, ypi, cpi, opi, yoff, uoff, voff, ooff, one, nvec)
        for f in range(nf):
            fr = np.empty((h, 2 * w), np.uint8); fr[:, fmt - 2::2] = oracle.equalize_hist(Y[f]) if op == 0 else oracle.clahe(Y[f], clip, tx, ty)
            fr[:, 3 - fmt::2] = np.repeat(uvrow(f), 2, axis=0) if uvm == 1 else 128          # chroma row r under output rows 2r and 2r + 1
            want = np.full(d_outs[f].numel(), 0x5A, np.uint8); want[ooff[f]: ooff[f] + opi * h].reshape(h, opi)[:, : 2 * w] = fr
            got = xfer.to_host(d_outs[f])
            if not np.array_equal(got, want):
                fail("yuv420_to_packed422_frames", w, h, nf, op, sfmt, fmt, uvm, clip, tx, ty, ypi, cpi, opi, yoff, uoff, voff, ooff, perm, f, np.flatnonzero(got != want)[:8])
            if not np.array_equal(xfer.to_host(dy[f]), hy[f]) or not np.array_equal(xfer.to_host(du[f]), hu[f]) or (planar and not np.array_equal(xfer.to_host(dv[f]), hv[f])):
                fail("yuv420_to_packed422_frames wrote its input", w, h, nf, op, f)
        n["yuv420p422list"] += 1
    else:           # 4:2:0 codes
        w, h = int(rng.integers(1, 60)) * (16 if rng.integers(0, 2) else 2), int(rng.integers(1, 40)) * 2
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if not np.array_equal(ctx.cvt_color_420(bgr, mi_lumaeq.COLOR_BGR2YUV_I420), oracle.bgr_to_i420(bgr)): fail("i420", w, h)
        nv = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
        if not np.array_equal(ctx.cvt_color_420(nv, mi_lumaeq.COLOR_YUV2BGR_NV12), oracle.nv12_to_bgr(nv, w, h)): fail("nv12->bgr", w, h)
        n["420"] += 1
    if time.time() - last > 15:
        last = time.time(); print(f"[{last - t0:5.0f} s] cases {n}", flush=True)
print(f"stress_random: {sum(n.values())} cases {n} in {time.time() - t0:.0f} s, no mismatch")
