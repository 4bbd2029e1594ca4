"""The seeded cases of the mi_*_yuv420_to_packed422_frames_dev sweep and the documented rule (include/mi_lumaeq.h) restated as a function
from a case to its class and its counter deltas.  No GPU and no library is needed here: tests/test_yuv420_to_packed422_frames_abi.py
asserts the class counts on the CPU, tests/test_gpu_yuv420_to_packed422_frames.py runs the same cases on the GPU."""
import numpy as np

SWEEP_SEED, SWEEP_CASES = 16, 32
CLASSES = ("vector-onepass", "vector-twopass", "byte-frames", "fill128")
FMT_YUY2, FMT_UYVY = 2, 3
UV_FILL128, UV_COPY = 0, 1
# one count a call, the FRAMES of list calls by their walk, and the batch form's pair, which no list call moves
COUNTERS = ("yuv420_packed422_onepass", "yuv420_packed422_twopass", "yuv420_packed422_list_frames_vec", "yuv420_packed422_list_frames_bytes",
            "yuv420_packed422_vec", "yuv420_packed422_bytes")


def draw_case(rng):
    """W even <= 128, H even <= 48, 1..4 frames, the op, a tile grid, a clip limit, the packed format, the UV mode, the layout (NV12,
    I420 or YV12), three pitches and per frame the four addresses' offsets past a 16-byte boundary (y, c0, c1, out; the output's a
    multiple of 4; an NV12 frame has no c1).  `aim` only steers the draw towards the four classes; classify() does not look at it."""
    aim = int(rng.integers(0, 4))
    kind = "clahe" if (aim == 1 or rng.random() < 0.6) else "eq"
    n, fmt = int(rng.integers(1, 5)), int(rng.integers(FMT_YUY2, FMT_UYVY + 1))
    uv_mode = UV_FILL128 if aim == 3 else UV_COPY
    src = ("nv12", "i420", "yv12")[int(rng.integers(0, 3))]
    clip = float(rng.choice([0.0, 1.0, 2.0, 40.0]))
    tx, ty = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    if aim == 2 and rng.random() < 0.4:
        w, h = 2 * int(rng.integers(1, 65)), 2 * int(rng.integers(1, 25))
    else:
        w = 16 * tx * int(rng.integers(1, 8 // tx + 1))
        m = ty if ty % 2 == 0 else 2 * ty
        h = m * int(rng.integers(1, 48 // m + 1))
    if aim == 1 and rng.random() < 0.7:
        ty = next((t for t in range(ty + 1, ty + 4) if h % t and t <= h), ty)      # a grid that does not divide the frame: REFLECT_101 padding
    crow = w if src == "nv12" else w // 2
    if aim == 2 and rng.random() < 0.5:
        yp, cp, op = w + int(rng.integers(0, 24)), crow + int(rng.integers(0, 24)), 2 * w + 4 * int(rng.integers(0, 6))
    else:
        yp = (w + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
        cp = (crow + 7) // 8 * 8 + 8 * int(rng.integers(0, 3)) if src != "nv12" else (crow + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
        op = (2 * w + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
    skews = []
    for k in range(n):
        s = [0, 8 * int(rng.integers(0, 2)), 8 * int(rng.integers(0, 2)), 0] if src != "nv12" else [0, 0, 0, 0]
        if aim in (2, 3) and rng.random() < (0.6 if aim == 2 else 0.4):
            i = int(rng.integers(0, 4))
            s[i] += int(rng.choice([4, 8])) if i == 3 else int(rng.choice([1, 4, 8]))
        if src == "nv12":
            s[2] = 0
        skews.append(tuple(s))
    return dict(kind=kind, w=w, h=h, n=n, tx=tx, ty=ty, clip=clip, fmt=fmt, uv_mode=uv_mode, src=src, y_pitch=yp, c_pitch=cp, out_pitch=op,
                skews=skews)


def onepass_shape(w, h, tx, ty, max_pairs):
    """the batch form's one-pass shape: the tile grid divides the frame, tile width a multiple of 16, tiles_x + 1 pair tables in LDS"""
    return w % tx == 0 and h % ty == 0 and (w // tx) % 16 == 0 and tx + 1 <= max_pairs


def classify(case, max_pairs):
    """The class of a case and the deltas of COUNTERS, from the header's words alone.  clahe_fp_contract is off."""
    w, h, tx, ty, sk = case["w"], case["h"], case["tx"], case["ty"], case["skews"]
    yp, cp, op, n = case["y_pitch"], case["c_pitch"], case["out_pitch"], case["n"]
    clahe, copy, planar = case["kind"] == "clahe", case["uv_mode"] == UV_COPY, case["src"] != "nv12"
    # under MI_UV_FILL128 the chroma addresses and the chroma pitch decide nothing
    shape = w % 16 == 0 and yp % 16 == 0 and op % 16 == 0 and (not copy or cp % (8 if planar else 16) == 0)

    def chroma(s):
        return not copy or (s[1] % 8 == 0 and s[2] % 8 == 0 if planar else s[1] % 16 == 0)
    addr = [s[0] % 16 == 0 and s[3] % 16 == 0 and chroma(s) for s in sk]
    one = not clahe or (onepass_shape(w, h, tx, ty, max_pairs) and shape and all(addr))
    if not one:                             # the pack reads the luma from aligned scratch planes: the y address drops out of the rule
        addr = [s[3] % 16 == 0 and chroma(s) for s in sk]
    nvec = sum(addr) if shape else 0
    name = "fill128" if not copy else "byte-frames" if nvec < n else ("vector-onepass" if one else "vector-twopass")
    return name, (int(one), int(not one), nvec, n - nvec, 0, 0)


def sweep_cases(seed=SWEEP_SEED):
    rng = np.random.default_rng(seed)
    return [draw_case(rng) for _ in range(SWEEP_CASES)]


def class_counts(cases, max_pairs):
    names = [classify(k, max_pairs)[0] for k in cases]
    return {name: names.count(name) for name in CLASSES}
