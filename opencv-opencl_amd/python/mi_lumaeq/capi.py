"""ctypes binding of include/mi_lumaeq.h.  Fails loudly when the HIP library is missing."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import sys
import weakref
from pathlib import Path

import numpy as np

_ROOT = Path(__file__).resolve().parents[2]          # opencv-opencl_amd/
_LIB_PATH = _ROOT / "lib" / "libmi_lumaeq.so"
_TEST_LIB_PATH = _ROOT / "lib" / "libmi_lumaeq_test.so"      # same sources + test hooks (-DMI_TEST_HOOKS); loaded by tests only

UV_FILL128, UV_COPY = 0, 1
STREAM_CTX = C.c_void_p(-1).value      # MI_STREAM_CTX: the context's private stream; 0/None = HIP null stream
KERNEL_NAMES = ["hist_partial_kernel", "equalize_lut_kernel", "lut_apply_kernel",
                "tile_hist_kernel", "tile_lut_kernel", "clahe_interp_kernel", "equalize_fused_kernel", "color_kernel",
                "fused_finish_kernel", "analyze_diff_kernel"]
COLOR_BGR2YUV, COLOR_YUV2BGR = 82, 84
COLOR_YUV2BGR_NV12, COLOR_BGR2YUV_I420 = 93, 128
OP_EQUALIZE, OP_CLAHE, OP_CHANNELS = 0, 1, 2
PIPE_UV_AUTO, PIPE_UV_HOST, PIPE_UV_DEVICE = 0, 1, 2
FMT_NV12, FMT_P010 = 0, 1              # MI_FMT_*: P010 = any 16-bit LE 4:2:0 semi-planar frame (P010 / P012 / P016)
FMT_YUY2, FMT_UYVY = 2, 3              # packed 8-bit 4:2:2: luma at byte 0 (YUY2 / YUYV / YVYU) or byte 1 (UYVY / VYUY) of each 2-byte pixel
ORDER_BGR, ORDER_RGB = 0, 1            # MI_ORDER_*: channel order of the interleaved side of the NV12 -> BGR and BGR -> NV12 forms
CHROMA_INTERLEAVED, CHROMA_PLANAR = 0, 1     # MI_CHROMA_*: the chroma of one side of the mi_*_yuv420* forms -- one plane of U, V pairs (NV12) or a U and a V plane (I420 / YV12)
ERR_BUSY = 6

# every extern "C" symbol include/mi_lumaeq.h declares (tests check the .so exports them all)
DECLARED_SYMBOLS = [
    "mi_ctx_create", "mi_ctx_destroy", "mi_ctx_device", "mi_ctx_last_hip_error", "mi_ctx_last_error_msg",
    "mi_status_str", "mi_version", "mi_device_count",
    "mi_equalize_hist_u8", "mi_clahe_u8", "mi_equalize_hist_nv12", "mi_clahe_nv12",
    "mi_equalize_hist_u8_batch_dev", "mi_clahe_u8_batch_dev",
    "mi_equalize_hist_nv12_batch_dev", "mi_clahe_nv12_batch_dev",
    "mi_hist_u8_batch_dev", "mi_equalize_lut_batch_dev", "mi_lut_apply_u8_batch_dev",
    "mi_clahe_tile_luts_batch_dev",
    "mi_ctx_set_profiling", "mi_ctx_profile_read", "mi_kernel_name",
    "mi_ctx_synchronize", "mi_ctx_set_option", "mi_ctx_get_stat",
    "mi_pipe_create", "mi_pipe_destroy", "mi_pipe_submit", "mi_pipe_wait", "mi_pipe_pending", "mi_pipe_depth",
    "mi_host_register", "mi_host_unregister", "mi_clahe_u16", "mi_clahe_u16_batch_dev",
    "mi_cvt_color_u8c3", "mi_cvt_color_u8c3_batch_dev", "mi_bgr_luma_op_u8c3", "mi_bgr_luma_op_u8c3_batch_dev",
    "mi_nv12_bgr_equalize", "mi_nv12_bgr_equalize_batch_dev", "mi_cvt_color_420_u8", "mi_cvt_color_420_u8_batch_dev",
    "mi_analyze_diff_u8", "mi_analyze_diff_u8_batch_dev",
    "mi_device_pci_bus_id", "mi_thread_bind_near_device",
    "mi_clahe_p010", "mi_clahe_p010_batch_dev",
    "mi_equalize_hist_nv12_frames_dev", "mi_clahe_nv12_frames_dev",
    "mi_clahe_p010_frames_dev",
    "mi_equalize_hist_packed422_batch_dev", "mi_clahe_packed422_batch_dev", "mi_equalize_hist_packed422", "mi_clahe_packed422",
    "mi_equalize_hist_packed422_frames_dev", "mi_clahe_packed422_frames_dev",
    "mi_equalize_hist_packed422_to_nv12_batch_dev", "mi_clahe_packed422_to_nv12_batch_dev",
    "mi_equalize_hist_packed422_to_nv12_frames_dev", "mi_clahe_packed422_to_nv12_frames_dev",
    "mi_equalize_hist_packed422_to_nv12", "mi_clahe_packed422_to_nv12",
    "mi_equalize_hist_packed422_to_yuv420_batch_dev", "mi_clahe_packed422_to_yuv420_batch_dev",
    "mi_equalize_hist_packed422_to_yuv420", "mi_clahe_packed422_to_yuv420",
    "mi_equalize_hist_packed422_to_yuv420_frames_dev", "mi_clahe_packed422_to_yuv420_frames_dev",
    "mi_equalize_hist_packed422_to_bgr_batch_dev", "mi_clahe_packed422_to_bgr_batch_dev",
    "mi_equalize_hist_packed422_to_bgr", "mi_clahe_packed422_to_bgr",
    "mi_equalize_hist_packed422_to_bgr_frames_dev", "mi_clahe_packed422_to_bgr_frames_dev",
    "mi_equalize_hist_packed422_to_bgra_batch_dev", "mi_clahe_packed422_to_bgra_batch_dev",
    "mi_equalize_hist_packed422_to_bgra", "mi_clahe_packed422_to_bgra",
    "mi_equalize_hist_packed422_to_bgra_frames_dev", "mi_clahe_packed422_to_bgra_frames_dev",
    "mi_equalize_hist_nv12_to_bgr_batch_dev", "mi_clahe_nv12_to_bgr_batch_dev", "mi_equalize_hist_nv12_to_bgr", "mi_clahe_nv12_to_bgr",
    "mi_equalize_hist_nv12_to_bgr_frames_dev", "mi_clahe_nv12_to_bgr_frames_dev",
    "mi_equalize_hist_bgr_to_nv12_batch_dev", "mi_clahe_bgr_to_nv12_batch_dev", "mi_equalize_hist_bgr_to_nv12", "mi_clahe_bgr_to_nv12",
    "mi_equalize_hist_bgr_to_nv12_frames_dev", "mi_clahe_bgr_to_nv12_frames_dev",
    "mi_equalize_hist_yuv420_batch_dev", "mi_clahe_yuv420_batch_dev", "mi_equalize_hist_yuv420", "mi_clahe_yuv420",
    "mi_equalize_hist_yuv420_frames_dev", "mi_clahe_yuv420_frames_dev",
    "mi_equalize_hist_yuv420_to_bgr_batch_dev", "mi_clahe_yuv420_to_bgr_batch_dev", "mi_equalize_hist_yuv420_to_bgr", "mi_clahe_yuv420_to_bgr",
    "mi_equalize_hist_yuv420_to_bgr_frames_dev", "mi_clahe_yuv420_to_bgr_frames_dev",
    "mi_equalize_hist_bgr_to_yuv420_batch_dev", "mi_clahe_bgr_to_yuv420_batch_dev", "mi_equalize_hist_bgr_to_yuv420", "mi_clahe_bgr_to_yuv420",
    "mi_equalize_hist_bgr_to_yuv420_frames_dev", "mi_clahe_bgr_to_yuv420_frames_dev",
    "mi_equalize_hist_bgr_to_packed422_batch_dev", "mi_clahe_bgr_to_packed422_batch_dev",
    "mi_equalize_hist_bgr_to_packed422", "mi_clahe_bgr_to_packed422",
    "mi_equalize_hist_bgr_to_packed422_frames_dev", "mi_clahe_bgr_to_packed422_frames_dev",
    "mi_equalize_hist_yuv420_to_packed422_batch_dev", "mi_clahe_yuv420_to_packed422_batch_dev",
    "mi_equalize_hist_yuv420_to_packed422", "mi_clahe_yuv420_to_packed422",
    "mi_equalize_hist_yuv420_to_packed422_frames_dev", "mi_clahe_yuv420_to_packed422_frames_dev",
    "mi_equalize_hist_bgra_to_yuv420_batch_dev", "mi_clahe_bgra_to_yuv420_batch_dev", "mi_equalize_hist_bgra_to_yuv420", "mi_clahe_bgra_to_yuv420",
    "mi_equalize_hist_bgra_to_yuv420_frames_dev", "mi_clahe_bgra_to_yuv420_frames_dev",
    "mi_equalize_hist_yuv420_to_bgra_batch_dev", "mi_clahe_yuv420_to_bgra_batch_dev", "mi_equalize_hist_yuv420_to_bgra", "mi_clahe_yuv420_to_bgra",
    "mi_equalize_hist_yuv420_to_bgra_frames_dev", "mi_clahe_yuv420_to_bgra_frames_dev",
    "mi_equalize_hist_bgra_to_packed422_batch_dev", "mi_clahe_bgra_to_packed422_batch_dev",
    "mi_equalize_hist_bgra_to_packed422", "mi_clahe_bgra_to_packed422",
    "mi_equalize_hist_bgra_to_packed422_frames_dev", "mi_clahe_bgra_to_packed422_frames_dev",
]

_K = len(KERNEL_NAMES)


class _Profile(C.Structure):
    _fields_ = [("total_ms", C.c_double * _K), ("launches", C.c_uint64 * _K), ("min_ms", C.c_double * _K), ("p10_ms", C.c_double * _K),
                ("p50_ms", C.c_double * _K), ("p90_ms", C.c_double * _K), ("max_ms", C.c_double * _K)]


class _NumaBinding(C.Structure):
    _fields_ = [("node", C.c_int), ("cpus", C.c_int), ("why", C.c_char * 192)]


class _PipeConfig(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("op", C.c_int), ("uv_mode", C.c_int), ("clip_limit", C.c_double),
                ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("depth", C.c_int), ("uv_policy", C.c_int), ("format", C.c_int)]


class Nv12FrameDev(C.Structure):
    """mi_nv12_frame_dev: one NV12 frame of a list, its four plane addresses (device pointers)."""
    _fields_ = [("y_in", C.c_void_p), ("uv_in", C.c_void_p), ("y_out", C.c_void_p), ("uv_out", C.c_void_p)]


class Packed422FrameDev(C.Structure):
    """mi_packed422_frame_dev: one packed 4:2:2 frame of a list, its input and output address (device pointers)."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p)]


class Packed422Nv12FrameDev(C.Structure):
    """mi_packed422_nv12_frame_dev: one frame of a packed 4:2:2 -> NV12 list, its input and its two output plane addresses (device
    pointers)."""
    _fields_ = [("in_", C.c_void_p), ("y_out", C.c_void_p), ("uv_out", C.c_void_p)]


class Packed422BgrFrameDev(C.Structure):
    """mi_packed422_bgr_frame_dev: one frame of a packed 4:2:2 -> BGR / RGB list, its input and its image address (device pointers)."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p)]


class Nv12BgrFrameDev(C.Structure):
    """mi_nv12_bgr_frame_dev: one frame of an NV12 -> BGR / RGB list, its two input plane addresses and its image address (device
    pointers)."""
    _fields_ = [("y", C.c_void_p), ("uv", C.c_void_p), ("out", C.c_void_p)]


class BgrNv12FrameDev(C.Structure):
    """mi_bgr_nv12_frame_dev: one frame of a BGR / RGB -> NV12 list, its image address and its two output plane addresses (device
    pointers)."""
    _fields_ = [("in_", C.c_void_p), ("y", C.c_void_p), ("uv", C.c_void_p)]


class BgrPacked422FrameDev(C.Structure):
    """mi_bgr_packed422_frame_dev: one frame of a BGR / RGB -> packed 4:2:2 list, its image address and its packed frame's address
    (device pointers)."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p)]


class Yuv420Planes(C.Structure):
    """mi_yuv420_planes: where the planes of one side of a mi_*_yuv420* call lie (device pointers for the batched forms, host pointers for
    the host forms).  c0 is always the U plane and c1 the V plane; an INTERLEAVED side has its UV plane in c0.  nv12() / i420() / yv12()
    describe tight frames of W*H*3/2 bytes starting at `base` (a raw address or a torch CUDA tensor)."""
    _fields_ = [("y", C.c_void_p), ("y_pitch", C.c_size_t), ("c0", C.c_void_p), ("c1", C.c_void_p), ("c_pitch", C.c_size_t),
                ("frame_stride", C.c_size_t), ("chroma", C.c_int)]

    @classmethod
    def nv12(cls, base, width, height):
        b, w, h = _dptr(base), int(width), int(height)
        return cls(b, w, b + w * h, None, w, w * h * 3 // 2, CHROMA_INTERLEAVED)

    @classmethod
    def i420(cls, base, width, height):
        b, w, h = _dptr(base), int(width), int(height)
        return cls(b, w, b + w * h, b + w * h + (w // 2) * (h // 2), w // 2, w * h * 3 // 2, CHROMA_PLANAR)

    @classmethod
    def yv12(cls, base, width, height):
        b, w, h = _dptr(base), int(width), int(height)
        return cls(b, w, b + w * h + (w // 2) * (h // 2), b + w * h, w // 2, w * h * 3 // 2, CHROMA_PLANAR)


class Yuv420FrameDev(C.Structure):
    """mi_yuv420_frame_dev: one frame of a mi_*_yuv420_frames_dev list, the addresses of its planes on both sides (device pointers).
    c0 is always the U plane and c1 the V plane (a YV12 frame exchanges the two); an INTERLEAVED side has its UV plane in c0 and its c1
    is ignored (None); with UV_FILL128 c0_in / c1_in are ignored."""
    _fields_ = [("y_in", C.c_void_p), ("c0_in", C.c_void_p), ("c1_in", C.c_void_p),
                ("y_out", C.c_void_p), ("c0_out", C.c_void_p), ("c1_out", C.c_void_p)]

    @classmethod
    def of(cls, y_in, c0_in, c1_in, y_out, c0_out, c1_out):
        """the same from torch CUDA tensors, raw device addresses or None"""
        return cls(*(None if p is None else _dptr(p) for p in (y_in, c0_in, c1_in, y_out, c0_out, c1_out)))


class Yuv420BgrFrameDev(C.Structure):
    """mi_yuv420_bgr_frame_dev: one frame of a mi_*_yuv420_to_bgr_frames_dev list, its three input plane addresses and its image address
    (device pointers).  c0 is always the U plane and c1 the V plane (a YV12 frame exchanges the two); an INTERLEAVED list has its UV
    plane in c0 and its c1 is ignored (None)."""
    _fields_ = [("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p), ("out", C.c_void_p)]

    @classmethod
    def of(cls, y, c0, c1, out):
        """the same from torch CUDA tensors, raw device addresses or None"""
        return cls(*(None if p is None else _dptr(p) for p in (y, c0, c1, out)))


class Yuv420Packed422FrameDev(C.Structure):
    """mi_yuv420_packed422_frame_dev: one frame of a mi_*_yuv420_to_packed422_frames_dev list, its three input plane addresses and its
    packed frame's address (device pointers).  c0 is always the U plane and c1 the V plane (a YV12 frame exchanges the two); an
    INTERLEAVED list has its UV plane in c0 and its c1 is ignored (None); with UV_FILL128 c0 and c1 are ignored (None)."""
    _fields_ = [("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p), ("out", C.c_void_p)]

    @classmethod
    def of(cls, y, c0, c1, out):
        """the same from torch CUDA tensors, raw device addresses or None"""
        return cls(*(None if p is None else _dptr(p) for p in (y, c0, c1, out)))


class BgrYuv420FrameDev(C.Structure):
    """mi_bgr_yuv420_frame_dev: one frame of a mi_*_bgr_to_yuv420_frames_dev list, its image address and its three output plane
    addresses (device pointers).  c0 is always the U plane and c1 the V plane (a YV12 frame exchanges the two); an INTERLEAVED list has
    its UV plane in c0 and its c1 is ignored (None)."""
    _fields_ = [("in_", C.c_void_p), ("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p)]

    @classmethod
    def of(cls, in_, y, c0, c1):
        """the same from torch CUDA tensors, raw device addresses or None"""
        return cls(*(None if p is None else _dptr(p) for p in (in_, y, c0, c1)))


_YUV420_FMTS = {"nv12": Yuv420Planes.nv12, "i420": Yuv420Planes.i420, "yv12": Yuv420Planes.yv12}


class MiError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        self.status = status
        super().__init__(f"{what}: {status_str(status)}" + (f" ({detail})" if detail else ""))


_lib = None
_test_lib = None


def lib_path() -> Path:
    return Path(os.environ.get("MI_LUMAEQ_LIB", str(_LIB_PATH)))


def lib() -> C.CDLL:
    """Load libmi_lumaeq.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        _lib = _load(lib_path())
    return _lib


def test_lib() -> C.CDLL:
    """libmi_lumaeq_test.so: the product sources built with the test hooks (options "fused_fault_inject", "fused_timeout_us",
    "hip_fail_after").  Tests pass it to Context(device, lib=test_lib()); nothing else loads it."""
    global _test_lib
    if _test_lib is None:
        _test_lib = _load(Path(os.environ.get("MI_LUMAEQ_TEST_LIB", str(_TEST_LIB_PATH))))
    return _test_lib


def _load(p: Path) -> C.CDLL:
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C opencv-opencl_amd/csrc` (there is no CPU fallback)")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).
    # If the library were loaded first it would bring in /opt/rocm's runtime and a later `import torch`
    # would start a second one (its devices then look absent to us).  Importing torch first makes the
    # dynamic loader resolve our NEEDED libamdhip64.so.7 to the copy torch already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(p))
    vp, sz, i, d, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int64
    L.mi_ctx_create.argtypes = [i, C.POINTER(vp)]
    L.mi_ctx_destroy.argtypes = [vp]; L.mi_ctx_destroy.restype = None
    L.mi_ctx_device.argtypes = [vp]
    L.mi_ctx_last_hip_error.argtypes = [vp]
    L.mi_ctx_last_error_msg.argtypes = [vp]; L.mi_ctx_last_error_msg.restype = C.c_char_p
    L.mi_status_str.argtypes = [i]; L.mi_status_str.restype = C.c_char_p
    L.mi_version.restype = C.c_char_p
    L.mi_kernel_name.argtypes = [i]; L.mi_kernel_name.restype = C.c_char_p
    L.mi_equalize_hist_u8.argtypes = [vp, vp, sz, vp, sz, i, i]
    L.mi_clahe_u8.argtypes = [vp, vp, sz, vp, sz, i, i, d, i, i]
    L.mi_equalize_hist_nv12.argtypes = [vp, vp, vp, i, i, i]
    L.mi_clahe_nv12.argtypes = [vp, vp, vp, i, i, i, d, i, i]
    L.mi_equalize_hist_u8_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, vp]
    L.mi_clahe_u8_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_nv12_batch_dev.argtypes = [vp, vp, vp, i, i, i, i, vp]
    L.mi_clahe_nv12_batch_dev.argtypes = [vp, vp, vp, i, i, i, i, d, i, i, vp]
    L.mi_hist_u8_batch_dev.argtypes = [vp, vp, sz, sz, i, i, i, vp, vp]
    L.mi_equalize_lut_batch_dev.argtypes = [vp, vp, i64, i, vp, vp]
    L.mi_lut_apply_u8_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, vp, vp]
    L.mi_clahe_tile_luts_batch_dev.argtypes = [vp, vp, sz, sz, i, i, i, d, i, i, vp, vp]
    L.mi_cvt_color_u8c3.argtypes = [vp, vp, sz, vp, sz, i, i, i]
    L.mi_cvt_color_u8c3_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, vp]
    L.mi_bgr_luma_op_u8c3.argtypes = [vp, vp, sz, vp, sz, i, i, i, d, i, i]
    L.mi_bgr_luma_op_u8c3_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, d, i, i, vp]
    L.mi_nv12_bgr_equalize.argtypes = [vp, vp, vp, i, i]
    L.mi_cvt_color_420_u8.argtypes = [vp, vp, sz, vp, sz, i, i, i]
    L.mi_cvt_color_420_u8_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, vp]
    L.mi_nv12_bgr_equalize_batch_dev.argtypes = [vp, vp, sz, vp, sz, i, i, i, vp]
    L.mi_clahe_u16.argtypes = [vp, vp, sz, vp, sz, i, i, d, i, i]
    L.mi_clahe_u16_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, d, i, i, vp]
    L.mi_clahe_p010.argtypes = [vp, vp, vp, i, i, i, d, i, i]
    L.mi_clahe_p010_batch_dev.argtypes = [vp, vp, vp, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_nv12_frames_dev.argtypes = [vp, C.POINTER(Nv12FrameDev), i, i, i, sz, sz, sz, sz, i, vp]
    L.mi_clahe_nv12_frames_dev.argtypes = [vp, C.POINTER(Nv12FrameDev), i, i, i, sz, sz, sz, sz, i, d, i, i, vp]
    L.mi_clahe_p010_frames_dev.argtypes = [vp, C.POINTER(Nv12FrameDev), i, i, i, sz, sz, sz, sz, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, vp]
    L.mi_clahe_packed422_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422.argtypes = [vp, vp, sz, vp, sz, i, i, i, i]
    L.mi_clahe_packed422.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, d, i, i]
    L.mi_equalize_hist_packed422_frames_dev.argtypes = [vp, C.POINTER(Packed422FrameDev), i, i, i, sz, sz, i, i, vp]
    L.mi_clahe_packed422_frames_dev.argtypes = [vp, C.POINTER(Packed422FrameDev), i, i, i, sz, sz, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_nv12_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, sz, i, i, i, i, i, vp]
    L.mi_clahe_packed422_to_nv12_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, sz, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_nv12_frames_dev.argtypes = [vp, C.POINTER(Packed422Nv12FrameDev), i, i, i, sz, sz, sz, i, i, vp]
    L.mi_clahe_packed422_to_nv12_frames_dev.argtypes = [vp, C.POINTER(Packed422Nv12FrameDev), i, i, i, sz, sz, sz, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_nv12.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, i, i]
    L.mi_clahe_packed422_to_nv12.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, i, i, d, i, i]
    L.mi_equalize_hist_packed422_to_bgr_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, vp]
    L.mi_clahe_packed422_to_bgr_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_bgr.argtypes = [vp, vp, sz, vp, sz, i, i, i, i]
    L.mi_clahe_packed422_to_bgr.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, d, i, i]
    L.mi_equalize_hist_packed422_to_bgr_frames_dev.argtypes = [vp, C.POINTER(Packed422BgrFrameDev), i, i, i, sz, sz, i, i, vp]
    L.mi_clahe_packed422_to_bgr_frames_dev.argtypes = [vp, C.POINTER(Packed422BgrFrameDev), i, i, i, sz, sz, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_bgra_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, vp]
    L.mi_clahe_packed422_to_bgra_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_bgra.argtypes = [vp, vp, sz, vp, sz, i, i, i, i]
    L.mi_clahe_packed422_to_bgra.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, d, i, i]
    L.mi_equalize_hist_packed422_to_bgra_frames_dev.argtypes = [vp, C.POINTER(Packed422BgrFrameDev), i, i, i, sz, sz, i, i, vp]
    L.mi_clahe_packed422_to_bgra_frames_dev.argtypes = [vp, C.POINTER(Packed422BgrFrameDev), i, i, i, sz, sz, i, i, d, i, i, vp]
    L.mi_equalize_hist_nv12_to_bgr_batch_dev.argtypes = [vp, vp, sz, vp, sz, sz, vp, sz, sz, i, i, i, i, vp]
    L.mi_clahe_nv12_to_bgr_batch_dev.argtypes = [vp, vp, sz, vp, sz, sz, vp, sz, sz, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_nv12_to_bgr.argtypes = [vp, vp, vp, sz, i, i, i]
    L.mi_clahe_nv12_to_bgr.argtypes = [vp, vp, vp, sz, i, i, i, d, i, i]
    L.mi_equalize_hist_nv12_to_bgr_frames_dev.argtypes = [vp, C.POINTER(Nv12BgrFrameDev), i, i, i, sz, sz, sz, i, vp]
    L.mi_clahe_nv12_to_bgr_frames_dev.argtypes = [vp, C.POINTER(Nv12BgrFrameDev), i, i, i, sz, sz, sz, i, d, i, i, vp]
    L.mi_equalize_hist_bgr_to_nv12_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, sz, i, i, i, i, i, vp]
    L.mi_clahe_bgr_to_nv12_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, sz, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgr_to_nv12.argtypes = [vp, vp, sz, vp, i, i, i, i]
    L.mi_clahe_bgr_to_nv12.argtypes = [vp, vp, sz, vp, i, i, i, i, d, i, i]
    L.mi_equalize_hist_bgr_to_nv12_frames_dev.argtypes = [vp, C.POINTER(BgrNv12FrameDev), i, i, i, sz, sz, sz, i, i, vp]
    L.mi_clahe_bgr_to_nv12_frames_dev.argtypes = [vp, C.POINTER(BgrNv12FrameDev), i, i, i, sz, sz, sz, i, i, d, i, i, vp]
    yp = C.POINTER(Yuv420Planes)
    L.mi_equalize_hist_yuv420_batch_dev.argtypes = [vp, yp, yp, i, i, i, i, vp]
    L.mi_clahe_yuv420_batch_dev.argtypes = [vp, yp, yp, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420.argtypes = [vp, yp, yp, i, i, i]
    L.mi_clahe_yuv420.argtypes = [vp, yp, yp, i, i, i, d, i, i]
    L.mi_equalize_hist_packed422_to_yuv420_batch_dev.argtypes = [vp, vp, sz, sz, yp, i, i, i, i, i, vp]
    L.mi_clahe_packed422_to_yuv420_batch_dev.argtypes = [vp, vp, sz, sz, yp, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_packed422_to_yuv420.argtypes = [vp, vp, sz, yp, i, i, i, i]
    L.mi_clahe_packed422_to_yuv420.argtypes = [vp, vp, sz, yp, i, i, i, i, d, i, i]
    L.mi_equalize_hist_packed422_to_yuv420_frames_dev.argtypes = [vp, C.POINTER(BgrYuv420FrameDev), i, i, i, sz, sz, sz, i, i, i, vp]
    L.mi_clahe_packed422_to_yuv420_frames_dev.argtypes = [vp, C.POINTER(BgrYuv420FrameDev), i, i, i, sz, sz, sz, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_frames_dev.argtypes = [vp, C.POINTER(Yuv420FrameDev), i, i, i, sz, sz, i, sz, sz, i, i, vp]
    L.mi_clahe_yuv420_frames_dev.argtypes = [vp, C.POINTER(Yuv420FrameDev), i, i, i, sz, sz, i, sz, sz, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_bgr_batch_dev.argtypes = [vp, yp, vp, sz, sz, i, i, i, i, vp]
    L.mi_clahe_yuv420_to_bgr_batch_dev.argtypes = [vp, yp, vp, sz, sz, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_bgr_frames_dev.argtypes = [vp, C.POINTER(Yuv420BgrFrameDev), i, i, i, sz, sz, i, sz, i, vp]
    L.mi_clahe_yuv420_to_bgr_frames_dev.argtypes = [vp, C.POINTER(Yuv420BgrFrameDev), i, i, i, sz, sz, i, sz, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_bgr.argtypes = [vp, yp, vp, sz, i, i, i]
    L.mi_clahe_yuv420_to_bgr.argtypes = [vp, yp, vp, sz, i, i, i, d, i, i]
    L.mi_equalize_hist_bgr_to_yuv420_batch_dev.argtypes = [vp, vp, sz, sz, yp, i, i, i, i, i, vp]
    L.mi_clahe_bgr_to_yuv420_batch_dev.argtypes = [vp, vp, sz, sz, yp, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgr_to_yuv420.argtypes = [vp, vp, sz, yp, i, i, i, i]
    L.mi_clahe_bgr_to_yuv420.argtypes = [vp, vp, sz, yp, i, i, i, i, d, i, i]
    L.mi_equalize_hist_bgr_to_yuv420_frames_dev.argtypes = [vp, C.POINTER(BgrYuv420FrameDev), i, i, i, sz, sz, sz, i, i, i, vp]
    L.mi_clahe_bgr_to_yuv420_frames_dev.argtypes = [vp, C.POINTER(BgrYuv420FrameDev), i, i, i, sz, sz, sz, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgra_to_yuv420_batch_dev.argtypes = [vp, vp, sz, sz, yp, i, i, i, i, i, vp]
    L.mi_clahe_bgra_to_yuv420_batch_dev.argtypes = [vp, vp, sz, sz, yp, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgra_to_yuv420.argtypes = [vp, vp, sz, yp, i, i, i, i]
    L.mi_clahe_bgra_to_yuv420.argtypes = [vp, vp, sz, yp, i, i, i, i, d, i, i]
    L.mi_equalize_hist_bgra_to_yuv420_frames_dev.argtypes = [vp, C.POINTER(BgrYuv420FrameDev), i, i, i, sz, sz, sz, i, i, i, vp]
    L.mi_clahe_bgra_to_yuv420_frames_dev.argtypes = [vp, C.POINTER(BgrYuv420FrameDev), i, i, i, sz, sz, sz, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_bgra_batch_dev.argtypes = [vp, yp, vp, sz, sz, i, i, i, i, vp]
    L.mi_clahe_yuv420_to_bgra_batch_dev.argtypes = [vp, yp, vp, sz, sz, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_bgra.argtypes = [vp, yp, vp, sz, i, i, i]
    L.mi_clahe_yuv420_to_bgra.argtypes = [vp, yp, vp, sz, i, i, i, d, i, i]
    L.mi_equalize_hist_yuv420_to_bgra_frames_dev.argtypes = [vp, C.POINTER(Yuv420BgrFrameDev), i, i, i, sz, sz, i, sz, i, vp]
    L.mi_clahe_yuv420_to_bgra_frames_dev.argtypes = [vp, C.POINTER(Yuv420BgrFrameDev), i, i, i, sz, sz, i, sz, i, d, i, i, vp]
    L.mi_equalize_hist_bgr_to_packed422_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, i, vp]
    L.mi_clahe_bgr_to_packed422_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgr_to_packed422.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, i]
    L.mi_clahe_bgr_to_packed422.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, i, d, i, i]
    L.mi_equalize_hist_bgr_to_packed422_frames_dev.argtypes = [vp, C.POINTER(BgrPacked422FrameDev), i, i, i, sz, sz, i, i, i, vp]
    L.mi_clahe_bgr_to_packed422_frames_dev.argtypes = [vp, C.POINTER(BgrPacked422FrameDev), i, i, i, sz, sz, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgra_to_packed422_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, i, vp]
    L.mi_clahe_bgra_to_packed422_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_bgra_to_packed422.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, i]
    L.mi_clahe_bgra_to_packed422.argtypes = [vp, vp, sz, vp, sz, i, i, i, i, i, d, i, i]
    L.mi_equalize_hist_bgra_to_packed422_frames_dev.argtypes = [vp, C.POINTER(BgrPacked422FrameDev), i, i, i, sz, sz, i, i, i, vp]
    L.mi_clahe_bgra_to_packed422_frames_dev.argtypes = [vp, C.POINTER(BgrPacked422FrameDev), i, i, i, sz, sz, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_packed422_batch_dev.argtypes = [vp, yp, vp, sz, sz, i, i, i, i, i, vp]
    L.mi_clahe_yuv420_to_packed422_batch_dev.argtypes = [vp, yp, vp, sz, sz, i, i, i, i, i, d, i, i, vp]
    L.mi_equalize_hist_yuv420_to_packed422.argtypes = [vp, yp, vp, sz, i, i, i, i]
    L.mi_clahe_yuv420_to_packed422.argtypes = [vp, yp, vp, sz, i, i, i, i, d, i, i]
    L.mi_equalize_hist_yuv420_to_packed422_frames_dev.argtypes = [vp, C.POINTER(Yuv420Packed422FrameDev), i, i, i, sz, sz, i, sz, i, i, vp]
    L.mi_clahe_yuv420_to_packed422_frames_dev.argtypes = [vp, C.POINTER(Yuv420Packed422FrameDev), i, i, i, sz, sz, i, sz, i, i, d, i, i, vp]
    L.mi_analyze_diff_u8.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, i, vp]
    L.mi_analyze_diff_u8_batch_dev.argtypes = [vp, vp, sz, sz, vp, sz, sz, vp, sz, sz, i, i, i, i, vp, vp]
    L.mi_host_register.argtypes = [vp, sz]
    L.mi_host_unregister.argtypes = [vp]
    L.mi_ctx_synchronize.argtypes = [vp, vp]
    L.mi_ctx_set_option.argtypes = [vp, C.c_char_p, i]
    L.mi_ctx_get_stat.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]
    L.mi_pipe_create.argtypes = [vp, C.POINTER(_PipeConfig), C.POINTER(vp)]
    L.mi_pipe_destroy.argtypes = [vp]; L.mi_pipe_destroy.restype = None
    L.mi_pipe_submit.argtypes = [vp, vp, vp, C.c_uint64]
    L.mi_pipe_wait.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(vp)]
    L.mi_pipe_pending.argtypes = [vp]
    L.mi_pipe_depth.argtypes = [vp]
    L.mi_ctx_set_profiling.argtypes = [vp, i]
    L.mi_ctx_profile_read.argtypes = [vp, C.POINTER(_Profile), i]
    L.mi_device_pci_bus_id.argtypes = [i, C.c_char_p, sz]
    L.mi_thread_bind_near_device.argtypes = [i, C.POINTER(_NumaBinding)]
    return L


def status_str(s: int) -> str:
    try:
        return lib().mi_status_str(int(s)).decode()
    except Exception:
        return f"status {s}"


def version() -> str:
    return lib().mi_version().decode()


def device_count() -> int:
    return int(lib().mi_device_count())


def device_pci_bus_id(device: int) -> str:
    buf = C.create_string_buffer(64)
    rc = lib().mi_device_pci_bus_id(int(device), buf, 64)
    if rc != 0:
        raise MiError(rc, "mi_device_pci_bus_id")
    return buf.value.decode()


def bind_thread_near_device(device: int) -> dict:
    """Bind the CALLING thread to the CPUs of the device's NUMA node (mi_thread_bind_near_device): call before Context(device).
    Returns {"node", "cpus", "why"}; never raises for a platform that reports no node."""
    b = _NumaBinding()
    rc = lib().mi_thread_bind_near_device(int(device), C.byref(b))
    if rc != 0:
        raise MiError(rc, "mi_thread_bind_near_device", b.why.decode(errors="replace"))
    return {"node": int(b.node), "cpus": int(b.cpus), "why": b.why.decode(errors="replace")}


def host_register(a: np.ndarray) -> None:
    """Pin a caller-owned numpy buffer (mi_host_register); keep `a` alive until host_unregister(a)."""
    rc = lib().mi_host_register(a.ctypes.data, a.nbytes)
    if rc != 0:
        raise MiError(rc, "mi_host_register")


def host_unregister(a: np.ndarray) -> None:
    rc = lib().mi_host_unregister(a.ctypes.data)
    if rc != 0:
        raise MiError(rc, "mi_host_unregister")


def _host2d(a: np.ndarray, name: str) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2:
        raise MiError(2, name, "expected a 2-D uint8 ndarray (CV_8UC1)")
    if a.size and a.strides[1] != 1:
        raise MiError(1, name, "pixel stride must be 1")
    return a


def _step(a: np.ndarray) -> int:
    return int(a.strides[0]) if a.shape[0] > 1 else max(int(a.strides[0]), a.shape[1])


def _dptr(t) -> int:
    """Device pointer of a torch CUDA tensor (or a raw int)."""
    if isinstance(t, int):
        return t
    if not t.is_cuda:
        raise MiError(1, "device pointer", "tensor is not on a HIP device")
    return int(t.data_ptr())


def _plane_pitch(planes, given, width: int, what: str) -> int:
    """Row pitch in bytes of a list of planes: `given`, else the row stride shared by the 2-D tensors among them, else `width`."""
    if given is not None:
        return int(given)
    strides = {int(p.stride(-2)) * p.element_size() for p in planes if not isinstance(p, int) and p is not None and p.dim() >= 2}
    if len(strides) > 1:
        raise MiError(1, what, f"the planes have different row pitches {sorted(strides)}: one call takes one pitch")
    return strides.pop() if strides else int(width)


def _frame_list(inputs, outputs, width, pitches, what):
    """inputs / outputs: sequences of (y, uv) pairs (torch CUDA tensors, raw device addresses, uv may be None); outputs None =
    in place.  Returns the mi_nv12_frame_dev array and the four pitches (y_in, uv_in, y_out, uv_out)."""
    inputs = list(inputs)
    outputs = inputs if outputs is None else list(outputs)
    if len(outputs) != len(inputs):
        raise MiError(1, what, f"{len(inputs)} inputs but {len(outputs)} outputs")
    y_in, uv_in = [f[0] for f in inputs], [f[1] for f in inputs]
    y_out, uv_out = [f[0] for f in outputs], [f[1] for f in outputs]
    p = [_plane_pitch(pl, g, width, what) for pl, g in zip((y_in, uv_in, y_out, uv_out), pitches)]
    arr = (Nv12FrameDev * max(1, len(inputs)))()
    for k in range(len(inputs)):
        arr[k] = Nv12FrameDev(_dptr(y_in[k]), None if uv_in[k] is None else _dptr(uv_in[k]), _dptr(y_out[k]),
                               None if uv_out[k] is None else _dptr(uv_out[k]))
    return arr, len(inputs), p


def _packed422_list(inputs, outputs, width, in_pitch, out_pitch, what):
    """inputs / outputs: sequences of packed frames (torch CUDA tensors or raw device addresses); outputs None = in place.  Returns
    the mi_packed422_frame_dev array, its length and the two pitches (given, else the 2-D tensors' row stride, else 2 * width)."""
    inputs = list(inputs)
    outputs = inputs if outputs is None else list(outputs)
    if len(outputs) != len(inputs):
        raise MiError(1, what, f"{len(inputs)} inputs but {len(outputs)} outputs")
    ip = _plane_pitch(inputs, in_pitch, 2 * int(width), what)
    op = _plane_pitch(outputs, out_pitch, 2 * int(width), what)
    arr = (Packed422FrameDev * max(1, len(inputs)))()
    for k in range(len(inputs)):
        arr[k] = Packed422FrameDev(_dptr(inputs[k]), _dptr(outputs[k]))
    return arr, len(inputs), ip, op


def _packed422_nv12_list(inputs, y_outputs, uv_outputs, width, in_pitch, y_pitch, uv_pitch, what):
    """inputs / y_outputs / uv_outputs: sequences of equal length (torch CUDA tensors or raw device addresses).  Returns the
    mi_packed422_nv12_frame_dev array, its length and the three pitches (given, else the 2-D tensors' row stride, else 2 * width for
    the input and width for the planes)."""
    inputs, y_outputs, uv_outputs = list(inputs), list(y_outputs), list(uv_outputs)
    if not (len(inputs) == len(y_outputs) == len(uv_outputs)):
        raise MiError(1, what, f"{len(inputs)} inputs but {len(y_outputs)} Y and {len(uv_outputs)} UV outputs")
    ip = _plane_pitch(inputs, in_pitch, 2 * int(width), what)
    yp = _plane_pitch(y_outputs, y_pitch, int(width), what)
    up = _plane_pitch(uv_outputs, uv_pitch, int(width), what)
    arr = (Packed422Nv12FrameDev * max(1, len(inputs)))()
    for k in range(len(inputs)):
        arr[k] = Packed422Nv12FrameDev(_dptr(inputs[k]), _dptr(y_outputs[k]), _dptr(uv_outputs[k]))
    return arr, len(inputs), ip, yp, up


def _packed422_bgr_list(inputs, outs, width, in_pitch, out_pitch, what, px=3):
    """inputs / outs: sequences of equal length (torch CUDA tensors or raw device addresses).  Returns the mi_packed422_bgr_frame_dev
    array, its length and the two pitches (given, else the row stride of the tensors -- H x pitch frames, H x 3W or H x W x 3 images --
    else 2 * width for the frames and 3 * width for the images).  px = 4: four-channel images (H x 4W or H x W x 4, 4 * width)."""
    inputs, outs = list(inputs), list(outs)
    if len(inputs) != len(outs):
        raise MiError(1, what, f"{len(inputs)} inputs but {len(outs)} images")
    ip = _plane_pitch(inputs, in_pitch, 2 * int(width), what)
    # an H x W x 3 image's rows are its first axis: seen as H x 3W for the pitch
    rows = [o if isinstance(o, int) or o is None or o.dim() != 3 else o[:, :, 0] for o in outs]
    op = int(out_pitch) if out_pitch is not None else _plane_pitch(rows, None, px * int(width), what)
    arr = (Packed422BgrFrameDev * max(1, len(inputs)))()
    for k in range(len(inputs)):
        arr[k] = Packed422BgrFrameDev(_dptr(inputs[k]), _dptr(outs[k]))
    return arr, len(inputs), ip, op


def _nv12_bgr_list(ys, uvs, outs, width, y_pitch, uv_pitch, out_pitch, what):
    """ys / uvs / outs: sequences of equal length (torch CUDA tensors or raw device addresses).  Returns the mi_nv12_bgr_frame_dev
    array, its length and the three pitches (given, else the row stride of the tensors -- H x W planes, H x 3W or H x W x 3 images --
    else width for the planes and 3 * width for the images)."""
    ys, uvs, outs = list(ys), list(uvs), list(outs)
    if not (len(ys) == len(uvs) == len(outs)):
        raise MiError(1, what, f"{len(ys)} Y planes but {len(uvs)} UV planes and {len(outs)} images")
    yp = _plane_pitch(ys, y_pitch, int(width), what)
    up = _plane_pitch(uvs, uv_pitch, int(width), what)
    # an H x W x 3 image's rows are its first axis: seen as H x 3W for the pitch
    rows = [o if isinstance(o, int) or o is None or o.dim() != 3 else o[:, :, 0] for o in outs]
    op = int(out_pitch) if out_pitch is not None else _plane_pitch(rows, None, 3 * int(width), what)
    arr = (Nv12BgrFrameDev * max(1, len(ys)))()
    for k in range(len(ys)):
        arr[k] = Nv12BgrFrameDev(_dptr(ys[k]), _dptr(uvs[k]), _dptr(outs[k]))
    return arr, len(ys), yp, up, op


def _bgr_nv12_list(ins, ys, uvs, width, in_pitch, y_pitch, uv_pitch, what):
    """ins / ys / uvs: sequences of equal length (torch CUDA tensors or raw device addresses).  Returns the mi_bgr_nv12_frame_dev
    array, its length and the three pitches (given, else the row stride of the tensors -- H x 3W or H x W x 3 images, H x W planes --
    else 3 * width for the images and width for the planes)."""
    ins, ys, uvs = list(ins), list(ys), list(uvs)
    if not (len(ins) == len(ys) == len(uvs)):
        raise MiError(1, what, f"{len(ins)} images but {len(ys)} Y planes and {len(uvs)} UV planes")
    # an H x W x 3 image's rows are its first axis: seen as H x 3W for the pitch
    rows = [o if isinstance(o, int) or o is None or o.dim() != 3 else o[:, :, 0] for o in ins]
    ip = int(in_pitch) if in_pitch is not None else _plane_pitch(rows, None, 3 * int(width), what)
    yp = _plane_pitch(ys, y_pitch, int(width), what)
    up = _plane_pitch(uvs, uv_pitch, int(width), what)
    arr = (BgrNv12FrameDev * max(1, len(ins)))()
    for k in range(len(ins)):
        arr[k] = BgrNv12FrameDev(_dptr(ins[k]), _dptr(ys[k]), _dptr(uvs[k]))
    return arr, len(ins), ip, yp, up


def _bgr_packed422_list(ins, outs, width, in_pitch, out_pitch, what, ch=3):
    """ins / outs: sequences of equal length (torch CUDA tensors or raw device addresses).  Returns the mi_bgr_packed422_frame_dev
    array, its length and the two pitches (given, else the row stride of the tensors -- H x 3W or H x W x 3 images, H x pitch frames --
    else 3 * width for the images and 2 * width for the frames).  ch = 4: four-channel images (H x 4W or H x W x 4, 4 * width)."""
    ins, outs = list(ins), list(outs)
    if len(ins) != len(outs):
        raise MiError(1, what, f"{len(ins)} images but {len(outs)} frames")
    # an H x W x 3 image's rows are its first axis: seen as H x 3W for the pitch
    rows = [o if isinstance(o, int) or o is None or o.dim() != 3 else o[:, :, 0] for o in ins]
    ip = int(in_pitch) if in_pitch is not None else _plane_pitch(rows, None, ch * int(width), what)
    op = _plane_pitch(outs, out_pitch, 2 * int(width), what)
    arr = (BgrPacked422FrameDev * max(1, len(ins)))()
    for k in range(len(ins)):
        arr[k] = BgrPacked422FrameDev(_dptr(ins[k]), _dptr(outs[k]))
    return arr, len(ins), ip, op


_live_contexts: "weakref.WeakSet[Context]" = weakref.WeakSet()


def _close_live_contexts() -> None:
    """atexit: destroy every context while the HIP runtime is still up.  Destroying one from ``__del__`` during
    interpreter finalisation can run after the runtime's own teardown (hipFree on a dead runtime)."""
    for c in list(_live_contexts):
        c.close()


atexit.register(_close_live_contexts)


class Context:
    """mi_ctx wrapper.  One per (thread x device), like the reference's per-worker OpenCL objects."""

    def __init__(self, device: int = 0, lib: "C.CDLL | None" = None):
        self._L = lib if lib is not None else globals()["lib"]()
        self._h = C.c_void_p()
        rc = self._L.mi_ctx_create(int(device), C.byref(self._h))
        if rc != 0:
            raise MiError(rc, f"mi_ctx_create(device={device})")
        _live_contexts.add(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            h, self._h = self._h, None
            self._L.mi_ctx_destroy(h)

    def __del__(self):
        # Never call into the library while the interpreter is finalising: the atexit hook has already closed
        # every live context, and anything that slipped past it is leaked rather than freed on a dead runtime.
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc: int, what: str):
        if rc != 0:
            raise MiError(rc, what, self._L.mi_ctx_last_error_msg(self._h).decode())

    # ---- host-pointer forms (numpy = stand-in for cv::Mat memory) ----
    def equalize_hist(self, src: np.ndarray, dst: np.ndarray | None = None) -> np.ndarray:
        src = _host2d(src, "equalize_hist")
        if dst is None or dst.shape != src.shape or dst.dtype != np.uint8:
            dst = np.empty(src.shape, np.uint8)      # Mat::create semantics: reallocate only on mismatch
        _host2d(dst, "equalize_hist")
        h, w = src.shape
        self._chk(self._L.mi_equalize_hist_u8(self._h, src.ctypes.data, _step(src), dst.ctypes.data, _step(dst), w, h),
                  "mi_equalize_hist_u8")
        return dst

    def clahe(self, src: np.ndarray, clip_limit: float = 40.0, tiles_x: int = 8, tiles_y: int = 8,
              dst: np.ndarray | None = None) -> np.ndarray:
        src = _host2d(src, "clahe")
        if dst is None or dst.shape != src.shape or dst.dtype != np.uint8:
            dst = np.empty(src.shape, np.uint8)
        h, w = src.shape
        self._chk(self._L.mi_clahe_u8(self._h, src.ctypes.data, _step(src), dst.ctypes.data, _step(dst), w, h,
                                    float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_u8")
        return dst

    def equalize_hist_nv12(self, frame: np.ndarray, width: int, height: int, uv_mode: int = UV_FILL128,
                           out: np.ndarray | None = None) -> np.ndarray:
        n = width * height + (width * height) // 2
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        if frame.size < n:
            raise MiError(1, "equalize_hist_nv12", "frame smaller than W*H*3/2")
        if out is None:
            out = np.empty(n, np.uint8)
        self._chk(self._L.mi_equalize_hist_nv12(self._h, frame.ctypes.data, out.ctypes.data, width, height, uv_mode),
                  "mi_equalize_hist_nv12")
        return out

    def clahe_nv12(self, frame: np.ndarray, width: int, height: int, uv_mode: int = UV_FILL128,
                   clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8,
                   out: np.ndarray | None = None) -> np.ndarray:
        n = width * height + (width * height) // 2
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        if frame.size < n:
            raise MiError(1, "clahe_nv12", "frame smaller than W*H*3/2")
        if out is None:
            out = np.empty(n, np.uint8)
        self._chk(self._L.mi_clahe_nv12(self._h, frame.ctypes.data, out.ctypes.data, width, height, uv_mode,
                                      float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_nv12")
        return out

    # ---- device-resident batched forms (torch tensors only carry the memory) ----
    def equalize_hist_batch_dev(self, src, dst, width, height, n_frames, src_step=None, src_frame=None,
                                dst_step=None, dst_frame=None, stream=0):
        ss = width if src_step is None else src_step
        ds = width if dst_step is None else dst_step
        sf = ss * height if src_frame is None else src_frame
        df = ds * height if dst_frame is None else dst_frame
        self._chk(self._L.mi_equalize_hist_u8_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df,
                                                      width, height, n_frames, stream), "mi_equalize_hist_u8_batch_dev")

    def clahe_batch_dev(self, src, dst, width, height, n_frames, clip_limit, tiles_x, tiles_y,
                        src_step=None, src_frame=None, dst_step=None, dst_frame=None, stream=0):
        ss = width if src_step is None else src_step
        ds = width if dst_step is None else dst_step
        sf = ss * height if src_frame is None else src_frame
        df = ds * height if dst_frame is None else dst_frame
        self._chk(self._L.mi_clahe_u8_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df, width, height,
                                              n_frames, float(clip_limit), tiles_x, tiles_y, stream),
                  "mi_clahe_u8_batch_dev")

    def equalize_hist_nv12_batch_dev(self, d_in, d_out, width, height, n_frames, uv_mode=UV_FILL128, stream=0):
        self._chk(self._L.mi_equalize_hist_nv12_batch_dev(self._h, _dptr(d_in), _dptr(d_out), width, height,
                                                        n_frames, uv_mode, stream), "mi_equalize_hist_nv12_batch_dev")

    def clahe_nv12_batch_dev(self, d_in, d_out, width, height, n_frames, uv_mode=UV_FILL128,
                             clip_limit=2.0, tiles_x=8, tiles_y=8, stream=0):
        self._chk(self._L.mi_clahe_nv12_batch_dev(self._h, _dptr(d_in), _dptr(d_out), width, height, n_frames,
                                                uv_mode, float(clip_limit), tiles_x, tiles_y, stream),
                  "mi_clahe_nv12_batch_dev")

    # ---- NV12 frames as a list of pitched planes (decoder surfaces, tensor lists) ----
    def equalize_hist_nv12_frames(self, inputs, outputs, width, height, uv_mode=UV_FILL128, y_in_pitch=None, uv_in_pitch=None,
                                  y_out_pitch=None, uv_out_pitch=None, stream=0):
        """mi_equalize_hist_nv12_frames_dev.  inputs / outputs: lists of (y, uv) planes -- torch CUDA tensors or raw device
        addresses; uv of an input may be None with UV_FILL128; outputs=None processes every frame in place.  A pitch left at None
        is the row stride of the 2-D uint8 tensors given for that plane (all frames must agree), or the width."""
        arr, n, p = _frame_list(inputs, outputs, width, (y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch), "equalize_hist_nv12_frames")
        self._chk(self._L.mi_equalize_hist_nv12_frames_dev(self._h, arr, n, int(width), int(height), p[0], p[1], p[2], p[3],
                                                         int(uv_mode), stream), "mi_equalize_hist_nv12_frames_dev")

    def clahe_nv12_frames(self, inputs, outputs, width, height, uv_mode=UV_FILL128, clip_limit=2.0, tiles_x=8, tiles_y=8,
                          y_in_pitch=None, uv_in_pitch=None, y_out_pitch=None, uv_out_pitch=None, stream=0):
        """mi_clahe_nv12_frames_dev; arguments as equalize_hist_nv12_frames, plus the CLAHE parameters."""
        arr, n, p = _frame_list(inputs, outputs, width, (y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch), "clahe_nv12_frames")
        self._chk(self._L.mi_clahe_nv12_frames_dev(self._h, arr, n, int(width), int(height), p[0], p[1], p[2], p[3], int(uv_mode),
                                                 float(clip_limit), int(tiles_x), int(tiles_y), stream), "mi_clahe_nv12_frames_dev")

    # ---- the reference's own check: cv::absdiff + xf::cv::analyzeDiff (1frameMeasure.cpp:91-100) ----
    def analyze_diff(self, a: np.ndarray, b: np.ndarray | None = None, threshold: int = 1, want_diff: bool = False):
        """Host planes.  Returns {"above", "max_diff", "min_diff", "total", "err_per"} (+ "diff" = |a - b| when asked);
        b = None: `a` already is a difference image."""
        a = _host2d(a, "analyze_diff")
        h, w = a.shape
        if b is not None:
            b = _host2d(b, "analyze_diff")
            if b.shape != a.shape:
                raise ValueError("analyze_diff: planes differ in size")
        diff = np.empty((h, w), np.uint8) if want_diff else None
        out = (C.c_uint32 * 4)()
        self._chk(self._L.mi_analyze_diff_u8(self._h, a.ctypes.data, _step(a), b.ctypes.data if b is not None else None,
                                           _step(b) if b is not None else 0, diff.ctypes.data if want_diff else None, w, w, h,
                                           int(threshold), C.cast(out, C.c_void_p)), "mi_analyze_diff_u8")
        r = {"above": int(out[0]), "max_diff": int(out[1]), "min_diff": int(out[2]), "total": int(out[3]),
             "err_per": 100.0 * out[0] / out[3] if out[3] else 0.0}
        if want_diff:
            r["diff"] = diff
        return r

    def analyze_diff_batch_dev(self, a, b, width, height, n_frames, d_stats, threshold=1, diff=None, a_step=None, a_frame=None,
                               b_step=None, b_frame=None, diff_step=None, diff_frame=None, stream=0):
        """Device planes; d_stats = n_frames x 4 uint32 (above, max, min, total) in device memory."""
        as_ = width if a_step is None else a_step
        bs_ = width if b_step is None else b_step
        ds_ = width if diff_step is None else diff_step
        af = as_ * height if a_frame is None else a_frame
        bf = bs_ * height if b_frame is None else b_frame
        df = ds_ * height if diff_frame is None else diff_frame
        self._chk(self._L.mi_analyze_diff_u8_batch_dev(self._h, _dptr(a), as_, af, _dptr(b) if b is not None else None, bs_, bf,
                                                     _dptr(diff) if diff is not None else None, ds_, df, width, height, n_frames,
                                                     int(threshold), _dptr(d_stats), stream), "mi_analyze_diff_u8_batch_dev")

    # ---- stages ----
    def hist_batch_dev(self, src, width, height, n_frames, d_hist, src_step=None, src_frame=None, stream=0):
        ss = width if src_step is None else src_step
        sf = ss * height if src_frame is None else src_frame
        self._chk(self._L.mi_hist_u8_batch_dev(self._h, _dptr(src), ss, sf, width, height, n_frames,
                                             _dptr(d_hist), stream), "mi_hist_u8_batch_dev")

    def equalize_lut_batch_dev(self, d_hist, total, n_frames, d_lut, stream=0):
        self._chk(self._L.mi_equalize_lut_batch_dev(self._h, _dptr(d_hist), int(total), n_frames, _dptr(d_lut), stream),
                  "mi_equalize_lut_batch_dev")

    def lut_apply_batch_dev(self, src, dst, width, height, n_frames, d_lut, src_step=None, src_frame=None,
                            dst_step=None, dst_frame=None, stream=0):
        ss = width if src_step is None else src_step
        ds = width if dst_step is None else dst_step
        sf = ss * height if src_frame is None else src_frame
        df = ds * height if dst_frame is None else dst_frame
        self._chk(self._L.mi_lut_apply_u8_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df, width, height,
                                                  n_frames, _dptr(d_lut), stream), "mi_lut_apply_u8_batch_dev")

    def clahe_tile_luts_batch_dev(self, src, width, height, n_frames, clip_limit, tiles_x, tiles_y, d_luts,
                                  src_step=None, src_frame=None, stream=0):
        ss = width if src_step is None else src_step
        sf = ss * height if src_frame is None else src_frame
        self._chk(self._L.mi_clahe_tile_luts_batch_dev(self._h, _dptr(src), ss, sf, width, height, n_frames,
                                                     float(clip_limit), tiles_x, tiles_y, _dptr(d_luts), stream),
                  "mi_clahe_tile_luts_batch_dev")

    # ---- 16-bit CLAHE (N4) ----
    def clahe16(self, src: np.ndarray, clip_limit: float = 40.0, tiles_x: int = 8, tiles_y: int = 8) -> np.ndarray:
        if not isinstance(src, np.ndarray) or src.dtype != np.uint16 or src.ndim != 2:
            raise MiError(2, "clahe16", "expected a 2-D uint16 ndarray (CV_16UC1)")
        if src.size and src.strides[1] != 2:
            raise MiError(1, "clahe16", "pixel stride must be 2")
        dst = np.empty(src.shape, np.uint16)
        h, w = src.shape
        sstep = int(src.strides[0]) if h > 1 else max(int(src.strides[0]), w * 2)
        self._chk(self._L.mi_clahe_u16(self._h, src.ctypes.data, sstep, dst.ctypes.data, w * 2, w, h, float(clip_limit),
                                     int(tiles_x), int(tiles_y)), "mi_clahe_u16")
        return dst

    def clahe16_batch_dev(self, src, dst, width, height, n_frames, clip_limit, tiles_x, tiles_y, stream=0, src_step=None,
                          src_frame=None, dst_step=None, dst_frame=None):
        """Steps and frame strides in bytes; tight (2*W, step * H) when not given."""
        ss = width * 2 if src_step is None else src_step
        ds = width * 2 if dst_step is None else dst_step
        sf = ss * height if src_frame is None else src_frame
        df = ds * height if dst_frame is None else dst_frame
        self._chk(self._L.mi_clahe_u16_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df, width, height, n_frames,
                                               float(clip_limit), tiles_x, tiles_y, stream), "mi_clahe_u16_batch_dev")

    # ---- 16-bit 4:2:0 frames: P010 / P012 / P016 ----
    def clahe_p010(self, frame: np.ndarray, width: int, height: int, uv_mode: int = UV_FILL128, clip_limit: float = 2.0,
                   tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_p010 on a host frame: a contiguous uint16 array of 3*W*H/2 samples (e.g. shape (3H/2, W)).  `out` may be
        `frame` (in place); otherwise a new array of the frame's shape is returned."""
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint16 or not frame.flags.c_contiguous:
            raise MiError(2, "clahe_p010", "expected a contiguous uint16 ndarray (P010 frame)")
        if width >= 0 and height >= 0 and frame.size < width * height * 3 // 2:
            raise MiError(1, "clahe_p010", "frame smaller than W*H*3/2 samples")
        if out is None:
            out = np.empty_like(frame)
        elif out.dtype != np.uint16 or not out.flags.c_contiguous or out.size < frame.size:
            raise MiError(1, "clahe_p010", "out must be a contiguous uint16 array as large as the frame")
        self._chk(self._L.mi_clahe_p010(self._h, frame.ctypes.data, out.ctypes.data, int(width), int(height), int(uv_mode),
                                      float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_p010")
        return out

    def clahe_p010_batch_dev(self, d_in, d_out, width, height, n_frames, uv_mode=UV_FILL128, clip_limit=2.0, tiles_x=8, tiles_y=8,
                             stream=0):
        """mi_clahe_p010_batch_dev: n_frames P010 frames at a pitch of 3*W*H bytes (device memory; d_in may be d_out)."""
        self._chk(self._L.mi_clahe_p010_batch_dev(self._h, _dptr(d_in), _dptr(d_out), int(width), int(height), int(n_frames),
                                                int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_p010_batch_dev")

    def clahe_p010_frames(self, inputs, outputs, width, height, uv_mode=UV_FILL128, clip_limit=2.0, tiles_x=8, tiles_y=8,
                          y_in_pitch=None, uv_in_pitch=None, y_out_pitch=None, uv_out_pitch=None, stream=0):
        """mi_clahe_p010_frames_dev: a list of P010 / P012 / P016 frames, each its own pitched (y, uv) planes -- 2-D int16 / uint16 torch
        CUDA tensors (W samples per row; the row stride in bytes gives the pitch) or raw device addresses; outputs None = in place.
        A pitch not given is the tensors' row stride, or 2 * W."""
        arr, n, p = _frame_list(inputs, outputs, 2 * int(width), (y_in_pitch, uv_in_pitch, y_out_pitch, uv_out_pitch), "clahe_p010_frames")
        self._chk(self._L.mi_clahe_p010_frames_dev(self._h, arr, n, int(width), int(height), p[0], p[1], p[2], p[3], int(uv_mode),
                                                 float(clip_limit), int(tiles_x), int(tiles_y), stream), "mi_clahe_p010_frames_dev")

    # ---- packed 4:2:2 frames: YUY2 / UYVY (capture devices) ----
    @staticmethod
    def _packed_host(a, width, name):
        a = _host2d(a, name)
        if a.shape[1] < 2 * width:
            raise MiError(1, name, "a packed 4:2:2 frame is an H x pitch-bytes uint8 array with at least 2*W bytes per row")
        return a

    def equalize_hist_packed422(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                                out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_packed422 on a host frame: an H x pitch-bytes uint8 array (pitch = the row stride, >= 2*W; a view with
        padded rows is fine).  `out` may be `frame` (in place); otherwise a new tight H x 2W array is returned."""
        frame = self._packed_host(frame, width, "equalize_hist_packed422")
        h = frame.shape[0]
        if out is None:
            out = np.empty((h, 2 * width), np.uint8)
        out = self._packed_host(out, width, "equalize_hist_packed422")
        self._chk(self._L.mi_equalize_hist_packed422(self._h, frame.ctypes.data, _step(frame), out.ctypes.data, _step(out),
                                                   int(width), int(h), int(fmt), int(uv_mode)), "mi_equalize_hist_packed422")
        return out

    def clahe_packed422(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY, clip_limit: float = 2.0,
                        tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_packed422; arguments as equalize_hist_packed422, plus the CLAHE parameters."""
        frame = self._packed_host(frame, width, "clahe_packed422")
        h = frame.shape[0]
        if out is None:
            out = np.empty((h, 2 * width), np.uint8)
        out = self._packed_host(out, width, "clahe_packed422")
        self._chk(self._L.mi_clahe_packed422(self._h, frame.ctypes.data, _step(frame), out.ctypes.data, _step(out), int(width), int(h),
                                           int(fmt), int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_packed422")
        return out

    def equalize_hist_packed422_batch_dev(self, d_in, d_out, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                          in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_packed422_batch_dev: n_frames packed frames in device memory (torch tensors or raw addresses); pitches
        default to 2*W, frame strides to pitch * H; d_out may be d_in (in place)."""
        ip = 2 * width if in_pitch is None else in_pitch
        op = 2 * width if out_pitch is None else out_pitch
        fi = ip * height if in_frame is None else in_frame
        fo = op * height if out_frame is None else out_frame
        self._chk(self._L.mi_equalize_hist_packed422_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                             int(n_frames), int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_packed422_batch_dev")

    def clahe_packed422_batch_dev(self, d_in, d_out, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY, clip_limit=2.0,
                                  tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_packed422_batch_dev; arguments as equalize_hist_packed422_batch_dev, plus the CLAHE parameters."""
        ip = 2 * width if in_pitch is None else in_pitch
        op = 2 * width if out_pitch is None else out_pitch
        fi = ip * height if in_frame is None else in_frame
        fo = op * height if out_frame is None else out_frame
        self._chk(self._L.mi_clahe_packed422_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                     int(n_frames), int(fmt), int(uv_mode), float(clip_limit), int(tiles_x),
                                                     int(tiles_y), stream), "mi_clahe_packed422_batch_dev")

    def equalize_hist_packed422_frames(self, inputs, outputs, width, height, fmt=FMT_YUY2, uv_mode=UV_COPY, in_pitch=None,
                                       out_pitch=None, stream=0):
        """mi_equalize_hist_packed422_frames_dev.  inputs / outputs: lists of packed frames, each its own buffer -- torch CUDA tensors
        or raw device addresses; outputs None = every frame in place.  A pitch left at None is the row stride of the 2-D tensors of
        that side, or 2 * width."""
        arr, n, ip, op = _packed422_list(inputs, outputs, width, in_pitch, out_pitch, "equalize_hist_packed422_frames")
        self._chk(self._L.mi_equalize_hist_packed422_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(fmt), int(uv_mode),
                                                              stream), "mi_equalize_hist_packed422_frames_dev")

    def clahe_packed422_frames(self, inputs, outputs, width, height, fmt=FMT_YUY2, uv_mode=UV_COPY, clip_limit=2.0, tiles_x=8,
                               tiles_y=8, in_pitch=None, out_pitch=None, stream=0):
        """mi_clahe_packed422_frames_dev; arguments as equalize_hist_packed422_frames, plus the CLAHE parameters."""
        arr, n, ip, op = _packed422_list(inputs, outputs, width, in_pitch, out_pitch, "clahe_packed422_frames")
        self._chk(self._L.mi_clahe_packed422_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(fmt), int(uv_mode),
                                                      float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_packed422_frames_dev")

    @staticmethod
    def _nv12_out(d_y_out, d_uv_out, width, height, y_pitch, uv_pitch, out_frame):
        """Addresses and strides of the NV12 side; d_uv_out None: the UV plane directly behind the Y plane (y_pitch * H further)."""
        yp = int(width) if y_pitch is None else int(y_pitch)
        up = int(width) if uv_pitch is None else int(uv_pitch)
        y = _dptr(d_y_out)
        uv = _dptr(d_uv_out) if d_uv_out is not None else (y + yp * int(height) if y else y)
        fo = yp * int(height) + up * (int(height) // 2) if out_frame is None else int(out_frame)
        return y, yp, uv, up, fo

    def equalize_hist_packed422_to_nv12_batch_dev(self, d_in, d_y_out, d_uv_out, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                                  in_pitch=None, in_frame=None, y_pitch=None, uv_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_packed422_to_nv12_batch_dev: n_frames packed frames in, NV12 frames out (torch tensors or raw addresses).
        Tight layouts are the defaults: in_pitch 2*W, in_frame in_pitch * H, y_pitch = uv_pitch = W, out_frame = y_pitch * H +
        uv_pitch * H/2; d_uv_out None puts the UV plane directly behind the Y plane (one tight NV12 batch in d_y_out)."""
        ip = 2 * width if in_pitch is None else in_pitch
        fi = ip * height if in_frame is None else in_frame
        y, yp, uv, up, fo = self._nv12_out(d_y_out, d_uv_out, width, height, y_pitch, uv_pitch, out_frame)
        self._chk(self._L.mi_equalize_hist_packed422_to_nv12_batch_dev(self._h, _dptr(d_in), ip, fi, y, yp, uv, up, fo, int(width),
                                                                     int(height), int(n_frames), int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_packed422_to_nv12_batch_dev")

    def clahe_packed422_to_nv12_batch_dev(self, d_in, d_y_out, d_uv_out, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                          clip_limit=2.0, tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, y_pitch=None,
                                          uv_pitch=None, out_frame=None, stream=0):
        """mi_clahe_packed422_to_nv12_batch_dev; arguments as equalize_hist_packed422_to_nv12_batch_dev, plus the CLAHE parameters."""
        ip = 2 * width if in_pitch is None else in_pitch
        fi = ip * height if in_frame is None else in_frame
        y, yp, uv, up, fo = self._nv12_out(d_y_out, d_uv_out, width, height, y_pitch, uv_pitch, out_frame)
        self._chk(self._L.mi_clahe_packed422_to_nv12_batch_dev(self._h, _dptr(d_in), ip, fi, y, yp, uv, up, fo, int(width), int(height),
                                                             int(n_frames), int(fmt), int(uv_mode), float(clip_limit), int(tiles_x),
                                                             int(tiles_y), stream), "mi_clahe_packed422_to_nv12_batch_dev")

    def equalize_hist_packed422_to_nv12_frames(self, inputs, y_outputs, uv_outputs, width, height, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                               in_pitch=None, y_pitch=None, uv_pitch=None, stream=0):
        """mi_equalize_hist_packed422_to_nv12_frames_dev.  inputs: the packed frames, y_outputs / uv_outputs: the NV12 planes, each
        its own buffer -- lists of torch CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row
        stride of the 2-D tensors of that list, or the tight one (2 * width; width)."""
        arr, n, ip, yp, up = _packed422_nv12_list(inputs, y_outputs, uv_outputs, width, in_pitch, y_pitch, uv_pitch,
                                                  "equalize_hist_packed422_to_nv12_frames")
        self._chk(self._L.mi_equalize_hist_packed422_to_nv12_frames_dev(self._h, arr, n, int(width), int(height), ip, yp, up, int(fmt),
                                                                      int(uv_mode), stream),
                  "mi_equalize_hist_packed422_to_nv12_frames_dev")

    def clahe_packed422_to_nv12_frames(self, inputs, y_outputs, uv_outputs, width, height, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                       clip_limit=2.0, tiles_x=8, tiles_y=8, in_pitch=None, y_pitch=None, uv_pitch=None, stream=0):
        """mi_clahe_packed422_to_nv12_frames_dev; arguments as equalize_hist_packed422_to_nv12_frames, plus the CLAHE parameters."""
        arr, n, ip, yp, up = _packed422_nv12_list(inputs, y_outputs, uv_outputs, width, in_pitch, y_pitch, uv_pitch,
                                                  "clahe_packed422_to_nv12_frames")
        self._chk(self._L.mi_clahe_packed422_to_nv12_frames_dev(self._h, arr, n, int(width), int(height), ip, yp, up, int(fmt),
                                                              int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_packed422_to_nv12_frames_dev")

    def _nv12_host_out(self, width, h, y_out, uv_out, name):
        """The two host planes of a packed 4:2:2 -> NV12 call: given (2-D uint8 arrays of at least W bytes per row, any pitch) or new
        tight ones."""
        if y_out is None:
            y_out = np.empty((h, width), np.uint8)
        if uv_out is None:
            uv_out = np.empty((h // 2, width), np.uint8)
        y_out, uv_out = _host2d(y_out, name), _host2d(uv_out, name)
        if y_out.shape[1] < width or uv_out.shape[1] < width or y_out.shape[0] != h or uv_out.shape[0] != h // 2:
            raise MiError(1, name, "the NV12 planes are an H x pitch and an H/2 x pitch uint8 array with at least W bytes per row")
        return y_out, uv_out

    def equalize_hist_packed422_to_nv12(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                                        y_out: np.ndarray | None = None, uv_out: np.ndarray | None = None):
        """mi_equalize_hist_packed422_to_nv12 on a host frame: an H x pitch-bytes uint8 array (pitch >= 2*W) in, the (Y, UV) planes
        out -- `y_out` (H rows) / `uv_out` (H/2 rows) when given, views with padded rows or odd addresses included, else new tight
        H x W and H/2 x W arrays."""
        name = "equalize_hist_packed422_to_nv12"
        frame = self._packed_host(frame, width, name)
        h = frame.shape[0]
        y_out, uv_out = self._nv12_host_out(int(width), h, y_out, uv_out, name)
        self._chk(self._L.mi_equalize_hist_packed422_to_nv12(self._h, frame.ctypes.data, _step(frame), y_out.ctypes.data, _step(y_out),
                                                           uv_out.ctypes.data, _step(uv_out), int(width), int(h), int(fmt),
                                                           int(uv_mode)), "mi_equalize_hist_packed422_to_nv12")
        return y_out, uv_out

    def clahe_packed422_to_nv12(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                                clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8,
                                y_out: np.ndarray | None = None, uv_out: np.ndarray | None = None):
        """mi_clahe_packed422_to_nv12; arguments as equalize_hist_packed422_to_nv12, plus the CLAHE parameters."""
        name = "clahe_packed422_to_nv12"
        frame = self._packed_host(frame, width, name)
        h = frame.shape[0]
        y_out, uv_out = self._nv12_host_out(int(width), h, y_out, uv_out, name)
        self._chk(self._L.mi_clahe_packed422_to_nv12(self._h, frame.ctypes.data, _step(frame), y_out.ctypes.data, _step(y_out),
                                                   uv_out.ctypes.data, _step(uv_out), int(width), int(h), int(fmt), int(uv_mode),
                                                   float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_packed422_to_nv12")
        return y_out, uv_out

    # ---- packed 4:2:2 in, 4:2:0 frames (I420 / YV12 planes, or NV12) out: the halved chroma de-interleaved by the launch that writes the luma ----
    def equalize_hist_packed422_to_yuv420_batch_dev(self, d_in, dst, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                                    in_pitch=None, in_frame=None, stream=0):
        """mi_equalize_hist_packed422_to_yuv420_batch_dev.  d_in: the packed frames (a torch tensor or a raw address); dst: a
        Yuv420Planes holding device addresses (Yuv420Planes.i420 / .yv12 / .nv12 for tight batches, the fields themselves for pitched
        or separately allocated planes).  The tight input is the default: in_pitch 2*W, in_frame = in_pitch * H."""
        ip = 2 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        self._chk(self._L.mi_equalize_hist_packed422_to_yuv420_batch_dev(self._h, _dptr(d_in), ip, fi, C.byref(dst), int(width),
                                                                       int(height), int(n_frames), int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_packed422_to_yuv420_batch_dev")

    def clahe_packed422_to_yuv420_batch_dev(self, d_in, dst, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY, clip_limit=2.0,
                                            tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, stream=0):
        """mi_clahe_packed422_to_yuv420_batch_dev; arguments as equalize_hist_packed422_to_yuv420_batch_dev, plus the CLAHE parameters."""
        ip = 2 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        self._chk(self._L.mi_clahe_packed422_to_yuv420_batch_dev(self._h, _dptr(d_in), ip, fi, C.byref(dst), int(width), int(height),
                                                               int(n_frames), int(fmt), int(uv_mode), float(clip_limit), int(tiles_x),
                                                               int(tiles_y), stream), "mi_clahe_packed422_to_yuv420_batch_dev")

    def equalize_hist_packed422_to_yuv420_frames_dev(self, frames, width, height, in_pitch, y_pitch, c_pitch, chroma, fmt=FMT_YUY2,
                                                     uv_mode=UV_COPY, stream=0):
        """mi_equalize_hist_packed422_to_yuv420_frames_dev.  frames: BgrYuv420FrameDev entries {in, y, c0, c1}, one per frame, every
        packed frame and every plane at its own device address (a capture pool in, a software encoder's frame pool out); one shape, one
        set of pitches and one chroma layout for the call."""
        arr, n = self._bgr_yuv420_list(frames)
        self._chk(self._L.mi_equalize_hist_packed422_to_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(in_pitch),
                                                                        int(y_pitch), int(c_pitch), int(chroma), int(fmt), int(uv_mode),
                                                                        stream), "mi_equalize_hist_packed422_to_yuv420_frames_dev")

    def clahe_packed422_to_yuv420_frames_dev(self, frames, width, height, in_pitch, y_pitch, c_pitch, chroma, fmt=FMT_YUY2,
                                             uv_mode=UV_COPY, clip_limit=2.0, tiles_x=8, tiles_y=8, stream=0):
        """mi_clahe_packed422_to_yuv420_frames_dev; arguments as equalize_hist_packed422_to_yuv420_frames_dev, plus the CLAHE parameters."""
        arr, n = self._bgr_yuv420_list(frames)
        self._chk(self._L.mi_clahe_packed422_to_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(in_pitch), int(y_pitch),
                                                                int(c_pitch), int(chroma), int(fmt), int(uv_mode), float(clip_limit),
                                                                int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_packed422_to_yuv420_frames_dev")

    def _packed422_yuv420_host(self, frame, width, dst_fmt, out, planes, name):
        frame = self._packed_host(frame, width, name)
        h, w = frame.shape[0], int(width)
        if planes is not None:
            return frame, h, None, planes
        if dst_fmt not in _YUV420_FMTS:
            raise MiError(1, name, 'dst_fmt must be "nv12", "i420" or "yv12"')
        if out is None:
            out = np.empty(w * h * 3 // 2, np.uint8)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size == w * h * 3 // 2):
            raise MiError(1, name, "out is a contiguous uint8 array of W*H*3/2 bytes")
        return frame, h, out, _YUV420_FMTS[dst_fmt](out.ctypes.data, w, h)

    def equalize_hist_packed422_to_yuv420(self, frame: np.ndarray, width: int, dst_fmt: str = "i420", fmt: int = FMT_YUY2,
                                          uv_mode: int = UV_COPY, out: np.ndarray | None = None, planes: Yuv420Planes | None = None):
        """mi_equalize_hist_packed422_to_yuv420 on a host frame: an H x pitch-bytes uint8 array (pitch >= 2*W) in, the tight frame of
        W*H*3/2 bytes out, its chroma laid out as dst_fmt in {"nv12", "i420", "yv12"} says -- `out` when given, else a new array.
        `planes`: a Yuv420Planes of host addresses (any address, any pitch) to write instead; nothing is returned then."""
        frame, h, out, b = self._packed422_yuv420_host(frame, width, dst_fmt, out, planes, "equalize_hist_packed422_to_yuv420")
        self._chk(self._L.mi_equalize_hist_packed422_to_yuv420(self._h, frame.ctypes.data, _step(frame), C.byref(b), int(width), int(h),
                                                             int(fmt), int(uv_mode)), "mi_equalize_hist_packed422_to_yuv420")
        return out

    def clahe_packed422_to_yuv420(self, frame: np.ndarray, width: int, dst_fmt: str = "i420", fmt: int = FMT_YUY2,
                                  uv_mode: int = UV_COPY, clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8,
                                  out: np.ndarray | None = None, planes: Yuv420Planes | None = None):
        """mi_clahe_packed422_to_yuv420; arguments as equalize_hist_packed422_to_yuv420, plus the CLAHE parameters."""
        frame, h, out, b = self._packed422_yuv420_host(frame, width, dst_fmt, out, planes, "clahe_packed422_to_yuv420")
        self._chk(self._L.mi_clahe_packed422_to_yuv420(self._h, frame.ctypes.data, _step(frame), C.byref(b), int(width), int(h),
                                                     int(fmt), int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y)),
                  "mi_clahe_packed422_to_yuv420")
        return out

    # ---- packed 4:2:2 in, interleaved BGR / RGB out in the pass that maps the luma: every row keeps its own chroma ----
    def equalize_hist_packed422_to_bgr_batch_dev(self, d_in, d_out, width, height, n_frames, fmt=FMT_YUY2, order=ORDER_BGR,
                                                 in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_packed422_to_bgr_batch_dev: n_frames packed frames in, interleaved BGR / RGB images out (torch tensors or
        raw addresses).  fmt says the chroma order too: FMT_YUY2 is Y0 U Y1 V, FMT_UYVY is U Y0 V Y1.  Tight layouts are the defaults:
        in_pitch 2*W, in_frame in_pitch * H, out_pitch 3*W, out_frame out_pitch * H."""
        ip = 2 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_packed422_to_bgr_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width),
                                                                    int(height), int(n_frames), int(fmt), int(order), stream),
                  "mi_equalize_hist_packed422_to_bgr_batch_dev")

    def clahe_packed422_to_bgr_batch_dev(self, d_in, d_out, width, height, n_frames, fmt=FMT_YUY2, order=ORDER_BGR, clip_limit=2.0,
                                         tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_packed422_to_bgr_batch_dev; arguments as equalize_hist_packed422_to_bgr_batch_dev, plus the CLAHE parameters."""
        ip = 2 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_packed422_to_bgr_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                            int(n_frames), int(fmt), int(order), float(clip_limit), int(tiles_x),
                                                            int(tiles_y), stream), "mi_clahe_packed422_to_bgr_batch_dev")

    def equalize_hist_packed422_to_bgr_frames(self, inputs, outs, width, height, fmt=FMT_YUY2, order=ORDER_BGR, in_pitch=None,
                                              out_pitch=None, stream=0):
        """mi_equalize_hist_packed422_to_bgr_frames_dev.  inputs: the packed frames, outs: the images, each its own buffer -- lists of
        torch CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row stride of the 2-D tensors of
        that list (H x W x 3 images: of their first axis), or the tight one (2 * width; 3 * width)."""
        arr, n, ip, op = _packed422_bgr_list(inputs, outs, width, in_pitch, out_pitch, "equalize_hist_packed422_to_bgr_frames")
        self._chk(self._L.mi_equalize_hist_packed422_to_bgr_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(fmt),
                                                                     int(order), stream),
                  "mi_equalize_hist_packed422_to_bgr_frames_dev")

    def clahe_packed422_to_bgr_frames(self, inputs, outs, width, height, fmt=FMT_YUY2, order=ORDER_BGR, clip_limit=2.0, tiles_x=8,
                                      tiles_y=8, in_pitch=None, out_pitch=None, stream=0):
        """mi_clahe_packed422_to_bgr_frames_dev; arguments as equalize_hist_packed422_to_bgr_frames, plus the CLAHE parameters."""
        arr, n, ip, op = _packed422_bgr_list(inputs, outs, width, in_pitch, out_pitch, "clahe_packed422_to_bgr_frames")
        self._chk(self._L.mi_clahe_packed422_to_bgr_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(fmt), int(order),
                                                             float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_packed422_to_bgr_frames_dev")

    def _packed_bgr_host(self, frame, width, out, name):
        frame = self._packed_host(frame, width, name)
        h = frame.shape[0]
        if out is None:
            out = np.empty((h, max(int(width), 0), 3), np.uint8)
        out = self._host3(out, name)
        if out.shape[:2] != (h, width):
            raise MiError(1, name, "out must be an H x W x 3 uint8 array (rows may be padded)")
        return frame, out, (int(out.strides[0]) if h > 1 else max(int(out.strides[0]), 3 * int(width)))

    def equalize_hist_packed422_to_bgr(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, order: int = ORDER_BGR,
                                       out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_packed422_to_bgr on a host frame: an H x pitch-bytes uint8 array (pitch >= 2*W) in, the H x W x 3 image
        out -- `out` when given (a view with padded rows or at an odd address included), else a new tight array."""
        frame, out, step = self._packed_bgr_host(frame, int(width), out, "equalize_hist_packed422_to_bgr")
        self._chk(self._L.mi_equalize_hist_packed422_to_bgr(self._h, frame.ctypes.data, _step(frame), out.ctypes.data, step, int(width),
                                                          int(frame.shape[0]), int(fmt), int(order)), "mi_equalize_hist_packed422_to_bgr")
        return out

    def clahe_packed422_to_bgr(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, order: int = ORDER_BGR,
                               clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_packed422_to_bgr; arguments as equalize_hist_packed422_to_bgr, plus the CLAHE parameters."""
        frame, out, step = self._packed_bgr_host(frame, int(width), out, "clahe_packed422_to_bgr")
        self._chk(self._L.mi_clahe_packed422_to_bgr(self._h, frame.ctypes.data, _step(frame), out.ctypes.data, step, int(width),
                                                  int(frame.shape[0]), int(fmt), int(order), float(clip_limit), int(tiles_x),
                                                  int(tiles_y)), "mi_clahe_packed422_to_bgr")
        return out

    # ---- packed 4:2:2 in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out: the methods above with a pixel of four bytes ----
    def equalize_hist_packed422_to_bgra_batch_dev(self, d_in, d_out, width, height, n_frames, fmt=FMT_YUY2, order=ORDER_BGR,
                                                  in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_packed422_to_bgra_batch_dev: n_frames packed frames in, interleaved BGRA / RGBA images out (torch tensors or
        raw addresses).  fmt says the chroma order too: FMT_YUY2 is Y0 U Y1 V, FMT_UYVY is U Y0 V Y1.  Tight layouts are the defaults:
        in_pitch 2*W, in_frame in_pitch * H, out_pitch 4*W, out_frame out_pitch * H."""
        ip = 2 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 4 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_packed422_to_bgra_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width),
                                                                     int(height), int(n_frames), int(fmt), int(order), stream),
                  "mi_equalize_hist_packed422_to_bgra_batch_dev")

    def clahe_packed422_to_bgra_batch_dev(self, d_in, d_out, width, height, n_frames, fmt=FMT_YUY2, order=ORDER_BGR, clip_limit=2.0,
                                          tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_packed422_to_bgra_batch_dev; arguments as equalize_hist_packed422_to_bgra_batch_dev, plus the CLAHE parameters."""
        ip = 2 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 4 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_packed422_to_bgra_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                             int(n_frames), int(fmt), int(order), float(clip_limit), int(tiles_x),
                                                             int(tiles_y), stream), "mi_clahe_packed422_to_bgra_batch_dev")

    def equalize_hist_packed422_to_bgra_frames(self, inputs, outs, width, height, fmt=FMT_YUY2, order=ORDER_BGR, in_pitch=None,
                                               out_pitch=None, stream=0):
        """mi_equalize_hist_packed422_to_bgra_frames_dev.  inputs: the packed frames, outs: the images, each its own buffer -- lists of
        torch CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row stride of the 2-D tensors of
        that list (H x W x 4 images: of their first axis), or the tight one (2 * width; 4 * width)."""
        arr, n, ip, op = _packed422_bgr_list(inputs, outs, width, in_pitch, out_pitch, "equalize_hist_packed422_to_bgra_frames", px=4)
        self._chk(self._L.mi_equalize_hist_packed422_to_bgra_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(fmt),
                                                                      int(order), stream),
                  "mi_equalize_hist_packed422_to_bgra_frames_dev")

    def clahe_packed422_to_bgra_frames(self, inputs, outs, width, height, fmt=FMT_YUY2, order=ORDER_BGR, clip_limit=2.0, tiles_x=8,
                                       tiles_y=8, in_pitch=None, out_pitch=None, stream=0):
        """mi_clahe_packed422_to_bgra_frames_dev; arguments as equalize_hist_packed422_to_bgra_frames, plus the CLAHE parameters."""
        arr, n, ip, op = _packed422_bgr_list(inputs, outs, width, in_pitch, out_pitch, "clahe_packed422_to_bgra_frames", px=4)
        self._chk(self._L.mi_clahe_packed422_to_bgra_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(fmt), int(order),
                                                              float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_packed422_to_bgra_frames_dev")

    def _packed_bgra_host(self, frame, width, out, name):
        frame = self._packed_host(frame, width, name)
        h = frame.shape[0]
        if out is None:
            out = np.empty((h, max(int(width), 0), 4), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 3 or out.shape[2] != 4:
            raise MiError(2, name, "expected an HxWx4 uint8 ndarray (CV_8UC4)")
        if out.size and (out.strides[2] != 1 or out.strides[1] != 4):
            raise MiError(1, name, "pixels must be interleaved")
        if out.shape[:2] != (h, width):
            raise MiError(1, name, "out must be an H x W x 4 uint8 array (rows may be padded)")
        return frame, out, (int(out.strides[0]) if h > 1 else max(int(out.strides[0]), 4 * int(width)))

    def equalize_hist_packed422_to_bgra(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, order: int = ORDER_BGR,
                                        out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_packed422_to_bgra on a host frame: an H x pitch-bytes uint8 array (pitch >= 2*W) in, the H x W x 4 image
        out -- `out` when given (a view with padded rows or at an odd address included), else a new tight array."""
        frame, out, step = self._packed_bgra_host(frame, int(width), out, "equalize_hist_packed422_to_bgra")
        self._chk(self._L.mi_equalize_hist_packed422_to_bgra(self._h, frame.ctypes.data, _step(frame), out.ctypes.data, step, int(width),
                                                           int(frame.shape[0]), int(fmt), int(order)), "mi_equalize_hist_packed422_to_bgra")
        return out

    def clahe_packed422_to_bgra(self, frame: np.ndarray, width: int, fmt: int = FMT_YUY2, order: int = ORDER_BGR,
                                clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_packed422_to_bgra; arguments as equalize_hist_packed422_to_bgra, plus the CLAHE parameters."""
        frame, out, step = self._packed_bgra_host(frame, int(width), out, "clahe_packed422_to_bgra")
        self._chk(self._L.mi_clahe_packed422_to_bgra(self._h, frame.ctypes.data, _step(frame), out.ctypes.data, step, int(width),
                                                   int(frame.shape[0]), int(fmt), int(order), float(clip_limit), int(tiles_x),
                                                   int(tiles_y)), "mi_clahe_packed422_to_bgra")
        return out

    # ---- NV12 in, interleaved BGR / RGB out in the pass that maps the luma ----
    @staticmethod
    def _nv12_in(d_y, d_uv, width, height, y_pitch, uv_pitch, in_frame):
        """Addresses and strides of the NV12 side; d_uv None: the UV plane directly behind the Y plane (y_pitch * H further)."""
        yp = int(width) if y_pitch is None else int(y_pitch)
        up = int(width) if uv_pitch is None else int(uv_pitch)
        y = _dptr(d_y)
        uv = _dptr(d_uv) if d_uv is not None else (y + yp * int(height) if y else y)
        fi = yp * int(height) + up * (int(height) // 2) if in_frame is None else int(in_frame)
        return y, yp, uv, up, fi

    def equalize_hist_nv12_to_bgr_batch_dev(self, d_y, d_uv, d_out, width, height, n_frames, order=ORDER_BGR, y_pitch=None, uv_pitch=None,
                                            in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_nv12_to_bgr_batch_dev: n_frames NV12 frames in, interleaved BGR / RGB images out (torch tensors or raw
        addresses).  Tight layouts are the defaults: y_pitch = uv_pitch = W, in_frame = y_pitch * H + uv_pitch * H/2, out_pitch 3*W,
        out_frame = out_pitch * H; d_uv None puts the UV plane directly behind the Y plane (one tight NV12 batch in d_y)."""
        y, yp, uv, up, fi = self._nv12_in(d_y, d_uv, width, height, y_pitch, uv_pitch, in_frame)
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_nv12_to_bgr_batch_dev(self._h, y, yp, uv, up, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                               int(n_frames), int(order), stream),
                  "mi_equalize_hist_nv12_to_bgr_batch_dev")

    def clahe_nv12_to_bgr_batch_dev(self, d_y, d_uv, d_out, width, height, n_frames, order=ORDER_BGR, clip_limit=2.0, tiles_x=8, tiles_y=8,
                                    y_pitch=None, uv_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_nv12_to_bgr_batch_dev; arguments as equalize_hist_nv12_to_bgr_batch_dev, plus the CLAHE parameters."""
        y, yp, uv, up, fi = self._nv12_in(d_y, d_uv, width, height, y_pitch, uv_pitch, in_frame)
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_nv12_to_bgr_batch_dev(self._h, y, yp, uv, up, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                       int(n_frames), int(order), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_nv12_to_bgr_batch_dev")

    def equalize_hist_nv12_to_bgr_frames(self, ys, uvs, outs, width, height, order=ORDER_BGR, y_pitch=None, uv_pitch=None,
                                         out_pitch=None, stream=0):
        """mi_equalize_hist_nv12_to_bgr_frames_dev.  ys / uvs: the Y and UV planes, outs: the images, each its own buffer -- lists of
        torch CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row stride of the 2-D tensors of
        that list (H x W x 3 images: of their rows), or the tight one (width; 3 * width)."""
        arr, n, yp, up, op = _nv12_bgr_list(ys, uvs, outs, width, y_pitch, uv_pitch, out_pitch, "equalize_hist_nv12_to_bgr_frames")
        self._chk(self._L.mi_equalize_hist_nv12_to_bgr_frames_dev(self._h, arr, n, int(width), int(height), yp, up, op, int(order), stream),
                  "mi_equalize_hist_nv12_to_bgr_frames_dev")

    def clahe_nv12_to_bgr_frames(self, ys, uvs, outs, width, height, order=ORDER_BGR, clip_limit=2.0, tiles_x=8, tiles_y=8,
                                 y_pitch=None, uv_pitch=None, out_pitch=None, stream=0):
        """mi_clahe_nv12_to_bgr_frames_dev; arguments as equalize_hist_nv12_to_bgr_frames, plus the CLAHE parameters."""
        arr, n, yp, up, op = _nv12_bgr_list(ys, uvs, outs, width, y_pitch, uv_pitch, out_pitch, "clahe_nv12_to_bgr_frames")
        self._chk(self._L.mi_clahe_nv12_to_bgr_frames_dev(self._h, arr, n, int(width), int(height), yp, up, op, int(order),
                                                        float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_nv12_to_bgr_frames_dev")

    def _nv12_bgr_host(self, nv12, width, height, out, name):
        if not isinstance(nv12, np.ndarray) or nv12.dtype != np.uint8 or not nv12.flags.c_contiguous:
            raise MiError(2, name, "expected a contiguous uint8 ndarray")
        if width >= 0 and height >= 0 and nv12.size != width * height * 3 // 2:
            raise MiError(1, name, "NV12 frame must hold width*height*3/2 bytes")
        if out is None:
            out = np.empty((max(height, 0), max(width, 0), 3), np.uint8)
        out = self._host3(out, name)
        if out.shape[:2] != (height, width):
            raise MiError(1, name, "out must be an H x W x 3 uint8 array (rows may be padded)")
        return out, (int(out.strides[0]) if height > 1 else max(int(out.strides[0]), 3 * width))

    def equalize_hist_nv12_to_bgr(self, nv12: np.ndarray, width: int, height: int, order: int = ORDER_BGR,
                                  out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_nv12_to_bgr on a tight host NV12 frame: the H x W x 3 image out -- `out` when given (a view with padded rows
        included), else a new tight array."""
        out, step = self._nv12_bgr_host(nv12, int(width), int(height), out, "equalize_hist_nv12_to_bgr")
        self._chk(self._L.mi_equalize_hist_nv12_to_bgr(self._h, nv12.ctypes.data, out.ctypes.data, step, int(width), int(height), int(order)),
                  "mi_equalize_hist_nv12_to_bgr")
        return out

    def clahe_nv12_to_bgr(self, nv12: np.ndarray, width: int, height: int, order: int = ORDER_BGR, clip_limit: float = 2.0,
                          tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_nv12_to_bgr; arguments as equalize_hist_nv12_to_bgr, plus the CLAHE parameters."""
        out, step = self._nv12_bgr_host(nv12, int(width), int(height), out, "clahe_nv12_to_bgr")
        self._chk(self._L.mi_clahe_nv12_to_bgr(self._h, nv12.ctypes.data, out.ctypes.data, step, int(width), int(height), int(order),
                                             float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_nv12_to_bgr")
        return out

    # ---- interleaved BGR / RGB in, NV12 out: convert and count in one pass, then map the luma in place ----
    def equalize_hist_bgr_to_nv12_batch_dev(self, d_in, d_y_out, d_uv_out, width, height, n_frames, order=ORDER_BGR, uv_mode=UV_COPY,
                                            in_pitch=None, in_frame=None, y_pitch=None, uv_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_bgr_to_nv12_batch_dev: n_frames interleaved BGR / RGB images in, NV12 frames out (torch tensors or raw
        addresses).  Tight layouts are the defaults: in_pitch 3*W, in_frame in_pitch * H, y_pitch = uv_pitch = W, out_frame =
        y_pitch * H + uv_pitch * H/2; d_uv_out None puts the UV plane directly behind the Y plane (one tight NV12 batch in d_y_out)."""
        ip = 3 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        y, yp, uv, up, fo = self._nv12_out(d_y_out, d_uv_out, width, height, y_pitch, uv_pitch, out_frame)
        self._chk(self._L.mi_equalize_hist_bgr_to_nv12_batch_dev(self._h, _dptr(d_in), ip, fi, y, yp, uv, up, fo, int(width), int(height),
                                                               int(n_frames), int(order), int(uv_mode), stream),
                  "mi_equalize_hist_bgr_to_nv12_batch_dev")

    def clahe_bgr_to_nv12_batch_dev(self, d_in, d_y_out, d_uv_out, width, height, n_frames, order=ORDER_BGR, uv_mode=UV_COPY,
                                    clip_limit=2.0, tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, y_pitch=None, uv_pitch=None,
                                    out_frame=None, stream=0):
        """mi_clahe_bgr_to_nv12_batch_dev; arguments as equalize_hist_bgr_to_nv12_batch_dev, plus the CLAHE parameters."""
        ip = 3 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        y, yp, uv, up, fo = self._nv12_out(d_y_out, d_uv_out, width, height, y_pitch, uv_pitch, out_frame)
        self._chk(self._L.mi_clahe_bgr_to_nv12_batch_dev(self._h, _dptr(d_in), ip, fi, y, yp, uv, up, fo, int(width), int(height),
                                                       int(n_frames), int(order), int(uv_mode), float(clip_limit), int(tiles_x),
                                                       int(tiles_y), stream), "mi_clahe_bgr_to_nv12_batch_dev")

    def equalize_hist_bgr_to_nv12_frames(self, ins, ys, uvs, width, height, order=ORDER_BGR, uv_mode=UV_COPY, in_pitch=None, y_pitch=None,
                                         uv_pitch=None, stream=0):
        """mi_equalize_hist_bgr_to_nv12_frames_dev.  ins: the images, ys / uvs: the Y and UV planes, each its own buffer -- lists of
        torch CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row stride of the 2-D tensors of
        that list (H x W x 3 images: of their rows), or the tight one (3 * width; width)."""
        arr, n, ip, yp, up = _bgr_nv12_list(ins, ys, uvs, width, in_pitch, y_pitch, uv_pitch, "equalize_hist_bgr_to_nv12_frames")
        self._chk(self._L.mi_equalize_hist_bgr_to_nv12_frames_dev(self._h, arr, n, int(width), int(height), ip, yp, up, int(order),
                                                                int(uv_mode), stream), "mi_equalize_hist_bgr_to_nv12_frames_dev")

    def clahe_bgr_to_nv12_frames(self, ins, ys, uvs, width, height, order=ORDER_BGR, uv_mode=UV_COPY, clip_limit=2.0, tiles_x=8,
                                 tiles_y=8, in_pitch=None, y_pitch=None, uv_pitch=None, stream=0):
        """mi_clahe_bgr_to_nv12_frames_dev; arguments as equalize_hist_bgr_to_nv12_frames, plus the CLAHE parameters."""
        arr, n, ip, yp, up = _bgr_nv12_list(ins, ys, uvs, width, in_pitch, y_pitch, uv_pitch, "clahe_bgr_to_nv12_frames")
        self._chk(self._L.mi_clahe_bgr_to_nv12_frames_dev(self._h, arr, n, int(width), int(height), ip, yp, up, int(order), int(uv_mode),
                                                        float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_bgr_to_nv12_frames_dev")

    def _bgr_nv12_host(self, img, out, name):
        img = self._host3(img, name)
        h, w = img.shape[:2]
        if out is None:
            out = np.empty(w * h * 3 // 2, np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.size != w * h * 3 // 2:
            raise MiError(1, name, "out must be a contiguous uint8 array of width*height*3/2 bytes")
        return img, h, w, (int(img.strides[0]) if h > 1 else max(int(img.strides[0]), 3 * w)), out

    def equalize_hist_bgr_to_nv12(self, img: np.ndarray, order: int = ORDER_BGR, uv_mode: int = UV_COPY,
                                  out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_bgr_to_nv12 on a host image: an H x W x 3 uint8 array in (a view with padded rows included), the tight NV12
        frame of W*H*3/2 bytes out -- `out` when given, else a new array."""
        img, h, w, step, out = self._bgr_nv12_host(img, out, "equalize_hist_bgr_to_nv12")
        self._chk(self._L.mi_equalize_hist_bgr_to_nv12(self._h, img.ctypes.data, step, out.ctypes.data, w, h, int(order), int(uv_mode)),
                  "mi_equalize_hist_bgr_to_nv12")
        return out

    def clahe_bgr_to_nv12(self, img: np.ndarray, order: int = ORDER_BGR, uv_mode: int = UV_COPY, clip_limit: float = 2.0,
                          tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_bgr_to_nv12; arguments as equalize_hist_bgr_to_nv12, plus the CLAHE parameters."""
        img, h, w, step, out = self._bgr_nv12_host(img, out, "clahe_bgr_to_nv12")
        self._chk(self._L.mi_clahe_bgr_to_nv12(self._h, img.ctypes.data, step, out.ctypes.data, w, h, int(order), int(uv_mode),
                                             float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_bgr_to_nv12")
        return out

    # ---- 4:2:0 frames whose sides say where their planes lie: I420 / YV12 / NV12 in, any of them out ----
    def equalize_hist_yuv420_batch_dev(self, src, dst, width, height, n_frames, uv_mode=UV_COPY, stream=0):
        """mi_equalize_hist_yuv420_batch_dev.  src / dst: Yuv420Planes holding device addresses (Yuv420Planes.nv12 / .i420 / .yv12 for
        tight batches, the fields themselves for pitched or separately allocated planes)."""
        self._chk(self._L.mi_equalize_hist_yuv420_batch_dev(self._h, C.byref(src), C.byref(dst), int(width), int(height), int(n_frames),
                                                          int(uv_mode), stream), "mi_equalize_hist_yuv420_batch_dev")

    def clahe_yuv420_batch_dev(self, src, dst, width, height, n_frames, uv_mode=UV_COPY, clip_limit=2.0, tiles_x=8, tiles_y=8, stream=0):
        """mi_clahe_yuv420_batch_dev; arguments as equalize_hist_yuv420_batch_dev, plus the CLAHE parameters."""
        self._chk(self._L.mi_clahe_yuv420_batch_dev(self._h, C.byref(src), C.byref(dst), int(width), int(height), int(n_frames),
                                                  int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_yuv420_batch_dev")

    @staticmethod
    def _yuv420_list(frames):
        """frames: a sequence of Yuv420FrameDev, or a ctypes array of them.  Returns the array and its length."""
        if isinstance(frames, C.Array):
            return frames, len(frames)
        frames = list(frames)
        arr = (Yuv420FrameDev * max(1, len(frames)))()
        for k, f in enumerate(frames):
            arr[k] = f
        return arr, len(frames)

    def equalize_hist_yuv420_frames_dev(self, frames, width, height, y_in_pitch, c_in_pitch, in_chroma, y_out_pitch, c_out_pitch,
                                        out_chroma, uv_mode=UV_COPY, stream=0):
        """mi_equalize_hist_yuv420_frames_dev.  frames: Yuv420FrameDev entries, one per frame, every plane at its own device address (a
        decoder's frame pool in, an encoder's surface pool out); one shape, one set of pitches and one layout per side for the call."""
        arr, n = self._yuv420_list(frames)
        self._chk(self._L.mi_equalize_hist_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(y_in_pitch), int(c_in_pitch),
                                                           int(in_chroma), int(y_out_pitch), int(c_out_pitch), int(out_chroma),
                                                           int(uv_mode), stream), "mi_equalize_hist_yuv420_frames_dev")

    def clahe_yuv420_frames_dev(self, frames, width, height, y_in_pitch, c_in_pitch, in_chroma, y_out_pitch, c_out_pitch, out_chroma,
                                uv_mode=UV_COPY, clip_limit=2.0, tiles_x=8, tiles_y=8, stream=0):
        """mi_clahe_yuv420_frames_dev; arguments as equalize_hist_yuv420_frames_dev, plus the CLAHE parameters."""
        arr, n = self._yuv420_list(frames)
        self._chk(self._L.mi_clahe_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(y_in_pitch), int(c_in_pitch),
                                                   int(in_chroma), int(y_out_pitch), int(c_out_pitch), int(out_chroma), int(uv_mode),
                                                   float(clip_limit), int(tiles_x), int(tiles_y), stream), "mi_clahe_yuv420_frames_dev")

    @staticmethod
    def _yuv420_host(frame, width, height, src_fmt, dst_fmt, out, name):
        n = int(width) * int(height) * 3 // 2
        if src_fmt not in _YUV420_FMTS or dst_fmt not in _YUV420_FMTS:
            raise MiError(1, name, 'src_fmt / dst_fmt must be "nv12", "i420" or "yv12"')
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or not frame.flags.c_contiguous or frame.size != n:
            raise MiError(1, name, "frame must be a contiguous uint8 array of width*height*3/2 bytes")
        if out is None:
            out = np.empty(n, np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.size != n:
            raise MiError(1, name, "out must be a contiguous uint8 array of width*height*3/2 bytes")
        return _YUV420_FMTS[src_fmt](frame.ctypes.data, width, height), _YUV420_FMTS[dst_fmt](out.ctypes.data, width, height), out

    def equalize_hist_yuv420(self, frame: np.ndarray, width: int, height: int, src_fmt: str, dst_fmt: str, uv_mode: int = UV_COPY,
                             out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_yuv420 on a tight host frame of W*H*3/2 bytes: src_fmt / dst_fmt in {"nv12", "i420", "yv12"} say how the
        chroma of `frame` and of the result lies; the result is `out` when given, else a new array."""
        a, b, out = self._yuv420_host(frame, width, height, src_fmt, dst_fmt, out, "equalize_hist_yuv420")
        self._chk(self._L.mi_equalize_hist_yuv420(self._h, C.byref(a), C.byref(b), int(width), int(height), int(uv_mode)),
                  "mi_equalize_hist_yuv420")
        return out

    def clahe_yuv420(self, frame: np.ndarray, width: int, height: int, src_fmt: str, dst_fmt: str, uv_mode: int = UV_COPY,
                     clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_yuv420; arguments as equalize_hist_yuv420, plus the CLAHE parameters."""
        a, b, out = self._yuv420_host(frame, width, height, src_fmt, dst_fmt, out, "clahe_yuv420")
        self._chk(self._L.mi_clahe_yuv420(self._h, C.byref(a), C.byref(b), int(width), int(height), int(uv_mode), float(clip_limit),
                                        int(tiles_x), int(tiles_y)), "mi_clahe_yuv420")
        return out

    # ---- 4:2:0 frames (I420 / YV12 planes, or NV12) in, interleaved BGR / RGB out in the pass that maps the luma ----
    def equalize_hist_yuv420_to_bgr_batch_dev(self, src, d_out, width, height, n_frames, order=ORDER_BGR, out_pitch=None, out_frame=None,
                                              stream=0):
        """mi_equalize_hist_yuv420_to_bgr_batch_dev.  src: a Yuv420Planes holding device addresses (Yuv420Planes.i420 / .yv12 / .nv12 for
        tight batches, the fields themselves for pitched or separately allocated planes); d_out: the images (a torch tensor or a raw
        address).  The tight output is the default: out_pitch 3*W, out_frame = out_pitch * H."""
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_yuv420_to_bgr_batch_dev(self._h, C.byref(src), _dptr(d_out), op, fo, int(width), int(height),
                                                                 int(n_frames), int(order), stream),
                  "mi_equalize_hist_yuv420_to_bgr_batch_dev")

    def clahe_yuv420_to_bgr_batch_dev(self, src, d_out, width, height, n_frames, order=ORDER_BGR, clip_limit=2.0, tiles_x=8, tiles_y=8,
                                      out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_yuv420_to_bgr_batch_dev; arguments as equalize_hist_yuv420_to_bgr_batch_dev, plus the CLAHE parameters."""
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_yuv420_to_bgr_batch_dev(self._h, C.byref(src), _dptr(d_out), op, fo, int(width), int(height),
                                                         int(n_frames), int(order), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_yuv420_to_bgr_batch_dev")

    @staticmethod
    def _yuv420_bgr_list(frames):
        """frames: a sequence of Yuv420BgrFrameDev, or a ctypes array of them.  Returns the array and its length."""
        if isinstance(frames, C.Array):
            return frames, len(frames)
        frames = list(frames)
        arr = (Yuv420BgrFrameDev * max(1, len(frames)))()
        for k, f in enumerate(frames):
            arr[k] = f
        return arr, len(frames)

    def equalize_hist_yuv420_to_bgr_frames_dev(self, frames, width, height, y_pitch, c_pitch, chroma, order=ORDER_BGR, out_pitch=None,
                                               stream=0):
        """mi_equalize_hist_yuv420_to_bgr_frames_dev.  frames: Yuv420BgrFrameDev entries, one per frame, every plane and every image at
        its own device address (a software decoder's frame pool in, an image pool out); one shape, one set of pitches and one chroma
        layout for the call.  The tight image is the default: out_pitch 3*W."""
        arr, n = self._yuv420_bgr_list(frames)
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        self._chk(self._L.mi_equalize_hist_yuv420_to_bgr_frames_dev(self._h, arr, n, int(width), int(height), int(y_pitch), int(c_pitch),
                                                                  int(chroma), op, int(order), stream),
                  "mi_equalize_hist_yuv420_to_bgr_frames_dev")

    def clahe_yuv420_to_bgr_frames_dev(self, frames, width, height, y_pitch, c_pitch, chroma, order=ORDER_BGR, clip_limit=2.0, tiles_x=8,
                                       tiles_y=8, out_pitch=None, stream=0):
        """mi_clahe_yuv420_to_bgr_frames_dev; arguments as equalize_hist_yuv420_to_bgr_frames_dev, plus the CLAHE parameters."""
        arr, n = self._yuv420_bgr_list(frames)
        op = 3 * int(width) if out_pitch is None else int(out_pitch)
        self._chk(self._L.mi_clahe_yuv420_to_bgr_frames_dev(self._h, arr, n, int(width), int(height), int(y_pitch), int(c_pitch),
                                                          int(chroma), op, int(order), float(clip_limit), int(tiles_x), int(tiles_y),
                                                          stream), "mi_clahe_yuv420_to_bgr_frames_dev")

    def _yuv420_bgr_host(self, frame, width, height, src_fmt, out, name):
        if src_fmt not in _YUV420_FMTS:
            raise MiError(1, name, 'src_fmt must be "nv12", "i420" or "yv12"')
        out, step = self._nv12_bgr_host(frame, width, height, out, name)
        return _YUV420_FMTS[src_fmt](frame.ctypes.data, width, height), out, step

    def equalize_hist_yuv420_to_bgr(self, frame: np.ndarray, width: int, height: int, src_fmt: str, order: int = ORDER_BGR,
                                    out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_yuv420_to_bgr on a tight host frame of W*H*3/2 bytes whose chroma lies as src_fmt in {"nv12", "i420", "yv12"}
        says: the H x W x 3 image out -- `out` when given (a view with padded rows included), else a new tight array."""
        a, out, step = self._yuv420_bgr_host(frame, int(width), int(height), src_fmt, out, "equalize_hist_yuv420_to_bgr")
        self._chk(self._L.mi_equalize_hist_yuv420_to_bgr(self._h, C.byref(a), out.ctypes.data, step, int(width), int(height), int(order)),
                  "mi_equalize_hist_yuv420_to_bgr")
        return out

    def clahe_yuv420_to_bgr(self, frame: np.ndarray, width: int, height: int, src_fmt: str, order: int = ORDER_BGR,
                            clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_yuv420_to_bgr; arguments as equalize_hist_yuv420_to_bgr, plus the CLAHE parameters."""
        a, out, step = self._yuv420_bgr_host(frame, int(width), int(height), src_fmt, out, "clahe_yuv420_to_bgr")
        self._chk(self._L.mi_clahe_yuv420_to_bgr(self._h, C.byref(a), out.ctypes.data, step, int(width), int(height), int(order),
                                               float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_yuv420_to_bgr")
        return out

    # ---- interleaved BGR / RGB in, 4:2:0 frames (I420 / YV12 planes, or NV12) out: convert and count in one pass, then map the luma in place ----
    def equalize_hist_bgr_to_yuv420_batch_dev(self, d_in, dst, width, height, n_frames, order=ORDER_BGR, uv_mode=UV_COPY, in_pitch=None,
                                              in_frame=None, stream=0):
        """mi_equalize_hist_bgr_to_yuv420_batch_dev.  d_in: the images (a torch tensor or a raw address); dst: a Yuv420Planes holding
        device addresses (Yuv420Planes.i420 / .yv12 / .nv12 for tight batches, the fields themselves for pitched or separately allocated
        planes).  The tight input is the default: in_pitch 3*W, in_frame = in_pitch * H."""
        ip = 3 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        self._chk(self._L.mi_equalize_hist_bgr_to_yuv420_batch_dev(self._h, _dptr(d_in), ip, fi, C.byref(dst), int(width), int(height),
                                                                 int(n_frames), int(order), int(uv_mode), stream),
                  "mi_equalize_hist_bgr_to_yuv420_batch_dev")

    def clahe_bgr_to_yuv420_batch_dev(self, d_in, dst, width, height, n_frames, order=ORDER_BGR, uv_mode=UV_COPY, clip_limit=2.0,
                                      tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, stream=0):
        """mi_clahe_bgr_to_yuv420_batch_dev; arguments as equalize_hist_bgr_to_yuv420_batch_dev, plus the CLAHE parameters."""
        ip = 3 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        self._chk(self._L.mi_clahe_bgr_to_yuv420_batch_dev(self._h, _dptr(d_in), ip, fi, C.byref(dst), int(width), int(height),
                                                         int(n_frames), int(order), int(uv_mode), float(clip_limit), int(tiles_x),
                                                         int(tiles_y), stream), "mi_clahe_bgr_to_yuv420_batch_dev")

    def _bgr_yuv420_host(self, img, dst_fmt, out, name):
        if dst_fmt not in _YUV420_FMTS:
            raise MiError(1, name, 'dst_fmt must be "nv12", "i420" or "yv12"')
        img, h, w, step, out = self._bgr_nv12_host(img, out, name)
        return img, h, w, step, out, _YUV420_FMTS[dst_fmt](out.ctypes.data, w, h)

    def equalize_hist_bgr_to_yuv420(self, img: np.ndarray, dst_fmt: str = "i420", order: int = ORDER_BGR, uv_mode: int = UV_COPY,
                                    out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_bgr_to_yuv420 on a host image: an H x W x 3 uint8 array in (a view with padded rows included), the tight frame
        of W*H*3/2 bytes out, its chroma laid out as dst_fmt in {"nv12", "i420", "yv12"} says -- `out` when given, else a new array."""
        img, h, w, step, out, b = self._bgr_yuv420_host(img, dst_fmt, out, "equalize_hist_bgr_to_yuv420")
        self._chk(self._L.mi_equalize_hist_bgr_to_yuv420(self._h, img.ctypes.data, step, C.byref(b), w, h, int(order), int(uv_mode)),
                  "mi_equalize_hist_bgr_to_yuv420")
        return out

    def clahe_bgr_to_yuv420(self, img: np.ndarray, dst_fmt: str = "i420", order: int = ORDER_BGR, uv_mode: int = UV_COPY,
                            clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_bgr_to_yuv420; arguments as equalize_hist_bgr_to_yuv420, plus the CLAHE parameters."""
        img, h, w, step, out, b = self._bgr_yuv420_host(img, dst_fmt, out, "clahe_bgr_to_yuv420")
        self._chk(self._L.mi_clahe_bgr_to_yuv420(self._h, img.ctypes.data, step, C.byref(b), w, h, int(order), int(uv_mode),
                                               float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_bgr_to_yuv420")
        return out

    @staticmethod
    def _bgr_yuv420_list(frames):
        """frames: a sequence of BgrYuv420FrameDev, or a ctypes array of them.  Returns the array and its length."""
        if isinstance(frames, C.Array):
            return frames, len(frames)
        frames = list(frames)
        arr = (BgrYuv420FrameDev * max(1, len(frames)))()
        for k, f in enumerate(frames):
            arr[k] = f
        return arr, len(frames)

    def equalize_hist_bgr_to_yuv420_frames_dev(self, frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order=ORDER_BGR,
                                               uv_mode=UV_COPY, stream=0):
        """mi_equalize_hist_bgr_to_yuv420_frames_dev.  frames: BgrYuv420FrameDev entries, one per frame, every image and every plane at
        its own device address (an image pool in, a software encoder's frame pool out); one shape, one set of pitches and one chroma
        layout for the call."""
        arr, n = self._bgr_yuv420_list(frames)
        self._chk(self._L.mi_equalize_hist_bgr_to_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(in_pitch), int(y_pitch),
                                                                  int(c_pitch), int(chroma), int(order), int(uv_mode), stream),
                  "mi_equalize_hist_bgr_to_yuv420_frames_dev")

    def clahe_bgr_to_yuv420_frames_dev(self, frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order=ORDER_BGR, uv_mode=UV_COPY,
                                       clip_limit=2.0, tiles_x=8, tiles_y=8, stream=0):
        """mi_clahe_bgr_to_yuv420_frames_dev; arguments as equalize_hist_bgr_to_yuv420_frames_dev, plus the CLAHE parameters."""
        arr, n = self._bgr_yuv420_list(frames)
        self._chk(self._L.mi_clahe_bgr_to_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(in_pitch), int(y_pitch),
                                                          int(c_pitch), int(chroma), int(order), int(uv_mode), float(clip_limit),
                                                          int(tiles_x), int(tiles_y), stream), "mi_clahe_bgr_to_yuv420_frames_dev")

    # ---- four-channel BGRA / RGBA (CV_8UC4) in, 4:2:0 frames (I420 / YV12 planes, or NV12) out: the fourth byte takes no part ----
    def equalize_hist_bgra_to_yuv420_batch_dev(self, d_in, dst, width, height, n_frames, order=ORDER_BGR, uv_mode=UV_COPY, in_pitch=None,
                                               in_frame=None, stream=0):
        """mi_equalize_hist_bgra_to_yuv420_batch_dev.  d_in: the four-byte-per-pixel images (a torch tensor or a raw address); dst: a
        Yuv420Planes holding device addresses (Yuv420Planes.i420 / .yv12 / .nv12 for tight batches, the fields themselves for pitched or
        separately allocated planes).  The tight input is the default: in_pitch 4*W, in_frame = in_pitch * H."""
        ip = 4 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        self._chk(self._L.mi_equalize_hist_bgra_to_yuv420_batch_dev(self._h, _dptr(d_in), ip, fi, C.byref(dst), int(width), int(height),
                                                                  int(n_frames), int(order), int(uv_mode), stream),
                  "mi_equalize_hist_bgra_to_yuv420_batch_dev")

    def clahe_bgra_to_yuv420_batch_dev(self, d_in, dst, width, height, n_frames, order=ORDER_BGR, uv_mode=UV_COPY, clip_limit=2.0,
                                       tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, stream=0):
        """mi_clahe_bgra_to_yuv420_batch_dev; arguments as equalize_hist_bgra_to_yuv420_batch_dev, plus the CLAHE parameters."""
        ip = 4 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        self._chk(self._L.mi_clahe_bgra_to_yuv420_batch_dev(self._h, _dptr(d_in), ip, fi, C.byref(dst), int(width), int(height),
                                                          int(n_frames), int(order), int(uv_mode), float(clip_limit), int(tiles_x),
                                                          int(tiles_y), stream), "mi_clahe_bgra_to_yuv420_batch_dev")

    def _bgra_yuv420_host(self, img, dst_fmt, out, name):
        if dst_fmt not in _YUV420_FMTS:
            raise MiError(1, name, 'dst_fmt must be "nv12", "i420" or "yv12"')
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4:
            raise MiError(2, name, "expected an HxWx4 uint8 ndarray (CV_8UC4)")
        if img.size and (img.strides[2] != 1 or img.strides[1] != 4):
            raise MiError(1, name, "pixels must be interleaved")
        h, w = img.shape[:2]
        if out is None:
            out = np.empty(w * h * 3 // 2, np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.c_contiguous or out.size != w * h * 3 // 2:
            raise MiError(1, name, "out must be a contiguous uint8 array of width*height*3/2 bytes")
        step = int(img.strides[0]) if h > 1 else max(int(img.strides[0]), 4 * w)
        return img, h, w, step, out, _YUV420_FMTS[dst_fmt](out.ctypes.data, w, h)

    def equalize_hist_bgra_to_yuv420(self, img: np.ndarray, dst_fmt: str = "i420", order: int = ORDER_BGR, uv_mode: int = UV_COPY,
                                     out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_bgra_to_yuv420 on a host image: an H x W x 4 uint8 array in (a view with padded rows included), the tight
        frame of W*H*3/2 bytes out, its chroma laid out as dst_fmt in {"nv12", "i420", "yv12"} says -- `out` when given, else a new array."""
        img, h, w, step, out, b = self._bgra_yuv420_host(img, dst_fmt, out, "equalize_hist_bgra_to_yuv420")
        self._chk(self._L.mi_equalize_hist_bgra_to_yuv420(self._h, img.ctypes.data, step, C.byref(b), w, h, int(order), int(uv_mode)),
                  "mi_equalize_hist_bgra_to_yuv420")
        return out

    def clahe_bgra_to_yuv420(self, img: np.ndarray, dst_fmt: str = "i420", order: int = ORDER_BGR, uv_mode: int = UV_COPY,
                             clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_bgra_to_yuv420; arguments as equalize_hist_bgra_to_yuv420, plus the CLAHE parameters."""
        img, h, w, step, out, b = self._bgra_yuv420_host(img, dst_fmt, out, "clahe_bgra_to_yuv420")
        self._chk(self._L.mi_clahe_bgra_to_yuv420(self._h, img.ctypes.data, step, C.byref(b), w, h, int(order), int(uv_mode),
                                                float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_bgra_to_yuv420")
        return out

    def equalize_hist_bgra_to_yuv420_frames_dev(self, frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order=ORDER_BGR,
                                                uv_mode=UV_COPY, stream=0):
        """mi_equalize_hist_bgra_to_yuv420_frames_dev.  frames: BgrYuv420FrameDev entries, one per frame, every four-byte-per-pixel image
        and every plane at its own device address (a surface pool in, an encoder's frame pool out); one shape, one set of pitches and
        one chroma layout for the call (c1 is ignored on an interleaved list)."""
        arr, n = self._bgr_yuv420_list(frames)
        self._chk(self._L.mi_equalize_hist_bgra_to_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(in_pitch), int(y_pitch),
                                                                   int(c_pitch), int(chroma), int(order), int(uv_mode), stream),
                  "mi_equalize_hist_bgra_to_yuv420_frames_dev")

    def clahe_bgra_to_yuv420_frames_dev(self, frames, width, height, in_pitch, y_pitch, c_pitch, chroma, order=ORDER_BGR, uv_mode=UV_COPY,
                                        clip_limit=2.0, tiles_x=8, tiles_y=8, stream=0):
        """mi_clahe_bgra_to_yuv420_frames_dev; arguments as equalize_hist_bgra_to_yuv420_frames_dev, plus the CLAHE parameters."""
        arr, n = self._bgr_yuv420_list(frames)
        self._chk(self._L.mi_clahe_bgra_to_yuv420_frames_dev(self._h, arr, n, int(width), int(height), int(in_pitch), int(y_pitch),
                                                           int(c_pitch), int(chroma), int(order), int(uv_mode), float(clip_limit),
                                                           int(tiles_x), int(tiles_y), stream), "mi_clahe_bgra_to_yuv420_frames_dev")

    # ---- 4:2:0 frames (I420 / YV12 planes, or NV12) in, four-channel BGRA / RGBA (CV_8UC4, A = 255) out in the pass that maps the luma ----
    def equalize_hist_yuv420_to_bgra_batch_dev(self, src, d_out, width, height, n_frames, order=ORDER_BGR, out_pitch=None, out_frame=None,
                                               stream=0):
        """mi_equalize_hist_yuv420_to_bgra_batch_dev.  src: a Yuv420Planes holding device addresses (Yuv420Planes.i420 / .yv12 / .nv12 for
        tight batches, the fields themselves for pitched or separately allocated planes); d_out: the four-byte-per-pixel images (a torch
        tensor or a raw address).  The tight output is the default: out_pitch 4*W, out_frame = out_pitch * H."""
        op = 4 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_yuv420_to_bgra_batch_dev(self._h, C.byref(src), _dptr(d_out), op, fo, int(width), int(height),
                                                                  int(n_frames), int(order), stream),
                  "mi_equalize_hist_yuv420_to_bgra_batch_dev")

    def clahe_yuv420_to_bgra_batch_dev(self, src, d_out, width, height, n_frames, order=ORDER_BGR, clip_limit=2.0, tiles_x=8, tiles_y=8,
                                       out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_yuv420_to_bgra_batch_dev; arguments as equalize_hist_yuv420_to_bgra_batch_dev, plus the CLAHE parameters."""
        op = 4 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_yuv420_to_bgra_batch_dev(self._h, C.byref(src), _dptr(d_out), op, fo, int(width), int(height),
                                                          int(n_frames), int(order), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_yuv420_to_bgra_batch_dev")

    def equalize_hist_yuv420_to_bgra_frames_dev(self, frames, width, height, y_pitch, c_pitch, chroma, order=ORDER_BGR, out_pitch=None,
                                                stream=0):
        """mi_equalize_hist_yuv420_to_bgra_frames_dev.  frames: Yuv420BgrFrameDev entries, one per frame, every plane and every
        four-byte-per-pixel image at its own device address (a decoder's frame pool in, a surface pool out; c1 None on an interleaved
        list); one shape, one set of pitches and one chroma layout for the call.  The tight image is the default: out_pitch 4*W."""
        arr, n = self._yuv420_bgr_list(frames)
        op = 4 * int(width) if out_pitch is None else int(out_pitch)
        self._chk(self._L.mi_equalize_hist_yuv420_to_bgra_frames_dev(self._h, arr, n, int(width), int(height), int(y_pitch), int(c_pitch),
                                                                   int(chroma), op, int(order), stream),
                  "mi_equalize_hist_yuv420_to_bgra_frames_dev")

    def clahe_yuv420_to_bgra_frames_dev(self, frames, width, height, y_pitch, c_pitch, chroma, order=ORDER_BGR, clip_limit=2.0, tiles_x=8,
                                        tiles_y=8, out_pitch=None, stream=0):
        """mi_clahe_yuv420_to_bgra_frames_dev; arguments as equalize_hist_yuv420_to_bgra_frames_dev, plus the CLAHE parameters."""
        arr, n = self._yuv420_bgr_list(frames)
        op = 4 * int(width) if out_pitch is None else int(out_pitch)
        self._chk(self._L.mi_clahe_yuv420_to_bgra_frames_dev(self._h, arr, n, int(width), int(height), int(y_pitch), int(c_pitch),
                                                           int(chroma), op, int(order), float(clip_limit), int(tiles_x), int(tiles_y),
                                                           stream), "mi_clahe_yuv420_to_bgra_frames_dev")

    def _yuv420_bgra_host(self, frame, width, height, src_fmt, out, name):
        if src_fmt not in _YUV420_FMTS:
            raise MiError(1, name, 'src_fmt must be "nv12", "i420" or "yv12"')
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or not frame.flags.c_contiguous:
            raise MiError(2, name, "expected a contiguous uint8 ndarray")
        if width >= 0 and height >= 0 and frame.size != width * height * 3 // 2:
            raise MiError(1, name, "4:2:0 frame must hold width*height*3/2 bytes")
        if out is None:
            out = np.empty((max(height, 0), max(width, 0), 4), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 3 or out.shape[2] != 4:
            raise MiError(2, name, "expected an HxWx4 uint8 ndarray (CV_8UC4)")
        if out.size and (out.strides[2] != 1 or out.strides[1] != 4):
            raise MiError(1, name, "pixels must be interleaved")
        if out.shape[:2] != (height, width):
            raise MiError(1, name, "out must be an H x W x 4 uint8 array (rows may be padded)")
        step = int(out.strides[0]) if height > 1 else max(int(out.strides[0]), 4 * width)
        return _YUV420_FMTS[src_fmt](frame.ctypes.data, width, height), out, step

    def equalize_hist_yuv420_to_bgra(self, frame: np.ndarray, width: int, height: int, src_fmt: str, order: int = ORDER_BGR,
                                     out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_yuv420_to_bgra on a tight host frame of W*H*3/2 bytes whose chroma lies as src_fmt in {"nv12", "i420", "yv12"}
        says: the H x W x 4 image out, A = 255 -- `out` when given (a view with padded rows included), else a new tight array."""
        a, out, step = self._yuv420_bgra_host(frame, int(width), int(height), src_fmt, out, "equalize_hist_yuv420_to_bgra")
        self._chk(self._L.mi_equalize_hist_yuv420_to_bgra(self._h, C.byref(a), out.ctypes.data, step, int(width), int(height), int(order)),
                  "mi_equalize_hist_yuv420_to_bgra")
        return out

    def clahe_yuv420_to_bgra(self, frame: np.ndarray, width: int, height: int, src_fmt: str, order: int = ORDER_BGR,
                             clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_yuv420_to_bgra; arguments as equalize_hist_yuv420_to_bgra, plus the CLAHE parameters."""
        a, out, step = self._yuv420_bgra_host(frame, int(width), int(height), src_fmt, out, "clahe_yuv420_to_bgra")
        self._chk(self._L.mi_clahe_yuv420_to_bgra(self._h, C.byref(a), out.ctypes.data, step, int(width), int(height), int(order),
                                                float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_yuv420_to_bgra")
        return out

    # ---- interleaved BGR / RGB in, packed 4:2:2 (YUY2 / UYVY) out: convert and count in one pass, then map the luma in place ----
    def equalize_hist_bgr_to_packed422_batch_dev(self, d_in, d_out, width, height, n_frames, order=ORDER_BGR, fmt=FMT_YUY2,
                                                 uv_mode=UV_COPY, in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_bgr_to_packed422_batch_dev: n_frames interleaved BGR / RGB images in, packed 4:2:2 frames out (torch tensors
        or raw addresses).  Tight layouts are the defaults: in_pitch 3*W, in_frame = in_pitch * H, out_pitch 2*W, out_frame =
        out_pitch * H."""
        ip = 3 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_bgr_to_packed422_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width),
                                                                    int(height), int(n_frames), int(order), int(fmt), int(uv_mode),
                                                                    stream), "mi_equalize_hist_bgr_to_packed422_batch_dev")

    def clahe_bgr_to_packed422_batch_dev(self, d_in, d_out, width, height, n_frames, order=ORDER_BGR, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                         clip_limit=2.0, tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, out_pitch=None,
                                         out_frame=None, stream=0):
        """mi_clahe_bgr_to_packed422_batch_dev; arguments as equalize_hist_bgr_to_packed422_batch_dev, plus the CLAHE parameters."""
        ip = 3 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_bgr_to_packed422_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                            int(n_frames), int(order), int(fmt), int(uv_mode), float(clip_limit),
                                                            int(tiles_x), int(tiles_y), stream), "mi_clahe_bgr_to_packed422_batch_dev")

    def equalize_hist_bgr_to_packed422_frames(self, ins, outs, width, height, order=ORDER_BGR, fmt=FMT_YUY2, uv_mode=UV_COPY, in_pitch=None,
                                              out_pitch=None, stream=0):
        """mi_equalize_hist_bgr_to_packed422_frames_dev.  ins: the images, outs: the packed frames, each its own buffer -- lists of torch
        CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row stride of the 2-D tensors of that
        list (H x W x 3 images: of their rows), or the tight one (3 * width; 2 * width)."""
        arr, n, ip, op = _bgr_packed422_list(ins, outs, width, in_pitch, out_pitch, "equalize_hist_bgr_to_packed422_frames")
        self._chk(self._L.mi_equalize_hist_bgr_to_packed422_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(order),
                                                                     int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_bgr_to_packed422_frames_dev")

    def clahe_bgr_to_packed422_frames(self, ins, outs, width, height, order=ORDER_BGR, fmt=FMT_YUY2, uv_mode=UV_COPY, clip_limit=2.0,
                                      tiles_x=8, tiles_y=8, in_pitch=None, out_pitch=None, stream=0):
        """mi_clahe_bgr_to_packed422_frames_dev; arguments as equalize_hist_bgr_to_packed422_frames, plus the CLAHE parameters."""
        arr, n, ip, op = _bgr_packed422_list(ins, outs, width, in_pitch, out_pitch, "clahe_bgr_to_packed422_frames")
        self._chk(self._L.mi_clahe_bgr_to_packed422_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(order), int(fmt),
                                                             int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_bgr_to_packed422_frames_dev")

    def _bgr_packed422_host(self, img, out, name):
        img = self._host3(img, name)
        h, w = img.shape[:2]
        if out is None:
            out = np.empty((h, 2 * w), np.uint8)
        out = self._packed_host(out, w, name)
        if out.shape[0] != h:
            raise MiError(1, name, "out must have one row per image row")
        return img, h, w, (int(img.strides[0]) if h > 1 else max(int(img.strides[0]), 3 * w)), out

    def equalize_hist_bgr_to_packed422(self, img: np.ndarray, order: int = ORDER_BGR, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                                       out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_bgr_to_packed422 on a host image: an H x W x 3 uint8 array in (a view with padded rows included), the packed
        frame out -- `out` when given (an H x pitch-bytes uint8 array, pitch >= 2*W; a view with padded rows is fine), else a new tight
        H x 2W array."""
        img, h, w, step, out = self._bgr_packed422_host(img, out, "equalize_hist_bgr_to_packed422")
        self._chk(self._L.mi_equalize_hist_bgr_to_packed422(self._h, img.ctypes.data, step, out.ctypes.data, _step(out), w, h, int(order),
                                                          int(fmt), int(uv_mode)), "mi_equalize_hist_bgr_to_packed422")
        return out

    def clahe_bgr_to_packed422(self, img: np.ndarray, order: int = ORDER_BGR, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                               clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_bgr_to_packed422; arguments as equalize_hist_bgr_to_packed422, plus the CLAHE parameters."""
        img, h, w, step, out = self._bgr_packed422_host(img, out, "clahe_bgr_to_packed422")
        self._chk(self._L.mi_clahe_bgr_to_packed422(self._h, img.ctypes.data, step, out.ctypes.data, _step(out), w, h, int(order), int(fmt),
                                                  int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_bgr_to_packed422")
        return out

    # ---- four-channel BGRA / RGBA (CV_8UC4) in, packed 4:2:2 (YUY2 / UYVY) out: the fourth byte ignored, stage 2 as above ----
    def equalize_hist_bgra_to_packed422_batch_dev(self, d_in, d_out, width, height, n_frames, order=ORDER_BGR, fmt=FMT_YUY2,
                                                 uv_mode=UV_COPY, in_pitch=None, in_frame=None, out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_bgra_to_packed422_batch_dev: n_frames four-channel BGRA / RGBA (CV_8UC4) images in, packed 4:2:2 frames out (torch tensors
        or raw addresses).  Tight layouts are the defaults: in_pitch 4*W, in_frame = in_pitch * H, out_pitch 2*W, out_frame =
        out_pitch * H."""
        ip = 4 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_bgra_to_packed422_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width),
                                                                    int(height), int(n_frames), int(order), int(fmt), int(uv_mode),
                                                                    stream), "mi_equalize_hist_bgra_to_packed422_batch_dev")

    def clahe_bgra_to_packed422_batch_dev(self, d_in, d_out, width, height, n_frames, order=ORDER_BGR, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                         clip_limit=2.0, tiles_x=8, tiles_y=8, in_pitch=None, in_frame=None, out_pitch=None,
                                         out_frame=None, stream=0):
        """mi_clahe_bgra_to_packed422_batch_dev; arguments as equalize_hist_bgra_to_packed422_batch_dev, plus the CLAHE parameters."""
        ip = 4 * int(width) if in_pitch is None else int(in_pitch)
        fi = ip * int(height) if in_frame is None else int(in_frame)
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_bgra_to_packed422_batch_dev(self._h, _dptr(d_in), ip, fi, _dptr(d_out), op, fo, int(width), int(height),
                                                            int(n_frames), int(order), int(fmt), int(uv_mode), float(clip_limit),
                                                            int(tiles_x), int(tiles_y), stream), "mi_clahe_bgra_to_packed422_batch_dev")

    def equalize_hist_bgra_to_packed422_frames(self, ins, outs, width, height, order=ORDER_BGR, fmt=FMT_YUY2, uv_mode=UV_COPY, in_pitch=None,
                                              out_pitch=None, stream=0):
        """mi_equalize_hist_bgra_to_packed422_frames_dev.  ins: the images, outs: the packed frames, each its own buffer -- lists of torch
        CUDA tensors or raw device addresses, one entry per frame.  A pitch left at None is the row stride of the 2-D tensors of that
        list (H x W x 4 images: of their rows), or the tight one (4 * width; 2 * width)."""
        arr, n, ip, op = _bgr_packed422_list(ins, outs, width, in_pitch, out_pitch, "equalize_hist_bgra_to_packed422_frames", ch=4)
        self._chk(self._L.mi_equalize_hist_bgra_to_packed422_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(order),
                                                                     int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_bgra_to_packed422_frames_dev")

    def clahe_bgra_to_packed422_frames(self, ins, outs, width, height, order=ORDER_BGR, fmt=FMT_YUY2, uv_mode=UV_COPY, clip_limit=2.0,
                                      tiles_x=8, tiles_y=8, in_pitch=None, out_pitch=None, stream=0):
        """mi_clahe_bgra_to_packed422_frames_dev; arguments as equalize_hist_bgra_to_packed422_frames, plus the CLAHE parameters."""
        arr, n, ip, op = _bgr_packed422_list(ins, outs, width, in_pitch, out_pitch, "clahe_bgra_to_packed422_frames", ch=4)
        self._chk(self._L.mi_clahe_bgra_to_packed422_frames_dev(self._h, arr, n, int(width), int(height), ip, op, int(order), int(fmt),
                                                             int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_clahe_bgra_to_packed422_frames_dev")

    def _bgra_packed422_host(self, img, out, name):
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4:
            raise MiError(2, name, "expected an HxWx4 uint8 ndarray (CV_8UC4)")
        if img.size and (img.strides[2] != 1 or img.strides[1] != 4):
            raise MiError(1, name, "pixels must be interleaved")
        h, w = img.shape[:2]
        if out is None:
            out = np.empty((h, 2 * w), np.uint8)
        out = self._packed_host(out, w, name)
        if out.shape[0] != h:
            raise MiError(1, name, "out must have one row per image row")
        return img, h, w, (int(img.strides[0]) if h > 1 else max(int(img.strides[0]), 4 * w)), out

    def equalize_hist_bgra_to_packed422(self, img: np.ndarray, order: int = ORDER_BGR, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                                       out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_bgra_to_packed422 on a host image: an H x W x 4 uint8 array in (a view with padded rows included), the packed
        frame out -- `out` when given (an H x pitch-bytes uint8 array, pitch >= 2*W; a view with padded rows is fine), else a new tight
        H x 2W array."""
        img, h, w, step, out = self._bgra_packed422_host(img, out, "equalize_hist_bgra_to_packed422")
        self._chk(self._L.mi_equalize_hist_bgra_to_packed422(self._h, img.ctypes.data, step, out.ctypes.data, _step(out), w, h, int(order),
                                                          int(fmt), int(uv_mode)), "mi_equalize_hist_bgra_to_packed422")
        return out

    def clahe_bgra_to_packed422(self, img: np.ndarray, order: int = ORDER_BGR, fmt: int = FMT_YUY2, uv_mode: int = UV_COPY,
                               clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_bgra_to_packed422; arguments as equalize_hist_bgra_to_packed422, plus the CLAHE parameters."""
        img, h, w, step, out = self._bgra_packed422_host(img, out, "clahe_bgra_to_packed422")
        self._chk(self._L.mi_clahe_bgra_to_packed422(self._h, img.ctypes.data, step, out.ctypes.data, _step(out), w, h, int(order), int(fmt),
                                                  int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y)), "mi_clahe_bgra_to_packed422")
        return out

    # ---- 4:2:0 frames (NV12, or I420 / YV12 planes) in, packed 4:2:2 (YUY2 / UYVY) out in the pass that maps the luma ----
    def equalize_hist_yuv420_to_packed422_batch_dev(self, src, d_out, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                                    out_pitch=None, out_frame=None, stream=0):
        """mi_equalize_hist_yuv420_to_packed422_batch_dev.  src: a Yuv420Planes holding device addresses (Yuv420Planes.nv12 / .i420 /
        .yv12 for tight batches, the fields themselves for pitched or separately allocated planes); d_out: the packed frames (a torch
        tensor or a raw address).  The tight output is the default: out_pitch 2*W, out_frame = out_pitch * H."""
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_equalize_hist_yuv420_to_packed422_batch_dev(self._h, C.byref(src), _dptr(d_out), op, fo, int(width),
                                                                       int(height), int(n_frames), int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_yuv420_to_packed422_batch_dev")

    def clahe_yuv420_to_packed422_batch_dev(self, src, d_out, width, height, n_frames, fmt=FMT_YUY2, uv_mode=UV_COPY, clip_limit=2.0,
                                            tiles_x=8, tiles_y=8, out_pitch=None, out_frame=None, stream=0):
        """mi_clahe_yuv420_to_packed422_batch_dev; arguments as equalize_hist_yuv420_to_packed422_batch_dev, plus the CLAHE parameters."""
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        fo = op * int(height) if out_frame is None else int(out_frame)
        self._chk(self._L.mi_clahe_yuv420_to_packed422_batch_dev(self._h, C.byref(src), _dptr(d_out), op, fo, int(width), int(height),
                                                               int(n_frames), int(fmt), int(uv_mode), float(clip_limit), int(tiles_x),
                                                               int(tiles_y), stream), "mi_clahe_yuv420_to_packed422_batch_dev")

    @staticmethod
    def _yuv420_packed422_list(frames):
        """frames: a sequence of Yuv420Packed422FrameDev, or a ctypes array of them.  Returns the array and its length."""
        if isinstance(frames, C.Array):
            return frames, len(frames)
        frames = list(frames)
        arr = (Yuv420Packed422FrameDev * max(1, len(frames)))()
        for k, f in enumerate(frames):
            arr[k] = f
        return arr, len(frames)

    def equalize_hist_yuv420_to_packed422_frames_dev(self, frames, width, height, y_pitch, c_pitch, chroma, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                                     out_pitch=None, stream=0):
        """mi_equalize_hist_yuv420_to_packed422_frames_dev.  frames: Yuv420Packed422FrameDev entries, one per frame, every plane and
        every packed frame at its own device address (a decoder's surface pool in, a playout or v4l2 buffer pool out); one shape, one
        set of pitches, one chroma layout, one format and one uv_mode for the call.  The tight frame is the default: out_pitch 2*W."""
        arr, n = self._yuv420_packed422_list(frames)
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        self._chk(self._L.mi_equalize_hist_yuv420_to_packed422_frames_dev(self._h, arr, n, int(width), int(height), int(y_pitch),
                                                                        int(c_pitch), int(chroma), op, int(fmt), int(uv_mode), stream),
                  "mi_equalize_hist_yuv420_to_packed422_frames_dev")

    def clahe_yuv420_to_packed422_frames_dev(self, frames, width, height, y_pitch, c_pitch, chroma, fmt=FMT_YUY2, uv_mode=UV_COPY,
                                             clip_limit=2.0, tiles_x=8, tiles_y=8, out_pitch=None, stream=0):
        """mi_clahe_yuv420_to_packed422_frames_dev; arguments as equalize_hist_yuv420_to_packed422_frames_dev, plus the CLAHE
        parameters."""
        arr, n = self._yuv420_packed422_list(frames)
        op = 2 * int(width) if out_pitch is None else int(out_pitch)
        self._chk(self._L.mi_clahe_yuv420_to_packed422_frames_dev(self._h, arr, n, int(width), int(height), int(y_pitch), int(c_pitch),
                                                                int(chroma), op, int(fmt), int(uv_mode), float(clip_limit), int(tiles_x),
                                                                int(tiles_y), stream), "mi_clahe_yuv420_to_packed422_frames_dev")

    def _yuv420_packed422_host(self, frame, width, height, src_fmt, out, name):
        if isinstance(frame, Yuv420Planes):                 # host addresses and pitches of the caller's own planes
            a = frame
        else:
            if src_fmt not in _YUV420_FMTS:
                raise MiError(1, name, 'src_fmt must be "nv12", "i420" or "yv12"')
            if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or not frame.flags.c_contiguous:
                raise MiError(2, name, "expected a contiguous uint8 ndarray")
            if width >= 0 and height >= 0 and frame.size != width * height * 3 // 2:
                raise MiError(1, name, "a 4:2:0 frame must hold width*height*3/2 bytes")
            a = _YUV420_FMTS[src_fmt](frame.ctypes.data, width, height)
        if out is None:
            out = np.empty((max(height, 0), 2 * max(width, 0)), np.uint8)
        out = self._packed_host(out, width, name)
        if out.shape[0] != height:
            raise MiError(1, name, "out must have one row per frame row")
        return a, out

    def equalize_hist_yuv420_to_packed422(self, frame, width: int, height: int, src_fmt: str = "nv12", fmt: int = FMT_YUY2,
                                          uv_mode: int = UV_COPY, out: np.ndarray | None = None) -> np.ndarray:
        """mi_equalize_hist_yuv420_to_packed422 on a tight host frame of W*H*3/2 bytes whose chroma lies as src_fmt in {"nv12", "i420",
        "yv12"} says (or a Yuv420Planes of host addresses; src_fmt is then ignored): the packed frame out -- `out` when given (an
        H x pitch-bytes uint8 array, pitch >= 2*W; a view with padded rows is fine), else a new tight H x 2W array."""
        a, out = self._yuv420_packed422_host(frame, int(width), int(height), src_fmt, out, "equalize_hist_yuv420_to_packed422")
        self._chk(self._L.mi_equalize_hist_yuv420_to_packed422(self._h, C.byref(a), out.ctypes.data, _step(out), int(width), int(height),
                                                             int(fmt), int(uv_mode)), "mi_equalize_hist_yuv420_to_packed422")
        return out

    def clahe_yuv420_to_packed422(self, frame, width: int, height: int, src_fmt: str = "nv12", fmt: int = FMT_YUY2,
                                  uv_mode: int = UV_COPY, clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8,
                                  out: np.ndarray | None = None) -> np.ndarray:
        """mi_clahe_yuv420_to_packed422; arguments as equalize_hist_yuv420_to_packed422, plus the CLAHE parameters."""
        a, out = self._yuv420_packed422_host(frame, int(width), int(height), src_fmt, out, "clahe_yuv420_to_packed422")
        self._chk(self._L.mi_clahe_yuv420_to_packed422(self._h, C.byref(a), out.ctypes.data, _step(out), int(width), int(height),
                                                     int(fmt), int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y)),
                  "mi_clahe_yuv420_to_packed422")
        return out

    # ---- colour-domain neighbours (N3) ----
    @staticmethod
    def _host3(a, name):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise MiError(2, name, "expected an HxWx3 uint8 ndarray (CV_8UC3)")
        if a.size and (a.strides[2] != 1 or a.strides[1] != 3):
            raise MiError(1, name, "pixels must be interleaved")
        return a

    def cvt_color(self, src: np.ndarray, code: int, dst: np.ndarray | None = None) -> np.ndarray:
        src = self._host3(src, "cvt_color")
        if dst is None or dst.shape != src.shape:
            dst = np.empty(src.shape, np.uint8)
        h, w = src.shape[:2]
        self._chk(self._L.mi_cvt_color_u8c3(self._h, src.ctypes.data, int(src.strides[0]) if h > 1 else w * 3, dst.ctypes.data,
                                          int(dst.strides[0]) if h > 1 else w * 3, w, h, int(code)), "mi_cvt_color_u8c3")
        return dst

    def bgr_luma_op(self, src: np.ndarray, op: int = OP_EQUALIZE, clip_limit: float = 3.0, tiles_x: int = 4, tiles_y: int = 4,
                    dst: np.ndarray | None = None) -> np.ndarray:
        src = self._host3(src, "bgr_luma_op")
        if dst is None or dst.shape != src.shape:
            dst = np.empty(src.shape, np.uint8)
        h, w = src.shape[:2]
        self._chk(self._L.mi_bgr_luma_op_u8c3(self._h, src.ctypes.data, int(src.strides[0]) if h > 1 else w * 3, dst.ctypes.data,
                                            int(dst.strides[0]) if h > 1 else w * 3, w, h, int(op), float(clip_limit),
                                            int(tiles_x), int(tiles_y)), "mi_bgr_luma_op_u8c3")
        return dst

    def cvt_color_batch_dev(self, src, dst, width, height, n_frames, code, stream=0, src_step=None, src_frame=None, dst_step=None,
                            dst_frame=None):
        """Steps and frame strides in bytes; tight (3*W, step * H) when not given."""
        ss = width * 3 if src_step is None else src_step
        ds = width * 3 if dst_step is None else dst_step
        sf = ss * height if src_frame is None else src_frame
        df = ds * height if dst_frame is None else dst_frame
        self._chk(self._L.mi_cvt_color_u8c3_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df, width, height, n_frames,
                                                    int(code), stream), "mi_cvt_color_u8c3_batch_dev")

    def bgr_luma_op_batch_dev(self, src, dst, width, height, n_frames, op=OP_EQUALIZE, clip_limit=3.0, tiles_x=4, tiles_y=4, stream=0,
                              src_step=None, src_frame=None, dst_step=None, dst_frame=None):
        """Steps and frame strides in bytes; tight (3*W, step * H) when not given."""
        ss = width * 3 if src_step is None else src_step
        ds = width * 3 if dst_step is None else dst_step
        sf = ss * height if src_frame is None else src_frame
        df = ds * height if dst_frame is None else dst_frame
        self._chk(self._L.mi_bgr_luma_op_u8c3_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df, width, height, n_frames,
                                                      int(op), float(clip_limit), int(tiles_x), int(tiles_y), stream),
                  "mi_bgr_luma_op_u8c3_batch_dev")

    def cvt_color_420(self, src: np.ndarray, code: int, dst: np.ndarray | None = None) -> np.ndarray:
        """cv::cvtColor with COLOR_BGR2YUV_I420 (HxWx3 -> (H*3/2)xW) or COLOR_YUV2BGR_NV12 ((H*3/2)xW -> HxWx3)."""
        if not isinstance(src, np.ndarray) or src.dtype != np.uint8:
            raise MiError(2, "cvt_color_420", "expected a uint8 ndarray")
        if code == COLOR_BGR2YUV_I420:
            src = self._host3(src, "cvt_color_420")
            h, w = src.shape[:2]
            shape = (h * 3 // 2, w)
        else:
            src = _host2d(src, "cvt_color_420")
            if src.shape[0] % 3:
                raise MiError(1, "cvt_color_420", "NV12 matrix must have H*3/2 rows")
            h, w = src.shape[0] * 2 // 3, src.shape[1]
            shape = (h, w, 3)
        if dst is None or dst.shape != shape:
            dst = np.empty(shape, np.uint8)
        sstep = int(src.strides[0]) if src.shape[0] > 1 else max(int(src.strides[0]), 1)
        dstep = int(dst.strides[0]) if dst.shape[0] > 1 else max(int(dst.strides[0]), 1)
        self._chk(self._L.mi_cvt_color_420_u8(self._h, src.ctypes.data, sstep, dst.ctypes.data, dstep, w, h, int(code)), "mi_cvt_color_420_u8")
        return dst

    def cvt_color_420_batch_dev(self, src, dst, width, height, n_frames, code, stream=0, src_step=None, src_frame=None, dst_step=None,
                                dst_frame=None):
        """Steps and frame strides in bytes; when not given, tight: the CV_8UC3 side 3*W and step * H, the planar side W and
        step * H*3/2."""
        enc = code == COLOR_BGR2YUV_I420
        ss = (width * 3 if enc else width) if src_step is None else src_step
        ds = (width if enc else width * 3) if dst_step is None else dst_step
        sf = (ss * height if enc else ss * height * 3 // 2) if src_frame is None else src_frame
        df = (ds * height * 3 // 2 if enc else ds * height) if dst_frame is None else dst_frame
        self._chk(self._L.mi_cvt_color_420_u8_batch_dev(self._h, _dptr(src), ss, sf, _dptr(dst), ds, df, width, height, n_frames,
                                                      int(code), stream), "mi_cvt_color_420_u8_batch_dev")

    def nv12_bgr_equalize(self, nv12: np.ndarray, width: int, height: int, out: np.ndarray | None = None) -> np.ndarray:
        """NV12 -> BGR -> equalizeHist on B, G, R -> NV12 (BASELINE.json config 5 read literally)."""
        if not isinstance(nv12, np.ndarray) or nv12.dtype != np.uint8 or not nv12.flags.c_contiguous:
            raise MiError(2, "nv12_bgr_equalize", "expected a contiguous uint8 ndarray")
        if width >= 0 and height >= 0 and nv12.size != width * height * 3 // 2:
            raise MiError(1, "nv12_bgr_equalize", "NV12 frame must hold width*height*3/2 bytes")
        if out is None:
            out = np.empty_like(nv12)
        self._chk(self._L.mi_nv12_bgr_equalize(self._h, nv12.ctypes.data, out.ctypes.data, int(width), int(height)), "mi_nv12_bgr_equalize")
        return out

    def nv12_bgr_equalize_batch_dev(self, src, dst, width, height, n_frames, stream=0, frame_stride=None, in_frame=None, out_frame=None):
        """Frame strides in bytes: in_frame / out_frame per side, else frame_stride for both, else tight (W*H*3/2)."""
        fs = width * height * 3 // 2 if frame_stride is None else int(frame_stride)
        fi = fs if in_frame is None else int(in_frame)
        fo = fs if out_frame is None else int(out_frame)
        self._chk(self._L.mi_nv12_bgr_equalize_batch_dev(self._h, _dptr(src), fi, _dptr(dst), fo, width, height, n_frames, stream),
                  "mi_nv12_bgr_equalize_batch_dev")

    def synchronize(self, stream=0):
        """Wait for `stream`; raises only if the fused path met a frame it refused to repair (see get_stat)."""
        self._chk(self._L.mi_ctx_synchronize(self._h, stream), "mi_ctx_synchronize")

    def get_stat(self, name: str) -> int:
        """Sticky counters of the fused path's fail-soft machinery (mi_ctx_get_stat); synchronise the work's stream first."""
        v = C.c_uint64(0)
        self._chk(self._L.mi_ctx_get_stat(self._h, name.encode(), C.byref(v)), "mi_ctx_get_stat")
        return int(v.value)

    def set_option(self, name: str, value: int):
        self._chk(self._L.mi_ctx_set_option(self._h, name.encode(), int(value)), "mi_ctx_set_option")

    # ---- profiling ----
    def set_profiling(self, on):
        """False / 0: off.  True / 1: HIP events around every kernel.  2: every kernel but the housekeeping launch behind a fused kernel."""
        self._chk(self._L.mi_ctx_set_profiling(self._h, int(on)), "mi_ctx_set_profiling")

    def profile_read(self, reset: bool = True) -> dict:
        p = _Profile()
        self._chk(self._L.mi_ctx_profile_read(self._h, C.byref(p), 1 if reset else 0), "mi_ctx_profile_read")
        return {KERNEL_NAMES[k]: {"total_ms": p.total_ms[k], "launches": int(p.launches[k]), "min_ms": p.min_ms[k], "p10_ms": p.p10_ms[k],
                                  "p50_ms": p.p50_ms[k], "p90_ms": p.p90_ms[k], "max_ms": p.max_ms[k]} for k in range(_K)}


class Pipe:
    """mi_pipe wrapper: asynchronous in-order frame pipeline on one context.  NV12 (format=FMT_NV12): numpy uint8 arrays of W*H*3/2
    bytes; P010 (format=FMT_P010, op=OP_CLAHE): contiguous uint16 arrays of W*H*3/2 samples, e.g. shape (3H/2, W); packed 4:2:2
    (format=FMT_YUY2 / FMT_UYVY): contiguous uint8 arrays of 2*W*H bytes, e.g. shape (H, 2W).
    The arrays handed to submit() are kept alive until wait() returns them."""

    def __init__(self, ctx: Context, width: int, height: int, op: int = OP_EQUALIZE, uv_mode: int = UV_FILL128,
                 clip_limit: float = 2.0, tiles_x: int = 8, tiles_y: int = 8, depth: int = 0, uv_policy: int = PIPE_UV_AUTO,
                 format: int = FMT_NV12):
        self._ctx = ctx
        self._h = C.c_void_p()
        self._held = {}
        cfg = _PipeConfig(int(width), int(height), int(op), int(uv_mode), float(clip_limit), int(tiles_x), int(tiles_y), int(depth), int(uv_policy),
                          int(format))
        ctx._chk(self._ctx._L.mi_pipe_create(ctx._h, C.byref(cfg), C.byref(self._h)), "mi_pipe_create")
        self.format = int(format)
        self._dtype = np.uint16 if self.format == FMT_P010 else np.uint8
        if self.format in (FMT_YUY2, FMT_UYVY):
            self.frame_bytes = 2 * width * height
        else:
            self.frame_bytes = width * height * 3 // 2 * np.dtype(self._dtype).itemsize

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            h, self._h = self._h, None
            self._ctx._L.mi_pipe_destroy(h)
            self._held.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def pending(self) -> int:
        return int(self._ctx._L.mi_pipe_pending(self._h))

    @property
    def depth(self) -> int:
        return int(self._ctx._L.mi_pipe_depth(self._h))

    def submit(self, frame_in: np.ndarray, frame_out: np.ndarray, tag: int) -> bool:
        """False when the pipe is full (MI_ERR_BUSY: call wait() first)."""
        for a in (frame_in, frame_out):
            if not isinstance(a, np.ndarray) or a.dtype != self._dtype or not a.flags.c_contiguous or a.nbytes < self.frame_bytes:
                raise MiError(1, "mi_pipe_submit", "frames must be contiguous uint8 (NV12, packed 4:2:2) / uint16 (P010) arrays of a whole frame")
        rc = self._ctx._L.mi_pipe_submit(self._h, frame_in.ctypes.data, frame_out.ctypes.data, int(tag))
        if rc == ERR_BUSY:
            return False
        self._ctx._chk(rc, "mi_pipe_submit")
        self._held[int(tag)] = (frame_in, frame_out)
        return True

    def wait(self):
        """Blocks for the oldest pending frame; returns (tag, output array)."""
        tag, ptr = C.c_uint64(0), C.c_void_p()
        rc = self._ctx._L.mi_pipe_wait(self._h, C.byref(tag), C.byref(ptr))
        held = self._held.pop(int(tag.value), (None, None))
        self._ctx._chk(rc, "mi_pipe_wait")
        return int(tag.value), held[1]
