"""P010 frame lists (mi_clahe_p010_frames_dev) at the ABI level, without a GPU: the header declares the entry point and the
mi_p010_frame_dev alias of mi_nv12_frame_dev, the C and C++ compilers agree on its layout with the Python binding, both libraries
export the symbol, and a null context is refused without touching a device."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import mi_lumaeq
from mi_lumaeq import capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mi_lumaeq.h"
SYMBOL = "mi_clahe_p010_frames_dev"
MI_ERR_BAD_ARG = 1


def test_header_declares_p010_frame_list_form():
    txt = HEADER.read_text()
    m = re.search(rf"\bmi_status\s+{SYMBOL}\s*\((.*?)\)\s*;", txt, re.S)
    assert m, SYMBOL
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["mi_ctx* ctx", "const mi_p010_frame_dev* frames", "int n_frames", "int width", "int height",
                      "size_t y_in_pitch", "size_t uv_in_pitch", "size_t y_out_pitch", "size_t uv_out_pitch",
                      "mi_uv_mode uv_mode", "double clip_limit", "int tiles_x", "int tiles_y", "void* stream"], params
    assert re.search(r"typedef\s+mi_nv12_frame_dev\s+mi_p010_frame_dev\s*;", txt)
    assert SYMBOL in mi_lumaeq.DECLARED_SYMBOLS
    assert not re.search(r"\bmi_equalize_hist_p010", txt), "OpenCV's equalizeHist is 8-bit only: no 16-bit form"
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", txt), "a symbol was added, no struct grew: the minor version stays"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "the new launches are charged to the existing profiling slots"


LAYOUT = ('int main(void) { mi_nv12_frame_dev* same = (mi_p010_frame_dev*)0; (void)same;\n'
          ' printf("%zu %zu %zu %zu %zu\\n", sizeof(mi_p010_frame_dev), offsetof(mi_p010_frame_dev, y_in),'
          ' offsetof(mi_p010_frame_dev, uv_in), offsetof(mi_p010_frame_dev, y_out), offsetof(mi_p010_frame_dev, uv_out)); return 0; }\n')


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++11")])
def test_alias_layout_matches_c_compiler(tmp_path, lang, std):
    compiler = shutil.which("cc" if lang == "c" else "c++") or shutil.which("gcc" if lang == "c" else "g++")
    if compiler is None:
        pytest.fail(f"no {lang} compiler on PATH")
    src = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi_lumaeq.h"\n' + LAYOUT)
    exe = tmp_path / "probe.bin"
    subprocess.run([compiler, f"-std={std}", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    size, off_y_in, off_uv_in, off_y_out, off_uv_out = map(int, out.split())
    S = capi.Nv12FrameDev
    assert size == ctypes.sizeof(S) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert (off_y_in, off_uv_in, off_y_out, off_uv_out) == (S.y_in.offset, S.uv_in.offset, S.y_out.offset, S.uv_out.offset)


def test_libraries_export_p010_frame_list_form(built_lib):
    for L in (built_lib, capi.test_lib()):
        assert hasattr(L, SYMBOL), f"{L._name} does not export {SYMBOL}"


def test_null_context_is_bad_arg_without_a_device(built_lib):
    """A null context is refused before any HIP call: no device is needed, and the frame list is not touched."""
    L = built_lib
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf)
    frames = (capi.Nv12FrameDev * 2)(capi.Nv12FrameDev(p, p + 64, p, p + 64), capi.Nv12FrameDev(p, p + 64, p, p + 64))
    before = bytes(frames)
    assert L.mi_clahe_p010_frames_dev(None, frames, 2, 8, 4, 16, 16, 16, 16, 1, 2.0, 2, 2, None) == MI_ERR_BAD_ARG
    assert L.mi_clahe_p010_frames_dev(None, None, 0, 0, 0, 0, 0, 0, 0, 0, 2.0, 8, 8, None) == MI_ERR_BAD_ARG
    assert bytes(frames) == before and not any(buf)
