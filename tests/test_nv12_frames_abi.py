"""NV12 frame lists (mi_*_nv12_frames_dev) at the ABI level, without a GPU: the header declares the two entry points and the
mi_nv12_frame_dev struct and compiles as C99 and C++11, the struct's layout from the C compiler matches the Python binding, both
libraries export the symbols, and a null context is refused without touching a device."""
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
SYMBOLS = ("mi_equalize_hist_nv12_frames_dev", "mi_clahe_nv12_frames_dev")
MI_ERR_BAD_ARG = 1


def test_header_declares_frame_list_forms():
    txt = HEADER.read_text()
    for s in SYMBOLS:
        assert re.search(rf"\bmi_status\s+{s}\s*\(\s*mi_ctx\s*\*\s*\w+\s*,\s*const\s+mi_nv12_frame_dev\s*\*", txt), s
        assert s in mi_lumaeq.DECLARED_SYMBOLS
    body = re.search(r"typedef struct mi_nv12_frame_dev\s*\{(.*?)\}\s*mi_nv12_frame_dev;", txt, re.S).group(1)
    decls = [re.sub(r"\s+", " ", d.strip()) for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls == ["const void* y_in", "const void* uv_in", "void* y_out", "void* uv_out"], decls
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", txt), "symbols were added, no struct grew: the minor version stays"
    assert re.search(r"\bMI_K_COUNT\s*=\s*10\b", txt), "the new launches are charged to the existing profiling slots"


def _compile(tmp_path, compiler, std, src_name, body):
    src = tmp_path / src_name
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi_lumaeq.h"\n' + body)
    exe = tmp_path / (src_name + ".bin")
    subprocess.run([compiler, f"-std={std}", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), "-o", str(exe), str(src)],
                   check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


LAYOUT = ('int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mi_nv12_frame_dev), offsetof(mi_nv12_frame_dev, y_in),'
          ' offsetof(mi_nv12_frame_dev, uv_in), offsetof(mi_nv12_frame_dev, y_out), offsetof(mi_nv12_frame_dev, uv_out)); return 0; }\n')


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++11")])
def test_frame_struct_layout_matches_c_compiler(tmp_path, lang, std):
    compiler = shutil.which("cc" if lang == "c" else "c++") or shutil.which("gcc" if lang == "c" else "g++")
    if compiler is None:
        pytest.fail(f"no {lang} compiler on PATH")
    out = _compile(tmp_path, compiler, std, "probe." + ("c" if lang == "c" else "cpp"), LAYOUT)
    size, off_y_in, off_uv_in, off_y_out, off_uv_out = map(int, out.split())
    S = capi.Nv12FrameDev
    assert size == ctypes.sizeof(S) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert (off_y_in, off_uv_in, off_y_out, off_uv_out) == (S.y_in.offset, S.uv_in.offset, S.y_out.offset, S.uv_out.offset)


def test_libraries_export_frame_list_forms(built_lib):
    for L in (built_lib, capi.test_lib()):
        for s in SYMBOLS:
            assert hasattr(L, s), f"{L._name} does not export {s}"


def test_null_context_is_bad_arg_without_a_device(built_lib):
    """A null context is refused before any HIP call: no device is needed, and the frame list is not touched."""
    L = built_lib
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    frames = (capi.Nv12FrameDev * 2)(capi.Nv12FrameDev(p, p + 32, p, p + 32), capi.Nv12FrameDev(p, p + 32, p, p + 32))
    before = bytes(frames)
    assert L.mi_equalize_hist_nv12_frames_dev(None, frames, 2, 8, 4, 8, 8, 8, 8, 1, None) == MI_ERR_BAD_ARG
    assert L.mi_clahe_nv12_frames_dev(None, frames, 2, 8, 4, 8, 8, 8, 8, 1, 2.0, 2, 2, None) == MI_ERR_BAD_ARG
    assert L.mi_equalize_hist_nv12_frames_dev(None, None, 0, 0, 0, 0, 0, 0, 0, 0, None) == MI_ERR_BAD_ARG
    assert bytes(frames) == before and not any(buf)
