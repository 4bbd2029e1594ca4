"""P010 / P012 / P016 frames at the ABI level, without a GPU: the header declares the two entry points and MI_FMT_P010, the product
library exports them, mi_pipe_config grew a trailing `format` member whose layout the Python binding mirrors (checked against the
real C compiler), the entry points refuse a null context without touching a device, and the host's share of a frame -- the chroma
half, filled with 0x8000 or copied (csrc/host/p010_chroma.hpp) -- is exact and stays inside its range under ASan + UBSan."""
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
MI_ERR_BAD_ARG = 1


def _header() -> str:
    return HEADER.read_text()


def test_header_declares_p010_forms():
    txt = _header()
    assert re.search(r"\bmi_status\s+mi_clahe_p010\s*\(", txt)
    assert re.search(r"\bmi_status\s+mi_clahe_p010_batch_dev\s*\(", txt)
    assert re.search(r"\bMI_FMT_NV12\s*=\s*0\b", txt) and re.search(r"\bMI_FMT_P010\s*=\s*1\b", txt)
    assert re.search(r"#define\s+MI_LUMAEQ_VERSION_MINOR\s+3\b", txt), "mi_pipe_config grew: the minor version moves to 3"
    assert "mi_clahe_p010" in mi_lumaeq.DECLARED_SYMBOLS and "mi_clahe_p010_batch_dev" in mi_lumaeq.DECLARED_SYMBOLS
    assert (mi_lumaeq.FMT_NV12, mi_lumaeq.FMT_P010) == (0, 1)


def test_pipe_config_format_is_last_member():
    body = re.search(r"typedef struct mi_pipe_config\s*\{(.*?)\}\s*mi_pipe_config;", _header(), re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert re.fullmatch(r"int\s+format", decls[-1]), decls
    names = [f[0] for f in capi._PipeConfig._fields_]
    assert names[-1] == "format" and len(names) == len(set(names))


def test_library_exports_p010_forms(built_lib):
    for s in ("mi_clahe_p010", "mi_clahe_p010_batch_dev"):
        assert hasattr(built_lib, s), f"libmi_lumaeq.so does not export {s}"


def test_pipe_config_layout_matches_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH (cc / gcc)")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi_lumaeq.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(mi_pipe_config), offsetof(mi_pipe_config, format),'
                   ' offsetof(mi_pipe_config, uv_policy)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-Wall", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    size, off_format, off_policy = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == ctypes.sizeof(capi._PipeConfig)
    assert off_format == capi._PipeConfig.format.offset
    assert off_policy == capi._PipeConfig.uv_policy.offset
    assert off_format > off_policy


def test_null_context_is_bad_arg_without_a_device(built_lib):
    """A null context is refused before any HIP call: no device is needed to get MI_ERR_BAD_ARG, and nothing runs on the CPU."""
    L = built_lib
    buf = (ctypes.c_uint16 * (8 * 8 * 3 // 2))()
    assert L.mi_clahe_p010(None, buf, buf, 8, 8, 0, 2.0, 2, 2) == MI_ERR_BAD_ARG
    assert L.mi_clahe_p010_batch_dev(None, ctypes.addressof(buf), ctypes.addressof(buf), 8, 8, 1, 1, 2.0, 2, 2, None) == MI_ERR_BAD_ARG
    assert all(v == 0 for v in buf), "the host frame must not be touched"


def test_host_chroma_helper_under_sanitizers(tmp_path):
    """csrc/host/p010_chroma.hpp compiled for the host only with -fsanitize=address,undefined (tests/cxx/test_p010_chroma.cpp)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++ on PATH")
    exe = tmp_path / "test_p010_chroma"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(ROOT / "tests" / "cxx" / "test_p010_chroma.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout
