"""Warm start at the C boundary, without a GPU: include/dekf.h declares dekf_set_warm_start / dekf_get_warm_status, the library
exports them, the ctypes binding lists them, both refuse a null handle, and the header still compiles as C99 with them — while
the ABI version and the layout of dekf_params stay what they were (the symbols are additive)."""
import ctypes as C
import os
import re
import subprocess

from decentralized_ekf_mhe_amd import capi, go1_params
from decentralized_ekf_mhe_amd.params import DekfParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dekf_set_warm_start", "dekf_get_warm_status")


def _header():
    return open(os.path.join(ROOT, "include", "dekf.h")).read()


def test_header_declares_both_symbols():
    hdr = _header()
    assert re.search(r"dekf_status\s+dekf_set_warm_start\s*\(\s*dekf_handle\s+h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_warm_status\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*warm\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)


def test_library_exports_and_binding_lists_them():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
    assert capi.PROTOTYPES["dekf_set_warm_start"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.PROTOTYPES["dekf_get_warm_status"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    lib = capi.load()
    assert lib.dekf_abi_version() == capi.DEKF_ABI_VERSION == 4
    p = DekfParams()
    lib.dekf_default_params(C.byref(p))
    assert bytes(p) == bytes(go1_params())


def test_null_handle_is_invalid():
    lib = capi.load()
    assert lib.dekf_set_warm_start(None, 1) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_warm_start(None, 0) == capi.DEKF_ERR_INVALID
    w = (C.c_int * 4)()
    assert lib.dekf_get_warm_status(None, C.cast(w, C.c_void_p), capi.DEKF_HOST) == capi.DEKF_ERR_INVALID


def test_header_compiles_as_c99_with_the_warm_start_calls(tmp_path):
    src = tmp_path / "warm_client.c"
    src.write_text(
        '#include <stdio.h>\n#include "dekf.h"\n'
        "int main(void) {\n"
        "    int warm[4] = {7, 7, 7, 7};\n"
        "    dekf_status a = dekf_set_warm_start((dekf_handle)0, 1);\n"
        "    dekf_status b = dekf_get_warm_status((dekf_handle)0, warm, DEKF_HOST);\n"
        '    printf("set %d get %d\\n", (int)a, (int)b);\n'
        "    return 0;\n}\n")
    lib_dir = os.path.join(ROOT, "decentralized_ekf_mhe_amd", "csrc")
    exe = tmp_path / "warm_client"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", lib_dir, "-ldekf", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID}" in out.stdout, out.stdout
