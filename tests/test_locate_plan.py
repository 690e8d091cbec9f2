"""CPU-side checks of the scrub locate step's boundary (include/tfs_ec.h tfs_ec_locate,
DESIGN.md §3.15): the plan that the first call builds, checked by a stand-alone program
under the host's address and undefined-behaviour sanitizers (tools/locate_plan_check.cpp;
no Python runs under a sanitizer), the exported symbols, the result layout, and the calls
that fail before they touch a device."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

LOCATE = ["tfs_ec_locate_device", "tfs_ec_locate"]


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "locate_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "locate_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "locate plan ok: 55 coders" in out.stdout   # pn = 2 .. 11, dn = 1 .. 12 - pn


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_ec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    for name in LOCATE:
        assert hasattr(L, name), name
        assert name in ec.EXPORTED and name in declared
    assert hasattr(L, "tfs_ec_locate_set_piece")
    assert callable(ec.ErasureCode.locate) and callable(ec.ErasureCode.locate_device)
    assert len(ec.lib().tfs_ec_locate_device.argtypes) == 8 and len(ec.lib().tfs_ec_locate.argtypes) == 7


def test_result_layout(tmp_path):
    import tfs_amd.ec as ec
    d = ec.LOCATE_RESULT_DTYPE
    assert d.itemsize == 8
    assert [d.fields[f][1] for f in ("kind", "member", "parity", "diff_bytes", "flags", "reserved")] == [0, 1, 2, 4, 6, 7]
    assert (ec.LOCATE_CLEAN, ec.LOCATE_PARITY, ec.LOCATE_DATA, ec.LOCATE_NONE, ec.LOCATE_CONFIRMED) == (0, 1, 2, 3, 1)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "tfs_ec.h"\n'
                   "_Static_assert(sizeof(tfs_ec_locate_result) == 8, \"size\");\n"
                   "_Static_assert(offsetof(tfs_ec_locate_result, member) == 1, \"member\");\n"
                   "_Static_assert(offsetof(tfs_ec_locate_result, parity) == 2, \"parity\");\n"
                   "_Static_assert(offsetof(tfs_ec_locate_result, diff_bytes) == 4, \"diff_bytes\");\n"
                   "_Static_assert(offsetof(tfs_ec_locate_result, flags) == 6, \"flags\");\n"
                   "_Static_assert(TFS_EC_LOCATE_CLEAN == 0 && TFS_EC_LOCATE_PARITY == 1 && TFS_EC_LOCATE_DATA == 2 && "
                   "TFS_EC_LOCATE_NONE == 3 && TFS_EC_LOCATE_CONFIRMED == 1u, \"kinds\");\n"
                   "int main(void) { return tfs_ec_locate(0, 0, 0, 0, 0, 0, 0) == "
                   "tfs_ec_locate_device(0, 0, 0, 0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_calls_fail_without_a_device():
    import tfs_amd.ec as ec
    L = ec.lib()
    res = (ctypes.c_uint8 * 8)()
    assert L.tfs_ec_locate(None, None, 1024, None, 1, res, None) == -1016
    assert L.tfs_ec_locate_device(None, None, 1024, None, 1, res, None, None) == -1016
    assert L.tfs_ec_locate_set_piece(None, 4) == -1016


def test_product_library_carries_the_kernel_and_the_layers_resolve():
    blob = open(os.path.join(ROOT, "tfs_amd", "libtfs_crc.so"), "rb").read()
    assert b"ec_locate_kernel" in blob
    import tfs_amd.dataserver as ds
    assert hasattr(ds.lib(), "tfs_ds_scrub_locate_family") and callable(ds.scrub_locate_family)
