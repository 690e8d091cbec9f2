"""CPU-side checks of the parity update's boundary (include/tfs_ec.h tfs_ec_update, DESIGN.md
§3.16): the covering units and deltas of a changed range, the list checks and the (p, member) mask
offset, checked by a stand-alone program under the host's address and undefined-behaviour
sanitizers (tools/update_delta_check.cpp; no Python runs under a sanitizer), the exported symbols,
and the calls that fail before they touch a device."""
import os
import re
import subprocess

from conftest import ROOT

UPDATE = ["tfs_ec_update_device", "tfs_ec_update"]


def test_delta_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "update_delta_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "update_delta_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "update delta ok: 9 ranges, 9 lists, 66 coders" in out.stdout   # pn = 1 .. 11, dn = 1 .. 12 - pn


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_ec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    for name in UPDATE:
        assert hasattr(L, name), name
        assert name in ec.EXPORTED and name in declared
    assert hasattr(L, "tfs_ec_update_set_piece")
    assert callable(ec.ErasureCode.update) and callable(ec.ErasureCode.update_device)
    assert len(ec.lib().tfs_ec_update_device.argtypes) == 9 and len(ec.lib().tfs_ec_update.argtypes) == 8


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_ec.h"\n#include "tfs_crc_testing.h"\n'
                   "int main(void) { return tfs_ec_update(0, 0, 0, 0, 0, 0, 0, 0) == "
                   "tfs_ec_update_device(0, 0, 0, 0, 0, 0, 0, 0, 0) && tfs_ec_update_set_piece(0, 0); }\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_calls_fail_without_a_device():
    import tfs_amd.ec as ec
    L = ec.lib()
    assert L.tfs_ec_update(None, 0, None, 1024, None, 1, None, None) == -1016
    assert L.tfs_ec_update_device(None, 0, None, 1024, None, 1, None, None, None) == -1016
    assert L.tfs_ec_update_set_piece(None, 4) == -1016


def test_product_library_carries_the_kernel_and_the_layers_resolve():
    blob = open(os.path.join(ROOT, "tfs_amd", "libtfs_crc.so"), "rb").read()
    assert b"ec_update_kernel" in blob
    import tfs_amd.dataserver as ds
    assert hasattr(ds.lib(), "tfs_ds_unlink_file_family") and hasattr(ds.lib(), "tfs_ds_write_member_range")
    assert callable(ds.unlink_file_family) and callable(ds.write_member_range)
