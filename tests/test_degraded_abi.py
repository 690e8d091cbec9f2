"""CPU-side checks of the degraded read's boundary (include/tfs_ec.h): the library
exports both forms, the job struct has the header's layout, the header compiles
as C, and without a coder the calls fail with a TFS status."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "tfs_ec.h")


def test_library_exports_read_degraded():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    for name in ("tfs_ec_read_degraded", "tfs_ec_read_degraded_device"):
        assert hasattr(L, name), name
        assert name in ec.EXPORTED
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert {"tfs_ec_read_degraded", "tfs_ec_read_degraded_device"} <= set(re.findall(r"\b(tfs_\w+)\s*\(", src))


def test_read_job_layout():
    import tfs_amd.ec as ec
    d = ec.READ_JOB_DTYPE
    assert d.itemsize == 32
    assert [d.fields[f][1] for f in ("file_id", "out_offset", "offset", "size", "flags", "reserved")] == \
        [0, 8, 16, 20, 24, 28]
    assert ec.READ_RANGE == 1


def test_header_layout_as_c(tmp_path):
    """The header compiles as C99 and its struct is the 32 bytes the binding assumes."""
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "tfs_ec.h"\n'
                   "_Static_assert(sizeof(tfs_ec_read_job) == 32, \"size\");\n"
                   "_Static_assert(offsetof(tfs_ec_read_job, out_offset) == 8, \"out_offset\");\n"
                   "_Static_assert(offsetof(tfs_ec_read_job, offset) == 16, \"offset\");\n"
                   "_Static_assert(offsetof(tfs_ec_read_job, size) == 20, \"size_\");\n"
                   "_Static_assert(offsetof(tfs_ec_read_job, flags) == 24, \"flags\");\n"
                   "_Static_assert(TFS_EC_READ_RANGE == 1u, \"range\");\n"
                   "int main(void) { return tfs_ec_read_degraded(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == "
                   "tfs_ec_read_degraded_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_coder_is_a_parameter_error():
    import tfs_amd.ec as ec
    L = ec.lib()
    job = (ctypes.c_uint8 * 32)()
    out = (ctypes.c_uint8 * 1024)()
    crc, st, nbad = ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_uint32()
    assert L.tfs_ec_read_degraded(None, None, None, 1024, 0, job, 1, out, 1024, ctypes.byref(crc),
                                  ctypes.byref(st), ctypes.byref(nbad)) == -1016
    assert L.tfs_ec_read_degraded_device(None, None, None, 1024, 0, job, 1, out, 1024, ctypes.byref(crc),
                                         ctypes.byref(st), ctypes.byref(nbad), None) == -1016
    assert nbad.value == 0
