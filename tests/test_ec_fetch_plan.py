"""CPU-side checks of the task chunk calls' boundary (include/tfs_ec_fetch.h, DESIGN.md
§3.24): the host arithmetic -- every call check in the header's order, the expected n,
the capacity, the tile words lane by lane, the check's fold and its verdicts against
Func::crc bit by bit -- checked by a stand-alone program under the host's address and
undefined-behaviour sanitizers (tools/ec_fetch_plan_check.cpp; no Python runs under a
sanitizer), the header as C99, the layouts, the exported symbols, the helpers at the cuts
and the calls that fail before they touch a device."""
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

FETCH = ["tfs_ec_fetch_cap", "tfs_ec_fetch_expect", "tfs_ec_fetch_parse", "tfs_ec_marshal_task_device",
         "tfs_ec_marshal_task", "tfs_ec_reinstate_task_device", "tfs_ec_reinstate_task"]
PARAM, INCOMPLETE = -1016, 1


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ec_fetch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "ec_fetch_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ec fetch plan ok: 51 frames" in out.stdout  # (7 lengths in 4096 + 10 in 8192) x 3 versions


def test_header_is_c99_and_the_layouts(tmp_path):
    import tfs_amd.ec as ec
    assert ec.FETCH_CFG_DTYPE.itemsize == 8 and ec.FETCH_RESULT_DTYPE.itemsize == 16
    assert [ec.FETCH_RESULT_DTYPE.fields[f][1] for f in ("status", "n", "data_file_size", "crc")] == [0, 4, 8, 12]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "tfs_ec_fetch.h"\n'
                   "typedef char a0[sizeof(tfs_ec_fetch_cfg) == 8 && sizeof(tfs_ec_fetch_result) == 16 ? 1 : -1];\n"
                   "typedef char a1[offsetof(tfs_ec_fetch_cfg, reserved) == 4 ? 1 : -1];\n"
                   "typedef char a2[offsetof(tfs_ec_fetch_result, n) == 4 ? 1 : -1];\n"
                   "typedef char a3[offsetof(tfs_ec_fetch_result, data_file_size) == 8 ? 1 : -1];\n"
                   "typedef char a4[offsetof(tfs_ec_fetch_result, crc) == 12 ? 1 : -1];\n"
                   "typedef char a5[TFS_RESP_READ_RAW_DATA_MESSAGE == 46 && TFS_EC_FETCH_HEAD == 28 && "
                   "TFS_EC_FETCH_OVERHEAD == 32 ? 1 : -1];\n"
                   "int main(void) { return tfs_ec_fetch_cap(0, 0, 4096) != 0; }\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_ec_fetch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    assert declared == set(FETCH)
    for name in FETCH:
        assert hasattr(L, name) and name in ec.EXPORTED
    for cls in (ec.MarshalSession, ec.ReinstateSession):
        assert callable(cls.task) and callable(cls.task_device)


def test_cap_at_the_cuts():
    import tfs_amd.ec as ec
    c, f = ec.frames_cfg(4096), ec.fetch_cfg()
    assert ec.fetch_cap(c, f, 4096) == 36 + 4096 and ec.fetch_cap(c, f, 1024) == 36 + 1024
    assert ec.fetch_cap(c, f, 3 * 4096 + 2048) == 3 * (4096 + 32) + 36 + 2048
    assert ec.fetch_cap(c, ec.fetch_cfg(4096 + 32), 2 * 4096) == 4096 + 32 + 36 + 4096      # the default, spelled out
    assert ec.fetch_cap(c, ec.fetch_cfg(8192), 3 * 4096) == 2 * 8192 + 36 + 4096
    assert ec.fetch_cap(ec.frames_cfg(1 << 20), f, 64 << 20) == 63 * ((1 << 20) + 32) + 36 + (1 << 20)
    for bad in (ec.fetch_cfg(4096 + 24), ec.fetch_cfg(4096 + 28), ec.fetch_cfg(4096 + 36), ec.fetch_cfg(8), ec.fetch_cfg(0, 1)):
        assert ec.fetch_cap(c, bad, 4096) == 0
    for bad in (ec.frames_cfg(0), ec.frames_cfg(1024), ec.frames_cfg(4096, frame_stride=4096 + 56), ec.frames_cfg(4096, reserved=1)):
        assert ec.fetch_cap(bad, f, 4096) == 0
    assert ec.fetch_cap(c, f, 0) == 0 and ec.fetch_cap(c, f, -4096) == 0
    assert ec.fetch_cap(None, f, 4096) == 0 and ec.fetch_cap(c, None, 4096) == 0


def test_expect_at_the_cuts():
    import tfs_amd.ec as ec
    sizes, dn, total = [70001, 8192, 4096, 1, 0], 5, 70656

    def e(member, offset, requested=4096):
        return ec.fetch_expect(sizes, dn, total, member, offset, requested)
    assert [e(0, o) for o in (0, 65536, 69632)] == [4096, 4096, 369] and e(0, 69632, 1024) == 369
    assert [e(1, o) for o in (0, 4096, 8192, 12288)] == [4096, 4096, 0, 0]
    assert [e(2, o) for o in (0, 4096)] == [4096, 0]
    assert [e(3, o) for o in (0, 4096)] == [1, 0] and e(4, 0) == 0
    assert e(0, 0, 8192) == 8192 and e(1, 0, 16384) == 8192 and e(1, 8191, 4096) == 1
    for parity in (5, 6, 7, 11):                                   # a parity source's block_len is total
        assert e(parity, 0) == 4096 and e(parity, 69632, 1024) == 1024 and e(parity, total) == 0
    assert e(0, 0, 0) == 0
    assert e(-1, 0) == -1 and e(12, 0) == -1 and e(0, -1) == -1 and e(0, 0, -1) == -1
    assert ec.fetch_expect(None, dn, total, 0, 0, 4096) == -1


def test_parse():
    import tfs_amd.ec as ec
    from tfs_amd.packet import read_raw_reply_frame
    f = read_raw_reply_frame(b"abcdefg", 123456, 2, 9)
    assert len(f) == 32 + 7 and ec.fetch_parse(f) == (0, 7, 123456)
    assert ec.fetch_parse(f + b"zz") == (0, 7, 123456)
    assert ec.fetch_parse(f[:-1])[0] == INCOMPLETE and ec.fetch_parse(f[:31])[0] == INCOMPLETE
    assert ec.fetch_parse(b"")[0] == PARAM
    assert ec.fetch_parse(read_raw_reply_frame(b"", -5))[:2] == (0, 0) and ec.fetch_parse(read_raw_reply_frame(b"", -5))[2] == -5
    err = bytearray(read_raw_reply_frame(b"", 0))
    err[24:28] = (-8016).to_bytes(4, "little", signed=True)      # set_length(status): the source's error reply
    assert ec.fetch_parse(err) == (-8016, 0, 0)
    L = ec.lib()
    b = np.frombuffer(f, np.uint8)
    assert L.tfs_ec_fetch_parse(b.ctypes.data, b.size, None, None) == PARAM


def test_null_calls_fail_without_a_device():
    import tfs_amd.ec as ec
    L = ec.lib()
    c, f = ec.frames_cfg(4096), ec.fetch_cfg()
    r = np.zeros(4, ec.FETCH_RESULT_DTYPE)
    assert L.tfs_ec_marshal_task_device(None, c.ctypes.data, f.ctypes.data, None, None, 0, r.ctypes.data, 0, 4096, None) == PARAM
    assert L.tfs_ec_marshal_task(None, c.ctypes.data, f.ctypes.data, None, None, 0, r.ctypes.data, 0, 4096) == PARAM
    assert L.tfs_ec_reinstate_task_device(None, c.ctypes.data, f.ctypes.data, None, None, 0, r.ctypes.data, 0, 4096, None) == PARAM
    assert L.tfs_ec_reinstate_task(None, c.ctypes.data, f.ctypes.data, None, None, 0, r.ctypes.data, 0, 4096) == PARAM


def test_product_library_carries_the_kernels():
    blob = open(os.path.join(ROOT, "tfs_amd", "libtfs_crc.so"), "rb").read()
    assert b"ec_task_kernel" in blob and b"ec_fetch_check_kernel" in blob and b"ec_task_seal_kernel" in blob
