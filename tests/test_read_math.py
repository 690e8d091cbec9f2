"""CPU-side checks of the read replies (include/tfs_read.h): the two
identities the one-pass reply rests on, against zlib and the oracle; the plan arithmetic
of tfs_amd/csrc/read_reply_plan.h, checked by a stand-alone program under the host's
address and undefined-behaviour sanitizers (tools/read_reply_plan_check.cpp; no Python runs
under a sanitizer); the header in C99 and C11; the exported symbols, the struct sizes and
the calls that fail before they touch a device.

With L = le32(|D|), D the data and T the trailer of the body:

  crc(FLAG, L || D)      = shift(crc(FLAG, L), |D|) ^ crc(0, D)
  crc(FLAG, L || D || T) = crc(seed = crc(FLAG, L || D), T)
"""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

FLAG = pk.TFS_PACKET_FLAG_V1
READ = ["tfs_read_frame_cap", "tfs_read_reply_device", "tfs_read_reply"]
M32 = 0xFFFFFFFF


def zcrc(seed, data):
    """Func::crc(seed, data) (no inversions) through zlib's CRC-32."""
    return zlib.crc32(data, seed ^ M32) ^ M32


def trailers(nd):
    info = synth_bytes(900 + nd, 36).tobytes()
    return [b"", struct.pack("<i", 0), struct.pack("<i", 36) + info]


@pytest.mark.parametrize("nd", [0, 1, 3, 4, 31, 32, 1023, 1024, 1025, 65536, (2 << 20) + 1])
def test_identities_against_zlib(oracle, nd):
    import tfs_amd.crc as crc
    d = synth_bytes(17 + nd, nd).tobytes()
    L = struct.pack("<i", nd)
    pre = crc.combine(zcrc(FLAG, L), 0, nd)  # shift(crc(FLAG, L), |D|)
    head = pre ^ zcrc(0, d)
    assert head == zcrc(FLAG, L + d)
    if nd <= 65536:
        assert head == ocrc(oracle, FLAG, L + d) and zcrc(0, d) == ocrc(oracle, 0, d)
    for t in trailers(nd):
        assert zcrc(head, t) == zcrc(FLAG, L + d + t), (nd, len(t))


def test_reply_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "read_reply_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "read_reply_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "read plan ok: 556 jobs, 22 span lists" in out.stdout


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_read.h"\n'
                   "int main(void) {\n"
                   "  tfs_read_job j; tfs_read_result r;\n"
                   "  (void)r; j.pcode = TFS_RESP_READ_DATA_MESSAGE_V2;\n"
                   "  return tfs_read_reply(0, 0, 0, &j, 1, 0, 0, 0, 0) == tfs_read_reply_device(0, 0, 0, &j, 1, 0, 0, 0, 0, 0)\n"
                   "         && tfs_read_frame_cap(&j) && sizeof(tfs_read_job) == 48 && sizeof(tfs_read_result) == 16;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_read.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    assert declared == set(READ)
    for name in READ:
        assert hasattr(L, name), name
        assert name in crc.EXPORTED
    assert hasattr(L, "tfs_read_set_piece") and "tfs_read_set_piece" in crc.EXPORTED
    assert len(L.tfs_read_reply_device.argtypes) == 10 and len(L.tfs_read_reply.argtypes) == 9
    assert callable(crc.Context.read_reply) and callable(crc.Context.read_reply_device)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tfs_read_reply" in integ and "tfs_read_set_piece" not in integ


def test_struct_sizes_and_layout():
    import tfs_amd.crc as crc
    assert crc.READ_JOB_DTYPE.itemsize == 48 and crc.READ_RESULT_DTYPE.itemsize == 16
    assert crc.READ_JOB_DTYPE.fields["size"][1] == 32 and crc.READ_JOB_DTYPE.fields["pcode"][1] == 44
    assert crc.READ_JOB_DTYPE.fields["version"][1] == 46
    assert crc.READ_RESULT_DTYPE.fields["frame_crc"][1] == 12


def _job(size, ro, rl, pcode):
    import tfs_amd.crc as crc
    j = np.zeros(1, crc.READ_JOB_DTYPE)
    j["size"], j["read_offset"], j["read_len"], j["pcode"], j["version"] = size, ro, rl, pcode, 2
    return j


def test_frame_cap_is_host_arithmetic():
    import tfs_amd.crc as crc
    assert crc.read_frame_cap(_job(36 + 1000, 0, 1000, 8)) == 28 + 1000
    assert crc.read_frame_cap(_job(36 + 1000, 0, 5000, 39)) == 28 + 1000 + 40     # cut at the payload's end
    assert crc.read_frame_cap(_job(36 + 1000, 10, 100, 63)) == 28 + 100 + 4
    assert crc.read_frame_cap(_job(36, 0, 100, 39)) == 68 and crc.read_frame_cap(_job(35, 0, 100, 8)) == 28
    assert crc.read_frame_cap(_job(36 + 1000, 0, 1000, 9)) == 0
    assert crc.lib().tfs_read_frame_cap(None) == 0


def test_null_calls_fail_without_a_device():
    import tfs_amd.crc as crc
    L = crc.lib()
    j = _job(136, 0, 100, 8)
    buf = (ctypes.c_uint8 * 256)()
    res = np.zeros(1, crc.READ_RESULT_DTYPE)
    p = ctypes.addressof(buf)
    assert L.tfs_read_reply(None, p, 256, j.ctypes.data, 1, p, 256, res.ctypes.data, None) == -1016
    assert L.tfs_read_reply_device(None, p, 256, j.ctypes.data, 1, p, 256, res.ctypes.data, None, None) == -1016
    assert L.tfs_read_set_piece(None, 4096) == -1016


def test_product_library_carries_one_form_of_the_kernel():
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")], capture_output=True, text=True,
                         check=True).stdout
    forms = set(re.findall(r"(read_reply_kernel(?:<[^>]*>)?)\(", out))
    assert forms == {"read_reply_kernel"}, forms
