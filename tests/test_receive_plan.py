"""CPU-side checks of the receive session's boundary (include/tfs_receive.h): the host
arithmetic of tfs_amd/csrc/receive_plan.h, checked by a stand-alone program under the host's
address and undefined-behaviour sanitizers (tools/receive_plan_check.cpp; no Python runs under
a sanitizer); the header in C99 and C11; the exported symbols and the struct layouts;
tfs_receive_parse; the calls that fail before they touch a device; the kernels' names."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tfs_amd import packet as pk

RECEIVE = ["tfs_receive_granule", "tfs_receive_parse", "tfs_receive_begin", "tfs_receive_frames_device",
           "tfs_receive_frames", "tfs_receive_finish", "tfs_receive_free"]
PARAM = -1016


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "receive_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "receive_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"receive plan ok: (\d+) layouts, (\d+) units, (\d+) records", out.stdout)
    assert m and int(m.group(1)) == 300 and int(m.group(2)) > 2000 and int(m.group(3)) > 500, out.stdout


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_receive.h"\n'
                   '#include "tfs_ec.h"\n'
                   "int main(void) {\n"
                   "  tfs_receive_cfg c; tfs_receive_desc d; tfs_receive_part p; tfs_receive* s = 0;\n"
                   "  c.image_cap = TFS_RECEIVE_GRANULE; d.data_len = 0; p.status = 0;\n"
                   "  return tfs_receive_begin(0, &c, 0, &s) == tfs_receive_frames_device(s, 0, &d, 1, &p, 0, 0)\n"
                   "         && tfs_receive_frames(s, 0, 0, &d, 1, &p, 0) && tfs_receive_finish(s, 0, 0, 0, 0, 0, 0)\n"
                   "         && tfs_receive_free(s) && tfs_receive_granule() && tfs_receive_parse(0, 0, 0, &d)\n"
                   "         && sizeof(tfs_receive_cfg) == 16 && sizeof(tfs_receive_desc) == 24\n"
                   "         && sizeof(tfs_receive_part) == 16 && TFS_EXIT_SIZE_INVALID == -16002;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    alone = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                            os.path.join(ROOT, "include", "tfs_receive.h")], capture_output=True, text=True)
    assert alone.returncode == 0, alone.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_receive.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tfs_\w+)\s*\(", src)) == set(RECEIVE)
    for name in RECEIVE:
        assert hasattr(L, name), name
        assert name in crc.EXPORTED
    assert len(L.tfs_receive_frames_device.argtypes) == 7 and len(L.tfs_receive_finish.argtypes) == 7
    for attr in ("frames", "frames_device", "finish"):
        assert callable(getattr(crc.ReceiveSession, attr))
    assert L.tfs_receive_granule() == crc.receive_granule()
    hdr = open(os.path.join(ROOT, "include", "tfs_receive.h")).read()
    assert re.search(r"#define TFS_RECEIVE_GRANULE %d\b" % crc.receive_granule(), hdr)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tfs_receive_begin" in integ and "dataservice.cpp:2487-2566" in integ


def test_struct_layouts():
    import tfs_amd.crc as crc
    c, d, p = crc.RECEIVE_CFG_DTYPE, crc.RECEIVE_DESC_DTYPE, crc.RECEIVE_PART_DTYPE
    assert (c.itemsize, d.itemsize, p.itemsize) == (16, 24, 16)
    assert [c.fields[k][1] for k in ("block_id", "image_cap", "reserved")] == [0, 4, 8]
    assert [d.fields[k][1] for k in ("frame_off", "avail", "data_offset", "data_len", "reserved")] == [0, 8, 12, 16, 20]
    assert [p.fields[k][1] for k in ("status", "crc", "flag", "reserved")] == [0, 4, 8, 12]


def test_parse_is_host_arithmetic():
    import tfs_amd.crc as crc
    body = struct.pack("<IQiiiQ", 9, 0, 123456, 100, 0, 0) + bytes(100) + struct.pack("<i", 0)
    f = np.frombuffer(pk.frame_v1(body, 35, 2, 77), np.uint8).copy()
    rc, d = crc.receive_parse(f, frame_off=4242)
    assert rc == 0 and d[0].tolist() == (4242, f.size, 123456, 100, 0)
    rc, d = crc.receive_parse(f, frame_off=1, avail=56)        # the header and WriteDataInfo are enough
    assert rc == 0 and d[0].tolist() == (1, 56, 123456, 100, 0)
    rc, d = crc.receive_parse(f, frame_off=1, avail=55)
    assert rc == crc.TFS_PACKET_INCOMPLETE and d[0].tolist() == (0, 0, 0, 0, 0)
    f[36:44] = np.frombuffer(struct.pack("<ii", -5, -7), np.uint8)   # what the frame says, however absurd
    rc, d = crc.receive_parse(f)
    assert rc == 0 and d[0].tolist() == (0, f.size, -5, -7, 0)
    L = crc.lib()
    assert L.tfs_receive_parse(None, 100, 0, d.ctypes.data) == PARAM
    assert L.tfs_receive_parse(f.ctypes.data, 100, 0, None) == PARAM


def test_null_calls_fail_without_a_device():
    """The first check of every call comes before any device is touched: a NULL context or
    session, whatever else is wrong with the call."""
    import tfs_amd.crc as crc
    L = crc.lib()
    h = ctypes.c_void_p()
    worse = crc.receive_cfg(-1, reserved=(1, 1))     # would be TFS_EXIT_SIZE_INVALID
    good = crc.receive_cfg(4096, 7)
    buf = np.zeros(8192, np.uint8)
    p = buf.ctypes.data
    descs = np.zeros(2, crc.RECEIVE_DESC_DTYPE)
    descs["avail"], descs["data_len"] = 100, 40
    before = descs.copy()
    assert L.tfs_receive_begin(None, worse.ctypes.data, None, ctypes.byref(h)) == PARAM
    assert L.tfs_receive_begin(None, good.ctypes.data, p, ctypes.byref(h)) == PARAM and h.value is None
    assert L.tfs_receive_begin(None, None, None, None) == PARAM
    assert L.tfs_receive_frames_device(None, p, descs.ctypes.data, 2, p + 4096, p + 8000, None) == PARAM
    assert L.tfs_receive_frames_device(None, None, None, 5, None, None, 2) == PARAM
    assert L.tfs_receive_frames(None, p, 4096, descs.ctypes.data, 2, p + 4096, p + 8000) == PARAM
    assert L.tfs_receive_finish(None, None, 3, p, p + 64, p + 128, p + 192) == PARAM
    assert L.tfs_receive_free(None) == PARAM
    assert not buf.any() and (descs == before).all()


def test_product_library_carries_one_form_of_the_kernels():
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")], capture_output=True, text=True,
                         check=True).stdout
    forms = set(re.findall(r"(receive\w*_kernel(?:<[^>]*>)?)\(", out))
    assert forms == {"receive_kernel", "receive_fold_kernel", "receive_finish_kernel"}, forms
