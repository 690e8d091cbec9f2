"""CPU-side checks of the replicate session's boundary (include/tfs_replicate.h): the plan
arithmetic of tfs_amd/csrc/replicate_plan.h, checked by a stand-alone program under the
host's address and undefined-behaviour sanitizers (tools/replicate_plan_check.cpp; no Python
runs under a sanitizer); the header in C99 and C11; the exported symbols and the struct size;
the calls that fail before they touch a device; tfs_replicate_frame_count."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

REPLICATE = ["tfs_replicate_frame_count", "tfs_replicate_begin", "tfs_replicate_frames_device", "tfs_replicate_frames",
             "tfs_replicate_finish", "tfs_replicate_free"]
PARAM = -1016


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "replicate_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "replicate_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"replicate plan ok: (\d+) layouts, (\d+) units, (\d+) calls", out.stdout)
    assert m and int(m.group(1)) == 300 and int(m.group(2)) > 5000 and int(m.group(3)) > 300, out.stdout


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_replicate.h"\n'
                   '#include "tfs_ec.h"\n'
                   "int main(void) {\n"
                   "  tfs_replicate_cfg c; tfs_replicate* s = 0;\n"
                   "  c.new_block = TFS_RAW_PARITY_DATA; c.frame_len = TFS_MAX_READ_SIZE;\n"
                   "  return tfs_replicate_begin(0, &c, 0, 0, &s) == tfs_replicate_frames_device(s, 0, 0, 0, 0, 0, 0)\n"
                   "         && tfs_replicate_frames(s, 0, 0, 0, 0, 0) && tfs_replicate_finish(s, 0, 0, 0, 0)\n"
                   "         && tfs_replicate_free(s) && tfs_replicate_frame_count(&c)\n"
                   "         && sizeof(tfs_replicate_cfg) == 32 && TFS_RAW_FRAME_OVERHEAD == 60\n"
                   "         && TFS_WRITE_RAW_DATA_MESSAGE == 35 && TFS_EXIT_SIZE_INVALID == -16002;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    alone = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                            os.path.join(ROOT, "include", "tfs_replicate.h")], capture_output=True, text=True)
    assert alone.returncode == 0, alone.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_replicate.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tfs_\w+)\s*\(", src)) == set(REPLICATE)
    for name in REPLICATE:
        assert hasattr(L, name), name
        assert name in crc.EXPORTED
    assert len(L.tfs_replicate_frames_device.argtypes) == 7 and len(L.tfs_replicate_begin.argtypes) == 5
    assert callable(crc.ReplicateSession.frames) and callable(crc.ReplicateSession.frames_device)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tfs_replicate_begin" in integ and "task.cpp:1025-1090" in integ


def test_cfg_layout():
    import tfs_amd.crc as crc
    f = crc.REPLICATE_CFG_DTYPE.fields
    assert crc.REPLICATE_CFG_DTYPE.itemsize == 32
    assert [f[k][1] for k in ("packet_id", "block_id", "total", "frame_len", "frame_stride", "new_block", "version",
                              "reserved")] == [0, 8, 12, 16, 20, 24, 26, 28]


def test_frame_count_is_host_arithmetic():
    import tfs_amd.crc as crc
    for fl in (1024, 1 << 20):
        for total, want in ((0, 1), (1, 1), (fl - 1, 1), (fl, 1), (fl + 1, 2)):
            assert crc.replicate_frame_count(crc.replicate_cfg(total, fl)) == want, (total, fl)
    assert crc.lib().tfs_replicate_frame_count(None) == 0
    assert crc.replicate_frame_count(crc.replicate_cfg(-1, 1024)) == 0
    assert crc.replicate_frame_count(crc.replicate_cfg(10, 0)) == 0


def test_null_calls_fail_without_a_device():
    """The first check of every call comes before any device is touched: a NULL context or
    session, whatever else is wrong with the call."""
    import tfs_amd.crc as crc
    L = crc.lib()
    h = ctypes.c_void_p()
    worse = crc.replicate_cfg(-1, 1000, new_block=7, reserved=1, frame_stride=3)   # would be TFS_EXIT_SIZE_INVALID
    good = crc.replicate_cfg(4096, 1024)
    buf = np.zeros(8192, np.uint8)
    p = buf.ctypes.data
    assert L.tfs_replicate_begin(None, worse.ctypes.data, None, 3, ctypes.byref(h)) == PARAM
    assert L.tfs_replicate_begin(None, good.ctypes.data, None, 0, ctypes.byref(h)) == PARAM and h.value is None
    assert L.tfs_replicate_begin(None, None, None, 0, None) == PARAM
    assert L.tfs_replicate_frames_device(None, p, 0, 1024, p + 4096, 4096, None) == PARAM
    assert L.tfs_replicate_frames_device(None, None, 512, -1, None, 0, 2) == PARAM
    assert L.tfs_replicate_frames(None, p, 0, 1024, p + 4096, 4096) == PARAM
    assert L.tfs_replicate_finish(None, None, None, None, None) == PARAM
    assert L.tfs_replicate_free(None) == PARAM
    assert not buf.any()


def test_product_library_carries_one_form_of_the_kernels():
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")], capture_output=True, text=True,
                         check=True).stdout
    forms = set(re.findall(r"(replicate\w*_kernel(?:<[^>]*>)?)\(", out))
    assert forms == {"replicate_kernel", "replicate_fold_kernel", "replicate_finish_kernel"}, forms
