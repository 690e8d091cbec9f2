"""CPU-side checks of the mirror sync boundary (include/tfs_mirror.h): the plan arithmetic of
tfs_amd/csrc/mirror_plan.h, checked by a stand-alone program under the host's address and
undefined-behaviour sanitizers (tools/mirror_plan_check.cpp; no Python runs under a sanitizer);
the header in C99 and C11; the exported symbols and the struct sizes; tfs_mirror_frame_count and
tfs_mirror_span at the frame cuts; the calls that fail before they touch a device; the kernels'
names."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MIRROR = ["tfs_mirror_frame_count", "tfs_mirror_span", "tfs_mirror_frames_device", "tfs_mirror_frames"]
PARAM = -1016


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "mirror_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "mirror_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"mirror plan ok: (\d+) layouts, (\d+) frames, (\d+) units", out.stdout)
    assert m and int(m.group(1)) >= 300 and int(m.group(2)) > 3000 and int(m.group(3)) > int(m.group(2)), out.stdout


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_mirror.h"\n'
                   '#include "tfs_write.h"\n'
                   '#include "tfs_replicate.h"\n'
                   "int main(void) {\n"
                   "  tfs_mirror_cfg c; tfs_mirror_job j; tfs_mirror_result r;\n"
                   "  c.first_len = TFS_MAX_READ_SIZE - 36; c.frame_len = TFS_MAX_READ_SIZE; j.size = 100; r.status = 0;\n"
                   "  return tfs_mirror_frames_device(0, &c, 0, 0, &j, 1, 0, 0, 0, 0, &r, 0, 0)\n"
                   "         == tfs_mirror_frames(0, &c, 0, 0, &j, 1, 0, 0, 0, 0, &r, 0)\n"
                   "         && tfs_mirror_frame_count(&c, 100) && tfs_mirror_span(&c, &j)\n"
                   "         && sizeof(tfs_mirror_cfg) == 16 && sizeof(tfs_mirror_job) == 64\n"
                   "         && sizeof(tfs_mirror_result) == 16 && TFS_MIRROR_MAX_DS == TFS_WRITE_MAX_DS\n"
                   "         && TFS_WRITE_DATA_MESSAGE == 9 && TFS_MIRROR_FRAME_HEAD == 60;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    alone = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                            os.path.join(ROOT, "include", "tfs_mirror.h")], capture_output=True, text=True)
    assert alone.returncode == 0, alone.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_mirror.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tfs_\w+)\s*\(", src)) == set(MIRROR)
    for name in MIRROR:
        assert hasattr(L, name), name
        assert name in crc.EXPORTED
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")],
                              capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(tfs_mirror_\w+)\b", exported)) == set(MIRROR)
    assert len(L.tfs_mirror_frames_device.argtypes) == 13 and len(L.tfs_mirror_frames.argtypes) == 12
    assert callable(crc.Context.mirror_frames) and callable(crc.Context.mirror_frames_device)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tfs_mirror_frames" in integ and "sync_backup.cpp:315-472" in integ


def test_struct_layouts():
    import tfs_amd.crc as crc
    assert (crc.MIRROR_CFG_DTYPE.itemsize, crc.MIRROR_JOB_DTYPE.itemsize, crc.MIRROR_RESULT_DTYPE.itemsize) == (16, 64, 16)
    f = crc.MIRROR_JOB_DTYPE.fields
    assert [f[k][1] for k in ("src_offset", "frame_offset", "file_id", "file_number", "packet_id", "block_id", "size",
                              "ds_first", "ds_count", "reserved")] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56]
    f = crc.MIRROR_CFG_DTYPE.fields
    assert [f[k][1] for k in ("first_len", "frame_len", "is_server", "version", "reserved")] == [0, 4, 8, 12, 14]
    f = crc.MIRROR_RESULT_DTYPE.fields
    assert [f[k][1] for k in ("status", "n_frames", "span_len", "file_crc")] == [0, 4, 8, 12]


@pytest.mark.parametrize("first_len,frame_len", [(1024 - 36, 1024), (40000, 32768), ((1 << 20) - 36, 1 << 20), (5, 3)])
@pytest.mark.parametrize("ds_count", [0, 2, 27])
def test_frame_count_and_span_at_the_cuts(first_len, frame_len, ds_count):
    import tfs_amd.crc as crc
    cfg = crc.mirror_cfg(first_len, frame_len)
    head = 60 + 8 * ds_count
    for n, want in ((1, 1), (first_len - 1, 1), (first_len, 1), (first_len + 1, 2), (first_len + frame_len, 2),
                    (first_len + frame_len + 1, 3)):
        if n < 1:
            continue
        assert crc.mirror_frame_count(cfg, n + 36) == want, (n, want)
        j = np.zeros(1, crc.MIRROR_JOB_DTYPE)
        j["size"], j["ds_count"] = n + 36, ds_count
        assert crc.mirror_span(cfg, j) == want * head + n, (n, want)


def test_frame_count_and_span_refuse_bad_input():
    import tfs_amd.crc as crc
    L = crc.lib()
    good = crc.mirror_cfg(1000, 300)
    j = np.zeros(1, crc.MIRROR_JOB_DTYPE)
    j["size"] = 500
    assert L.tfs_mirror_frame_count(None, 500) == 0 and L.tfs_mirror_span(None, j.ctypes.data) == 0
    assert L.tfs_mirror_span(good.ctypes.data, None) == 0
    for size in (36, 20, 0, -1):
        assert crc.mirror_frame_count(good, size) == 0
        j["size"] = size
        assert crc.mirror_span(good, j) == 0
    for bad in (crc.mirror_cfg(0, 300), crc.mirror_cfg(1000, 0), crc.mirror_cfg(-5, 300), crc.mirror_cfg(1000, -1)):
        assert crc.mirror_frame_count(bad, 500) == 0
    j["size"], j["ds_count"] = 500, 28
    assert crc.mirror_span(good, j) == 0


def test_null_calls_fail_without_a_device():
    """The first check of every call comes before any device is touched: a NULL context, whatever
    else is wrong with the call."""
    import tfs_amd.crc as crc
    L = crc.lib()
    good, worse = crc.mirror_cfg(1000, 300), crc.mirror_cfg(0, -1, reserved=1)
    jobs = np.zeros(2, crc.MIRROR_JOB_DTYPE)
    jobs["size"] = 100
    ds = np.zeros(4, np.uint64)
    buf = np.zeros(8192, np.uint8)
    res = np.zeros(2, crc.MIRROR_RESULT_DTYPE)
    nbad = np.zeros(1, np.uint32)
    p = buf.ctypes.data
    for cfg in (good, worse):
        assert L.tfs_mirror_frames_device(None, cfg.ctypes.data, p, 4096, jobs.ctypes.data, 2, ds.ctypes.data, 4,
                                          p + 4096, 4096, res.ctypes.data, nbad.ctypes.data, None) == PARAM
        assert L.tfs_mirror_frames(None, cfg.ctypes.data, p, 4096, jobs.ctypes.data, 2, ds.ctypes.data, 4, p + 4096,
                                   4096, res.ctypes.data, nbad.ctypes.data) == PARAM
    assert L.tfs_mirror_frames_device(None, None, None, 5, None, 3, None, 2, None, 1, None, None, 2) == PARAM
    assert L.tfs_mirror_frames(None, None, None, 5, None, 3, None, 2, None, 1, None, None) == PARAM
    assert not buf.any() and not res.view(np.uint8).any() and nbad[0] == 0


def test_product_library_carries_one_form_of_the_kernels():
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")], capture_output=True, text=True,
                         check=True).stdout
    forms = set(re.findall(r"(mirror\w*_kernel(?:<[^>]*>)?)\(", out))
    assert forms == {"mirror_kernel", "mirror_job_fold_kernel", "mirror_frame_fold_kernel"}, forms
