"""CPU-side checks of the file repair boundary (include/tfs_repair.h): the plan arithmetic of
tfs_amd/csrc/repair_plan.h, checked by a stand-alone program under the host's address and
undefined-behaviour sanitizers (tools/repair_plan_check.cpp; no Python runs under a sanitizer);
the header in C99 and C11; the exported symbols and the struct sizes; tfs_repair_frame_count and
tfs_repair_span at the frame cuts; tfs_repair_parse; the calls that fail before they touch a
device; the kernels' names."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tfs_amd import packet as pk

REPAIR = ["tfs_repair_frame_count", "tfs_repair_span", "tfs_repair_parse", "tfs_repair_frames_device",
          "tfs_repair_frames"]
PARAM, INCOMPLETE = -1016, 1


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "repair_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "repair_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"repair plan ok: (\d+) layouts, (\d+) incoming frames, (\d+) outgoing frames, (\d+) units", out.stdout)
    assert m, out.stdout
    layouts, n_in, n_out, units = (int(g) for g in m.groups())
    assert layouts >= 300 and n_in > 3000 and n_out > 3000 and units > max(n_in, n_out), out.stdout


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_repair.h"\n'
                   '#include "tfs_mirror.h"\n'
                   '#include "tfs_write.h"\n'
                   "int main(void) {\n"
                   "  tfs_repair_cfg c; tfs_repair_job j; tfs_repair_in f; tfs_repair_result r;\n"
                   "  c.frame_len = TFS_MAX_READ_SIZE; j.stat_size = 100; f.data_len = 1; r.status = 0;\n"
                   "  return tfs_repair_frames_device(0, &c, 0, 0, &f, 1, &j, 1, 0, 0, 0, 0, &r, 0, 0)\n"
                   "         == tfs_repair_frames(0, &c, 0, 0, &f, 1, &j, 1, 0, 0, 0, 0, &r, 0)\n"
                   "         && tfs_repair_frame_count(&c, 100) && tfs_repair_span(&c, &j)\n"
                   "         && tfs_repair_parse(0, 0, 0, 8, 1, &f)\n"
                   "         && sizeof(tfs_repair_cfg) == 12 && sizeof(tfs_repair_job) == 72\n"
                   "         && sizeof(tfs_repair_in) == 24 && sizeof(tfs_repair_result) == 24\n"
                   "         && TFS_WRITE_DATA_MESSAGE == 9 && TFS_WRITE_MAX_DS == 27 && TFS_REPAIR_IN_HEAD == 28;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    alone = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                            os.path.join(ROOT, "include", "tfs_repair.h")], capture_output=True, text=True)
    assert alone.returncode == 0, alone.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_repair.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tfs_\w+)\s*\(", src)) == set(REPAIR)
    for name in REPAIR:
        assert hasattr(L, name), name
        assert name in crc.EXPORTED
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")],
                              capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(tfs_repair_\w+)\b", exported)) == set(REPAIR)
    assert len(L.tfs_repair_frames_device.argtypes) == 15 and len(L.tfs_repair_frames.argtypes) == 14
    assert callable(crc.Context.repair_frames) and callable(crc.Context.repair_frames_device)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tfs_repair_frames" in integ and "file_repair.cpp:81-197" in integ


def test_struct_layouts():
    import tfs_amd.crc as crc
    assert (crc.REPAIR_IN_DTYPE.itemsize, crc.REPAIR_JOB_DTYPE.itemsize, crc.REPAIR_CFG_DTYPE.itemsize,
            crc.REPAIR_RESULT_DTYPE.itemsize) == (24, 72, 12, 24)
    f = crc.REPAIR_IN_DTYPE.fields
    assert [f[k][1] for k in ("frame_off", "avail", "data_len", "pcode", "trailer", "reserved")] == [0, 8, 12, 16, 18, 20]
    f = crc.REPAIR_JOB_DTYPE.fields
    assert [f[k][1] for k in ("frame_offset", "file_id", "file_number", "packet_id", "stat_size", "block_id", "in_first",
                              "in_count", "ds_first", "ds_count", "stat_crc", "check_crc", "reserved")] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68]
    f = crc.REPAIR_CFG_DTYPE.fields
    assert [f[k][1] for k in ("frame_len", "is_server", "version", "reserved")] == [0, 4, 8, 10]
    f = crc.REPAIR_RESULT_DTYPE.fields
    assert [f[k][1] for k in ("status", "n_frames", "span_len", "file_crc", "bad_in", "flags")] == [0, 4, 8, 12, 16, 20]


@pytest.mark.parametrize("frame_len", [1024, 16384, 1 << 20, 3])
@pytest.mark.parametrize("ds_count", [0, 2, 27])
def test_frame_count_and_span_at_the_cuts(frame_len, ds_count):
    import tfs_amd.crc as crc
    cfg = crc.repair_cfg(frame_len)
    head = 60 + 8 * ds_count
    for n, want in ((1, 1), (frame_len - 1, 1), (frame_len, 1), (frame_len + 1, 2), (2 * frame_len, 2),
                    (2 * frame_len + 1, 3)):
        assert crc.repair_frame_count(cfg, n) == want, (n, want)
        j = np.zeros(1, crc.REPAIR_JOB_DTYPE)
        j["stat_size"], j["ds_count"] = n, ds_count
        assert crc.repair_span(cfg, j) == want * head + n, (n, want)


def test_frame_count_and_span_refuse_bad_input():
    import tfs_amd.crc as crc
    L = crc.lib()
    good = crc.repair_cfg(300)
    j = np.zeros(1, crc.REPAIR_JOB_DTYPE)
    j["stat_size"] = 500
    assert L.tfs_repair_frame_count(None, 500) == 0 and L.tfs_repair_span(None, j.ctypes.data) == 0
    assert L.tfs_repair_span(good.ctypes.data, None) == 0
    for size in (0, -1, -(1 << 40)):
        assert crc.repair_frame_count(good, size) == 0
        j["stat_size"] = size
        assert crc.repair_span(good, j) == 0
    for bad in (crc.repair_cfg(0), crc.repair_cfg(-5)):
        assert crc.repair_frame_count(bad, 500) == 0
    j["stat_size"], j["ds_count"] = 500, 28
    assert crc.repair_span(good, j) == 0
    j["ds_count"] = 27
    assert crc.repair_span(good, j) == 2 * (60 + 8 * 27) + 500


def test_parse():
    import tfs_amd.crc as crc
    fi = bytes(range(36))
    for pcode in (8, 39, 63):
        first = np.frombuffer(pk.read_reply_frame(b"x" * 700, pcode, 2, 9, file_info=fi), np.uint8)
        later = np.frombuffer(pk.read_reply_frame(b"y" * 33, pcode, 2, 10), np.uint8)
        assert first.size == 28 + 700 + (0 if pcode == 8 else 40) and later.size == 28 + 33 + (0 if pcode == 8 else 4)
        rc, d = crc.repair_parse(first, pcode, True, frame_off=12345)
        assert rc == 0
        assert (int(d["frame_off"][0]), int(d["avail"][0]), int(d["data_len"][0]), int(d["pcode"][0]),
                int(d["trailer"][0]), int(d["reserved"][0])) == (12345, first.size, 700, pcode, 0 if pcode == 8 else 40, 0)
        rc, d = crc.repair_parse(later, pcode, False, frame_off=(1 << 33) + 5, avail=100)
        assert rc == 0
        assert (int(d["frame_off"][0]), int(d["avail"][0]), int(d["data_len"][0]), int(d["pcode"][0]),
                int(d["trailer"][0])) == ((1 << 33) + 5, 100, 33, pcode, 0 if pcode == 8 else 4)
        assert crc.repair_parse(first[:27], pcode, True)[0] == INCOMPLETE
        assert crc.repair_parse(first[:28], pcode, True)[0] == 0
    # the source's error reply: set_length(status), the negative value comes back and *out stays
    err = np.frombuffer(pk.frame_v1(struct.pack("<i", -8074), 8, 2, 3), np.uint8)
    L = crc.lib()
    d = np.zeros(1, crc.REPAIR_IN_DTYPE)
    d["data_len"] = 77
    assert L.tfs_repair_parse(err.ctypes.data, err.size, 0, 8, 1, d.ctypes.data) == -8074
    assert int(d["data_len"][0]) == 77 and int(d["avail"][0]) == 0
    assert L.tfs_repair_parse(None, 100, 0, 8, 1, d.ctypes.data) == PARAM
    assert L.tfs_repair_parse(err.ctypes.data, err.size, 0, 8, 1, None) == PARAM
    assert L.tfs_repair_parse(err.ctypes.data, err.size, 0, 9, 1, d.ctypes.data) == PARAM


def test_null_calls_fail_without_a_device():
    """The first check of every call comes before any device is touched: a NULL context, whatever
    else is wrong with the call."""
    import tfs_amd.crc as crc
    L = crc.lib()
    good, worse = crc.repair_cfg(300), crc.repair_cfg(-1, reserved=1)
    jobs = np.zeros(2, crc.REPAIR_JOB_DTYPE)
    jobs["stat_size"], jobs["in_count"] = 100, 1
    ins = np.zeros(2, crc.REPAIR_IN_DTYPE)
    ds = np.zeros(4, np.uint64)
    buf = np.zeros(8192, np.uint8)
    res = np.zeros(2, crc.REPAIR_RESULT_DTYPE)
    nbad = np.zeros(1, np.uint32)
    p = buf.ctypes.data
    for cfg in (good, worse):
        assert L.tfs_repair_frames_device(None, cfg.ctypes.data, p, 4096, ins.ctypes.data, 2, jobs.ctypes.data, 2,
                                          ds.ctypes.data, 4, p + 4096, 4096, res.ctypes.data, nbad.ctypes.data,
                                          None) == PARAM
        assert L.tfs_repair_frames(None, cfg.ctypes.data, p, 4096, ins.ctypes.data, 2, jobs.ctypes.data, 2,
                                   ds.ctypes.data, 4, p + 4096, 4096, res.ctypes.data, nbad.ctypes.data) == PARAM
    assert L.tfs_repair_frames_device(None, None, None, 5, None, 4, None, 3, None, 2, None, 1, None, None, 2) == PARAM
    assert L.tfs_repair_frames(None, None, None, 5, None, 4, None, 3, None, 2, None, 1, None, None) == PARAM
    assert not buf.any() and not res.view(np.uint8).any() and nbad[0] == 0


def test_product_library_carries_one_form_of_the_kernels():
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "tfs_amd", "libtfs_crc.so")], capture_output=True, text=True,
                         check=True).stdout
    forms = set(re.findall(r"(repair\w*_kernel(?:<[^>]*>)?)\(", out))
    assert forms == {"repair_kernel", "repair_in_fold_kernel", "repair_job_fold_kernel", "repair_out_fold_kernel"}, forms
