"""CPU-side checks of the degraded read replies' boundary (include/tfs_ec_read.h): the host
plan of tfs_amd/csrc/ec_reply_plan.h -- covering sets (every unit exactly once, nothing else), span overlap,
parameter errors, the packed host images and the staged frames -- checked on random job lists against a
brute-force restatement by a stand-alone program under the host's address and undefined-behaviour sanitizers
(tools/degraded_reply_plan_check.cpp; no Python runs under a sanitizer); the exported symbols, the job layout
and the calls that fail before they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

REPLY = ["tfs_ec_read_reply_device", "tfs_ec_read_reply"]


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "degraded_reply_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tools", "degraded_reply_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"degraded reply plan ok: (\d+) jobs, (\d+) lists, (\d+) with overlapping spans", out.stdout)
    assert m and int(m.group(1)) >= 4000 and int(m.group(2)) >= 300 and int(m.group(3)) >= 20, out.stdout


def test_symbols_layout_and_null_calls():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = ec.lib()
    for name in REPLY:
        assert hasattr(L, name) and name in ec.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "tfs_ec_read.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(tfs_\w+)\s*\(", src))) == sorted(REPLY)
    assert '#include "tfs_ec.h"' in hdr and '#include "tfs_read.h"' in hdr
    # the job: a tfs_read_job, the refuse mask behind it
    assert ec.REPLY_JOB_DTYPE.itemsize == 56
    assert ec.REPLY_JOB_DTYPE.names[:len(crc.READ_JOB_DTYPE.names)] == crc.READ_JOB_DTYPE.names
    for f in crc.READ_JOB_DTYPE.names:
        assert ec.REPLY_JOB_DTYPE.fields[f][1] == crc.READ_JOB_DTYPE.fields[f][1]
    assert ec.REPLY_JOB_DTYPE.fields["refuse_flags"][1] == 48 and ec.REPLY_JOB_DTYPE.fields["reserved"][1] == 52
    rj = np.zeros(3, crc.READ_JOB_DTYPE)
    rj["src_offset"], rj["size"], rj["pcode"] = [5, 6, 7], 100, 39
    j = ec.ErasureCode.reply_jobs(rj, refuse_flags=[1, 2, 7])
    assert j["src_offset"].tolist() == [5, 6, 7] and j["refuse_flags"].tolist() == [1, 2, 7] and (j["pcode"] == 39).all()
    # a NULL coder is refused before anything else, in both forms
    nul = ctypes.c_void_p()
    assert L.tfs_ec_read_reply(nul, None, None, 1024, 0, None, 0, None, 0, None, None) == -1016
    assert L.tfs_ec_read_reply_device(nul, None, None, 1024, 0, None, 0, None, 0, None, None, None) == -1016


def test_sizeof_job_in_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tfs_ec_read.h"\n#include <stddef.h>\n'
                   "typedef char a[sizeof(tfs_ec_reply_job) == 56 ? 1 : -1];\n"
                   "typedef char b[offsetof(tfs_ec_reply_job, refuse_flags) == 48 ? 1 : -1];\n"
                   "typedef char c[sizeof(tfs_read_result) == 16 ? 1 : -1];\nint main(void) { return 0; }\n")
    for std in ("c99", "c11"):
        r = subprocess.run(["gcc", "-x", "c", "-std=" + std, "-Wall", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
