"""CPU-side checks of the marshalling session's boundary (include/tfs_ec.h): the plan
that tfs_ec_marshal_begin builds, checked by a stand-alone program under the host's
address and undefined-behaviour sanitizers (tools/marshal_plan_check.cpp; no Python
runs under a sanitizer), the exported symbols, and the calls that fail before they
touch a device."""
import ctypes
import os
import subprocess

from conftest import ROOT

MARSHAL = ["tfs_ec_marshal_begin", "tfs_ec_marshal_encode_device", "tfs_ec_marshal_encode", "tfs_ec_marshal_finish",
           "tfs_ec_marshal_free"]


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "marshal_plan_check")
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc,
                           os.path.join(ROOT, "tools", "marshal_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "marshal plan ok" in out.stdout


def test_symbols_and_null_calls():
    import tfs_amd.ec as ec
    L = ec.lib()
    for name in MARSHAL:
        assert name in ec.EXPORTED and hasattr(L, name)
    h = ctypes.c_void_p()
    assert L.tfs_ec_marshal_begin(None, None, None, None, 1024, ctypes.byref(h)) == -1016 and not h.value
    assert L.tfs_ec_marshal_encode_device(None, None, 0, 4096, None) == -1016
    assert L.tfs_ec_marshal_encode(None, None, 0, 4096) == -1016
    assert L.tfs_ec_marshal_finish(None, None, None, None) == -1016
    assert L.tfs_ec_marshal_free(None) == -1016
