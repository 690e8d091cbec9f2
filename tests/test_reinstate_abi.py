"""CPU-side checks of the reinstate session's boundary (include/tfs_ec.h): the five
symbols, the calls that fail before they touch a device, and the kernel in the
product library."""
import ctypes
import os
import re

from conftest import ROOT

REINSTATE = ["tfs_ec_reinstate_begin", "tfs_ec_reinstate_decode_device", "tfs_ec_reinstate_decode",
             "tfs_ec_reinstate_finish", "tfs_ec_reinstate_free"]


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_ec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    for name in REINSTATE:
        assert hasattr(L, name), name
        assert name in ec.EXPORTED and name in declared
    assert hasattr(ec, "ReinstateSession")
    f = ec.lib().tfs_ec_reinstate_begin
    assert f.restype is ctypes.c_int and len(f.argtypes) == 6


def test_null_calls_fail_without_a_device():
    import tfs_amd.ec as ec
    L = ec.lib()
    h = ctypes.c_void_p()
    assert L.tfs_ec_reinstate_begin(None, None, None, None, 1024, ctypes.byref(h)) == -1016 and not h.value
    assert L.tfs_ec_reinstate_decode_device(None, None, 0, 4096, None) == -1016
    assert L.tfs_ec_reinstate_decode(None, None, 0, 4096) == -1016
    assert L.tfs_ec_reinstate_finish(None, None, None, None) == -1016
    assert L.tfs_ec_reinstate_free(None) == -1016


def test_product_library_carries_the_kernel():
    blob = open(os.path.join(ROOT, "tfs_amd", "libtfs_crc.so"), "rb").read()
    assert b"ec_reinstate_kernel" in blob
    import tfs_amd.dataserver as ds
    assert hasattr(ds.lib(), "tfs_ds_do_reinstate") and hasattr(ds, "do_reinstate")
