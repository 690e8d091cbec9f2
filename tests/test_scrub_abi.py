"""CPU-side checks of the scrub session's boundary (include/tfs_ec.h): the five
symbols, the calls that fail before they touch a device, the kernel in the
product library and the dataserver layer's two entry points."""
import ctypes
import os
import re

from conftest import ROOT

SCRUB = ["tfs_ec_scrub_begin", "tfs_ec_scrub_check_device", "tfs_ec_scrub_check", "tfs_ec_scrub_finish",
         "tfs_ec_scrub_free"]


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_ec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    for name in SCRUB:
        assert hasattr(L, name), name
        assert name in ec.EXPORTED and name in declared
    assert hasattr(ec, "ScrubSession")
    for m in ("check", "check_device", "finish", "free"):
        assert callable(getattr(ec.ScrubSession, m))
    f = ec.lib().tfs_ec_scrub_begin
    assert f.restype is ctypes.c_int and len(f.argtypes) == 6
    assert len(ec.lib().tfs_ec_scrub_finish.argtypes) == 6


def test_null_calls_fail_without_a_device():
    import tfs_amd.ec as ec
    L = ec.lib()
    h = ctypes.c_void_p()
    assert L.tfs_ec_scrub_begin(None, None, None, None, 1024, ctypes.byref(h)) == -1016 and not h.value
    assert L.tfs_ec_scrub_check_device(None, None, 0, 4096, None) == -1016
    assert L.tfs_ec_scrub_check(None, None, 0, 4096) == -1016
    assert L.tfs_ec_scrub_finish(None, None, None, None, None, None) == -1016
    assert L.tfs_ec_scrub_free(None) == -1016


def test_product_library_carries_the_kernel():
    blob = open(os.path.join(ROOT, "tfs_amd", "libtfs_crc.so"), "rb").read()
    assert b"ec_scrub_kernel" in blob and b"ec_scrub_count_kernel" in blob


def test_dataserver_layer_resolves():
    import tfs_amd.dataserver as ds
    L = ds.lib()
    assert hasattr(L, "tfs_ds_scrub_family") and hasattr(L, "tfs_ds_scrub_classify")
    assert callable(ds.scrub_family) and callable(ds.scrub_classify)
