"""CPU-side checks of the frame-emitting chunk calls' boundary (include/tfs_ec_frames.h,
DESIGN.md §3.23): the host arithmetic -- every call check in the header's order, the
capacity, each frame's constants against Func::crc bit by bit -- checked by a stand-alone
program under the host's address and undefined-behaviour sanitizers
(tools/ec_frames_plan_check.cpp; no Python runs under a sanitizer), the header as C99, the
configuration's layout, the exported symbols, and the calls that fail before they touch a
device."""
import os
import re
import subprocess

from conftest import ROOT

FRAMES = ["tfs_ec_frames_cap", "tfs_ec_marshal_frames_device", "tfs_ec_marshal_frames", "tfs_ec_reinstate_frames_device",
          "tfs_ec_reinstate_frames"]


def test_plan_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ec_frames_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program, not loaded beside it
                           os.path.join(ROOT, "tools", "ec_frames_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ec frames plan ok: 144 frames" in out.stdout  # 2 frame lengths x 4 last frames x 3 versions x 2 kinds x 3


def test_header_is_c99_and_the_cfg_layout(tmp_path):
    import tfs_amd.ec as ec
    d = ec.FRAMES_CFG_DTYPE
    assert d.itemsize == 160
    assert [d.fields[f][1] for f in ("frame_len", "frame_stride", "version", "reserved", "block_id", "packet_id")] == \
        [0, 4, 8, 10, 12, 64]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "tfs_ec_frames.h"\n'
                   "typedef char a0[sizeof(tfs_ec_frames_cfg) == 160 ? 1 : -1];\n"
                   "typedef char a1[offsetof(tfs_ec_frames_cfg, frame_stride) == 4 ? 1 : -1];\n"
                   "typedef char a2[offsetof(tfs_ec_frames_cfg, version) == 8 ? 1 : -1];\n"
                   "typedef char a3[offsetof(tfs_ec_frames_cfg, reserved) == 10 ? 1 : -1];\n"
                   "typedef char a4[offsetof(tfs_ec_frames_cfg, block_id) == 12 ? 1 : -1];\n"
                   "typedef char a5[offsetof(tfs_ec_frames_cfg, packet_id) == 64 ? 1 : -1];\n"
                   "typedef char a6[TFS_EC_MAX_MEMBERS == 12 && TFS_RAW_PARITY_DATA == 2 && TFS_RAW_NORMAL_DATA == 1 ? 1 : -1];\n"
                   "int main(void) { return tfs_ec_frames_cap(0, 4096) != 0; }\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbols_resolve_and_are_declared():
    import tfs_amd.crc as crc
    import tfs_amd.ec as ec
    L = crc.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfs_ec_frames.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tfs_\w+)\s*\(", src))
    assert declared == set(FRAMES)
    for name in FRAMES:
        assert hasattr(L, name) and name in ec.EXPORTED
    for cls in (ec.MarshalSession, ec.ReinstateSession):
        assert callable(cls.frames) and callable(cls.frames_device)


def test_cap_is_host_arithmetic():
    import tfs_amd.ec as ec
    c = ec.frames_cfg(4096)
    assert ec.frames_cap(c, 4096) == 60 + 4096 and ec.frames_cap(c, 1024) == 60 + 1024
    assert ec.frames_cap(c, 3 * 4096 + 2048) == 3 * (4096 + 64) + 60 + 2048
    assert ec.frames_cap(ec.frames_cfg(4096, frame_stride=8192), 3 * 4096) == 2 * 8192 + 60 + 4096
    assert ec.frames_cap(ec.frames_cfg(1 << 20), 64 << 20) == 63 * ((1 << 20) + 64) + 60 + (1 << 20)
    for bad in (ec.frames_cfg(0), ec.frames_cfg(1024), ec.frames_cfg(4096, frame_stride=4096 + 56),
                ec.frames_cfg(4096, frame_stride=4096 + 60), ec.frames_cfg(4096, reserved=1)):
        assert ec.frames_cap(bad, 4096) == 0
    assert ec.frames_cap(c, 0) == 0 and ec.frames_cap(c, -4096) == 0
    assert ec.lib().tfs_ec_frames_cap(None, 4096) == 0


def test_null_calls_fail_without_a_device():
    import tfs_amd.ec as ec
    L = ec.lib()
    c = ec.frames_cfg(4096)
    assert L.tfs_ec_marshal_frames_device(None, c.ctypes.data, None, None, 0, 0, 4096, None) == -1016
    assert L.tfs_ec_marshal_frames(None, c.ctypes.data, None, None, 0, 0, 4096) == -1016
    assert L.tfs_ec_reinstate_frames_device(None, c.ctypes.data, None, None, 0, 0, 4096, None) == -1016
    assert L.tfs_ec_reinstate_frames(None, c.ctypes.data, None, None, 0, 0, 4096) == -1016


def test_product_library_carries_the_kernels_and_the_layers_resolve():
    blob = open(os.path.join(ROOT, "tfs_amd", "libtfs_crc.so"), "rb").read()
    assert b"ec_frames_kernel" in blob and b"ec_frames_seal_kernel" in blob
    import tfs_amd.dataserver as ds
    assert hasattr(ds.lib(), "tfs_ds_ec_task_frames") and callable(ds.do_marshalling_frames) and \
        callable(ds.do_reinstate_frames)
