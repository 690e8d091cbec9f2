"""mirror_copy_files (tfs_amd/ds/mirror_sync.h): TfsMirrorBackup::copy_file over a batch of files of
one LogicBlockImage through one mirror sync call (include/tfs_mirror.h).  The sink receives exactly
the good files' frames, in order, each file's close after its last frame with its CRC; an id that is
not in the index is skipped as success; a deleted file is sent and an invalid one refused (the read
is forced); a rotten file reaches neither callback and is counted once in BlockCrcChecker.  Through
tfs_ds_mirror_copy_files and dataserver.mirror_copy_files (the binding calls the C entry point)."""
import struct
import zlib

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

CRC_ERR, INFO_ERR = -1010, -8016
SIZES = [5000, 1, 2500, 988, 989, 3000]
FIRST, FL, DEST = 1024 - 36, 1024, 0x5151


@pytest.fixture(scope="module")
def ds():
    from tfs_amd import dataserver
    dataserver.lib()
    return dataserver


def _block(ds, oracle, block_id=31):
    b = ds.LogicBlock(block_id)
    for i, ln in enumerate(SIZES):
        p = synth_bytes(900 + i, ln).tobytes()
        assert b.append(i + 1, p, ocrc(oracle, 0, p)) == 0
    return b


def _files(ids):
    """(file_id, file_number, packet_id, ds) per id; ds lists of 0, 1, 2 and 5 entries."""
    return [(fid, 0xA000 + fid, 7000 + 100 * k, [0xD500 + 16 * k + d for d in range((0, 1, 2, 5)[k % 4])])
            for k, fid in enumerate(ids)]


def _check_file_frames(frames, payload, file, version=2, is_server=0):
    """The frames of one file: sealed, numbered, and their data rebuilds the payload."""
    fid, fnum, pid, dsl = file
    got, want_off = b"", 0
    for k, f in enumerate(frames):
        f = f.tobytes()
        flag, length, pcode, ver, id_, crc = struct.unpack_from("<IihhQI", f)
        assert (flag, pcode, ver, id_) == (pk.TFS_PACKET_FLAG_V1, 9, version, pid + k) and length == len(f) - 24
        assert crc == zlib.crc32(f[24:], pk.TFS_PACKET_FLAG_V1 ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
        block_id, hfid, off, ln, srv, hnum = struct.unpack_from("<IQiiiQ", f, 24)
        assert (block_id, hfid, off, srv, hnum) == (DEST, fid, want_off, is_server, fnum)
        assert struct.unpack_from("<i", f, 56)[0] == len(dsl)
        assert list(struct.unpack_from("<%dQ" % len(dsl), f, 60)) == dsl
        head = 60 + 8 * len(dsl)
        assert ln == len(f) - head and ln == min(FIRST if k == 0 else FL, len(payload) - want_off)
        got += f[head:]
        want_off += ln
    assert got == payload


def _payloads(b):
    m, _ = b.metas()
    raw = b.raw().tobytes()
    return {int(x["file_id"]): raw[int(x["offset"]) + 36:int(x["offset"]) + int(x["size"])] for x in m}


def test_good_files_are_sent_in_order_and_closed(gpu_ctx, ds, oracle):
    b = _block(ds, oracle)
    pay = _payloads(b)
    chk = ds.BlockCrcChecker(4)
    files = _files([3, 1, 6, 2, 4, 5])
    r = ds.mirror_copy_files(gpu_ctx, b, files, DEST, FIRST, FL, checker=chk)
    assert r["rc"] == 0 and chk.errors(31) == 0
    at = 0
    for i, f in enumerate(files):
        n = int(r["files"][i]["n_frames"])
        assert n == max(1, 1 + -(-(len(pay[f[0]]) - FIRST) // FL)) and int(r["files"][i]["status"]) == 0
        assert r["frame_file"][at:at + n] == [i] * n and r["frame_k"][at:at + n] == list(range(n))
        _check_file_frames(r["frames"][at:at + n], pay[f[0]], f)
        at += n
        assert r["closes"][i] == (i, ocrc(oracle, 0, pay[f[0]]), at)   # after the file's last frame, with its CRC
        assert int(r["files"][i]["file_crc"]) == r["closes"][i][1]
    assert at == len(r["frames"]) and len(r["closes"]) == len(files)
    assert r["bytes"] == sum(f.size for f in r["frames"])
    chk.free()
    b.free()


def test_unknown_deleted_invalid_and_rotten_files(gpu_ctx, ds, oracle):
    from tfs_amd import crc
    b = _block(ds, oracle)
    m, _ = b.metas()
    off = {int(x["file_id"]): int(x["offset"]) for x in m}
    assert b.set_flag(2, crc.FI_DELETED) == 0 and b.set_flag(4, crc.FI_INVALID) == 0
    assert b.corrupt(off[6] + 36 + 1500, 0x04) == 0      # in the middle frame of file 6
    pay = _payloads(b)
    chk = ds.BlockCrcChecker(4)
    files = _files([1, 99, 6, 2, 4, 3])
    r = ds.mirror_copy_files(gpu_ctx, b, files, DEST, FIRST, FL, is_server=1, checker=chk)
    assert r["rc"] == 2
    st = r["files"]
    assert st["status"].tolist() == [0, 0, CRC_ERR, 0, INFO_ERR, 0]
    assert st["skipped"].tolist() == [0, 1, 0, 0, 0, 0]
    assert st["n_frames"].tolist() == [5, 0, 0, 1, 0, 3]
    assert chk.errors(31) == 1                                           # the rotten file, once
    assert int(st["file_crc"][2]) == ocrc(oracle, 0, pay[6])            # as recomputed, not as stored
    # the sink saw the good files only, in order; close came for each of them after its frames
    assert r["frame_file"] == [0] * 5 + [3] + [5] * 3
    assert r["frame_k"] == [0, 1, 2, 3, 4, 0, 0, 1, 2]
    assert r["closes"] == [(0, ocrc(oracle, 0, pay[1]), 5), (3, ocrc(oracle, 0, pay[2]), 6),
                           (5, ocrc(oracle, 0, pay[3]), 9)]
    _check_file_frames(r["frames"][0:5], pay[1], files[0], is_server=1)
    _check_file_frames(r["frames"][5:6], pay[2], files[3], is_server=1)   # deleted: sent (the read is forced)
    _check_file_frames(r["frames"][6:9], pay[3], files[5], is_server=1)
    chk.free()
    b.free()


def test_nothing_to_sync(gpu_ctx, ds, oracle):
    b = _block(ds, oracle)
    r = ds.mirror_copy_files(gpu_ctx, b, _files([77, 78]), DEST, FIRST, FL)
    assert r["rc"] == 0 and r["frames"] == [] and r["closes"] == []
    assert r["files"]["skipped"].tolist() == [1, 1] and not r["files"]["status"].any()
    r = ds.mirror_copy_files(gpu_ctx, b, [], DEST, FIRST, FL)
    assert r["rc"] == 0 and r["frames"] == [] and len(r["files"]) == 0
    b.free()
