"""replicate_block (tfs_amd/ds/replicate.h): ReplicateTask::do_replicate over a LogicBlockImage
through a replicate session (include/tfs_replicate.h).  A clean block: every frame reaches the
sink in order, sealed, and the commit callback is called once; one rotten record: all frames
sent, no commit, the record's status returned with the full verdict list and one BlockCrcChecker
error; an empty block: one frame and a commit.  Through tfs_ds_replicate_block and
dataserver.replicate_block (the binding calls the C entry point)."""
import struct
import zlib

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

CRC_ERR = -1010
SIZES = [5000, 1, 70000, 36, 20000, 3000]


@pytest.fixture(scope="module")
def ds():
    from tfs_amd import dataserver
    dataserver.lib()
    return dataserver


def _block(ds, oracle, sizes, block_id=21):
    b = ds.LogicBlock(block_id)
    for i, ln in enumerate(sizes):
        p = synth_bytes(800 + i, ln).tobytes()
        assert b.append(i + 1, p, ocrc(oracle, 0, p)) == 0
    return b


def _check_frames(r, raw, fl, dest, pid, new_block):
    """Every frame sealed, in order, and the data landed at offset_ rebuilds the data file."""
    nfr = max(1, -(-len(raw) // fl))
    assert r["order"] == list(range(nfr)) and len(r["frames"]) == nfr
    landed = bytearray(len(raw))
    for k, f in enumerate(r["frames"]):
        f = f.tobytes()
        flag, length, pcode, ver, id_, crc = struct.unpack_from("<IihhQI", f)
        assert (flag, pcode, ver, id_) == (pk.TFS_PACKET_FLAG_V1, 35, 2, pid + k) and length == len(f) - 24
        assert crc == zlib.crc32(f[24:], pk.TFS_PACKET_FLAG_V1 ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
        block_id, fid, off, ln, is_server, fnum = struct.unpack_from("<IQiiiQ", f, 24)
        assert (block_id, fid, off, is_server, fnum) == (dest, 0, k * fl, 0, 0) and ln == len(f) - 60
        assert ln == min(fl, len(raw) - k * fl)
        assert struct.unpack_from("<i", f, 56 + ln)[0] == (new_block if k == 0 else 0)
        landed[off:off + ln] = f[56:56 + ln]
    assert bytes(landed) == raw


@pytest.mark.parametrize("fl,per", [(4096, 8), (1024, 3), (1 << 20, 8)])
def test_clean_block_is_sent_and_committed(gpu_ctx, ds, oracle, fl, per):
    b = _block(ds, oracle, SIZES)
    chk = ds.BlockCrcChecker(4)
    r = ds.replicate_block(gpu_ctx, b, dest_block_id=77, packet_id=5000, frame_len=fl, frames_per_call=per, checker=chk)
    assert r["rc"] == 0 and r["commits"] == 1 and chk.errors(21) == 0
    _check_frames(r, b.raw().tobytes(), fl, 77, 5000, 1)
    assert r["file_ids"].tolist() == list(range(1, len(SIZES) + 1)) and not r["status"].any()
    m, _ = b.metas()
    raw = b.raw().tobytes()
    for i, mm in enumerate(m):
        o, s = int(mm["offset"]), int(mm["size"])
        assert int(r["crc"][i]) == ocrc(oracle, 0, raw[o + 36:o + s])
    chk.free()
    b.free()


def test_rotten_record_is_sent_but_not_committed(gpu_ctx, ds, oracle):
    b = _block(ds, oracle, SIZES)
    m, _ = b.metas()
    assert b.corrupt(int(m[2]["offset"]) + 36 + 40000, 0x10) == 0   # inside the 70,000-byte payload
    chk = ds.BlockCrcChecker(4)
    r = ds.replicate_block(gpu_ctx, b, dest_block_id=78, packet_id=9, frame_len=4096, frames_per_call=5,
                           new_block=2, checker=chk)
    assert r["rc"] == CRC_ERR and r["commits"] == 0
    assert r["status"].tolist() == [0, 0, CRC_ERR, 0, 0, 0]
    assert chk.errors(21) == 1
    _check_frames(r, b.raw().tobytes(), 4096, 78, 9, 2)            # faithful, sealed copies of the bytes as they are
    chk.free()
    b.free()


def test_empty_block_is_one_frame_and_a_commit(gpu_ctx, ds, oracle):
    b = _block(ds, oracle, [])
    r = ds.replicate_block(gpu_ctx, b, dest_block_id=79, packet_id=1, frame_len=4096)
    assert r["rc"] == 0 and r["commits"] == 1 and r["status"].size == 0
    assert len(r["frames"]) == 1 and r["frames"][0].size == 60 and r["bytes"] == 60
    _check_frames(r, b"", 4096, 79, 1, 1)
    b.free()
