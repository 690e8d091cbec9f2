"""reply_reads (tfs_amd/ds/read_reply.h): DataService::read_data / read_data_extra over a
LogicBlockImage with the reply made in one pass (include/tfs_read.h).  Live, deleted,
concealed, invalid and missing files with and without FORCE; a corrupt payload leaves as a
TFS_EXIT_CHECK_CRC_ERROR frame and one BlockCrcChecker error; every good reply's data equals
what read_file_verified returns; every frame passes PacketDecoder.  Through
tfs_ds_reply_reads and dataserver.reply_reads (the binding calls the C entry point)."""
import struct
import zlib

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

FI = 36
META_NOT_FOUND, INFO_ERR, CRC_ERR = -8025, -8016, -1010


@pytest.fixture(scope="module")
def ds():
    from tfs_amd import dataserver
    dataserver.lib()
    return dataserver


def _block(ds, oracle, sizes):
    b = ds.LogicBlock(9)
    pays = []
    for i, ln in enumerate(sizes):
        p = synth_bytes(700 + i, ln).tobytes()
        assert b.append(i + 1, p, ocrc(oracle, 0, p)) == 0
        pays.append(p)
    return b, pays


def _requests(ds, rows):
    req = np.zeros(len(rows), ds.READ_REQUEST_DTYPE)
    for k, (fid, ro, rl, pcode, force) in enumerate(rows):
        req[k] = (fid, 9000 + k, ro, rl, pcode, 2, force)
    return req


def _frame(frames, rep):
    o = int(rep["frame_offset"])
    return frames[o:o + int(rep["frame_len"])].tobytes()


def _sealed(frame):
    flag, length, pcode, ver, pid, crc = struct.unpack_from("<IihhQI", frame)
    assert flag == pk.TFS_PACKET_FLAG_V1 and length == len(frame) - 24
    assert crc == zlib.crc32(frame[24:], pk.TFS_PACKET_FLAG_V1 ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
    return pcode, pid, crc


def test_reply_reads_flags_force_and_missing(gpu_ctx, ds, oracle):
    b, pays = _block(ds, oracle, [65536, 3000, 0, 40, 5000, 1234])
    assert b.set_flag(2, 1) == 0       # FI_DELETED
    assert b.set_flag(4, 4) == 0       # FI_CONCEAL
    assert b.set_flag(6, 2) == 0       # FI_INVALID
    rows = [(1, 0, 1 << 20, 39, 0), (2, 0, 3000, 39, 0), (2, 0, 3000, 39, 1), (3, 0, 100, 63, 0),
            (4, 0, 40, 8, 0), (4, 0, 40, 8, 1), (6, 0, 1234, 39, 1), (77, 0, 10, 8, 0), (77, 0, 10, 63, 0),
            (5, 100, 200, 39, 0), (5, 0, 5000, 8, 0), (2, 10, 50, 39, 0)]
    want = [0, INFO_ERR, 0, 0, INFO_ERR, 0, INFO_ERR, META_NOT_FOUND, META_NOT_FOUND, 0, 0, 0]
    chk = ds.BlockCrcChecker(4)
    rc, frames, rep = ds.reply_reads(gpu_ctx, b, _requests(ds, rows), chk)
    assert rc == sum(1 for w in want if w) and chk.errors(9) == 0
    assert [int(s) for s in rep["status"]] == want
    raw = b.raw()
    m, _ = b.metas()
    for k, (fid, ro, rl, pcode, force) in enumerate(rows):
        f = _frame(frames, rep[k])
        got_pcode, pid, crc = _sealed(f)
        assert got_pcode == pcode and pid == 9000 + k and crc == int(rep[k]["frame_crc"])
        if want[k]:
            assert f[24:] == struct.pack("<i", want[k]) + (b"" if pcode == 8 else struct.pack("<i", 0))
            continue
        pay = pays[fid - 1]
        n = min(rl, len(pay) - ro)
        assert struct.unpack_from("<i", f, 24)[0] == n and f[28:28 + n] == pay[ro:ro + n]
        if pcode != 8 and ro == 0:
            o = int(m["offset"][fid - 1])
            fi = bytearray(raw[o:o + FI].tobytes())
            struct.pack_into("<i", fi, 12, len(pay))
            assert f[28 + n:] == struct.pack("<i", FI) + bytes(fi)
            assert int(rep[k]["file_crc"]) == ocrc(oracle, 0, pay)
        elif pcode != 8:
            assert f[28 + n:] == struct.pack("<i", 0) and int(rep[k]["file_crc"]) == 0
    # every frame decodes: walk them one by one (frames are placed, not packed)
    for k in range(len(rows)):
        drc, off, st, dcrc, consumed = ds.decode_stream(gpu_ctx, _frame(frames, rep[k]))
        assert drc == 0 and list(st) == [0] and consumed == int(rep[k]["frame_len"])
        assert int(dcrc[0]) == int(rep[k]["frame_crc"])
    chk.free()
    b.free()


def test_corrupt_payload_is_a_crc_error_frame_and_one_checker_error(gpu_ctx, ds, oracle):
    b, pays = _block(ds, oracle, [65536, 3000, 200])
    m, _ = b.metas()
    assert b.corrupt(int(m["offset"][1]) + FI + 17, 0x04) == 0
    chk = ds.BlockCrcChecker(4)
    rows = [(1, 0, 65536, 39, 0), (2, 0, 3000, 39, 0), (3, 0, 200, 8, 0), (2, 100, 50, 8, 0)]
    rc, frames, rep = ds.reply_reads(gpu_ctx, b, _requests(ds, rows), chk)
    assert rc == 1 and [int(s) for s in rep["status"]] == [0, CRC_ERR, 0, 0] and chk.errors(9) == 1
    f = _frame(frames, rep[1])
    _sealed(f)
    assert len(f) == 32 and f[24:] == struct.pack("<ii", CRC_ERR, 0)
    # a good reply's data is what read_file_verified returns for the same file
    for k, fid in ((0, 1), (2, 3)):
        vrc, data = b.read_file_verified(gpu_ctx, fid)
        f = _frame(frames, rep[k])
        n = struct.unpack_from("<i", f, 24)[0]
        assert vrc == 0 and f[28:28 + n] == data[FI:] == pays[fid - 1]
    assert b.read_file_verified(gpu_ctx, 2)[0] == CRC_ERR
    chk.free()
    b.free()


def test_frames_follow_the_source_alignment_and_fit_a_small_buffer(gpu_ctx, ds, oracle):
    b, pays = _block(ds, oracle, [100, 37, 2000, 5])
    rows = [(k + 1, ro, 1 << 20, 39, 0) for k in range(4) for ro in (0, 3)]
    rc, frames, rep = ds.reply_reads(gpu_ctx, b, _requests(ds, rows))
    assert rc == 0
    base = ds.lib().tfs_ds_block_data(b.h)
    m, _ = b.metas()
    ends = 0
    for k, (fid, ro, rl, pcode, force) in enumerate(rows):
        fo = int(rep[k]["frame_offset"])
        assert (fo + 28) % 16 == (base + int(m["offset"][fid - 1]) + FI + ro) % 16
        assert fo >= ends
        ends = fo + int(rep[k]["frame_len"])
    # the C entry point refuses a buffer the frames do not fit and says what they need
    rc2, frames2, rep2 = ds.reply_reads(gpu_ctx, b, _requests(ds, rows), cap=64)
    assert rc2 == -1016 and frames2.size == 64
    rc3, frames3, rep3 = ds.reply_reads(gpu_ctx, b, _requests(ds, rows), cap=frames.size)
    assert rc3 == 0 and frames3.tobytes() == frames.tobytes() and rep3.tobytes() == rep.tobytes()
    b.free()
