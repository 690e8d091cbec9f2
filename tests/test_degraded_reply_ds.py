"""reply_reads_degrade (tfs_amd/ds/degraded_reply.h): DataService::read_data_degrade over a Family and the
lost block's parity index with the reply made in one pass (include/tfs_ec_read.h).  Found and not-found
requests, deleted / concealed / invalid files with and without FORCE, a corrupt survivor as a sealed
TFS_EXIT_CHECK_CRC_ERROR frame and one BlockCrcChecker error, and frames that decode through decode_stream to
the payloads the intact block serves through reply_reads.  Through tfs_ds_reply_reads_degrade and
dataserver.reply_reads_degrade (the binding calls the C entry point)."""
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
K, M, LOST = 3, 2, 1
IDS = [100, 101, 102, 200, 201]


@pytest.fixture(scope="module")
def ds():
    from tfs_amd import dataserver
    dataserver.lib()
    return dataserver


@pytest.fixture(scope="module")
def family(gpu_ctx, ds, oracle):
    """Three data blocks of different lengths (not zero-extended: the layer extends them), the second one lost;
    its files 2, 4 and 6 deleted, concealed and invalid, on disk and in the index."""
    from tfs_amd.ec import ErasureCode
    blocks, pays = [], {}
    for i in range(K):
        b = ds.LogicBlock(IDS[i])
        for k, ln in enumerate((65536, 3000, 0, 40, 5000, 1234, 70001) if i == LOST else (50000 + 777 * i,) * (2 + i)):
            p = synth_bytes(900 + 50 * i + k, ln).tobytes()
            assert b.append(k + 1, p, ocrc(oracle, 0, p)) == 0
            if i == LOST:
                pays[k + 1] = p
        blocks.append(b)
    tb = blocks[LOST]
    at = {int(x["file_id"]): int(x["offset"]) for x in tb.metas()[0]}
    for fid, flag in ((2, 1), (4, 4), (6, 2)):
        assert tb.corrupt(at[fid] + 28, flag) == 0     # FileInfo.flag_ on disk
        assert tb.set_flag(fid, flag) == 0             # and in the index
    size = (max(b.raw().size for b in blocks) + 1023) // 1024 * 1024
    imgs = []
    for b in blocks:
        a = np.zeros(size, np.uint8)
        a[:b.raw().size] = b.raw()
        imgs.append(a)
    imgs += [np.zeros(size, np.uint8) for _ in range(M)]
    enc = ErasureCode(gpu_ctx, K, M)
    assert enc.rc == 0 and enc.encode(imgs, size) == 0
    enc.free()
    index = tb.metas()[0]
    return blocks, pays, imgs, index


def _fam(ds, blocks, imgs, data=None):
    data = data or [b.raw() for b in blocks]
    return ds.Family(K, M, IDS, [None if i == LOST else data[i] for i in range(K)] + list(imgs[K:]))


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


ROWS = [(1, 0, 1 << 20, 39, 0), (2, 0, 3000, 39, 0), (2, 0, 3000, 39, 1), (3, 0, 100, 63, 0),
        (4, 0, 40, 8, 0), (4, 0, 40, 8, 1), (6, 0, 1234, 39, 1), (77, 0, 10, 8, 0), (77, 0, 10, 63, 0),
        (5, 100, 200, 39, 0), (5, 0, 5000, 8, 0), (2, 10, 50, 39, 0), (7, 0, 70001, 63, 0), (7, 60000, 1 << 20, 39, 0),
        (1, 0, 0, 39, 0), (6, 5, 10, 8, 0)]
WANT = [0, INFO_ERR, 0, 0, INFO_ERR, 0, INFO_ERR, META_NOT_FOUND, META_NOT_FOUND, 0, 0, 0, 0, 0, 0, 0]


def test_found_missing_flags_and_force_equal_the_intact_block(gpu_ctx, ds, oracle, family):
    blocks, pays, imgs, index = family
    tb = blocks[LOST]
    chk = ds.BlockCrcChecker(4)
    rc, frames, rep = ds.reply_reads_degrade(gpu_ctx, _fam(ds, blocks, imgs), IDS[LOST], index, _requests(ds, ROWS), chk)
    assert rc == sum(1 for w in WANT if w) and chk.errors(IDS[LOST]) == 0
    assert [int(s) for s in rep["status"]] == WANT
    # the intact block serves the same requests through reply_reads: the same statuses and, frame by frame, bytes
    irc, iframes, irep = ds.reply_reads(gpu_ctx, tb, _requests(ds, ROWS))
    assert irc == rc and [int(s) for s in irep["status"]] == WANT
    offs = {int(x["file_id"]): int(x["offset"]) for x in index}
    for k, (fid, ro, rl, pcode, force) in enumerate(ROWS):
        f = _frame(frames, rep[k])
        got_pcode, pid, crc = _sealed(f)
        assert got_pcode == pcode and pid == 9000 + k and crc == int(rep[k]["frame_crc"])
        assert f == _frame(iframes, irep[k]), k
        if not WANT[k]:
            assert int(rep[k]["file_crc"]) == int(irep[k]["file_crc"])
        drc, off, st, dcrc, consumed = ds.decode_stream(gpu_ctx, f)
        assert drc == 0 and list(st) == [0] and consumed == len(f) and int(dcrc[0]) == crc
        if WANT[k]:
            assert f[24:] == struct.pack("<i", WANT[k]) + (b"" if pcode == 8 else struct.pack("<i", 0))
            continue
        pay = pays[fid]
        n = min(rl, len(pay) - ro)
        assert struct.unpack_from("<i", f, 24)[0] == n and f[28:28 + n] == pay[ro:ro + n]
        # each frame is placed on the slice's address in the lost member mod 16
        assert (int(rep[k]["frame_offset"]) + 28) % 16 == (offs[fid] + FI + ro) % 16
    ends = 0
    for r in rep:
        assert int(r["frame_offset"]) >= ends
        ends = int(r["frame_offset"]) + int(r["frame_len"])
    chk.free()


def test_corrupt_survivor_is_a_crc_error_frame_and_one_checker_error(gpu_ctx, ds, oracle, family):
    blocks, pays, imgs, index = family
    offs = {int(x["file_id"]): int(x["offset"]) for x in index}
    hurt = blocks[2].raw().copy()
    hurt[offs[7] + 40000] ^= 2
    fam = _fam(ds, blocks, imgs, data=[blocks[0].raw(), None, hurt])
    chk = ds.BlockCrcChecker(4)
    rows = [(1, 0, 65536, 39, 0), (7, 0, 70001, 39, 0), (5, 0, 5000, 8, 0), (7, 100, 50, 8, 0), (7, 0, 70001, 8, 0)]
    rc, frames, rep = ds.reply_reads_degrade(gpu_ctx, fam, IDS[LOST], index, _requests(ds, rows), chk)
    assert rc == 2 and [int(s) for s in rep["status"]] == [0, CRC_ERR, 0, 0, CRC_ERR]
    assert chk.errors(IDS[LOST]) == 2
    for k, want in ((1, struct.pack("<ii", CRC_ERR, 0)), (4, struct.pack("<i", CRC_ERR))):
        f = _frame(frames, rep[k])
        _sealed(f)
        assert f[24:] == want
        drc, off, st, dcrc, consumed = ds.decode_stream(gpu_ctx, f)
        assert drc == 0 and list(st) == [0]
        assert int(rep[k]["file_crc"]) not in (0, ocrc(oracle, 0, pays[7]))     # as recomputed on the wrong bytes
    for k, fid in ((0, 1), (2, 5)):
        f = _frame(frames, rep[k])
        _sealed(f)
        n = struct.unpack_from("<i", f, 24)[0]
        assert f[28:28 + n] == pays[fid]
    chk.free()


def test_family_errors_and_small_buffer(gpu_ctx, ds, family):
    blocks, pays, imgs, index = family
    fam = _fam(ds, blocks, imgs)
    req = _requests(ds, ROWS[:3])
    assert ds.reply_reads_degrade(gpu_ctx, fam, 555, index, req)[0] == -16008          # not in the family
    short = ds.Family(K, M, IDS, [None, None, blocks[2].raw(), None, imgs[4]])
    assert ds.reply_reads_degrade(gpu_ctx, short, IDS[LOST], index, req)[0] == -16004  # too few members
    rc, frames, rep = ds.reply_reads_degrade(gpu_ctx, fam, IDS[LOST], index, req)
    assert rc == 1
    rc2, frames2, rep2 = ds.reply_reads_degrade(gpu_ctx, fam, IDS[LOST], index, req, cap=64)
    assert rc2 == -1016 and frames2.size == 64
    rc3, frames3, rep3 = ds.reply_reads_degrade(gpu_ctx, fam, IDS[LOST], index, req, cap=frames.size)
    assert rc3 == 1 and frames3.tobytes() == frames.tobytes() and rep3.tobytes() == rep.tobytes()
    assert ds.reply_reads_degrade(gpu_ctx, fam, IDS[LOST], index, req[:0])[0] == 0
