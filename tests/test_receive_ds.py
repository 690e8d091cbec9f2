"""receive_block (tfs_amd/ds/receive.h): DataService::write_raw_data / batch_write_info over a new
LogicBlockImage through a receive session (include/tfs_receive.h).  dataserver.replicate_block's
frames go into dataserver.receive_block: a clean block is committed and serves every file; one
rotten source record: no commit, the status and the verdict list name it and BlockCrcChecker
counts it; one frame damaged in flight: the receive ends at that frame with its status; a parity
member without metas lands and commits."""
import struct
import zlib

import pytest

from conftest import ocrc
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

CRC_ERR, PARAM = -1010, -1016
SIZES = [5000, 1, 20000, 36, 9000, 3000]


@pytest.fixture(scope="module")
def ds():
    from tfs_amd import dataserver
    dataserver.lib()
    return dataserver


def _block(ds, oracle, sizes, block_id=21):
    b = ds.LogicBlock(block_id)
    for i, ln in enumerate(sizes):
        p = synth_bytes(900 + i, ln).tobytes()
        assert b.append(i + 1, p, ocrc(oracle, 0, p)) == 0
    return b


@pytest.mark.parametrize("fl,reads", [(4096, None), (1024, "each"), (1 << 20, None)])
def test_clean_block_is_committed(gpu_ctx, ds, oracle, fl, reads):
    src = _block(ds, oracle, SIZES)
    sent = ds.replicate_block(gpu_ctx, src, dest_block_id=77, packet_id=5000, frame_len=fl)
    assert sent["rc"] == 0
    m, _ = src.metas()
    dst = ds.LogicBlock(77)
    chk = ds.BlockCrcChecker(4)
    n = len(sent["frames"])
    r = ds.receive_block(gpu_ctx, dst, sent["frames"], m[::-1].copy(), reads=[1] * n if reads else None, checker=chk)
    assert r["rc"] == 0 and r["commits"] == 1 and chk.errors(77) == 0
    assert r["total"] == src.raw().size and r["new_block"] == 1 and len(r["parts"]) == n
    assert not r["parts"]["status"].any() and not r["status"].any()
    assert r["crc"].tolist() == sent["crc"][::-1].tolist()
    assert (dst.raw() == src.raw()).all()
    for i, ln in enumerate(SIZES):
        rc, got = dst.read_file(i + 1, ln + 36)
        assert rc == 0 and got[36:] == synth_bytes(900 + i, ln).tobytes() and got == src.read_file(i + 1, ln + 36)[1]
    nbad, st = ds.verify_block(gpu_ctx, dst)
    assert nbad == 0 and not st.any()
    for b in (src, dst):
        b.free()
    chk.free()


def test_rotten_source_record_is_not_committed(gpu_ctx, ds, oracle):
    src = _block(ds, oracle, SIZES)
    m, _ = src.metas()
    assert src.corrupt(int(m[2]["offset"]) + 36 + 11111, 0x10) == 0
    sent = ds.replicate_block(gpu_ctx, src, dest_block_id=78, frame_len=4096)      # sent under valid frame CRCs
    assert sent["rc"] == CRC_ERR and len(sent["frames"]) == -(-src.raw().size // 4096)
    dst = ds.LogicBlock(78)
    chk = ds.BlockCrcChecker(4)
    r = ds.receive_block(gpu_ctx, dst, sent["frames"], m, checker=chk)
    assert r["rc"] == CRC_ERR and r["commits"] == 0 and not r["parts"]["status"].any()
    assert r["status"].tolist() == [0, 0, CRC_ERR, 0, 0, 0] and chk.errors(78) == 1
    assert dst.raw().size == 0 and dst.read_file(1, 100)[0] != 0
    for b in (src, dst):
        b.free()
    chk.free()


def test_frame_damaged_in_flight_ends_the_receive(gpu_ctx, ds, oracle):
    src = _block(ds, oracle, SIZES)
    m, _ = src.metas()
    sent = ds.replicate_block(gpu_ctx, src, dest_block_id=79, frame_len=4096)
    frames = [f.copy() for f in sent["frames"]]
    frames[3][56 + 100] ^= 1
    dst = ds.LogicBlock(79)
    r = ds.receive_block(gpu_ctx, dst, frames, m, reads=[2, 3, len(frames) - 5])
    assert r["rc"] == CRC_ERR and r["commits"] == 0
    assert r["parts"]["status"].tolist() == [0, 0, 0, CRC_ERR]                # it ends at that frame
    assert dst.raw().size == 0
    frames = [f.copy() for f in sent["frames"]]
    frames[2][-4] = 1                                                          # flag_ on a frame at offset > 0
    struct.pack_into("<I", frames[2], 20, zlib.crc32(frames[2][24:].tobytes(), 0x4E534654 ^ 0xFFFFFFFF) ^ 0xFFFFFFFF)
    r = ds.receive_block(gpu_ctx, dst, frames, m)
    assert r["rc"] == PARAM and r["commits"] == 0 and len(r["parts"]) == 3 and not r["parts"]["status"].any()
    for b in (src, dst):
        b.free()


def test_parity_member_lands_and_commits(gpu_ctx, ds, oracle):
    src = _block(ds, oracle, [7000, 9000])
    sent = ds.replicate_block(gpu_ctx, src, dest_block_id=80, frame_len=1024, new_block=2)
    dst = ds.LogicBlock(80)
    r = ds.receive_block(gpu_ctx, dst, sent["frames"], None)
    assert r["rc"] == 0 and r["commits"] == 1 and r["new_block"] == 2 and r["status"].size == 0
    assert (dst.raw() == src.raw()).all() and len(dst.metas()[0]) == 0
    # an empty member: one frame, nothing to land
    empty = _block(ds, oracle, [])
    sent = ds.replicate_block(gpu_ctx, empty, dest_block_id=80, frame_len=1024, new_block=2)
    r = ds.receive_block(gpu_ctx, dst, sent["frames"], None)
    assert r["rc"] == 0 and r["commits"] == 1 and r["total"] == 0 and dst.raw().size == 0
    for b in (src, dst, empty):
        b.free()
