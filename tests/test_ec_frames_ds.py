"""The erasure-code tasks with their posts, through the dataserver harness (tfs_amd/ds/
ec_frames.h, tfs_amd/dataserver.py do_marshalling_frames / do_reinstate_frames): a round
trip.  A family of real LogicBlock images is marshalled into parity frames, which a
receive session (include/tfs_receive.h) lands as the parity blocks; members are then
killed, and the reinstate frames, fed to receive sessions on the servers that take the
rebuilt blocks, land the originals -- with the receive session's finish verifying every
record against the lost block's index."""
import numpy as np
import pytest

import ec_frames_expect as X
from test_reinstate_ds import FILL, IDS, K, M, marshalled, zero_extended  # noqa: F401  (marshalled: the fixture)

pytestmark = pytest.mark.gpu

PIDS = [(i + 1) << 32 for i in range(K + M)]


def land(ctx, frames, member, block_id, cap, metas=None):
    """The frames of `member`, in order, through a receive session: (image, crc, status, n_bad, total)."""
    import tfs_amd.crc as crc
    mine = [f for i, _, f in frames if i == member]
    assert [k for i, k, _ in frames if i == member] == list(range(len(mine)))
    base = np.concatenate(mine)
    descs = np.zeros(len(mine), crc.RECEIVE_DESC_DTYPE)
    o = 0
    for j, f in enumerate(mine):
        rc, d = crc.receive_parse(base[o:o + f.size], frame_off=o)
        assert rc == 0
        descs[j] = d[0]
        o += f.size
    d_img = crc.DeviceBuffer(ctx, cap + 64).upload(np.full(cap + 64, FILL, np.uint8))
    with crc.ReceiveSession(ctx, crc.receive_cfg(cap, block_id), d_img) as s:
        parts, nbad = s.frames(base, descs)
        assert nbad == 0 and (parts["status"] == 0).all()
        c, st, rbad, total = s.finish(metas)
    img = d_img.download(np.uint8, cap)
    d_img.free()
    return img, c, st, rbad, total


def test_marshalling_frames_land_the_parity(gpu_ctx, oracle, marshalled):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    fam = ds.Family(K, M, IDS, raws + [None] * M)
    rc, st, tot, frames = ds.do_marshalling_frames(gpu_ctx, fam, idx, frame_len=8192, chunk_len=16384, packet_ids=PIDS)
    assert rc == 0 and tot == total and all((s == 0).all() for s in st) and [len(s) for s in st] == [len(m) for m in idx]
    per = (total + 8191) // 8192
    assert len(frames) == M * per and {i for i, _, _ in frames} == set(range(K, K + M))
    for p in range(M):
        want = X.member_frames(oracle, parity[p], 8192, IDS[K + p], PIDS[K + p], True)
        got = [f.tobytes() for i, _, f in frames if i == K + p]
        assert got == want
        img, _, _, _, landed = land(gpu_ctx, frames, K + p, IDS[K + p], total)
        assert landed == total and (img == parity[p]).all()
    # call-level refusals of the harness
    assert ds.do_marshalling_frames(gpu_ctx, fam, idx, frame_len=1024)[0] == -1016
    assert ds.do_marshalling_frames(gpu_ctx, fam, idx, frame_len=8192, chunk_len=12288)[0] == -1016


def test_reinstate_frames_land_the_lost_blocks(gpu_ctx, oracle, marshalled):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    dead = {0, 2, K + 1}
    members = [None if i in dead else a for i, a in enumerate(raws + parity)]
    rc, st, tot, frames = ds.do_reinstate_frames(gpu_ctx, ds.Family(K, M, IDS, members), idx, frame_len=4096,
                                                 chunk_len=16384, packet_ids=PIDS)
    assert rc == 0 and tot == total and all((s == 0).all() for s in st)
    assert {i for i, _, _ in frames} == dead
    for i in sorted(dead):
        orig = zero_extended(raws[i], total) if i < K else parity[i - K]
        want = X.member_frames(oracle, orig, 4096, IDS[i], PIDS[i], i >= K)
        assert [f.tobytes() for m, _, f in frames if m == i] == want
        img, c, rst, rbad, landed = land(gpu_ctx, frames, i, IDS[i], total, idx[i] if i < K else None)
        assert landed == total and (img == orig).all()
        if i < K:  # the receive session verified every record of the lost block against its index
            assert rbad == 0 and len(rst) == len(idx[i]) and (rst == 0).all()
    # nothing lost: nothing done
    rc, st, tot, frames = ds.do_reinstate_frames(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, frame_len=4096)
    assert rc == 0 and tot == 0 and frames == [] and all(len(s) == 0 for s in st)


def test_reinstate_frames_count_what_a_corrupt_survivor_hurts(gpu_ctx, marshalled):
    """The same verdicts as do_reinstate over the same members; the frames are still sealed and land."""
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    dead = {0, 2, K + 1}
    hurt = raws[1].copy()
    hurt[int(idx[1][0]["offset"]) + 36 + 20000] ^= 0x08
    members = [None if i in dead else hurt if i == 1 else a for i, a in enumerate(raws + parity)]
    rebuilt = [np.full(total, FILL, np.uint8) if i in dead else None for i in range(K + M)]
    rc0, st0, _ = ds.do_reinstate(gpu_ctx, ds.Family(K, M, IDS, members), idx, rebuilt, chunk_len=16384)
    rc, st, tot, frames = ds.do_reinstate_frames(gpu_ctx, ds.Family(K, M, IDS, members), idx, frame_len=4096,
                                                 chunk_len=16384, packet_ids=PIDS)
    assert rc == rc0 and rc >= 1 and (np.concatenate(st) == np.concatenate(st0)).all()
    for i in sorted(dead):
        img, _, _, _, landed = land(gpu_ctx, frames, i, IDS[i], total)
        assert landed == total and (img == rebuilt[i]).all()
