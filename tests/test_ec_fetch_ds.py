"""The erasure-code tasks with their fetches and posts, through the dataserver harness
(tfs_amd/ds/ec_fetch.h, tfs_amd/dataserver.py do_marshalling_task / do_reinstate_task): a
round trip.  A family of real LogicBlock images is marshalled from fetched
RespReadRawDataMessage frames into parity frames, which a receive session lands as the
parity blocks; members are then killed, and the reinstate task, fed the survivors' frames,
makes frames that land the originals.  A fetch that answers with an error, an error reply
and a frame damaged in flight each end the task with their status before anything of that
chunk reaches the sink."""
import numpy as np
import pytest

import ec_fetch_expect as F
import ec_frames_expect as X
from test_ec_frames_ds import PIDS, land
from test_reinstate_ds import IDS, K, M, marshalled, zero_extended  # noqa: F401  (marshalled: the fixture)

pytestmark = pytest.mark.gpu


def fetcher(oracle, members, log=None, hook=None):
    """read_raw_data's stand-in over `members` (bytes per member index): the sealed frame of what the member has."""
    def fetch(member, k, offset, length):
        if log is not None:
            log.append((member, k, offset, length))
        a = members[member]
        f, _ = F.in_frame(oracle, a[offset:offset + length].tobytes(), a.size, 2, (member << 32) + k)
        return hook(member, k, f) if hook else f
    return fetch


def test_marshalling_task_then_reinstate_task(gpu_ctx, oracle, marshalled):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    fam = ds.Family(K, M, IDS, raws + [None] * M)
    log = []
    rc, st, tot, frames = ds.do_marshalling_task(gpu_ctx, fam, idx, fetcher(oracle, raws, log), frame_len=8192,
                                                 chunk_len=16384, packet_ids=PIDS)
    assert rc == 0 and tot == total and all((s == 0).all() for s in st) and [len(s) for s in st] == [len(m) for m in idx]
    # one fetch per (data member, frame) that has bytes, none past a member's end
    assert sorted(log) == sorted((i, o // 8192, o, min(8192, total - o)) for i in range(K)
                                 for o in range(0, total, 8192) if o < raws[i].size)
    for p in range(M):
        want = X.member_frames(oracle, parity[p], 8192, IDS[K + p], PIDS[K + p], True)
        assert [f.tobytes() for i, _, f in frames if i == K + p] == want
        img, _, _, _, landed = land(gpu_ctx, frames, K + p, IDS[K + p], total)
        assert landed == total and (img == parity[p]).all()
    # members are lost; the survivors' frames rebuild them
    dead = {0, 2, K + 1}
    everyone = raws + parity
    members = [None if i in dead else a for i, a in enumerate(everyone)]
    rc, st, tot, frames = ds.do_reinstate_task(gpu_ctx, ds.Family(K, M, IDS, members), idx, fetcher(oracle, everyone),
                                               frame_len=4096, chunk_len=16384, packet_ids=PIDS)
    assert rc == 0 and tot == total and all((s == 0).all() for s in st) and {i for i, _, _ in frames} == dead
    for i in sorted(dead):
        orig = zero_extended(raws[i], total) if i < K else parity[i - K]
        assert [f.tobytes() for m, _, f in frames if m == i] == X.member_frames(oracle, orig, 4096, IDS[i], PIDS[i], i >= K)
        img, c, rst, rbad, landed = land(gpu_ctx, frames, i, IDS[i], total, idx[i] if i < K else None)
        assert landed == total and (img == orig).all()
        if i < K:
            assert rbad == 0 and len(rst) == len(idx[i]) and (rst == 0).all()
    # nothing lost: nothing fetched, nothing done
    log = []
    rc, st, tot, frames = ds.do_reinstate_task(gpu_ctx, ds.Family(K, M, IDS, everyone), idx, fetcher(oracle, everyone, log),
                                               frame_len=4096)
    assert rc == 0 and tot == 0 and frames == [] and log == []


def test_a_failed_fetch_or_frame_ends_the_task_before_the_chunk_is_posted(gpu_ctx, oracle, marshalled):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    fam = ds.Family(K, M, IDS, raws + [None] * M)
    per_chunk = M * 2  # frames posted per chunk of two frames

    def run(hook):
        return ds.do_marshalling_task(gpu_ctx, fam, idx, fetcher(oracle, raws, hook=hook), frame_len=8192, chunk_len=16384,
                                      packet_ids=PIDS)

    # the fetch itself fails on frame 3 (the second chunk): the first chunk was posted, nothing of the second
    rc, _, _, frames = run(lambda m, k, f: -8013 if (m, k) == (1, 3) else f)
    assert rc == -8013 and len(frames) == per_chunk and {k for _, k, _ in frames} == {0, 1}
    # the source's error reply: set_length(status) in the body
    def error_reply(m, k, f):
        if (m, k) != (0, 2):
            return f
        b = bytearray(f[:32])
        b[4:8] = (8).to_bytes(4, "little")
        b[24:28] = (-8016).to_bytes(4, "little", signed=True)
        return bytes(b)
    rc, _, _, frames = run(error_reply)
    assert rc == -8016 and len(frames) == per_chunk
    # a frame damaged in flight, in the data and in the header: the check's status, before the sink sees the chunk
    def flip(at, member=2, frame=1):
        def hook(m, k, f):
            if (m, k) != (member, frame):
                return f
            b = bytearray(f)
            b[at] ^= 0x20
            return bytes(b)
        return hook
    rc, _, _, frames = run(flip(28 + 4000))
    assert rc == -1010 and frames == []
    rc, _, _, frames = run(flip(9, frame=2))
    assert rc == -1 and len(frames) == per_chunk
    # half a frame
    rc, _, _, frames = run(lambda m, k, f: f[:-3] if (m, k) == (3, 0) else f)
    assert rc == -1 and frames == []
