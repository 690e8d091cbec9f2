"""ReinstateTask::do_reinstate through the dataserver harness (tfs_amd/dataserver.py
do_reinstate over tfs_ec_reinstate_*): a family of real LogicBlock images gets its
parity from do_marshalling, loses two data members and one parity member, and is
reinstated in small chunks; a survivor that went bad in between is counted as the
oracle's decode of its bytes says."""
import numpy as np
import pytest

from conftest import ocrc
from test_reinstate import ec_oracle, erased_of, expected, member_slices  # noqa: F401  (ec_oracle: the fixture)
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

FI = 36
K, M = 4, 3
IDS = [300, 301, 302, 303, 400, 401, 402]
NO_ENOUGH_DATA = -16004
FILL = 0x5A


def sorted_index(b):
    m = b.metas()[0]
    return m[np.argsort(m["offset"], kind="stable")]


@pytest.fixture(scope="module")
def marshalled(gpu_ctx, oracle):
    """(raws, indexes, parity, total): four blocks of different lengths and their parity."""
    import tfs_amd.dataserver as ds
    blocks = []
    for i, lens in enumerate([(30000, 5, 40000, 1000, 12345, 100, 2000), (50001, 4095, 4096, 9), (777,) * 40 + (20000,),
                              (9000, 8191, 33, 25000)]):
        b = ds.LogicBlock(300 + i)
        for fid, n in enumerate(lens, 1):
            p = synth_bytes(7000 * i + fid, n).tobytes()
            assert b.append(fid, p, ocrc(oracle, 0, p)) == 0
        blocks.append(b)
    raws = [b.raw().copy() for b in blocks]
    idx = [sorted_index(b) for b in blocks]
    total = (max(r.size for r in raws) + 1023) // 1024 * 1024
    assert len({r.size for r in raws}) == K and total < 128 << 10
    parity = [np.zeros(total, np.uint8) for _ in range(M)]
    rc, st, tot = ds.do_marshalling(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=16384)
    assert rc == 0 and tot == total
    return raws, idx, parity, total


def zero_extended(a, total):
    b = np.zeros(total, np.uint8)
    b[:a.size] = a
    return b


def test_do_reinstate_rebuilds_and_verifies(gpu_ctx, marshalled):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    dead = {0, 2, K + 1}
    members = [None if i in dead else a for i, a in enumerate(raws + parity)]
    rebuilt = [np.full(total, FILL, np.uint8) if i in dead else None for i in range(K + M)]
    rc, st, tot = ds.do_reinstate(gpu_ctx, ds.Family(K, M, IDS, members), idx, rebuilt, chunk_len=16384)
    assert rc == 0 and tot == total and [len(s) for s in st] == [len(m) for m in idx]
    assert all((s == 0).all() for s in st)
    for i in (0, 2):
        assert (rebuilt[i] == zero_extended(raws[i], total)).all(), i
    assert (rebuilt[K + 1] == parity[1]).all()
    # call-level: a chunk length that is no multiple of 4096, a rebuilt buffer that is missing or too short
    fam = ds.Family(K, M, IDS, members)
    assert ds.do_reinstate(gpu_ctx, fam, idx, rebuilt, chunk_len=1024)[0] == -1016
    assert ds.do_reinstate(gpu_ctx, fam, idx, [None] * (K + M), chunk_len=16384)[0] == -1016
    short = [None if a is None else a[:total - 1024] for a in rebuilt]
    assert ds.do_reinstate(gpu_ctx, fam, idx, short, chunk_len=16384)[0] == -1016


def test_do_reinstate_counts_what_a_corrupt_survivor_hurts(gpu_ctx, oracle, ec_oracle, marshalled):  # noqa: F811
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    dead = {0, 2, K + 1}
    erased = erased_of(K, M, dead)
    sl = member_slices(idx)
    fam = [zero_extended(a, total) for a in raws] + [p.copy() for p in parity]
    sizes = [raws[i].size if erased[i] == 0 else total for i in range(K)]
    want = None
    for j in range(8):  # a payload byte of survivor 1's first file; the oracle must show a record hurt in 0, 1 and 2
        at = int(idx[1][0]["offset"]) + FI + 20000 + 137 * j
        f2 = [a.copy() for a in fam]
        f2[1][at] ^= 0x08
        _, _, est = expected(oracle, ec_oracle, K, M, erased, f2, idx, sizes, total)
        if all((est[sl[i]] != 0).any() for i in (0, 1, 2)):
            want = est
            break
    assert want is not None and (want[sl[3]] == 0).all()
    hurt = raws[1].copy()
    hurt[at] ^= 0x08
    members = [None if i in dead else hurt if i == 1 else a for i, a in enumerate(raws + parity)]
    rebuilt = [np.full(total, FILL, np.uint8) if i in dead else None for i in range(K + M)]
    rc, st, _ = ds.do_reinstate(gpu_ctx, ds.Family(K, M, IDS, members), idx, rebuilt, chunk_len=16384)
    assert rc == int((want != 0).sum()) and rc >= 3
    assert (np.concatenate(st) == want).all()


def test_nothing_lost_and_too_much_lost(gpu_ctx, marshalled):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = marshalled
    rebuilt = [np.full(total, FILL, np.uint8) for _ in range(K + M)]
    rc, st, tot = ds.do_reinstate(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, rebuilt, chunk_len=16384)
    assert rc == 0 and tot == 0 and all(len(s) == 0 for s in st)   # EXIT_NO_NEED_REINSTATE: nothing done
    assert all((a == FILL).all() for a in rebuilt)
    members = [None, None, raws[2], None, parity[0], None, parity[2]]  # three of seven left, four needed
    rc, _, _ = ds.do_reinstate(gpu_ctx, ds.Family(K, M, IDS, members), idx, rebuilt, chunk_len=16384)
    assert rc == NO_ENOUGH_DATA
    assert all((a == FILL).all() for a in rebuilt)
