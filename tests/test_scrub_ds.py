"""scrub_family through the dataserver harness (tfs_amd/dataserver.py scrub_family over
tfs_ec_scrub_*): a family of real LogicBlock images is marshalled, then scrubbed in small
chunks -- clean, with a rotten payload byte, with a rotten parity byte, and with a rotten
byte in the range of a deleted record, which no index entry covers."""
import numpy as np
import pytest

from test_marshal_ds import FI, K, M, build_blocks, sorted_index

pytestmark = pytest.mark.gpu

CRC_ERR = -1010
IDS = [300, 301, 302, 400, 401]


def marshalled(gpu_ctx, oracle, blocks, idx):
    """(raws, parity): the family as do_marshalling leaves it."""
    import tfs_amd.dataserver as ds
    raws = [b.raw() for b in blocks]
    total = (max(r.size for r in raws) + 1023) // 1024 * 1024
    parity = [np.full(total, 0xA5, np.uint8) for _ in range(M)]
    rc, _, tot = ds.do_marshalling(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=1 << 20)
    assert rc == 0 and tot == total
    return raws, parity, total


@pytest.fixture(scope="module")
def fam(gpu_ctx, oracle):
    blocks = build_blocks(oracle)
    idx = [sorted_index(b) for b in blocks]
    raws, parity, total = marshalled(gpu_ctx, oracle, blocks, idx)
    return blocks, idx, raws, parity, total


def clean(r):
    return not r["data_units"].any() and not r["parity_only_units"].any() and r["unattributed_units"] == 0 and \
        not r["suspect"].any()


@pytest.mark.parametrize("chunk", [4096, 8192, 1 << 20])
def test_scrub_family_clean(gpu_ctx, fam, chunk):
    import tfs_amd.dataserver as ds
    _, idx, raws, parity, total = fam
    before = [a.copy() for a in raws + parity]
    rc, r, tot = ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=chunk)
    assert rc == 0 and tot == total and clean(r)
    assert [len(s) for s in r["status"]] == [len(m) for m in idx] and all((s == 0).all() for s in r["status"])
    assert all((a == b).all() for a, b in zip(before, raws + parity))


def test_scrub_family_names_the_data_member(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    _, idx, raws, parity, _ = fam
    victim = 2                                                  # the 70,000-byte file of member 0
    hurt = raws[0].copy()
    hurt[int(idx[0][victim]["offset"]) + FI + 33333] ^= 0x20
    rc, r, _ = ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, [hurt] + raws[1:] + parity), idx, chunk_len=8192)
    assert rc == 1 + 1                                          # one record, one unit
    assert r["status"][0][victim] == CRC_ERR and sum(int((s != 0).sum()) for s in r["status"]) == 1
    assert r["data_units"].tolist() == [1, 0, 0] and not r["parity_only_units"].any() and r["unattributed_units"] == 0
    assert r["suspect"].tolist() == [1, 0, 0, 0, 0]


def test_scrub_family_names_the_parity_member(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    _, idx, raws, parity, total = fam
    hurt = parity[1].copy()
    hurt[total - 5] ^= 1
    rc, r, _ = ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, raws + [parity[0], hurt]), idx, chunk_len=8192)
    assert rc == 1 and all((s == 0).all() for s in r["status"])
    assert r["parity_only_units"].tolist() == [0, 1] and not r["data_units"].any() and r["unattributed_units"] == 0
    assert r["suspect"].tolist() == [0, 0, 0, 0, 1]


def test_scrub_family_deleted_record_is_unattributed(gpu_ctx, fam):
    """A deleted file stays in the block until compaction and is part of the code, but no index entry names it."""
    import tfs_amd.dataserver as ds
    _, idx, raws, parity, _ = fam
    gone = 2                                                    # the 4,096-byte file of member 1
    live = [idx[0], np.delete(idx[1], gone), idx[2]]
    rc, r, _ = ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), live, chunk_len=4096)
    assert rc == 0 and clean(r)
    hurt = raws[1].copy()
    assert int(idx[1][gone]["size"]) == FI + 4096
    hurt[int(idx[1][gone]["offset"]) + FI + 2] ^= 0x10
    rc, r, _ = ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, [raws[0], hurt, raws[2]] + parity), live, chunk_len=4096)
    assert rc == 1 and all((s == 0).all() for s in r["status"])
    assert r["unattributed_units"] == 1 and not r["data_units"].any() and not r["parity_only_units"].any()
    assert not r["suspect"].any()


def test_scrub_family_call_level(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    _, idx, raws, parity, total = fam
    assert ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=1024)[0] == -1016
    assert ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, raws + [parity[0], None]), idx, chunk_len=8192)[0] == -1016
    assert ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, raws + [parity[0], parity[1][:total - 1024]]), idx,
                           chunk_len=8192)[0] == -1016
