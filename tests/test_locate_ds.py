"""scrub_locate_family through the dataserver harness (tfs_amd/dataserver.py over scrub_and_locate and
tfs_ec_locate): a 5:3 family of block images is marshalled, then hurt where a scrub alone names
nobody -- a gap byte, a byte of a deleted record -- and where it does, plus a stale parity unit.
The expected member is the one the test hurt and the expected bytes are the ones it had before;
the scrub half is compared with what scrub_family reports for the same family."""
import numpy as np
import pytest

from conftest import ocrc
from test_marshal_ds import FI, build_blocks, sorted_index
from test_scrub import gapped_member
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

CRC_ERR = -1010
K, M = 5, 3
IDS = [300, 310, 301, 302, 304, 400, 401, 402]


def marshal(gpu_ctx, k, m, ids, raws, idx):
    import tfs_amd.dataserver as ds
    total = (max(r.size for r in raws) + 1023) // 1024 * 1024
    parity = [np.full(total, 0xA5, np.uint8) for _ in range(m)]
    rc, _, tot = ds.do_marshalling(gpu_ctx, ds.Family(k, m, ids, raws + parity), idx, chunk_len=1 << 20)
    assert rc == 0 and tot == total
    return parity, total


@pytest.fixture(scope="module")
def fam(gpu_ctx, oracle):
    """Members 0, 2, 3: tests/test_marshal_ds.py's blocks; member 1: an image with a 300-byte gap between two records
    (tests/test_scrub.py); member 4: one more block.  (raws, idx, parity, total, an offset inside member 1's gap)."""
    from tfs_amd.dataserver import LogicBlock
    blocks = build_blocks(oracle)
    extra = LogicBlock(304)
    for fid, n in enumerate((8000, 1, 33000, 600), 1):
        p = synth_bytes(9100 + fid, n).tobytes()
        assert extra.append(fid, p, ocrc(oracle, 0, p)) == 0
    gimg, gmt, g = gapped_member(oracle, 640)
    raws = [blocks[0].raw(), gimg, blocks[1].raw(), blocks[2].raw(), extra.raw()]
    idx = [sorted_index(blocks[0]), gmt, sorted_index(blocks[1]), sorted_index(blocks[2]), sorted_index(extra)]
    parity, total = marshal(gpu_ctx, K, M, IDS, raws, idx)
    return raws, idx, parity, total, g


def same_scrub(a, b):
    return all((x == y).all() for x, y in zip(a["status"], b["status"])) and \
        (a["data_units"] == b["data_units"]).all() and (a["parity_only_units"] == b["parity_only_units"]).all() and \
        a["unattributed_units"] == b["unattributed_units"] and (a["suspect"] == b["suspect"]).all()


def test_clean_family_examines_nothing(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total, _ = fam
    rc, s, l = ds.scrub_locate_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=8192)
    assert rc == 0 and s["findings"] == 0 and s["total"] == total
    assert l["examined_units"] == 0 and l["unlocated_units"] == 0 and not l["located_units"].any() and len(l["unit"]) == 0


def test_locates_what_the_scrub_cannot_name(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total, g = fam
    gone = 20                                                   # a 777-byte file of member 3, deleted from its index
    live = idx[:3] + [np.delete(idx[3], gone)] + idx[4:]
    victim = 2                                                  # the 70,000-byte file of member 0
    at = {1: g, 3: int(idx[3][gone]["offset"]) + FI + 2, 0: int(idx[0][victim]["offset"]) + FI + 33333}
    stale = 40
    assert len({x // 1024 for x in at.values()} | {stale}) == 4
    hurt = [a.copy() for a in raws]
    for m, x in at.items():
        hurt[m][x] ^= 0x10
    hpar = [a.copy() for a in parity]
    hpar[2][1024 * stale:1024 * stale + 1024] = synth_bytes(77, 1024)
    family = ds.Family(K, M, IDS, hurt + hpar)
    before = [a.copy() for a in hurt + hpar]
    rc0, s0, tot0 = ds.scrub_family(gpu_ctx, family, live, chunk_len=8192)
    rc, s, l = ds.scrub_locate_family(gpu_ctx, family, live, chunk_len=8192)
    assert rc == 0 and s["findings"] == rc0 == 1 + 4 and s["total"] == tot0 == total and same_scrub(s, s0)
    assert s["unattributed_units"] == 2 and s["data_units"].tolist() == [1, 0, 0, 0, 0]
    assert s["parity_only_units"].tolist() == [0, 0, 1] and s["status"][0][victim] == CRC_ERR
    assert l["located_units"].tolist() == [1, 1, 0, 1, 0] and l["unlocated_units"] == 0 and l["examined_units"] == 3
    assert l["member"].tolist() == [0, 1, 3] and l["unit"].tolist() == [at[m] // 1024 for m in (0, 1, 3)]
    assert l["confirmed"].all() and l["diff_bytes"].tolist() == [1, 1, 1] and l["bytes"].shape == (3, 1024)
    assert all((a == b).all() for a, b in zip(before, hurt + hpar))         # the harness writes nothing
    # the patches, applied up to each member's own length, give the members back
    fixed = [a.copy() for a in hurt]
    for m, u, b in zip(l["member"], l["unit"], l["bytes"]):
        n = min(1024, fixed[m].size - 1024 * int(u))
        fixed[m][1024 * int(u):1024 * int(u) + n] = b[:n]
        assert not b[n:].any()
    assert all((a == b).all() for a, b in zip(fixed, raws))
    rc2, s2, _ = ds.scrub_family(gpu_ctx, ds.Family(K, M, IDS, fixed + hpar), live, chunk_len=8192)
    assert rc2 == 1 and s2["parity_only_units"].tolist() == [0, 0, 1] and s2["unattributed_units"] == 0
    assert not s2["data_units"].any() and all((x == 0).all() for x in s2["status"])


def test_one_parity_member_locates_nothing(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    raws, idx, _, _, g = fam
    ids = [300, 310, 400]
    parity, total = marshal(gpu_ctx, 2, 1, ids, raws[:2], idx[:2])
    hurt = raws[1].copy()
    hurt[g] ^= 1
    rc, s, l = ds.scrub_locate_family(gpu_ctx, ds.Family(2, 1, ids, [raws[0], hurt] + parity), idx[:2], chunk_len=8192)
    assert rc == 0 and s["findings"] == 1 and s["unattributed_units"] == 1
    assert l["examined_units"] == 0 and l["unlocated_units"] == 0 and l["located_units"].tolist() == [0, 0]
    assert len(l["member"]) == 0 and l["bytes"].shape == (0, 1024)


def test_two_members_in_one_unit_stay_unlocated(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    raws, idx, parity, _, g = fam
    hurt = [a.copy() for a in raws]
    hurt[1][g] ^= 4
    hurt[4][1024 * (g // 1024) + 9] ^= 4                         # the same unit of another member
    hurt[2][5000] ^= 1                                           # and one unit that can be located
    rc, s, l = ds.scrub_locate_family(gpu_ctx, ds.Family(K, M, IDS, hurt + parity), idx, chunk_len=1 << 20)
    assert rc == 1 and l["unlocated_units"] == 1 and l["examined_units"] == 2
    assert l["located_units"].tolist() == [0, 0, 1, 0, 0] and l["member"].tolist() == [2] and l["unit"].tolist() == [4]
    assert (l["bytes"][0] == raws[2][4096:5120]).all() and g // 1024 != 4


def test_call_level(gpu_ctx, fam):
    import tfs_amd.dataserver as ds
    raws, idx, parity, total, _ = fam
    assert ds.scrub_locate_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=1024)[0] == -1016
    assert ds.scrub_locate_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity[:2] + [None]), idx, chunk_len=8192)[0] == -1016
