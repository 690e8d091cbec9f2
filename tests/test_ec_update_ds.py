"""unlink_file_family and write_member_range through the dataserver harness (tfs_amd/dataserver.py over
tfs_ec_update), on the 5:3 family of block images that tests/test_locate_ds.py marshals.

The reference's unlink rewrites the record's FileInfo in the data member (logic_block.cpp:649-656) and
leaves the parity bytes alone (unlink_file_parity, :539-577).  The first test pins what that does to a
family with the abilities the project had before; the others make the same change through the update
and find the family whole: a clean scrub, parity equal to jerasure's encode of the members as they now
are, and a reinstate of another member that rebuilds it byte for byte."""
import numpy as np
import pytest

from conftest import ocrc
from test_locate_ds import IDS, K, M, fam  # noqa: F401  (fam: the fixture, a marshalled 5:3 family)
from test_marshal_ds import FI
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode)
from test_scrub import encode
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

MTIME_AT = 20  # FileInfo::modify_time_ (include/tfs_crc.h)


def copies(fam):  # noqa: F811
    raws, idx, parity, total, _ = fam
    return [a.copy() for a in raws], idx, [p.copy() for p in parity], total


def zero_extended(a, total):
    b = np.zeros(total, np.uint8)
    b[:a.size] = a
    return b


def oracle_parity(ec_oracle, raws, total):  # noqa: F811
    return encode(ec_oracle, K, M, [zero_extended(a, total) for a in raws], total)


def record_in_one_unit(idx, member):
    """A record of `member` whose FileInfo lies inside one unit."""
    for x in idx[member]:
        if int(x["offset"]) // 1024 == (int(x["offset"]) + FI - 1) // 1024:
            return x
    raise AssertionError("no such record")


def straddling_record(idx):
    """(member, entry) of a record whose 36-byte FileInfo lies over a unit boundary."""
    for m in range(K):
        for x in idx[m]:
            if int(x["offset"]) // 1024 != (int(x["offset"]) + FI - 1) // 1024:
                return m, x
    raise AssertionError("no FileInfo of the family straddles a unit boundary")


def new_mtime(raw, off):
    """A modify_time_ that differs from the stored one in all four bytes."""
    old = int(np.frombuffer(raw[off + MTIME_AT:off + MTIME_AT + 4].tobytes(), "<i4")[0])
    return old ^ 0x01010101


def test_the_hazard_without_an_update(gpu_ctx, fam):  # noqa: F811
    """What the reference's unlink leaves behind, seen with scrub and locate alone: the FileInfo's unit is flagged in
    all three parity members, no record fails, and the locate step proposes to put the old FileInfo back."""
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = copies(fam)
    x = record_in_one_unit(idx, 1)
    off = int(x["offset"])
    before = raws[1].copy()
    raws[1][off + MTIME_AT:off + MTIME_AT + 4] = np.frombuffer(np.int32(new_mtime(before, off)).tobytes(), np.uint8)
    rc, s, l = ds.scrub_locate_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx, chunk_len=8192)
    assert rc == 0 and s["findings"] == 1 and s["unattributed_units"] == 1          # one unit, flagged in every parity member
    assert all((st == 0).all() for st in s["status"]) and not s["parity_only_units"].any()
    assert l["member"].tolist() == [1] and l["unit"].tolist() == [off // 1024] and l["diff_bytes"].tolist() == [4]
    u = off // 1024
    assert (l["bytes"][0][:min(1024, before.size - 1024 * u)] == before[1024 * u:1024 * u + 1024]).all()


@pytest.mark.parametrize("straddle", [False, True])
def test_unlink_file_family_keeps_the_family_whole(gpu_ctx, ec_oracle, fam, straddle):  # noqa: F811
    import tfs_amd.dataserver as ds
    raws, idx, parity, total = copies(fam)
    member, x = straddling_record(idx) if straddle else (1, record_in_one_unit(idx, 1))
    off = int(x["offset"])
    before = [a.copy() for a in raws]
    t = new_mtime(raws[member], off)
    family = ds.Family(K, M, IDS, raws + parity)
    assert ds.unlink_file_family(gpu_ctx, family, idx[member], IDS[member], int(x["file_id"]), t) == (2 if straddle else 1)
    # the data member: modify_time_ and nothing else
    want = before[member].copy()
    want[off + MTIME_AT:off + MTIME_AT + 4] = np.frombuffer(np.int32(t).tobytes(), np.uint8)
    assert (raws[member] == want).all() and all((raws[i] == before[i]).all() for i in range(K) if i != member)
    rc, s, tot = ds.scrub_family(gpu_ctx, family, idx, chunk_len=8192)
    assert rc == 0 and tot == total and all((st == 0).all() for st in s["status"])
    code = oracle_parity(ec_oracle, raws, total)
    assert all((p == c).all() for p, c in zip(parity, code))
    assert not all((p == q).all() for p, q in zip(parity, fam[2]))                 # and it did move
    # call-level: a block that is not in the family, a file that is not in the index
    assert ds.unlink_file_family(gpu_ctx, family, idx[member], 999, int(x["file_id"]), t) == -16008
    assert ds.unlink_file_family(gpu_ctx, family, idx[member], IDS[member], 987654321, t) == -8025


def test_a_rebuild_after_an_unlink(gpu_ctx, fam):  # noqa: F811
    """Member 3 and parity 0 are lost after an unlink in member 1.  With the update they are rebuilt byte for byte and
    every record verifies; after the same change made the reference's way, the rebuilt member 3 is wrong in that unit."""
    import tfs_amd.dataserver as ds
    x = record_in_one_unit(fam[1], 1)
    off, u = int(x["offset"]), int(x["offset"]) // 1024
    dead = {3, K}
    out = {}
    for updated in (True, False):
        raws, idx, parity, total = copies(fam)
        t = new_mtime(raws[1], off)
        if updated:
            assert ds.unlink_file_family(gpu_ctx, ds.Family(K, M, IDS, raws + parity), idx[1], IDS[1], int(x["file_id"]), t) == 1
        else:
            raws[1][off + MTIME_AT:off + MTIME_AT + 4] = np.frombuffer(np.int32(t).tobytes(), np.uint8)
        members = [None if i in dead else a for i, a in enumerate(raws + parity)]
        rebuilt = [np.full(total, 0xA5, np.uint8) if i in dead else None for i in range(K + M)]
        rc, st, tot = ds.do_reinstate(gpu_ctx, ds.Family(K, M, IDS, members), idx, rebuilt, chunk_len=8192)
        out[updated] = (rc, st, rebuilt, zero_extended(raws[3], total), parity[0])
        assert tot == total
    rc, st, rebuilt, m3, p0 = out[True]
    assert rc == 0 and all((s == 0).all() for s in st)
    assert (rebuilt[3] == m3).all() and (rebuilt[K] == p0).all()
    rc, st, rebuilt, m3, _ = out[False]
    diff = (rebuilt[3] != m3).reshape(-1, 1024).any(axis=1)
    assert diff[u] and int(diff.sum()) == 1                                       # a member nobody touched, wrong there


def test_write_member_range_over_a_whole_record(gpu_ctx, oracle, ec_oracle, fam):  # noqa: F811
    """A record rewritten in place -- new payload, and its FileInfo with the new CRC: the scrub is clean, the record
    verifies, and the parity is jerasure's encode of the members as they now are."""
    import tfs_amd.dataserver as ds
    from tfs_amd.crc import FILEINFO_DTYPE
    raws, idx, parity, total = copies(fam)
    member, victim = 0, 3                                                          # the 1,000-byte file of member 0
    x = idx[member][victim]
    off, size = int(x["offset"]), int(x["size"])
    assert size == 1000 + FI and off // 1024 != (off + size - 1) // 1024
    payload = synth_bytes(4242, size - FI).copy()
    fi = np.frombuffer(raws[member][off:off + FI].tobytes(), FILEINFO_DTYPE).copy()
    fi["crc_"] = ocrc(oracle, 0, payload.tobytes())
    fi["modify_time_"] = int(fi["modify_time_"][0]) + 1
    record = np.concatenate([np.frombuffer(fi.tobytes(), np.uint8), payload])
    family = ds.Family(K, M, IDS, raws + parity)
    n_units = (off + size - 1) // 1024 - off // 1024 + 1
    assert ds.write_member_range(gpu_ctx, family, member, off, record) == n_units
    assert (raws[member][off:off + size] == record).all()
    rc, s, _ = ds.scrub_family(gpu_ctx, family, idx, chunk_len=8192)
    assert rc == 0 and all((st == 0).all() for st in s["status"])
    assert all((p == c).all() for p, c in zip(parity, oracle_parity(ec_oracle, raws, total)))
    # call-level: a range past the member's end, a member that is no data member, no parity member held
    assert ds.write_member_range(gpu_ctx, family, member, raws[member].size - 10, record[:11]) == -1016
    assert ds.write_member_range(gpu_ctx, family, K, 0, record[:4]) == -1016
    held = ds.Family(K, M, IDS, raws + [None] * M)
    kept = raws[member].copy()
    assert ds.write_member_range(gpu_ctx, held, member, off, record[::-1].copy()) == -16001
    assert (raws[member] == kept).all()
