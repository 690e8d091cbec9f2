"""classify_scrub (tfs_amd/ds/ds_harness.cpp) through
tfs_ds_scrub_classify: the verdict over a hand-made tile map and hand-made
statuses.  No GPU.  A unit is 1 KiB; bit u of tile_map[p][T] is unit 4 T + u of
parity member p."""
import numpy as np
import pytest

OK, CRC_ERR, PARAM, INFO_ERR, SIZE_ERR, SYNC_ERR = 0, -1010, -1016, -8016, -8034, -8038


def tmap(pn, total, flagged):
    """flagged: {parity member: [units]}"""
    m = np.zeros((pn, (total + 4095) // 4096), np.uint8)
    for p, units in flagged.items():
        for u in units:
            m[p, u // 4] |= 1 << (u % 4)
    return m


def classify(dn, pn, total, indexes, status, flagged):
    import tfs_amd.dataserver as ds
    from tfs_amd.crc import META_DTYPE
    idx = [np.array(m, META_DTYPE) for m in indexes]
    return ds.scrub_classify(dn, pn, total, idx, status, tmap(pn, total, flagged))


def test_five_three():
    total = 40 * 1024
    # member 0: records over units 0-4 and 10-11; member 2: one over 10-19; member 4: one over 30-31; gaps elsewhere
    indexes = [[(1, 100, 5000), (2, 10 * 1024 + 5, 2000)], [], [(3, 10 * 1024, 10 * 1024)], [], [(4, 30 * 1024 + 1000, 1100)]]
    status = [OK, CRC_ERR, INFO_ERR, SYNC_ERR]
    flagged = {0: [2, 7, 10, 25, 30, 36], 1: [7, 10, 25, 30], 2: [10, 25, 30, 38]}
    rc, r = classify(5, 3, total, indexes, status, flagged)
    # unit 2: parity 0 alone; 7: two of three; 10: all, over failed records of members 0 and 2; 25: all, over a gap;
    # 30: all, over member 4's failed record; 36 and 38: one each
    assert r["parity_only_units"].tolist() == [3, 1, 1]
    assert r["data_units"].tolist() == [1, 0, 1, 0, 1]
    assert r["unattributed_units"] == 1
    assert r["suspect"].tolist() == [1, 0, 1, 0, 1, 1, 1, 1]
    assert rc == 3 + 7                                     # three records, seven flagged units


def test_all_flagged_over_a_record_that_passed_is_unattributed():
    """Only a failed record attributes; member 0's first record passed, so unit 2 has no name."""
    indexes = [[(1, 100, 5000)], [], [], [], []]
    rc, r = classify(5, 3, 8192, indexes, [OK], {0: [2], 1: [2], 2: [2]})
    assert r["unattributed_units"] == 1 and r["data_units"].sum() == 0 and r["suspect"].sum() == 0 and rc == 1


def test_failed_record_without_flagged_units_is_suspect():
    """A wrong FileInfo.crc_ field fails the record and changes the parity too, but a record can also fail with the
    map clean (an index that disagrees with an intact block): the member is suspect all the same."""
    rc, r = classify(2, 1, 8192, [[(1, 0, 3000)], [(2, 0, 100)]], [OK, INFO_ERR], {})
    assert r["suspect"].tolist() == [0, 1, 0] and r["data_units"].sum() == 0 and rc == 1


def test_records_rejected_at_begin_do_not_attribute():
    rc, r = classify(2, 1, 8192, [[(1, -5, 3000), (2, 4096, 20)], []], [PARAM, SIZE_ERR], {0: [0, 4]})
    assert r["unattributed_units"] == 2 and r["data_units"].sum() == 0 and r["suspect"].sum() == 0 and rc == 4


def test_two_one():
    """pn == 1: every flagged unit is 'all of them' -- with a failed record over it the member is named, without
    one it stays unattributed (a gap, a deleted record, or the parity itself)."""
    total = 12 * 1024
    indexes = [[(1, 0, 2048)], [(2, 5 * 1024 + 1023, 2)]]   # the second meets units 5 and 6 with one byte each
    rc, r = classify(2, 1, total, indexes, [CRC_ERR, CRC_ERR], {0: [0, 1, 2, 5, 6, 7, 11]})
    assert r["data_units"].tolist() == [2, 2]
    assert r["unattributed_units"] == 3                      # 2, 7, 11
    assert r["parity_only_units"].tolist() == [0]
    assert r["suspect"].tolist() == [1, 1, 0]
    assert rc == 2 + 7
    rc, r = classify(2, 1, total, indexes, [OK, OK], {0: [3]})
    assert r["unattributed_units"] == 1 and r["suspect"].sum() == 0 and rc == 1


@pytest.mark.parametrize("units", [1, 2, 3])
def test_last_unit_of_a_short_tile(units):
    """total is no multiple of 4,096: the last tile has `units` units, and the last one counts."""
    total = 8192 + 1024 * units
    last = 8 + units - 1
    rc, r = classify(5, 3, total, [[], [], [], [], [(9, total - 500, 500)]], [CRC_ERR],
                     {0: [last], 1: [last], 2: [last, last - 1]})
    assert r["data_units"].tolist() == [0, 0, 0, 0, 1]
    assert r["parity_only_units"].tolist() == [0, 0, 1]
    assert r["unattributed_units"] == 0 and rc == 1 + 2
    rc, r = classify(2, 1, total, [[], []], [], {0: [last]})
    assert r["unattributed_units"] == 1 and rc == 1


def test_call_level():
    import tfs_amd.dataserver as ds
    L = ds.lib()
    assert L.tfs_ds_scrub_classify(0, 1, 1024, None, None, None, None, None, None, None, None) == -1016
    assert L.tfs_ds_scrub_classify(2, 1, 1000, None, None, None, None, None, None, None, None) == -1016
    rc, r = classify(2, 1, 4096, [[], []], [], {})
    assert rc == 0 and r["suspect"].sum() == 0
