"""CPU tests of tests/ec_family.py, the seeded family generator behind tests/test_ec_lifecycle.py and the
geometry sweep of tests/test_ec.py: the committed seed list reaches every condition the GPU tests rely
on, the judges refuse one wrong bit, CRC, status, map bit, locate field or rebuilt byte and say where,
and oracle/ec_oracle.c agrees with the reference's own jerasure at every geometry with dn + pn <= 12
(tests/golden/ec_geometry_vectors.json, written by oracle/gen_golden_ec.py).
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import ec_family as F
from conftest import ROOT
from test_ec import ec_oracle, members, o_decode, o_encode  # noqa: F401  (ec_oracle: the fixture)
from test_scrub import encode


@pytest.fixture(scope="module")
def fams(oracle):
    return [F.make(oracle, s) for s in F.SEEDS]


def test_seed_list_coverage(fams):
    """Conditions over the list as a whole, not measurements; -s prints which seeds reach each."""
    assert 20 <= len(F.SEEDS) <= 28 and len(set(F.SEEDS)) == len(F.SEEDS)
    table = F.assert_seed_coverage(fams)
    for name, seeds in table.items():
        print("%-44s %s" % (name, " ".join(map(str, seeds))))
    print("geometries:", " ".join("%d:(%d,%d)" % (f.seed, f.dn, f.pn) for f in fams))
    with pytest.raises(AssertionError, match="reaches no family"):
        F.assert_seed_coverage([])
    with pytest.raises(AssertionError, match="reaches no family with: .*dn=11"):
        F.assert_seed_coverage([f for f in fams if f.dn != 11])
    with pytest.raises(AssertionError, match="two are needed|reaches no family"):   # one geometry with pn >= 5
        F.assert_seed_coverage([f for f in fams if f.pn < 5 or (f.dn, f.pn) == (5, 7)])


def test_families_are_what_the_issue_describes(oracle, fams):
    """Every family: the ranges of the generator, legal chunk sequences, at least dn alive, an unused member empty,
    at most one damage per unit, every damaged byte really changed and inside the place the generator names; the same
    seed gives the same family."""
    for f in fams:
        assert (f.dn, f.pn) in F.GEOMETRIES and 5 * 1024 <= f.total <= 64 * 1024 and f.total % 1024 == 0
        assert F.legal(f.chunks, f.total) and F.legal(f.chunks2, f.total) and f.chunks != f.chunks2
        assert f.erased.count(0) >= f.dn and 1 in f.erased and f.erased[f.dn:].count(-1) == 0
        for i in range(f.dn):
            mt = f.metas[i]
            assert f.sizes[i] <= f.total
            if f.erased[i] == -1:
                assert f.sizes[i] == 0 and not len(mt) and not f.data[i].any()
            if len(mt):
                assert 1 <= int((mt["size"] - F.FI).min()) and int((mt["size"] - F.FI).max()) <= 9000
                gaps = mt["offset"][1:] - (mt["offset"][:-1] + mt["size"][:-1])
                assert int(mt["offset"][0]) <= 300 and (gaps >= 0).all() and (gaps <= 300).all()
                assert int(mt["offset"][-1] + mt["size"][-1]) <= f.sizes[i]
        crc, st = F.records(oracle, f, f.data)
        assert (st == 0).all() and len(st) == sum(len(mt) for mt in f.metas) > 0
        assert len({d.unit for d in f.damages}) == len(f.damages) >= 3
        c = f.change
        assert len(set(c.units)) == len(c.units) and (f.new_data[c.member] != f.data[c.member]).any()
        changed = np.nonzero(f.new_data[c.member] != f.data[c.member])[0]
        assert set((changed // 1024).tolist()) <= set(c.units)
        for d in f.damages:
            assert d.kind in ("data1", "data2", "parity")
            for i, s, x in d.edits:
                assert x.all() and d.unit * 1024 <= s and s + len(x) <= d.unit * 1024 + 1024
            if d.kind == "parity":
                assert 0 < len(d.parity) < f.pn and [i - f.dn for i, _, _ in d.edits] == d.parity
            else:
                i, s, x = d.edits[0]
                assert any(a <= s and s + len(x) <= b for a, b in F._spans(f.metas[i], f.total, d.unit)[d.placement])
                assert len(d.edits) == (1 if d.kind == "data1" else 2) and 1 <= len(x) <= 1024
    again = F.make(oracle, F.SEEDS[5])
    f = fams[5]
    assert all((a == b).all() for a, b in zip(again.data, f.data)) and again.chunks == f.chunks and \
        again.erased == f.erased and [(d.unit, d.kind) for d in again.damages] == [(d.unit, d.kind) for d in f.damages]
    two = F.make(oracle, 5, geometry=(4, 3), units=9)
    assert (two.dn, two.pn, two.total) == (4, 3, 9216)


def test_every_seed_has_its_expectations(oracle, ec_oracle, fams):  # noqa: F811
    """The expectations of the GPU test exist for every seed without a GPU: the clean scrub is clean before and after
    the change, every damage shows in the map, and locate_wants's own conditions hold (a unit with data damage is
    flagged in every parity row, one with parity damage in exactly the damaged members')."""
    for f in fams:
        for data in (f.data, f.new_data):
            parity = encode(ec_oracle, f.dn, f.pn, data, f.total)
            assert not F.scrub(oracle, ec_oracle, f, data, parity)[3].any()
        hurt = F.apply_damages(f.new_data + parity, f.damages)
        crc, st, units, tmap = F.scrub(oracle, ec_oracle, f, hurt[:f.dn], hurt[f.dn:])
        listed = F.flagged(tmap)
        assert sorted(listed) == sorted(d.unit for d in f.damages), f.seed
        wants = F.locate_wants(f, f.new_data, listed, tmap)
        assert all(w["kind"] is not None or f.pn == 2 for w in wants)
        assert all(w["diff_bytes"] == int((hurt[w["member"]][w["unit"] * 1024:w["unit"] * 1024 + 1024] != w["fixed"]).sum())
                   for w in wants if w["kind"] == F.DATA)


def test_sweep_patterns():
    for dn, pn in F.GEOMETRIES:
        first, last, third = F.sweep_patterns(dn, pn)
        assert first.count(1) == pn and first[:min(dn, pn)] == [1] * min(dn, pn)
        assert last[dn:] == [1] * pn and not any(last[:dn])
        assert third.count(-1) == 1 and third.count(1) == pn - 1 and third.count(0) == dn


@pytest.fixture(scope="module")
def life(oracle, ec_oracle):  # noqa: F811
    """The oracle's own results of one family's life: seed 7, (9, 3), and seed 15, (9, 2), for the unasserted kind."""
    out = {}
    for seed in (7, 15):
        f = F.make(oracle, seed)
        parity = encode(ec_oracle, f.dn, f.pn, f.new_data, f.total)
        hurt = F.apply_damages(f.new_data + parity, f.damages)
        crc, st, units, tmap = F.scrub(oracle, ec_oracle, f, hurt[:f.dn], hurt[f.dn:])
        listed = F.flagged(tmap)
        wants = F.locate_wants(f, f.new_data, listed, tmap)
        res = np.zeros(len(listed), np.dtype([("kind", "i1"), ("member", "i1"), ("parity", "<u2"), ("diff_bytes", "<u2"),
                                              ("flags", "u1"), ("reserved", "u1")]))
        fixed = np.full((len(listed), 1024), F.FILL, np.uint8)
        for k, w in enumerate(wants):
            res[k] = (F.NONE if w["kind"] is None else w["kind"], w["member"], w["parity"], w["diff_bytes"], int(f.pn >= 3), 0)
            if w["fixed"] is not None:
                fixed[k] = w["fixed"]
        out[seed] = types_ns(f=f, parity=parity, hurt=hurt, crc=crc, st=st, units=units, tmap=tmap, listed=listed,
                             wants=wants, res=res, fixed=fixed)
    return out


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def test_the_judges_judge(life):
    """The oracle's own results pass; one change of each kind is refused with the place in the message."""
    x = life[7]
    f = x.f
    assert f.pn >= 3 and sorted(listed_kinds(x)) == ["data1", "data2", "parity"]
    names, nbad = F.flat(f), int((x.st != 0).sum())
    F.judge_bytes("parity", x.parity, [a.copy() for a in x.parity])
    F.judge_records("scrub", names, x.crc.copy(), x.st.copy(), nbad, x.crc, x.st)
    F.judge_map("scrub", x.units.copy(), x.tmap.copy(), x.units, x.tmap)
    F.judge_locate("locate", x.res.copy(), x.fixed.copy(), x.wants, f.pn)
    F.judge_bytes("reinstate", {2: f.data[2].copy(), 11: x.parity[2].copy()}, {2: f.data[2], 11: x.parity[2]})

    bad = [a.copy() for a in x.parity]
    bad[2][2 * 1024 + 77] ^= 0x10                                         # one parity bit
    with pytest.raises(AssertionError, match=r"parity: member 2 differs at byte 2125 \(unit 2\)"):
        F.judge_bytes("parity", bad, x.parity)
    crc = x.crc.copy()
    crc[4] ^= 1                                                            # one CRC
    with pytest.raises(AssertionError, match=r"scrub: crc of record 4 \(%d, " % names[4][0]):
        F.judge_records("scrub", names, crc, x.st, nbad, x.crc, x.st)
    st = x.st.copy()
    st[-1] = F.CRC_ERR if st[-1] == 0 else 0                               # one status
    with pytest.raises(AssertionError, match=r"scrub: status of record %d " % (len(st) - 1)):
        F.judge_records("scrub", names, x.crc, st, nbad, x.crc, x.st)
    with pytest.raises(AssertionError, match="n_bad is %d" % (nbad + 1)):
        F.judge_records("scrub", names, x.crc, x.st, nbad + 1, x.crc, x.st)
    tmap = x.tmap.copy()
    tmap[1, 3] ^= 4                                                        # one map bit
    with pytest.raises(AssertionError, match="scrub: map of parity 1 tile 3 is"):
        F.judge_map("scrub", x.units, tmap, x.units, x.tmap)
    units = x.units.copy()
    units[0] += 1
    with pytest.raises(AssertionError, match="scrub: parity units"):
        F.judge_map("scrub", units, x.tmap, x.units, x.tmap)
    k = next(k for k, w in enumerate(x.wants) if w["kind"] == F.DATA)
    for field in ("kind", "member", "diff_bytes", "parity", "flags", "reserved"):
        res = x.res.copy()                                                 # one locate field
        res[field][k] ^= 1
        with pytest.raises(AssertionError, match=r"locate: entry %d \(unit %d\): %s" % (k, x.listed[k], field.split("_")[0])):
            F.judge_locate("locate", res, x.fixed, x.wants, f.pn)
    fixed = x.fixed.copy()
    fixed[k, 1023] ^= 0x80                                                 # one rebuilt byte: a repaired unit's ...
    with pytest.raises(AssertionError, match=r"locate: entry %d \(unit %d\): repaired unit differs at byte 1023" % (k, x.listed[k])):
        F.judge_locate("locate", x.res, fixed, x.wants, f.pn)
    k2 = next(k for k, w in enumerate(x.wants) if w["kind"] != F.DATA)
    fixed = x.fixed.copy()
    fixed[k2, 0] = 0                                                       # ... a slot that is not to be written ...
    with pytest.raises(AssertionError, match=r"locate: entry %d \(unit %d\): repaired unit differs at byte 0" % (k2, x.listed[k2])):
        F.judge_locate("locate", x.res, fixed, x.wants, f.pn)
    got = {2: f.data[2].copy(), 11: x.parity[2].copy()}
    got[2][f.total - 1] ^= 1                                               # ... and a reinstated member's
    with pytest.raises(AssertionError, match=r"reinstate: member 2 differs at byte %d \(unit %d\)" % (f.total - 1, f.total // 1024 - 1)):
        F.judge_bytes("reinstate", got, {2: f.data[2], 11: x.parity[2]})
    with pytest.raises(AssertionError, match="reinstate: members"):
        F.judge_bytes("reinstate", {2: f.data[2]}, {2: f.data[2], 11: x.parity[2]})


def listed_kinds(x):
    by_unit = {d.unit: d.kind for d in x.f.damages}
    return {by_unit[u] for u in x.listed}


def test_two_parity_members_leave_the_kind_open(life):
    """pn == 2: two data members wrong in one unit may look like a third; any kind passes there, CONFIRMED does not."""
    x = life[15]
    assert x.f.pn == 2
    k = next(k for k, w in enumerate(x.wants) if w["kind"] is None)
    for kind in (F.DATA, F.NONE):
        res = x.res.copy()
        res["kind"][k] = kind
        F.judge_locate("locate", res, x.fixed, x.wants, 2)
    res = x.res.copy()
    res["flags"][k] = 1
    with pytest.raises(AssertionError, match=r"locate: entry %d \(unit %d\): flags" % (k, x.listed[k])):
        F.judge_locate("locate", res, x.fixed, x.wants, 2)


def sha(arrays):
    return hashlib.sha256(b"".join(a.tobytes() for a in arrays)).hexdigest()


def test_oracle_matches_reference_at_every_geometry(ec_oracle):  # noqa: F811
    with open(os.path.join(ROOT, "tests", "golden", "ec_geometry_vectors.json")) as fh:
        g = json.load(fh)
    size, cases = g["size"], g["cases"]
    assert size == 5 * 1024 and sorted((c["dn"], c["pn"]) for c in cases) == sorted(F.GEOMETRIES)
    assert os.path.getsize(fh.name) <= 59267
    seen = set()
    for c in cases:
        dn, pn = c["dn"], c["pn"]
        ms = members(dn, pn, size, g["seed"] + 100 * dn + pn)
        assert o_encode(ec_oracle, dn, pn, ms, size) == 0
        assert sha(ms[dn:]) == c["parity_sha256"], (dn, pn)
        assert len(c["decode"]) == 4
        for d in c["decode"]:
            er = d["erased"]
            work = [ms[i].copy() if er[i] == 0 else np.zeros(size, np.uint8) for i in range(dn + pn)]
            assert o_decode(ec_oracle, dn, pn, er, work, size) == d["rc"], (dn, pn, er)
            rebuilt = [i for i in range(dn + pn) if er[i] == 1 or (i < dn and er[i] != 0)]
            if d["rc"] == 0:
                assert sha([work[i] for i in rebuilt]) == d["sha256"], (dn, pn, er)
                assert all((work[i] == ms[i]).all() for i in rebuilt), (dn, pn, er)
            else:
                assert d["rc"] == -16004 and er.count(0) < dn
            seen.add(("unused" if -1 in er else "") + ("data" if 1 in er[:dn] else "") + ("parity" if 1 in er[dn:] else "") +
                     ("" if d["rc"] == 0 else " refused"))
    assert {"data", "parity", "unuseddataparity", "dataparity refused"} <= seen, seen
