"""The stripe-0 seed edge, on the CPU: the geometry model of tests/crc_geometry.py
agrees with a brute-force search, the closed-form edge list reaches the edge and
its neighbours do not, a write frame's prefix H never reaches it, and the
coverage condition the GPU tests apply to their placements rejects an empty or
lopsided list.  No GPU."""
import itertools

import pytest

import crc_geometry as cg


def test_constructed_cases_cross_and_neighbours_do_not():
    """(a) every constructed case is at the edge, in the class it was built for; no neighbour is."""
    cases = cg.edge_cases()
    assert len(cases) == 135
    assert min(e.length for e in cases) == 913 == cg.edge_length(3, 2, 112, 0)
    assert max(e.length for e in cases) < 33 * 1024 + 32
    for e in cases:
        assert e.residue in (125, 126, 127)
        for base in (0, 128, 4096 * 7, 0x7F0000000000):   # the residue alone decides
            addr = base + e.residue
            assert cg.seed_crosses(addr, e.length), e
            assert cg.classify(addr, e.length) == (e.s, e.ns, e.d), e
            g = cg.geo(addr, e.length)
            assert g.nstripes == e.ns and g.E - g.B16 == e.d and g.nvalid == 64 - e.d // 16
            assert g.end - g.B16 == e.t and g.s == e.s
            for r, ln in cg.neighbours(e):
                assert ln == e.length and r in (124, 120 + e.s)
                assert not cg.seed_crosses(base + r, ln), (e, r)
    assert [n[0] for n in cg.neighbours(cg.edge_case(2, 3, 16, 1))] == [124, 122]


def test_model_agrees_with_brute_force():
    """(b) over addresses 0..1023 and lengths 32..2999 the predicate's hit set is
    the closed form's: residues 125..127 only, 7,056 hits."""
    hits = {(a, n) for a in range(1024) for n in range(32, 3000) if cg.seed_crosses(a, n)}
    closed = set()
    for s, ns, d, t in itertools.product((1, 2, 3), range(2, 6), range(0, 128, 16), range(16)):
        n = cg.edge_length(s, ns, d, t)
        if 32 <= n <= 2999:
            for a in range((124 + s) % 128, 1024, 128):
                closed.add((a, n))
    assert hits == closed
    assert len(hits) == 7056
    assert {a % 128 for a, _ in hits} == {125, 126, 127}
    assert min(n for _, n in hits) == 913
    # shorter than kMinParallelLen: the byte loop, whatever the address
    assert not any(cg.seed_crosses(a, n) for a in range(256) for n in range(32))


def test_anchor_offset_moves_the_residue():
    """The record kernels' anchor offset (make_geo's aoff): the edge sits at residue
    aoff + 124 + s - 128 instead, same lengths."""
    for aoff in (0, 16, 64, 112):
        hits = {(a % 128, n) for a in range(128, 256) for n in range(32, 2200) if cg.seed_crosses(a, n, aoff)}
        assert {r for r, _ in hits} == {(aoff + 124 + s) % 128 for s in (1, 2, 3)}
        assert {n for r, n in hits if r == (aoff + 125) % 128} == \
            {n for n in range(32, 2200) if cg.seed_crosses(125, n)}
        g = cg.geo(1000, 5000, aoff)
        assert g.E % 128 == aoff and 0 <= g.E - g.B16 < 128 and g.sb0 <= g.A < g.sb0 + cg.STRIPE


def test_write_frame_prefix_never_crosses():
    """(c) the prefix H of a write frame (36 + 8 count bytes, count 0..27: at most 252)
    is shorter than the shortest payload at the edge (913), so it is one stripe
    at every address: short_chain needs no carry into a stripe 1."""
    for count in range(28):
        hlen = 36 + 8 * count
        for r in range(128):
            assert not cg.seed_crosses(4096 + r, hlen)
            assert cg.geo(4096 + r, hlen).nstripes == 1


def test_coverage_helper_rejects_empty_and_lopsided_lists():
    """(d) assert_edge_coverage: every (s, ns, d) class or a failure."""
    base = 1 << 20
    full = [(base + e.residue, e.length) for e in cg.edge_cases()]
    seen = cg.assert_edge_coverage(full)
    assert len(seen) == len(cg.EDGE_S) * len(cg.EDGE_NS) * len(cg.EDGE_D) == 45
    # one tail per class is enough; the neighbours add nothing
    cg.assert_edge_coverage([(base + e.residue, e.length) for e in cg.edge_cases(ts=(1,))] +
                            [(base + r, n) for e in cg.edge_cases() for r, n in cg.neighbours(e)])
    with pytest.raises(AssertionError):
        cg.assert_edge_coverage([])
    with pytest.raises(AssertionError):   # the neighbours alone
        cg.assert_edge_coverage([(base + r, n) for e in cg.edge_cases() for r, n in cg.neighbours(e)])
    with pytest.raises(AssertionError):   # the right lengths at offsets 16..63 of an aligned buffer
        cg.assert_edge_coverage([(base + 16 + e.s, e.length) for e in cg.edge_cases()])
    for drop in ({"s": 2}, {"ns": 17}, {"d": 112}):
        part = [(base + e.residue, e.length) for e in cg.edge_cases()
                if all(getattr(e, k) != v for k, v in drop.items())]
        with pytest.raises(AssertionError):
            cg.assert_edge_coverage(part)
    # the same list placed in a buffer whose base is 64 (mod 128) reaches nothing
    with pytest.raises(AssertionError):
        cg.assert_edge_coverage([(a + 64, n) for a, n in full])


def test_place_puts_a_payload_at_a_residue():
    for cursor in (0, 1, 127, 128, 1000):
        for r in (0, 124, 125, 127):
            a = cg.place(cursor, r)
            assert a >= cursor and a % 128 == r and a - cursor < 128
