"""One erasure-code family and its whole life from one integer seed (helper, not collected;
tests/test_ec_family.py is its CPU test, tests/test_ec_lifecycle.py and tests/test_ec.py drive the
GPU with it).

make(oracle, seed) draws, with numpy's PCG64 alone, a geometry, hand-laid member images
(tests/test_marshal.py's Image), two legal chunk sequences whose lengths are drawn per chunk, an
erasure vector, an unlink-like change of one data member and a damage list.  Everything a test
expects is composed here from the oracles and from what the generator itself did -- never from the
library: jerasure's encode (oracle_ec_encode) of the members as they are at that step, oracle_crc
and the FileInfo fields for records, the byte-wise difference for the scrub map, and for a located
unit the member that was damaged, the bytes it had and the count of bytes that were changed.

The judge_* functions compare a call's results with those expectations and name the place of the
first difference; the CPU test feeds them the oracle's own results, then one change of each kind.
"""
import types

import numpy as np

from test_marshal import FI, Image, padded
from test_reinstate import plan_of, record_status
from test_scrub import encode
from test_scrub import expected as scrub_expected

UNIT, TILE = 1024, 4096
OK, CRC_ERR, PARAM, INFO_ERR, SIZE_ERR, SYNC_ERR = 0, -1010, -1016, -8016, -8034, -8038
CLEAN, PARITY, DATA, NONE = 0, 1, 2, 3
CONFIRMED = 1
FILL = 0xA5
MAX_MEMBERS = 12
GEOMETRIES = [(dn, pn) for dn in range(1, MAX_MEMBERS) for pn in range(1, MAX_MEMBERS + 1 - dn)]
assert len(GEOMETRIES) == 66
PLACEMENTS = ("payload", "gap", "fileinfo")
# Chosen with the generator alone: a greedy cover of REQUIRED (below) over seeds 0..399 gave 23, 34, 69, 142,
# 163, 271 and 329; the others are the lowest seeds that each add a geometry.  test_ec_family.py refuses a
# list that misses a condition.
SEEDS = [0, 1, 2, 3, 4, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 23, 34, 69, 142, 163, 271, 329]


# ---------------------------------------------------------------- drawing --------

def chunk_sequence(rng, total):
    """A legal in-order sequence over [0, total): offsets on 4096, lengths on 1024 and on 4096 except at the
    end.  Every length is drawn on its own; about one in eight is the single chunk; a partial last tile is a
    chunk of its own more often than not."""
    tiles, tail = divmod(total, TILE)
    if rng.random() < 0.12:
        return [(0, total)]
    body = tiles * TILE if tail and rng.random() < 0.6 else total
    out, o = [], 0
    while o < body:
        n = int(rng.choice([1, 1, 2, 2, 3, 4, 5, 6, 8])) * TILE
        if o + n >= body:
            n = body - o
        out.append((o, n))
        o += n
    if body < total:
        out.append((body, total - body))
    return out


def legal(chunks, total):
    at = 0
    for o, n in chunks:
        if o != at or o % TILE or n <= 0 or n % UNIT or (n % TILE and o + n != total):
            return False
        at = o + n
    return at == total


def erasure_vector(rng, dn, pn):
    """0 alive, 1 dead, -1 not used: at least dn alive, at least one dead, one data member in four not used
    where the geometry has room for it (such a member has no records and no bytes)."""
    n = dn + pn
    e = [0] * n
    if pn >= 2 and dn >= 2 and rng.random() < 0.25:
        e[int(rng.integers(dn))] = -1
    room = pn - e.count(-1)
    ndead = room if rng.random() < 0.5 else int(rng.integers(1, room + 1))
    data = [int(i) for i in rng.permutation(dn) if e[i] == 0]
    par = [int(i) for i in dn + rng.permutation(pn)]
    mode = int(rng.integers(3))
    if mode == 0:
        order = data + par
    elif mode == 1:
        order = par + data
    else:
        order = [x for pair in zip(data, par) for x in pair] + data[len(par):] + par[len(data):]
    for i in order[:ndead]:
        e[i] = 1
    assert e.count(0) >= dn
    return e


def sweep_patterns(dn, pn):
    """Three vectors for the plain decode at any geometry: as many dead as pn allows with data first, the same
    with parity first, and one with a member that is not used (the last data member) beside pn - 1 dead."""
    n = dn + pn
    first = [1 if i < pn else 0 for i in range(n)]
    last = [1 if i >= dn else 0 for i in range(n)]
    third = [0] * n
    third[dn - 1] = -1
    order = [x for pair in zip(range(n - 1, dn - 1, -1), range(dn - 1)) for x in pair] + list(range(dn, n))
    for i in [i for k, i in enumerate(order) if i not in order[:k]][:pn - 1]:
        third[i] = 1
    for e in (first, last, third):
        assert e.count(0) >= dn and sum(1 for x in e if x) >= 1, e
    return [first, last, third]


def _draw_len(rng):
    r = rng.random()
    return int(rng.integers(1, 61)) if r < 0.3 else int(rng.integers(61, 2001)) if r < 0.7 else int(rng.integers(2001, 9001))


def _lay_member(oracle, rng, iseed, block_len, inner):
    """Records of 1 to 9,000 payload bytes with gaps of 0 to 300 random bytes, up to block_len.  Now and then a
    FileInfo is put across the next chunk or unit boundary, a payload made to end on one, or a burst of two dozen
    tiny records laid without gaps."""
    b = Image(oracle, iseed)
    while block_len - b.pos >= FI + 1:
        gap = 0 if rng.random() < 0.4 else int(rng.integers(0, 301))
        nbytes = _draw_len(rng)
        r = rng.random()
        ahead = [x for x in inner if x > b.pos + FI]
        t = ahead[0] if ahead and rng.random() < 0.6 else (b.pos + FI) // UNIT * UNIT + UNIT
        if r < 0.15:                                   # a FileInfo across the boundary t
            at = t - int(rng.integers(1, FI))
            if b.pos <= at <= b.pos + 300:
                gap = at - b.pos
        elif r < 0.30:                                 # a payload that ends on t
            if 1 <= t - (b.pos + gap + FI) <= 9000:
                nbytes = t - (b.pos + gap + FI)
        elif r < 0.38:                                 # a burst
            for _ in range(int(rng.integers(20, 31))):
                if block_len - b.pos < FI + 24:
                    break
                b.rec(int(rng.integers(1, 25)))
            continue
        at = b.pos + gap
        nbytes = min(nbytes, block_len - at - FI)
        if nbytes < 1:
            break
        b.rec(nbytes, at=at)
    return b.image(block_len)


def _spans(mt, total, u):
    """{placement: [(a, b)]} of unit u of a member: the pieces of FileInfos, of payloads, and of what no record covers."""
    lo, hi = u * UNIT, u * UNIT + UNIT
    out = {p: [] for p in PLACEMENTS}
    at = lo
    for x in mt:
        off, sz = int(x["offset"]), int(x["size"])
        if off + sz <= lo or off >= hi:
            continue
        if off > at:
            out["gap"].append((at, off))
        for name, a, b in (("fileinfo", off, off + FI), ("payload", off + FI, off + sz)):
            a, b = max(a, lo), min(b, hi)
            if a < b:
                out[name].append((a, b))
        at = max(at, min(off + sz, hi))
    if at < hi:
        out["gap"].append((at, hi))
    return out


def _edit(rng, a, b, most=UNIT):
    """(start, xor bytes): a run of 1 to min(b - a, most) bytes inside [a, b), every byte of it changed."""
    n = 1 if rng.random() < 0.3 else int(rng.integers(1, min(b - a, most) + 1))
    s = int(rng.integers(a, b - n + 1))
    return s, rng.integers(1, 256, n).astype(np.uint8)


def _draw_changes(rng, imgs, metas):
    """The unlink-like change: new FileInfo bytes for up to three records of one data member, and for one whose
    FileInfo lies across a unit boundary when the layout has one (the member is then chosen among those that do).  Mostly the flag and the time, as an unlink writes
    them; some hit the id, the size or the CRC field, so that the record earns another status."""
    from tfs_amd.crc import FILEINFO_DTYPE

    def across(mt):
        return [r for r, x in enumerate(mt) if int(x["offset"]) // UNIT != (int(x["offset"]) + FI - 1) // UNIT]
    have = [i for i, mt in enumerate(metas) if len(mt)]
    best = [i for i in have if across(metas[i])]
    j = int(rng.choice(best or have))
    mt = metas[j]
    recs = [int(r) for r in rng.choice(len(mt), min(3, len(mt)), replace=False)]
    if across(mt):
        recs.append(int(rng.choice(across(mt))))
    recs = list(dict.fromkeys(recs))
    new, kinds, units = imgs[j].copy(), [], set()
    for n, r in enumerate(recs):
        off = int(mt[r]["offset"])
        fi = np.frombuffer(new[off:off + FI].tobytes(), FILEINFO_DTYPE).copy()
        kind = "flag" if n == 0 or r == recs[-1] else str(rng.choice(["flag", "crc", "id", "size"]))
        if kind == "flag":
            fi["flag_"] |= 1
            fi["modify_time_"] = int(rng.integers(1, 1 << 30))
        elif kind == "crc":
            fi["crc_"] ^= np.uint32(1 << int(rng.integers(32)))
        elif kind == "id":
            fi["id_"] += 1
        else:
            fi["size_"] -= 1
        new[off:off + FI] = fi.view(np.uint8)
        kinds.append((r, kind))
        units.update(range(off // UNIT, (off + FI - 1) // UNIT + 1))
    units = [int(u) for u in rng.permutation(sorted(units))]
    return types.SimpleNamespace(member=j, records=kinds, units=units, image=new,
                                 across=any(int(mt[r]["offset"]) // UNIT != (int(mt[r]["offset"]) + FI - 1) // UNIT
                                            for r, _ in kinds))


def _draw_damages(rng, dn, pn, metas, total):
    """At most one damage per unit.  data1: 1 to 1,024 bytes of one data member, inside a payload, in a gap or
    over a FileInfo (`placement` says which); parity: bytes of a non-empty proper subset of the parity members;
    data2: two data members (the placement is the first one's).  A parity member has no records, so parity damage
    has no placement.  edits: (member, start, xor bytes)."""
    nu = total // UNIT
    units = [int(u) for u in rng.choice(nu, min(nu, int(rng.integers(3, 9))), replace=False)]
    if total % TILE and rng.random() < 0.5 and nu - 1 not in units:
        units[0] = nu - 1
    out = []
    for u in units:
        kinds = ["data1"] + (["parity"] if pn >= 2 else []) + (["data2"] if dn >= 2 else [])
        kind = str(rng.choice(kinds))
        d = types.SimpleNamespace(unit=u, kind=kind, placement=None, member=-1, members=[], parity=[], diff_bytes=0,
                                  edits=[])
        if kind == "parity":
            d.parity = sorted(int(p) for p in rng.choice(pn, int(rng.integers(1, pn)), replace=False))
            for p in d.parity:
                d.edits.append((dn + p,) + _edit(rng, u * UNIT, u * UNIT + UNIT, 32))
        else:
            want = str(rng.choice(PLACEMENTS))
            where = [(i, p, s) for i in range(dn) for p, ss in _spans(metas[i], total, u).items() for s in ss]
            pick = [w for w in where if w[1] == want] or where
            i, d.placement, (a, b) = pick[int(rng.integers(len(pick)))]
            s, x = _edit(rng, a, b)
            d.member, d.members, d.diff_bytes = i, [i], len(x)
            d.edits.append((i, s, x))
            if kind == "data2":
                i2 = int(rng.choice([x for x in range(dn) if x != i]))
                d.members.append(i2)
                d.edits.append((i2,) + _edit(rng, u * UNIT, u * UNIT + UNIT, 64))
                d.member, d.diff_bytes = -1, 0
        out.append(d)
    return out


def apply_damages(members, damages):
    out = [a.copy() for a in members]
    for d in damages:
        for i, s, x in d.edits:
            out[i][s:s + len(x)] ^= x
    return out


def make(oracle, seed, geometry=None, units=None):
    """The family of `seed`.  geometry and units override what the seed would draw (two families of one geometry)."""
    rng = np.random.default_rng(seed)
    dn, pn = GEOMETRIES[int(rng.integers(len(GEOMETRIES)))]
    nu = int(rng.integers(5, 65))
    if geometry:
        dn, pn = geometry
    total = (units or nu) * UNIT
    chunks = chunk_sequence(rng, total)
    chunks2 = chunk_sequence(rng, total)
    while chunks2 == chunks:
        chunks2 = chunk_sequence(rng, total)
    erased = erasure_vector(rng, dn, pn)
    used = [i for i in range(dn) if erased[i] != -1]
    longest = int(rng.choice(used))
    inner = sorted({o for o, _ in chunks[1:]})
    imgs, metas = [], []
    for i in range(dn):
        if erased[i] == -1:
            img, mt = Image(oracle, 0).image(0)
        elif i != longest and rng.random() < 0.15:          # no records: bytes that no index names
            img, mt = Image(oracle, 1000 * seed + i).image(int(rng.integers(0, total + 1)))
        else:
            block_len = int(rng.integers(total - UNIT + 1, total + 1)) if i == longest else \
                int(rng.integers(total // 4, total + 1))
            img, mt = _lay_member(oracle, rng, 1000 * seed + i, block_len, inner)
        imgs.append(img), metas.append(mt)
    assert len(metas[longest]) and max(a.size for a in imgs) > total - UNIT
    f = types.SimpleNamespace(seed=seed, dn=dn, pn=pn, total=total, chunks=chunks, chunks2=chunks2, erased=erased,
                              imgs=imgs, metas=metas, sizes=[a.size for a in imgs], data=padded(imgs, total))
    f.change = _draw_changes(rng, imgs, metas)
    f.new_data = [a for a in f.data]
    f.new_data[f.change.member] = padded([f.change.image], total)[0]
    f.damages = _draw_damages(rng, dn, pn, metas, total)
    assert legal(chunks, total) and legal(chunks2, total)
    return f


# ---------------------------------------------------------------- expectations --------

def records(oracle, f, data):
    """(crc, status) of every record over the data members as given, as expected() in tests/test_marshal.py has them."""
    crc, st = [], []
    for i in range(f.dn):
        for x in f.metas[i]:
            c, s = record_status(oracle, data[i], f.sizes[i], x)
            crc.append(c), st.append(s)
    return np.array(crc, np.uint32), np.array(st, np.int32)


def flat(f):
    return [(i, tuple(x)) for i in range(f.dn) for x in f.metas[i]]


def scrub(oracle, ec_oracle, f, data, parity):
    """(crc, status, parity_units, tile_map): the byte-wise difference of the stored parity and jerasure's encode of
    the data as given."""
    return scrub_expected(oracle, ec_oracle, f.dn, f.pn, data, f.sizes, f.metas, parity, f.total)


def flagged(tmap):
    """The units a scrub map names, as its rows yield them: row 0's ascending, then what later rows add."""
    out = []
    for p in range(tmap.shape[0]):
        for t in np.nonzero(tmap[p])[0]:
            out += [int(t) * 4 + u for u in range(4) if int(tmap[p, t]) >> u & 1]
    return list(dict.fromkeys(out))


def locate_wants(f, before, units, tmap):
    """Per listed unit what the damage there must yield: dict(kind (None: not asserted), member, diff_bytes, parity
    mask, fixed).  `before`: the data members before the damage.  The mask is the scrub map's column."""
    by_unit = {d.unit: d for d in f.damages}
    full = (1 << f.pn) - 1
    out = []
    for u in units:
        d = by_unit[u]
        mask = sum((int(tmap[p, u // 4]) >> (u % 4) & 1) << p for p in range(f.pn))
        w = dict(unit=u, kind=NONE, member=-1, diff_bytes=0, parity=mask, fixed=None)
        if d.kind == "data1":
            assert mask == full, (u, mask)
            w.update(kind=DATA, member=d.member, diff_bytes=d.diff_bytes, fixed=before[d.member][u * UNIT:u * UNIT + UNIT])
        elif d.kind == "parity":
            assert mask == sum(1 << p for p in d.parity), (u, mask)
            w.update(kind=PARITY)
        else:
            assert mask == full, (u, mask)
            if f.pn == 2:
                w.update(kind=None)
        out.append(w)
    return out


# ---------------------------------------------------------------- judges --------

def judge_bytes(what, got, want):
    """got, want: {member: bytes} or lists of members."""
    got = got if isinstance(got, dict) else dict(enumerate(got))
    want = want if isinstance(want, dict) else dict(enumerate(want))
    assert sorted(got) == sorted(want), "%s: members %r, expected %r" % (what, sorted(got), sorted(want))
    for i in sorted(got):
        assert got[i].size == want[i].size, "%s: member %d has %d bytes, expected %d" % (what, i, got[i].size, want[i].size)
        diff = np.nonzero(got[i] != want[i])[0]
        assert diff.size == 0, "%s: member %d differs at byte %d (unit %d): %#x, expected %#x; %d bytes differ" % (
            what, i, diff[0], diff[0] // UNIT, got[i][diff[0]], want[i][diff[0]], diff.size)


def judge_records(what, names, crc, st, nbad, want_crc, want_st):
    """names: flat(f)."""
    assert len(st) == len(want_st) == len(crc) == len(names), "%s: %d records, expected %d" % (what, len(st), len(want_st))
    bad = np.nonzero(st != want_st)[0]
    assert bad.size == 0, "%s: status of record %d %r is %d, expected %d; %d differ" % (
        what, bad[0], names[bad[0]], st[bad[0]], want_st[bad[0]], bad.size)
    bad = np.nonzero(crc != want_crc)[0]
    assert bad.size == 0, "%s: crc of record %d %r is %#x, expected %#x; %d differ" % (
        what, bad[0], names[bad[0]], crc[bad[0]], want_crc[bad[0]], bad.size)
    assert nbad == int((want_st != 0).sum()), "%s: n_bad is %d, expected %d" % (what, nbad, int((want_st != 0).sum()))


def judge_map(what, units, tmap, want_units, want_map):
    assert tmap.shape == want_map.shape, "%s: map shape %r, expected %r" % (what, tmap.shape, want_map.shape)
    bad = np.argwhere(tmap != want_map)
    assert bad.size == 0, "%s: map of parity %d tile %d is %#x, expected %#x; %d bytes differ" % (
        (what,) + tuple(int(x) for x in bad[0]) + (tmap[tuple(bad[0])], want_map[tuple(bad[0])], len(bad)))
    assert units.tolist() == want_units.tolist(), "%s: parity units %r, expected %r" % (what, units.tolist(), want_units.tolist())


def judge_locate(what, res, fixed, wants, pn, untouched=FILL):
    """wants: locate_wants().  untouched: what the rows of `fixed` hold where no repaired unit is due."""
    assert len(res) == len(wants) == len(fixed), "%s: %d results, expected %d" % (what, len(res), len(wants))
    for k, w in enumerate(wants):
        r, at = res[k], "%s: entry %d (unit %d)" % (what, k, w["unit"])
        assert int(r["flags"]) == (CONFIRMED if pn >= 3 else 0), "%s: flags %d" % (at, r["flags"])
        assert int(r["reserved"]) == 0, "%s: reserved %d" % (at, r["reserved"])
        assert int(r["parity"]) == w["parity"], "%s: parity mask %#x, expected %#x" % (at, r["parity"], w["parity"])
        if w["kind"] is None:
            continue
        for name in ("kind", "member", "diff_bytes"):
            assert int(r[name]) == w[name], "%s: %s is %d, expected %d" % (at, name, r[name], w[name])
        want = w["fixed"] if w["fixed"] is not None else np.full(UNIT, untouched, np.uint8)
        diff = np.nonzero(fixed[k] != want)[0]
        assert diff.size == 0, "%s: repaired unit differs at byte %d: %#x, expected %#x; %d bytes differ" % (
            at, diff[0], fixed[k][diff[0]], want[diff[0]], diff.size)


# ---------------------------------------------------------------- coverage --------

def features(f):
    """What a family reaches, as names; REQUIRED lists those a seed list must reach between its families."""
    s = {"pn=%d" % f.pn if f.pn <= 4 else "pn>=5"}
    lost_data = sum(1 for i in range(f.dn) if f.erased[i] != 0)
    if f.pn >= 5 and lost_data >= 5:
        s.add("data outputs in the second output group")
    s |= {n for n, c in (("dn+pn=12", f.dn + f.pn == 12), ("dn=1", f.dn == 1), ("dn=11", f.dn == 11)) if c}
    if -1 in f.erased[:f.dn]:
        s.add("a data member not used")
    lens = [n for _, n in f.chunks]
    s |= {n for n, c in (
        ("chunks: three lengths", len(set(lens)) >= 3),
        ("chunks: one grows", any(b > a for a, b in zip(lens, lens[1:]))),
        ("chunks: one shrinks before the end", any(b < a for a, b in zip(lens[:-1], lens[1:-1]))),
        ("chunks: an odd multiple of 4096", any(n % TILE == 0 and n // TILE % 2 and n > TILE for n in lens)),
        ("chunks: single", len(lens) == 1)) if c}
    if len(lens) > 1 and lens[-1] < TILE and lens[-2] != lens[-1]:
        s.add("chunks: a last one of %d units" % (lens[-1] // UNIT))
    inner = {o for o, _ in f.chunks[1:]}
    for i, mt in enumerate(f.metas):
        if not len(mt) and f.erased[i] != -1:
            s.add("a member without records")
        off, end = mt["offset"].astype(np.int64), mt["offset"].astype(np.int64) + mt["size"]
        for b in inner:
            if ((off < b) & (b < off + FI)).any():
                s.add("a FileInfo across a chunk boundary")
            if (end == b).any():
                s.add("a payload ends on a chunk boundary")
        starts = np.array(sorted(inner | {0}))
        if len(mt) and (np.searchsorted(starts, end - 1, "right") - np.searchsorted(starts, off, "right") >= 2).any():
            s.add("a record over three chunks")
        if (mt["size"] == FI + 1).any():
            s.add("a 37-byte record")
        if len(mt) and np.bincount(off // TILE).max() >= 20:
            s.add("20 records in a tile")
    for d in f.damages:
        s.add("damage: parity" if d.kind == "parity" else "damage: %s in a %s" % (d.kind, d.placement))
        if f.total % TILE and d.unit >= f.total // TILE * 4:
            s.add("damage in the last, partial tile")
    dd, dp = 1 in f.erased[:f.dn], 1 in f.erased[f.dn:]
    s.add("erased: data only" if dd and not dp else "erased: parity only" if dp and not dd else "erased: mixed")
    if plan_of(f.dn, f.pn, f.erased)[0][-1] >= f.dn:
        s.add("erased: parity among the sources")
    if f.change.across:
        s.add("change: a FileInfo across a unit boundary")
    if f.total % TILE:
        s.add("total ends in a partial tile")
    return s


REQUIRED = (["pn=%d" % p for p in (1, 2, 3, 4)] + ["pn>=5", "data outputs in the second output group", "dn+pn=12",
            "dn=1", "dn=11", "a data member not used", "chunks: three lengths", "chunks: one grows",
            "chunks: one shrinks before the end", "chunks: an odd multiple of 4096", "chunks: single"] +
            ["chunks: a last one of %d units" % u for u in (1, 2, 3)] +
            ["a FileInfo across a chunk boundary", "a payload ends on a chunk boundary", "a record over three chunks",
             "a 37-byte record", "20 records in a tile", "a member without records", "damage: parity"] +
            ["damage: %s in a %s" % (k, p) for k in ("data1", "data2") for p in PLACEMENTS] +
            ["damage in the last, partial tile", "erased: data only", "erased: parity only", "erased: mixed",
             "erased: parity among the sources", "change: a FileInfo across a unit boundary",
             "total ends in a partial tile"])


def assert_seed_coverage(fams):
    """Fails unless the families reach every condition of REQUIRED between them, two geometries with five or more
    parity members among them -- an empty or lopsided list cannot pass silently.  Returns {condition: seeds}."""
    seen = {}
    for f in fams:
        for name in features(f):
            seen.setdefault(name, []).append(f.seed)
    missing = [n for n in REQUIRED if n not in seen]
    assert not missing, "the seed list reaches no family with: %s (%d families)" % ("; ".join(missing), len(fams))
    wide = sorted({(f.dn, f.pn) for f in fams if f.pn >= 5})
    assert len(wide) >= 2, "geometries with pn >= 5: %r, two are needed" % (wide,)
    return {n: seen[n] for n in REQUIRED}
