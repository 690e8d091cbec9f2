"""Scrub session (include/tfs_ec.h tfs_ec_scrub_*): the stored parity of a
family compared with the code of its data members as read, chunk by chunk, with every
record of the data members verified in the same pass, and no member written.

Expected values are composed from what is already pinned: oracle_ec_encode runs over the
data members as given (corrupted ones included), and the expected bit for (p, unit) is
"stored parity p differs from that encode anywhere in the unit", computed in numpy; record
CRCs and statuses come from oracle_crc and the FileInfo fields (tests/test_reinstate.py's
record_status, the order of checks of tests/test_marshal.py's expected).  Images are laid
out by hand with tests/test_marshal.py's Image.  Unless a case says otherwise the chunk
buffers are reused across chunks.  Every run also checks that no member was written: the
device buffers are downloaded after the chunk's work and compared with what was uploaded,
and the host form is checked on the caller's arrays.
"""
import ctypes

import numpy as np
import pytest

from test_marshal import CHUNK, FI, Image, chunks_of, family, padded, up
from test_marshal import run as marshal_run
from test_marshal import placements  # noqa: F401  (the fixture: one member with every placement the walk branches on)
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode)
from test_reinstate import member_slices, ptrs, record_status
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

OK, CRC_ERR, PARAM, INFO_ERR, SIZE_ERR, SYNC_ERR = 0, -1010, -1016, -8016, -8034, -8038
DATA_INVALID, SIZE_INVALID, MATRIX_INVALID = -16001, -16002, -16003


def encode(ec_oracle, k, m, data, total):  # noqa: F811
    """jerasure's parity of the data members as given (arrays of `total` bytes)."""
    ms = [a.copy() for a in data] + [np.zeros(total, np.uint8) for _ in range(m)]
    assert ec_oracle.oracle_ec_encode(k, m, ptrs(ms), None, total) == 0
    return ms[k:]


def expected(oracle, ec_oracle, k, m, data, sizes, metas, parity, total):  # noqa: F811
    """(crc, status, parity_units, tile_map) from the oracles."""
    code = encode(ec_oracle, k, m, data, total)
    tm = np.zeros((m, (total + 4095) // 4096), np.uint8)
    units = np.zeros(m, np.uint32)
    for p in range(m):
        diff = (parity[p] != code[p]).reshape(total // 1024, 1024).any(axis=1)
        units[p] = int(diff.sum())
        for u in np.nonzero(diff)[0]:
            tm[p, u // 4] |= 1 << (u % 4)
    crc, st = [], []
    for i in range(k):
        for x in metas[i]:
            c, s = record_status(oracle, data[i], sizes[i], x)
            crc.append(c), st.append(s)
    return np.array(crc, np.uint32), np.array(st, np.int32), units, tm


def run(ctx, k, m, data, parity, metas, sizes, total, chunks, form="device", stream=None, reuse=True):
    """One whole session over the members as given; finish's result.  Asserts that no member byte was written."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, ScrubSession
    ec = ErasureCode(ctx, k, m)
    assert ec.rc == 0
    ses = ScrubSession(ec, metas, sizes, total)
    assert ses.rc == 0
    mem = list(data) + list(parity)
    if form == "host":
        given = [a.copy() for a in mem]
        for o, n in chunks:
            assert ses.check([a[o:o + n] for a in given], o, n) == 0
        assert all((a == b).all() for a, b in zip(given, mem))
    elif reuse:
        cmax = max(n for _, n in chunks)
        d = [crc.DeviceBuffer(ctx, cmax) for _ in mem]
        sync = (lambda: ctx.stream_sync(stream)) if stream else ctx.sync
        for o, n in chunks:
            for b, a in zip(d, mem):
                b.upload(a[o:o + n])
            assert ses.check_device(d, o, n, stream=stream) == 0
            sync()
            for i, (b, a) in enumerate(zip(d, mem)):
                assert (b.download(np.uint8, n) == a[o:o + n]).all(), (i, o)
    else:
        d = [crc.DeviceBuffer(ctx, total).upload(a) for a in mem]
        for o, n in chunks:
            assert ses.check_device([b.ptr + o for b in d], o, n, stream=stream) == 0
    res = ses.finish()
    if form == "device" and not reuse:
        for i, (b, a) in enumerate(zip(d, mem)):
            assert (b.download(np.uint8, total) == a).all(), i
    ses.free()
    ec.free()
    return res


def check(ctx, oracle, ec_oracle, k, m, data, parity, metas, sizes, total, chunks, **kw):  # noqa: F811
    ecrc, est, eunits, emap = expected(oracle, ec_oracle, k, m, data, sizes, metas, parity, total)
    crc, st, nbad, units, tmap, rc = run(ctx, k, m, data, parity, metas, sizes, total, chunks, **kw)
    assert rc == 0
    flat = [(i, x) for i in range(k) for x in metas[i]]
    bad = np.nonzero(st != est)[0]
    assert bad.size == 0, [(int(j), flat[j], int(st[j]), int(est[j])) for j in bad[:5]]
    bad = np.nonzero(crc != ecrc)[0]
    assert bad.size == 0, [(int(j), flat[j], hex(crc[j]), hex(ecrc[j])) for j in bad[:5]]
    assert nbad == int((est != 0).sum())
    assert tmap.shape == emap.shape
    bad = np.argwhere(tmap != emap)
    assert bad.size == 0, [(int(p), int(t), int(tmap[p, t]), int(emap[p, t])) for p, t in bad[:5]]
    assert units.tolist() == eunits.tolist()
    return crc, st, units, tmap


def only(tmap, where):
    """The map has exactly the bits {(p, unit)} of `where`."""
    want = np.zeros_like(tmap)
    for p, u in where:
        want[p, u // 4] |= 1 << (u % 4)
    return (tmap == want).all()


LENS = [70001, 98304, 65536 + 1024, 81920 - 7]  # test_marshal.py::test_coders


@pytest.mark.parametrize("k,m", [(5, 3), (2, 1), (8, 4), (6, 6)])
def test_clean_families(gpu_ctx, oracle, ec_oracle, k, m):  # noqa: F811
    """(6, 6) takes two launches per chunk: the second group compares without a walk."""
    imgs, metas = family(oracle, k, 10 * k + m, LENS)
    total = up(max(a.size for a in imgs), 1024)
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, k, m, data, total)
    crc, st, units, tmap = check(gpu_ctx, oracle, ec_oracle, k, m, data, parity, metas, sizes, total,
                                 chunks_of(total, 16384))
    assert (st == 0).all() and len(st) > 10 * k and (units == 0).all() and not tmap.any()
    mpar, (mcrc, mst, _, mrc) = marshal_run(gpu_ctx, k, m, imgs, metas, total, chunks_of(total, 16384))
    assert mrc == 0 and (mcrc == crc).all() and (mst == st).all()
    assert all((a == b).all() for a, b in zip(mpar, parity))


@pytest.fixture(scope="module")
def fam53(oracle, ec_oracle):  # noqa: F811
    """(5, 3): padded data, sizes, metas, total, and the clean parity."""
    imgs, metas = family(oracle, 5, 53, LENS)
    total = up(max(a.size for a in imgs), 1024)
    data = padded(imgs, total)
    return data, [a.size for a in imgs], metas, total, encode(ec_oracle, 5, 3, data, total)


def test_no_member_written(gpu_ctx, oracle, ec_oracle, fam53):  # noqa: F811
    """A family with a wrong parity byte and a wrong payload byte: whole members on the device, reused chunk
    buffers and the host form all leave every byte of all dn + pn members as given (asserted inside run)."""
    data, sizes, metas, total, parity = fam53
    d2, p2 = [a.copy() for a in data], [a.copy() for a in parity]
    d2[2][int(metas[2][1]["offset"]) + FI + 9] ^= 4
    p2[0][50000] ^= 1
    ref = None
    for kw in ({"reuse": False}, {}, {"form": "host"}):
        crc, st, units, tmap = check(gpu_ctx, oracle, ec_oracle, 5, 3, d2, p2, metas, sizes, total,
                                     chunks_of(total, 16384), **kw)
        ref = ref or (crc, st, units, tmap)
        assert all((a == b).all() for a, b in zip(ref, (crc, st, units, tmap)))
    assert tmap.any() and (st != 0).sum() == 1


def test_placements(gpu_ctx, oracle, ec_oracle, placements):  # noqa: F811
    """One chunk (no reuse), 4 KiB chunks and 16 KiB chunks: the same CRCs, statuses and map."""
    imgs, metas, total = placements
    assert CHUNK == 16384
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, 5, 3, data, total)
    ref = None
    for chunks, kw in [([(0, total)], {"reuse": False}), (chunks_of(total, 4096), {}), (chunks_of(total, CHUNK), {})]:
        crc, st, units, tmap = check(gpu_ctx, oracle, ec_oracle, 5, 3, data, parity, metas, sizes, total, chunks, **kw)
        assert (st == 0).all() and not tmap.any() and (units == 0).all()
        ref = ref or (crc, st)
        assert (crc == ref[0]).all() and (st == ref[1]).all()


@pytest.mark.parametrize("units", [1, 2, 3])
def test_short_last_tile(gpu_ctx, oracle, ec_oracle, units):  # noqa: F811
    """total is 1, 2, 3 units past a tile.  One wrong byte in the last existing unit of parity 1 and one in the unit
    before: exactly those bits, and the bits of units that do not exist are 0."""
    total = 65536 + 1024 * units
    b = Image(oracle, 40 + units).fill(total - 12000)
    b.rec(total - b.pos - FI)                            # up to the member's last byte, into the short tile
    img, mt = b.image()
    assert img.size == total
    imgs, metas = family(oracle, 2, 50 + units, [total - 1024 * units - 3, 30000])
    imgs, metas = [imgs[0], img, imgs[1]], [metas[0], mt, metas[1]]
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, 3, 2, data, total)
    last = total // 1024 - 1
    parity[1][total - 1] ^= 0x80
    parity[1][1024 * (last - 1) + 3] ^= 1
    for clen in (total, 8192):
        _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 3, 2, data, parity, metas, sizes, total,
                                chunks_of(total, clen))
        assert (st == 0).all() and pu.tolist() == [0, 2] and only(tmap, [(1, last), (1, last - 1)])
        assert tmap.shape[1] == 17 and int(tmap[1, 16]) < (1 << units)


def test_wrong_parity_byte(gpu_ctx, oracle, ec_oracle, fam53):  # noqa: F811
    """One byte of one parity member: exactly one bit in that member's row, the other rows zero, every record passes."""
    data, sizes, metas, total, parity = fam53
    unit = 37 * 1024
    offsets = [0, total - 1, 4095, 4096, 1023, 1024, 16383, 16384] + [unit + 128 * c + (29 * c + 5) % 128 for c in range(8)]
    for i, x in enumerate(offsets):
        p = i % 3
        hurt = [a if j != p else a.copy() for j, a in enumerate(parity)]
        hurt[p][x] ^= 1 << (i % 8)
        _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 5, 3, data, hurt, metas, sizes, total,
                                chunks_of(total, 16384))
        assert (st == 0).all(), x
        assert pu.tolist() == [int(j == p) for j in range(3)], x
        assert only(tmap, [(p, x // 1024)]), x


@pytest.mark.parametrize("k,m", [(5, 3), (6, 6)])
def test_wrong_data_byte_inside_a_payload(gpu_ctx, oracle, ec_oracle, k, m):  # noqa: F811
    """That record is a CRC error and every parity row has exactly that unit set -- all six rows in (6, 6), which
    reaches both launch groups."""
    imgs, metas = family(oracle, k, 7 * k + m, LENS)
    total = up(max(a.size for a in imgs), 1024)
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, k, m, data, total)
    r = len(metas[1]) // 2
    x = int(metas[1][r]["offset"]) + FI + 300
    data[1][x] ^= 0x20
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, k, m, data, parity, metas, sizes, total, chunks_of(total, 16384))
    sl = member_slices(metas)
    assert st[sl[1]][r] == CRC_ERR and int((st != 0).sum()) == 1   # n_bad == 1 is checked by check()
    assert pu.tolist() == [1] * m and only(tmap, [(p, x // 1024) for p in range(m)])


def gapped_member(oracle, seed):
    """Records with a 300-byte gap between two of them; returns (image, metas, an offset inside the gap)."""
    b = Image(oracle, seed)
    b.rec(5000)
    b.rec(9000)
    g = b.pos + 150
    b.gap(300)
    b.rec(4000)
    b.fill(60000)
    img, mt = b.image()
    return img, mt, g


def test_wrong_data_byte_in_a_gap(gpu_ctx, oracle, ec_oracle):  # noqa: F811
    """No record fails and every parity row has the unit set: the case no other call can see."""
    img, mt, g = gapped_member(oracle, 600)
    imgs, metas = family(oracle, 4, 610, [66000, 61440])
    imgs, metas = imgs[:2] + [img] + imgs[2:], metas[:2] + [mt] + metas[2:]
    total = up(max(a.size for a in imgs), 1024)
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, 5, 3, data, total)
    data[2][g] ^= 0x08
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 5, 3, data, parity, metas, sizes, total, chunks_of(total, 16384))
    assert (st == 0).all() and pu.tolist() == [1, 1, 1] and only(tmap, [(p, g // 1024) for p in range(3)])


def test_wrong_fileinfo(gpu_ctx, oracle, ec_oracle, fam53):  # noqa: F811
    """A flipped id byte and a flipped size_ byte: the two statuses, plus each unit in every row."""
    data, sizes, metas, total, parity = fam53
    d2 = [a.copy() for a in data]
    a_id, a_size = int(metas[0][2]["offset"]) + 3, int(metas[3][4]["offset"]) + 12
    d2[0][a_id] ^= 4
    d2[3][a_size] ^= 1
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 5, 3, d2, parity, metas, sizes, total, chunks_of(total, 16384))
    sl = member_slices(metas)
    assert st[sl[0]][2] == INFO_ERR and st[sl[3]][4] == SYNC_ERR and int((st != 0).sum()) == 2
    assert a_id // 1024 != a_size // 1024 and pu.tolist() == [2, 2, 2]
    assert only(tmap, [(p, a // 1024) for p in range(3) for a in (a_id, a_size)])


def test_zero_extension(gpu_ctx, oracle, ec_oracle):  # noqa: F811
    """A data member of 30,000 bytes beside 70,001-byte ones is clean; a non-zero byte in its chunk buffer past
    30,000 is flagged in every row."""
    imgs, metas = family(oracle, 3, 700, [70001, 30000, 70001])
    total = up(70001, 1024)
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    assert sizes[1] == 30000
    parity = encode(ec_oracle, 3, 2, data, total)
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 3, 2, data, parity, metas, sizes, total, chunks_of(total, 16384))
    assert (st == 0).all() and not tmap.any()
    data[1][40000] = 7
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 3, 2, data, parity, metas, sizes, total, chunks_of(total, 16384))
    assert (st == 0).all() and pu.tolist() == [1, 1] and only(tmap, [(0, 39), (1, 39)])


def test_rejected_before_the_pass(gpu_ctx, oracle, ec_oracle):  # noqa: F811
    """size <= 36, a record past sizes[i], a negative offset: reported from begin, the neighbours still verified,
    the map clean."""
    from tfs_amd.crc import META_DTYPE
    imgs, metas = family(oracle, 2, 200, [60000, 50000])
    total = up(60000, 1024)
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, 2, 1, data, total)
    out = []
    for i in range(2):
        mt = metas[i].tolist()
        mt.insert(3, (999, mt[3][1] - 40, 36))
        mt.insert(1, (998, -5, 100))
        mt.append((996, imgs[i].size - 100, 101))
        mt.append((995, imgs[i].size + 4096, 50))
        out.append(np.array(mt, META_DTYPE))
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 2, 1, data, parity, out, sizes, total, chunks_of(total, 8192))
    for sl, mt in zip(member_slices(out), metas):
        got = st[sl].tolist()
        assert got[1] == PARAM and got[4] == SIZE_ERR and got[-2:] == [PARAM, PARAM] and got.count(0) == len(mt)
    assert not tmap.any()


def test_no_records_is_the_compare_alone(gpu_ctx, oracle, ec_oracle):  # noqa: F811
    import tfs_amd.crc as crc
    imgs = [synth_bytes(900 + i, n) for i, n in enumerate((70000, 65536, 1))]
    total = 70656
    data, sizes = padded(imgs, total), [a.size for a in imgs]
    parity = encode(ec_oracle, 3, 2, data, total)
    none = [np.zeros(0, crc.META_DTYPE)] * 3
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 3, 2, data, parity, none, sizes, total, chunks_of(total, 4096))
    assert len(st) == 0 and not tmap.any()
    parity[1][70655] ^= 1
    data[2][0] ^= 1
    _, st, pu, tmap = check(gpu_ctx, oracle, ec_oracle, 3, 2, data, parity, none, sizes, total, chunks_of(total, 4096))
    assert pu.tolist() == [1, 2] and only(tmap, [(0, 0), (1, 0), (1, 68)])


def test_host_form_against_device_form(gpu_ctx, oracle, ec_oracle, fam53):  # noqa: F811
    data, sizes, metas, total, parity = fam53
    d2, p2 = [a.copy() for a in data], [a.copy() for a in parity]
    d2[0][int(metas[0][3]["offset"]) + FI + 7] ^= 1
    p2[2][12345] ^= 0x40
    a = check(gpu_ctx, oracle, ec_oracle, 5, 3, d2, p2, metas, sizes, total, chunks_of(total, 16384))
    b = check(gpu_ctx, oracle, ec_oracle, 5, 3, d2, p2, metas, sizes, total, chunks_of(total, 16384), form="host")
    assert all((x == y).all() for x, y in zip(a, b)) and (a[1] != 0).any() and a[3].any()


def test_call_level_errors(gpu_ctx, oracle, ec_oracle):  # noqa: F811
    """Every refused call launches nothing: the session still completes with a zero map."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, ScrubSession
    imgs, metas = family(oracle, 2, 400, [66000, 70000])
    sizes = [a.size for a in imgs]
    total = 70656
    data = padded(imgs, total)
    parity = encode(ec_oracle, 2, 1, data, total)
    ec = ErasureCode(gpu_ctx, 2, 1)

    def begin(mt=metas, sz=sizes, tot=total, coder=ec):
        s = ScrubSession(coder, mt, sz, tot)
        rc = s.rc
        if rc:
            assert not s.h.value
        s.free()
        return rc
    assert begin() == 0
    assert begin(tot=total + 100) == SIZE_INVALID and begin(tot=0) == SIZE_INVALID and begin(tot=-1024) == SIZE_INVALID
    assert begin(sz=[sizes[0], total + 1]) == DATA_INVALID and begin(sz=[-1, sizes[1]]) == DATA_INVALID
    swapped = metas[0].copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    assert begin(mt=[swapped, metas[1]]) == PARAM                       # unsorted
    over = metas[1].copy()
    over["size"][1] += 1
    assert begin(mt=[metas[0], over]) == PARAM                          # overlapping
    assert begin(tot=total + 100, sz=[total + 200, 0]) == SIZE_INVALID  # the size check comes before the members'
    h = ctypes.c_void_p()
    assert ec.L.tfs_ec_scrub_begin(None, None, None, None, total, ctypes.byref(h)) == PARAM
    # the chunk rules
    ses = ScrubSession(ec, metas, sizes, total)
    d = [crc.DeviceBuffer(gpu_ctx, total).upload(a) for a in data + parity]

    def at(o):
        return [b.ptr + o for b in d]
    s1, s2 = gpu_ctx.stream_create(), gpu_ctx.stream_create()
    try:
        assert ses.check_device(at(4096), 4096, 4096, stream=s1) == PARAM      # the first chunk is at 0 (skipped)
        assert ses.check_device(at(0), 0, 8192, stream=2) == PARAM             # hipStreamPerThread
        assert ses.check_device(at(0), 0, 1000, stream=s1) == PARAM            # len % 1024
        assert ses.check_device(at(0), 0, 5120, stream=s1) == PARAM            # len % 4096 before the end
        assert ses.check_device(at(0), 0, 0, stream=s1) == PARAM
        assert ses.check_device(at(0), 0, total + 1024, stream=s1) == PARAM    # past total
        assert ses.check_device([None] + at(0)[1:], 0, 8192, stream=s1) == DATA_INVALID   # a NULL data member
        assert ses.check_device(at(0)[:2] + [None], 0, 8192, stream=s1) == DATA_INVALID   # a NULL parity member
        assert ses.finish()[5] == PARAM                                        # nothing covered yet
        assert ses.check_device(at(0), 0, 8192, stream=s1) == 0
        assert ses.check_device(at(0), 0, 8192, stream=s1) == PARAM            # repeated
        assert ses.check_device(at(12288), 12288, 4096, stream=s1) == PARAM    # skipped
        assert ses.check_device(at(8192 + 512), 8192 + 512, 4096, stream=s1) == PARAM  # misaligned
        assert ses.check_device(at(8192), 8192, 4096, stream=s2) == PARAM      # a second stream
        assert ses.check_device(at(8192), 8192, 4096, stream=None) == PARAM    # the context's stream is another one too
        assert ses.check([np.zeros(4096, np.uint8)] * 3, 8192, 4096) == PARAM  # and so is the host form's
        assert ses.finish()[5] == PARAM                                        # before the end
        assert ses.check_device(at(8192), 8192, 2048, stream=s1) == PARAM      # offset + len != total
        assert ses.check_device(at(8192), 8192, total - 8192, stream=s1) == 0  # 1 KiB units to the end
        crc_, st, nbad, pu, tmap, rc = ses.finish()
        assert rc == 0 and (st == 0).all() and nbad == 0 and len(st) == len(metas[0]) + len(metas[1])
        assert not tmap.any() and pu.tolist() == [0]                           # no refused call left a word behind
        assert ses.check_device(at(0), 0, 8192, stream=s1) == PARAM            # a finished session takes no chunk
        for b, a in zip(d, data + parity):
            assert (b.download(np.uint8, total) == a).all()
    finally:
        ses.free()
        gpu_ctx.stream_destroy(s1)
        gpu_ctx.stream_destroy(s2)
        ec.free()
    dec_only = ErasureCode(gpu_ctx, 2, 1, [1, 0, 0])                           # any coder with an encoding matrix
    assert dec_only.rc == 0 and begin(coder=dec_only) == 0
    dec_only.free()
