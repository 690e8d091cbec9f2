"""Reinstate session (include/tfs_ec.h tfs_ec_reinstate_*): the dead
members of a family rebuilt chunk by chunk, with every record of every data member
verified in the same pass -- the survivors' from the bytes that feed the code, the
rebuilt members' from the bytes the code yields.

Expected values are composed from what is already pinned: oracle_ec_encode for the
parity of the zero-extended members, oracle_ec_decode for what a decode makes of the
survivors as they are (corrupted ones included), oracle_crc and the FileInfo fields of
those bytes for every CRC and status; tfs_ec_decode_device is a second witness for the
bytes.  Images are laid out by hand with tests/test_marshal.py's Image.  Unless a case
says otherwise the chunk buffers are reused across chunks and the outputs' buffers are
prefilled with a marker byte.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, ocrc
from test_marshal import CHUNK, FI, Image, chunks_of, family, padded, up
from test_marshal import placements  # noqa: F401  (the fixture: one member with every placement the walk branches on)
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

OK, CRC_ERR, PARAM, INFO_ERR, SIZE_ERR, SYNC_ERR = 0, -1010, -1016, -8016, -8034, -8038
DATA_INVALID, SIZE_INVALID, MATRIX_INVALID = -16001, -16002, -16003
FILL = 0xA5


@pytest.fixture(scope="module")
def ec_oracle():
    so = os.path.join(ROOT, "oracle", "liboracle_ec.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle_ec.so"])
    L = ctypes.CDLL(so)
    L.oracle_ec_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.oracle_ec_decode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_int]
    return L


def ptrs(ms):
    return (ctypes.c_void_p * len(ms))(*[a.ctypes.data for a in ms])


def erased_of(k, m, dead):
    """check_reinstate's marks: the first k present members alive, further ones unused, the lost ones dead."""
    e, alive = [], 0
    for i in range(k + m):
        if i in dead:
            e.append(1)
        else:
            e.append(0 if alive < k else -1)
            alive += 1
    return e


def plan_of(k, m, erased):
    """(sources, outputs) as ErasureCode::decode takes them: the first k alive; erased data, then dead parity."""
    src = [i for i in range(k + m) if erased[i] == 0][:k]
    out = [i for i in range(k) if erased[i] != 0] + [i for i in range(k, k + m) if erased[i] == 1]
    return src, out


def encode_family(ec_oracle, k, m, imgs, total):
    """The whole family as it was marshalled: the data members zero-extended to total, and their parity."""
    fam = padded(imgs, total) + [np.zeros(total, np.uint8) for _ in range(m)]
    assert ec_oracle.oracle_ec_encode(k, m, ptrs(fam), None, total) == 0
    return fam


def record_status(oracle, img, size, x):
    """(crc, status) of one index entry over the member's bytes, in the session's order of checks."""
    from tfs_amd.crc import FILEINFO_DTYPE
    off, sz = int(x["offset"]), int(x["size"])
    if off < 0 or off + sz > size:
        return 0, PARAM
    if sz <= FI:
        return 0, SIZE_ERR
    fi = np.frombuffer(img[off:off + FI].tobytes(), FILEINFO_DTYPE)[0]
    c = ocrc(oracle, 0, img[off + FI:off + sz].tobytes())
    return c, (INFO_ERR if int(fi["id_"]) != int(x["file_id"]) else SYNC_ERR if int(fi["size_"]) != sz else
               CRC_ERR if int(fi["crc_"]) != c else OK)


def expected(oracle, ec_oracle, k, m, erased, fam, metas, sizes, total):
    """(members after the oracle's decode of `fam` as it is, crc, status).  The bytes of the plan's outputs in
    `fam` do not matter: they are cleared first."""
    src, out = plan_of(k, m, erased)
    ms = [a.copy() for a in fam]
    for o in out:
        ms[o][:] = 0
    assert ec_oracle.oracle_ec_decode(k, m, (ctypes.c_int * (k + m))(*erased), ptrs(ms), None, total) == 0
    crc, st = [], []
    for i in range(k):
        for x in metas[i]:
            c, s = record_status(oracle, ms[i], sizes[i], x)
            crc.append(c), st.append(s)
    return ms, np.array(crc, np.uint32), np.array(st, np.int32)


def run(ctx, k, m, erased, fam, metas, sizes, total, chunks, form="device", stream=None, reuse=True):
    """One whole session: ({output member: bytes}, finish's result)."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, ReinstateSession
    ec = ErasureCode(ctx, k, m, erased)
    assert ec.rc == 0
    ses = ReinstateSession(ec, metas, sizes, total)
    assert ses.rc == 0
    src, out = plan_of(k, m, erased)
    got = {o: np.full(total, FILL, np.uint8) for o in out}
    n = k + m
    if form == "host":
        for o, ln in chunks:
            mem = [fam[i][o:o + ln].copy() if i in src else got[i][o:o + ln] if i in got else None for i in range(n)]
            assert ses.decode(mem, o, ln) == 0
    elif reuse:
        cmax = max(ln for _, ln in chunks)
        d = {i: crc.DeviceBuffer(ctx, cmax) for i in src + out}
        mem = [d.get(i) for i in range(n)]
        sync = (lambda: ctx.stream_sync(stream)) if stream else ctx.sync
        for o, ln in chunks:
            for i in src:
                d[i].upload(fam[i][o:o + ln])
            for i in out:
                d[i].upload(np.full(ln, FILL, np.uint8))
            assert ses.decode_device(mem, o, ln, stream=stream) == 0
            sync()
            for i in out:
                got[i][o:o + ln] = d[i].download(np.uint8, ln)
    else:
        d = {i: crc.DeviceBuffer(ctx, total).upload(fam[i] if i in src else got[i]) for i in src + out}
        for o, ln in chunks:
            assert ses.decode_device([d[i].ptr + o if i in d else None for i in range(n)], o, ln, stream=stream) == 0
    res = ses.finish()
    if form == "device" and not reuse:
        got = {i: d[i].download(np.uint8, total) for i in out}
    ses.free()
    ec.free()
    return got, res


def check(ctx, oracle, ec_oracle, k, m, erased, fam, metas, sizes, total, chunks, **kw):
    ems, ecrc, est = expected(oracle, ec_oracle, k, m, erased, fam, metas, sizes, total)
    got, (crc, st, nbad, rc) = run(ctx, k, m, erased, fam, metas, sizes, total, chunks, **kw)
    assert rc == 0
    assert sorted(got) == sorted(plan_of(k, m, erased)[1])
    for i, a in got.items():
        diff = np.nonzero(a != ems[i])[0]
        assert diff.size == 0, (i, int(diff[0]), int(diff.size))
    flat = [(i, x) for i in range(k) for x in metas[i]]
    bad = np.nonzero(st != est)[0]
    assert bad.size == 0, [(int(j), flat[j], int(st[j]), int(est[j])) for j in bad[:5]]
    bad = np.nonzero(crc != ecrc)[0]
    assert bad.size == 0, [(int(j), flat[j], hex(crc[j]), hex(ecrc[j])) for j in bad[:5]]
    assert nbad == int((est != 0).sum())
    return got, crc, st


def sizes_of(k, erased, imgs, total):
    """block_len of the alive data members; a lost member's records are checked against total."""
    return [imgs[i].size if erased[i] == 0 else total for i in range(k)]


def member_slices(metas):
    at, out = 0, []
    for mt in metas:
        out.append(slice(at, at + len(mt)))
        at += len(mt)
    return out


PATTERNS = [
    (5, 3, erased_of(5, 3, {1}), "one data member"),
    (5, 3, erased_of(5, 3, {1, 3, 5}), "two data, one parity"),
    (5, 3, erased_of(5, 3, {5, 6, 7}), "all parity: no output walk"),
    (5, 3, erased_of(5, 3, {0, 1, 2}), "three data: parity among the sources"),
    (2, 1, erased_of(2, 1, {0}), "2+1"),
    (8, 4, erased_of(8, 4, {0, 2, 5, 7}), "a full output group of data"),
    (6, 6, erased_of(6, 6, {0, 1, 2, 3, 4, 5}), "data outputs in the second launch"),
    (5, 3, [0, 0, -1, 0, 0, 0, 1, 0], "an unused data member"),
]


@pytest.mark.parametrize("k,m,erased,what", PATTERNS, ids=[p[3] for p in PATTERNS])
def test_coders_and_erasures(gpu_ctx, oracle, ec_oracle, k, m, erased, what):
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode
    lens = [70001, 40960, 65536 + 1024, 57344 - 7, 49152 + 300]
    imgs, metas = family(oracle, k, 20 * k + m, lens)
    total = up(max(a.size for a in imgs), 1024)
    fam = encode_family(ec_oracle, k, m, imgs, total)
    metas = [mt if erased[i] != -1 else mt[:0] for i, mt in enumerate(metas)]  # an unused member has no records
    sizes = sizes_of(k, erased, imgs, total)
    got, gcrc, st = check(gpu_ctx, oracle, ec_oracle, k, m, erased, fam, metas, sizes, total, chunks_of(total, 16384))
    assert (st == 0).all() and len(st) > 5 * (k - 1)
    for i, a in got.items():                       # the rebuilt bytes are the originals, zero-extended to total
        assert (a == fam[i]).all(), i
    # second witnesses: the plain decode, and the block verify of the original images
    src, out = plan_of(k, m, erased)
    d = [crc.DeviceBuffer(gpu_ctx, total).upload(fam[i] if i in src else np.full(total, FILL, np.uint8))
         for i in range(k + m)]
    ec = ErasureCode(gpu_ctx, k, m, erased)
    assert ec.decode_device(d, total) == 0
    gpu_ctx.sync()
    for i in out:
        assert (d[i].download(np.uint8, total) == got[i]).all()
    ec.free()
    for i, sl in enumerate(member_slices(metas)):
        if len(metas[i]):
            c2, s2, _, _ = gpu_ctx.block_verify(imgs[i], metas[i])
            assert (c2 == gcrc[sl]).all() and (s2 == 0).all()


@pytest.mark.parametrize("dead", [{1, 5}, {0, 6}], ids=["rebuilt", "surviving"])
def test_placements(gpu_ctx, oracle, ec_oracle, placements, dead):  # noqa: F811
    """Member 1 holds every placement the walk takes another path for: rebuilt (the output walk) and surviving
    beside a rebuilt member (the source walk).  One chunk, 4 KiB chunks and 16 KiB chunks agree."""
    imgs, metas, total = placements
    assert CHUNK == 16384
    erased = erased_of(5, 3, dead)
    fam = encode_family(ec_oracle, 5, 3, imgs, total)
    sizes = sizes_of(5, erased, imgs, total)
    ref = None
    for chunks, kw in [([(0, total)], {"reuse": False}), (chunks_of(total, 4096), {}), (chunks_of(total, CHUNK), {})]:
        got, crc, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, erased, fam, metas, sizes, total, chunks, **kw)
        assert (st == 0).all()
        if ref is None:
            ref = (got, crc)
        assert all((got[i] == ref[0][i]).all() for i in got) and (crc == ref[1]).all()
    assert all((got[i] == fam[i]).all() for i in got)


@pytest.mark.parametrize("units", [1, 2, 3])
def test_short_last_tile(gpu_ctx, oracle, ec_oracle, units):
    """total is 1, 2, 3 units past a tile; a record of the rebuilt member ends at its last byte, and so does one
    of a survivor."""
    total = 65536 + 1024 * units
    ends = []
    for seed in (40 + units, 60 + units):
        b = Image(oracle, seed).fill(total - 12000)
        b.rec(total - b.pos - FI)
        ends.append(b.image())
        assert ends[-1][0].size == total
    other = Image(oracle, 50 + units).fill(30000).image(30000)
    imgs, metas = [ends[0][0], other[0], ends[1][0]], [ends[0][1], other[1], ends[1][1]]
    erased = erased_of(3, 2, {0, 3})
    fam = encode_family(ec_oracle, 3, 2, imgs, total)
    for clen in (total, 8192):
        got, _, st = check(gpu_ctx, oracle, ec_oracle, 3, 2, erased, fam, metas, sizes_of(3, erased, imgs, total),
                           total, chunks_of(total, clen))
        assert (st == 0).all() and (got[0] == fam[0]).all()


def test_long_record_in_a_rebuilt_member(gpu_ctx, oracle, ec_oracle):
    """One record of 300 KiB (75 tiles: the fold's lanes take more than one step) in the rebuilt member."""
    b = Image(oracle, 90)
    b.rec(5000)
    long_rec = b.rec(300 << 10, at=6000 + 3)
    b.rec(777)
    img, mt = b.image()
    img2, mt2 = Image(oracle, 91).fill(100000).image()
    total = up(img.size, 1024)
    erased = erased_of(2, 1, {0})
    fam = encode_family(ec_oracle, 2, 1, [img, img2], total)
    _, crc, st = check(gpu_ctx, oracle, ec_oracle, 2, 1, erased, fam, [mt, mt2], [total, img2.size], total,
                       chunks_of(total, 32768))
    assert (st == 0).all()
    assert crc[long_rec] == ocrc(oracle, 0, img[6003 + FI:6003 + FI + (300 << 10)].tobytes())


@pytest.fixture(scope="module")
def hurt_family(oracle, ec_oracle):
    """(5, 3) with data 1, data 3 and parity 0 lost: sources are data 0, 2, 4 and parity 1, 2."""
    imgs, metas = family(oracle, 5, 500, [66000, 61440, 70001, 58000])
    total = up(max(a.size for a in imgs), 1024)
    return imgs, metas, total, encode_family(ec_oracle, 5, 3, imgs, total), erased_of(5, 3, {1, 3, 5})


def hurt_until(oracle, ec_oracle, hurt_family, member, candidates, want_members):
    """Flip one byte of survivor `member`, trying the candidate offsets in turn until the oracle shows at least one
    record failing in each of want_members.  Returns (family, expected status)."""
    imgs, metas, total, fam, erased = hurt_family
    sizes = sizes_of(5, erased, imgs, total)
    sl = member_slices(metas)
    for x in candidates:
        f2 = [a.copy() for a in fam]
        f2[member][x] ^= 0x40
        _, _, est = expected(oracle, ec_oracle, 5, 3, erased, f2, metas, sizes, total)
        if all((est[sl[i]] != 0).any() for i in want_members):
            return f2, est
    raise AssertionError("no candidate byte hurts a record in each of %r" % (want_members,))


def test_corrupt_surviving_data_member(gpu_ctx, oracle, ec_oracle, hurt_family):
    """A flipped payload byte of survivor 2: that record, plus exactly the rebuilt records the oracle's decode
    of the corrupted bytes says are hit."""
    imgs, metas, total, fam, erased = hurt_family
    sl = member_slices(metas)
    r = metas[2][len(metas[2]) // 2]
    cands = [int(r["offset"]) + FI + 100 + 131 * j for j in range(6)]
    f2, est = hurt_until(oracle, ec_oracle, hurt_family, 2, cands, (1, 2, 3))
    assert int((est[sl[2]] != 0).sum()) == 1 and (est[sl[0]] == 0).all() and (est[sl[4]] == 0).all()
    for clen in (total, 16384):
        got, _, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, erased, f2, metas, sizes_of(5, erased, imgs, total), total,
                           chunks_of(total, clen))
        assert (st == est).all() and (got[1] != fam[1]).any() and (got[3] != fam[3]).any()


def test_corrupt_surviving_parity_source(gpu_ctx, oracle, ec_oracle, hurt_family):
    """A flipped byte of parity 1, a source: only rebuilt records fail, the survivors' all pass."""
    imgs, metas, total, fam, erased = hurt_family
    sl = member_slices(metas)
    f2, est = hurt_until(oracle, ec_oracle, hurt_family, 6, [30000 + 517 * j for j in range(6)], (1, 3))
    assert all((est[sl[i]] == 0).all() for i in (0, 2, 4))
    _, _, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, erased, f2, metas, sizes_of(5, erased, imgs, total), total,
                     chunks_of(total, 16384))
    assert (st == est).all() and (st[sl[1]] != 0).any() and (st[sl[3]] != 0).any()


def test_wrong_index_entries_of_the_lost_member(gpu_ctx, oracle, ec_oracle, hurt_family):
    """The parity block's copy of the lost member's index disagrees with the rebuilt FileInfo."""
    imgs, metas, total, fam, erased = hurt_family
    sl = member_slices(metas)
    mt = [a.copy() for a in metas]
    mt[1]["file_id"][2] += 1
    mt[1]["size"][4] -= 1
    mt[3]["file_id"][0] ^= 1 << 40
    _, _, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, erased, fam, mt, sizes_of(5, erased, imgs, total), total,
                     chunks_of(total, 16384))
    assert st[sl[1]][2] == INFO_ERR and st[sl[1]][4] == SYNC_ERR and st[sl[3]][0] == INFO_ERR
    assert int((st != 0).sum()) == 3


def test_rejected_before_the_pass(gpu_ctx, oracle, ec_oracle):
    """size <= 36, a record past sizes[i], a negative offset, in the lost member's index and in a survivor's:
    reported from begin, and the neighbours still verified."""
    from tfs_amd.crc import META_DTYPE
    imgs, metas = family(oracle, 2, 200, [60000, 50000])
    total = up(60000, 1024)
    fam = encode_family(ec_oracle, 2, 1, imgs, total)
    erased = erased_of(2, 1, {0})
    sizes = [imgs[0].size, imgs[1].size]  # the lost member's block_len is known here
    out = []
    for i in range(2):
        mt = metas[i].tolist()
        mt.insert(3, (999, mt[3][1] - 40, 36))
        mt.insert(1, (998, -5, 100))
        mt.append((996, imgs[i].size - 100, 101))
        mt.append((995, imgs[i].size + 4096, 50))
        out.append(np.array(mt, META_DTYPE))
    _, _, st = check(gpu_ctx, oracle, ec_oracle, 2, 1, erased, fam, out, sizes, total, chunks_of(total, 8192))
    for sl, mt in zip(member_slices(out), metas):
        got = st[sl].tolist()
        assert got[1] == PARAM and got[4] == SIZE_ERR and got[-2:] == [PARAM, PARAM] and got.count(0) == len(mt)


def test_host_form_against_device_form(gpu_ctx, oracle, ec_oracle, hurt_family):
    imgs, metas, total, fam, erased = hurt_family
    f2 = [a.copy() for a in fam]
    f2[0][int(metas[0][3]["offset"]) + FI + 7] ^= 1
    sizes = sizes_of(5, erased, imgs, total)
    a, ca, sa = check(gpu_ctx, oracle, ec_oracle, 5, 3, erased, f2, metas, sizes, total, chunks_of(total, 16384))
    b, cb, sb = check(gpu_ctx, oracle, ec_oracle, 5, 3, erased, f2, metas, sizes, total, chunks_of(total, 16384),
                      form="host")
    assert (ca == cb).all() and (sa == sb).all() and (sa != 0).any()
    assert all((a[i] == b[i]).all() for i in a)


def test_call_level_errors(gpu_ctx, oracle, ec_oracle):
    """Every refused call launches nothing: the output buffers keep their fill, and the session still completes."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, ReinstateSession
    imgs, metas = family(oracle, 2, 400, [66000, 70000])
    total = 70656
    fam = encode_family(ec_oracle, 2, 1, imgs, total)
    erased = [1, 0, 0]
    sizes = [total, imgs[1].size]
    ec = ErasureCode(gpu_ctx, 2, 1, erased)
    assert ec.rc == 0

    def begin(mt=metas, sz=sizes, tot=total, coder=ec):
        s = ReinstateSession(coder, mt, sz, tot)
        rc = s.rc
        if rc:
            assert not s.h.value
        s.free()
        return rc
    assert begin() == 0
    enc_only = ErasureCode(gpu_ctx, 2, 1)
    assert begin(coder=enc_only) == MATRIX_INVALID                       # no decoding matrix
    enc_only.free()
    nothing = ErasureCode(gpu_ctx, 2, 1, [0, 0, 0])
    assert nothing.rc == 0 and begin(coder=nothing) == PARAM             # nothing to reinstate
    nothing.free()
    unused = ErasureCode(gpu_ctx, 2, 1, [0, -1, 0])
    assert unused.rc == 0 and begin(coder=unused) == PARAM               # metas on an unused member
    assert begin(coder=unused, mt=[metas[0], metas[1][:0]], sz=[imgs[0].size, total]) == 0
    unused.free()
    assert begin(tot=total + 100) == SIZE_INVALID and begin(tot=0) == SIZE_INVALID
    assert begin(sz=[total + 1, sizes[1]]) == DATA_INVALID
    over = metas[0].copy()
    over["size"][1] += 1
    assert begin(mt=[over, metas[1]]) == PARAM                           # overlapping
    swapped = metas[1].copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    assert begin(mt=[metas[0], swapped]) == PARAM                        # unsorted
    h = ctypes.c_void_p()
    assert ec.L.tfs_ec_reinstate_begin(None, None, None, None, total, ctypes.byref(h)) == PARAM
    # the chunk rules; the plan reads members 1 and 2 and rebuilds member 0
    ses = ReinstateSession(ec, metas, sizes, total)
    d = [crc.DeviceBuffer(gpu_ctx, total).upload(np.full(total, FILL, np.uint8)),
         crc.DeviceBuffer(gpu_ctx, total).upload(fam[1]), crc.DeviceBuffer(gpu_ctx, total).upload(fam[2])]

    def at(o):
        return [b.ptr + o for b in d]
    s1, s2 = gpu_ctx.stream_create(), gpu_ctx.stream_create()
    try:
        assert ses.decode_device(at(4096), 4096, 4096, stream=s1) == PARAM      # the first chunk is at 0 (skipped)
        assert ses.decode_device(at(0), 0, 8192, stream=2) == PARAM             # hipStreamPerThread
        assert ses.decode_device(at(0), 0, 1000, stream=s1) == PARAM            # len % 1024
        assert ses.decode_device(at(0), 0, 5120, stream=s1) == PARAM            # len % 4096 before the end
        assert ses.decode_device(at(0), 0, 0, stream=s1) == PARAM
        assert ses.decode_device(at(0), 0, total + 1024, stream=s1) == PARAM    # overlong
        assert ses.decode_device([d[0].ptr, None, d[2].ptr], 0, 8192, stream=s1) == DATA_INVALID  # a NULL source
        assert ses.decode_device([None, d[1].ptr, d[2].ptr], 0, 8192, stream=s1) == DATA_INVALID  # a NULL output
        assert ses.finish()[3] == PARAM                                         # nothing covered yet
        gpu_ctx.sync()
        assert (d[0].download(np.uint8, total) == FILL).all()
        assert ses.decode_device(at(0), 0, 8192, stream=s1) == 0
        assert ses.decode_device(at(0), 0, 8192, stream=s1) == PARAM            # repeated
        assert ses.decode_device(at(12288), 12288, 4096, stream=s1) == PARAM    # skipped
        assert ses.decode_device(at(8192 + 512), 8192 + 512, 4096, stream=s1) == PARAM  # misaligned
        assert ses.decode_device(at(8192), 8192, 4096, stream=s2) == PARAM      # a second stream
        assert ses.decode_device(at(8192), 8192, 4096, stream=None) == PARAM    # the context's stream is another one too
        assert ses.decode([np.zeros(4096, np.uint8)] * 3, 8192, 4096) == PARAM  # and so is the host form's
        assert ses.finish()[3] == PARAM                                         # before the end
        gpu_ctx.stream_sync(s1)
        assert (d[0].download(np.uint8, total)[8192:] == FILL).all()
        assert ses.decode_device(at(8192), 8192, 2048, stream=s1) == PARAM      # offset + len != total
        assert ses.decode_device(at(8192), 8192, total - 8192, stream=s1) == 0  # 1 KiB units to the end
        crc_, st, nbad, rc = ses.finish()
        assert rc == 0 and (st == 0).all() and nbad == 0 and len(st) == len(metas[0]) + len(metas[1])
        assert (d[0].download(np.uint8, total) == fam[0]).all()
        assert ses.decode_device(at(0), 0, 8192, stream=s1) == PARAM            # a finished session takes no chunk
    finally:
        ses.free()
        gpu_ctx.stream_destroy(s1)
        gpu_ctx.stream_destroy(s2)
        ec.free()


def test_no_records_is_the_plain_decode(gpu_ctx, oracle, ec_oracle):
    import tfs_amd.crc as crc
    imgs = [synth_bytes(900 + i, n) for i, n in enumerate((70000, 65536, 1))]
    total = 70656
    fam = encode_family(ec_oracle, 3, 2, imgs, total)
    erased = erased_of(3, 2, {1, 4})
    got, _, st = check(gpu_ctx, oracle, ec_oracle, 3, 2, erased, fam, [np.zeros(0, crc.META_DTYPE)] * 3,
                       sizes_of(3, erased, imgs, total), total, chunks_of(total, 4096))
    assert len(st) == 0 and (got[1] == fam[1]).all() and (got[4] == fam[4]).all()
