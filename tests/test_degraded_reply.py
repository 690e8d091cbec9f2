"""Degraded read replies (include/tfs_ec_read.h) on the GPU: the records of a lost data member
rebuilt from the survivors, verified and sealed into reply frames in one pass.  Every frame byte and result word
is compared with a frame built on the host (tests/degraded_reply_expect.py) and, for the equivalence test, byte
for byte with tfs_read_reply_device over the intact member.  5:3 families of 256 KiB members unless said."""
import struct

import numpy as np
import pytest

import degraded_reply_expect as E
from degraded_reply_expect import CRC_ERR, FI, INFO_ERR, OK, PARAM, SIZE_ERR, SYNC_ERR

pytestmark = pytest.mark.gpu

MEMBER = 256 << 10
PAYLOADS = [0, 1, 7, 8, 9, 35, 37, 987, 988, 1024, 4059, 4060, 4061, 32731, 32732, 32733, 70001]


@pytest.fixture(scope="module")
def ecl():
    return E.ec_lib()


@pytest.fixture(scope="module")
def eq_member(oracle):
    """The equivalence member: every payload length, FileInfos that straddle a 128-byte packet edge (H mod 128 =
    100, 120) and a 1 KiB unit edge (H mod 1024 = 1000, 1020), and plain ones."""
    m = E.Member(oracle, seed=3)
    places = [(128, 100), (1024, 1000), (8, 3), (128, 120), (1024, 1020), (1024, 0), (16, 9)]
    for k, n in enumerate(PAYLOADS):
        m.at(*places[k % len(places)], n)
    assert m.pos <= MEMBER
    hs = [off for _, off, _ in m.recs]
    assert any(h % 128 > 92 for h in hs) and any(h % 1024 > 988 for h in hs)
    return m, m.image(MEMBER)


def coder(ctx, k, m, erased):
    from tfs_amd.ec import ErasureCode
    dec = ErasureCode(ctx, k, m, erased)
    assert dec.rc == 0
    return dec


@pytest.mark.parametrize("also", [(), (0, 6)], ids=["target", "target+data+parity"])
def test_equivalence(gpu_ctx, oracle, eq_member, also):
    m, img = eq_member
    fam = E.Family(gpu_ctx, 5, 3, 2, img)
    er = fam.erased(also)
    dec = coder(gpu_ctx, 5, 3, er)
    for pcode in E.PCODES:
        jobs, cap = E.packed(m.recs, pcode=pcode, align_to=0)
        res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, cap, intact=True)
        assert (res["status"] == OK).all()
    dec.free()


@pytest.mark.parametrize("k,mm", [(2, 1), (10, 2), (8, 4)])
def test_equivalence_other_geometries(gpu_ctx, oracle, eq_member, k, mm):
    """2:1, and the two widest geometries that reach 10 data or 4 parity members: a family has at most 12
    (TFS_EC_MAX_MEMBERS, the reference's MAX_MARSHALLING_NUM), so 10:4 itself is refused by tfs_ec_config."""
    from tfs_amd.ec import ErasureCode
    assert ErasureCode(gpu_ctx, 10, 4).rc == PARAM
    m, img = eq_member
    fam = E.Family(gpu_ctx, k, mm, k - 1, img, seed=9 * k)
    er = fam.erased()
    dec = coder(gpu_ctx, k, mm, er)
    jobs, cap = E.packed(m.recs, pcode=[E.PCODES[i % 3] for i in range(len(m.recs))], align_to=0)
    res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, cap, intact=True)
    assert (res["status"] == OK).all()
    dec.free()


@pytest.mark.parametrize("nbytes", [100, 5000])
def test_alignment_all_128_pairs(gpu_ctx, oracle, nbytes):
    """All 16 frame_offset mod 16 x all 8 H mod 8, frames back to back over a prefilled buffer, the last one
    ending on the last byte of out; every byte outside the spans unchanged."""
    m = E.Member(oracle, seed=11 + nbytes)
    for h in range(8):
        for _ in range(16):
            m.at(8, h, nbytes)
    img = m.image()
    assert img.size <= 1 << 20
    fam = E.Family(gpu_ctx, 5, 3, 0, img)
    er = fam.erased()
    dec = coder(gpu_ctx, 5, 3, er)
    specs, fo = [], 5
    for k, (fid, off, size) in enumerate(m.recs):
        fo += (k % 16 - fo) % 16                      # frame_offset mod 16 = k mod 16, gaps of prefill between
        s = dict(src_offset=off, frame_offset=fo, file_id=fid, size=size, pcode=E.PCODES[k % 3])
        specs.append(s)
        fo += E.cap_of(E.make_jobs([s])[0])
    jobs = E.make_jobs(specs)
    assert {(int(j["frame_offset"]) % 16, int(j["src_offset"]) % 8) for j in jobs} == \
        {(a, b) for a in range(16) for b in range(8)}
    res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, fo)
    assert (res["status"] == OK).all()
    # packed back to back, every alignment as it falls
    jobs, cap = E.packed(m.recs, start=1)
    res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, cap)
    assert (res["status"] == OK).all()
    dec.free()


@pytest.fixture(scope="module")
def slice_family(gpu_ctx, oracle):
    m = E.Member(oracle, seed=21)
    m.at(1024, 1000, 150000)    # a long record whose FileInfo straddles a unit edge
    m.at(1024, 10, 900)         # a record inside one unit
    m.at(128, 60, 40000)
    img = m.image(MEMBER)
    return m, E.Family(gpu_ctx, 5, 3, 1, img)


def test_slices(gpu_ctx, oracle, slice_family):
    m, fam = slice_family
    er = fam.erased()
    dec = coder(gpu_ctx, 5, 3, er)
    long_, small, mid = m.recs
    cases = []
    for rec, ro, rl in [(long_, 1, 10), (long_, 100000, 1 << 20),      # cut at the payload's end
                        (long_, 149999, 5), (long_, 150000, 7),        # the last byte; at the end: n = 0
                        (small, 100, 50), (small, 5, 890),             # a slice inside one unit
                        (long_, 70000, 3000), (long_, 131072 - 1036 - 8, 16),   # units disjoint from the header's
                        (long_, 3000, 1), (long_, 2012, 4096),         # touching: the slice starts in the next unit
                        (long_, 0, 0), (small, 0, 0), (mid, 20000, 0),  # read_len == 0: the degrade stat
                        (mid, 0, 40000), (mid, 0, 39999), (mid, 1, 39999), (mid, 4036 - 60, 8192)]:
        for pcode in E.PCODES:
            cases.append(dict(rec=rec, read_offset=ro, read_len=rl, pcode=pcode))
    recs = [c.pop("rec") for c in cases]
    jobs, cap = E.packed(recs, start=2, read_offset=[c["read_offset"] for c in cases],
                         read_len=[c["read_len"] for c in cases], pcode=[c["pcode"] for c in cases])
    res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, cap, intact=True)
    assert (res["status"] == OK).all()
    # version 0: no header CRC
    jobs, cap = E.packed(m.recs, version=0, pcode=[8, 39, 63])
    res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, cap, intact=True)
    assert (res["frame_crc"] == 0).all() and (res["status"] == OK).all()
    dec.free()


def _status_family(gpu_ctx, oracle):
    m = E.Member(oracle, seed=31)
    ids = dict(good=m.at(1024, 100, 3000), bad_id=m.at(1024, 200, 3000), bad_size=m.at(1024, 300, 3000),
               victim=m.at(4096, 700, 6000), deleted=m.at(1024, 50, 2000, flag=E.DELETED),
               concealed=m.at(128, 90, 5000, flag=E.CONCEAL), bad_crc=m.at(1024, 400, 2500, crc_xor=0x10),
               other=m.at(4096, 100, 9000))
    img = m.image(MEMBER)
    img[m.recs[ids["bad_id"]][1]] ^= 1            # FileInfo.id_
    img[m.recs[ids["bad_size"]][1] + 12] ^= 4     # FileInfo.size_
    return m, ids, E.Family(gpu_ctx, 5, 3, 1, img)


def _status_cases(m, ids, fam):
    """(spec, expected status) of every per-job status; frame_offset is set by the caller."""
    r = {k: m.recs[v] for k, v in ids.items()}

    def job(name, **kw):
        fid, off, size = r[name]
        return dict(src_offset=off, file_id=fid, size=size, **kw)
    refuse = E.DELETED | E.INVALID | E.CONCEAL
    return [
        (job("good"), OK), (job("bad_id"), INFO_ERR), (job("bad_size", pcode=8), SYNC_ERR),
        (job("bad_crc", pcode=63), CRC_ERR), (job("bad_crc", read_offset=1, read_len=100), OK),
        (job("victim"), CRC_ERR), (job("victim", pcode=8), CRC_ERR), (job("other"), OK),
        # refuse_flags hit and not hit, on the first and on a later fragment
        (job("deleted", refuse_flags=refuse), INFO_ERR), (job("deleted", refuse_flags=E.INVALID), OK),
        (job("deleted", refuse_flags=refuse, read_len=10), INFO_ERR),
        (job("deleted", refuse_flags=refuse, read_offset=5, read_len=10), OK),
        (job("concealed", refuse_flags=refuse, pcode=8), INFO_ERR), (job("concealed", refuse_flags=0), OK),
        (job("good", refuse_flags=refuse), OK),
        # short records, and every parameter error
        (dict(job("good"), size=35), SIZE_ERR), (dict(job("good"), size=0, pcode=8), SIZE_ERR),
        (job("good", pcode=9), PARAM), (job("good", read_offset=-1), PARAM), (job("good", read_len=-1), PARAM),
        (job("good", read_offset=3001), PARAM), (job("good", read_offset=3000), OK),   # past / at the payload's end
        (dict(job("good"), src_offset=fam.size - 1000, size=1001), PARAM),     # the record passes size
        (dict(job("good"), src_offset=fam.size + 1024, size=100), PARAM),
        (dict(job("good"), frame_offset=-1), PARAM),                           # the span passes out_cap (set below)
    ]


def _hurt(fam, m, ids):
    hurt = [a.copy() for a in fam.members]
    hurt[3][m.recs[ids["victim"]][1] + FI + 2500] ^= 0x40      # a survivor byte under the victim's payload
    hurt[4][MEMBER - 700] ^= 0x08                              # and one in a unit no job covers
    return hurt


def _lay(cases, start=7):
    specs, fo = [], start
    for s, _ in cases:
        s = dict(s)
        if s.get("frame_offset") != -1:
            s["frame_offset"] = fo
            fo += max(E.cap_of(E.make_jobs([s])[0]), 0)
        specs.append(s)
    for s in specs:
        if s.get("frame_offset") == -1:
            s["frame_offset"] = max(fo - 10, 0)     # cap_of > 10: the span passes out_cap
    return E.make_jobs(specs), fo


def _verify_error_frames(ctx, out, jobs, res):
    """Every error frame passes tfs_packet_verify and carries the status."""
    fr = [(int(j["frame_offset"]), int(r["frame_len"])) for j, r in zip(jobs, res) if r["status"] not in (OK, PARAM)]
    assert fr
    crc, st, nbad = ctx.packet_verify(out, [o for o, _ in fr], [n for _, n in fr])[:3]
    assert nbad == 0 and (np.asarray(st) == 0).all()
    for (o, n), r in zip(fr, [r for r in res if r["status"] not in (OK, PARAM)]):
        assert n in (28, 32) and struct.unpack_from("<i", out, o + 24)[0] == int(r["status"])
        assert n == 28 or struct.unpack_from("<i", out, o + 28)[0] == 0


def test_statuses_mixed_and_alone(gpu_ctx, oracle, ecl):
    m, ids, fam = _status_family(gpu_ctx, oracle)
    er = fam.erased()
    dec = coder(gpu_ctx, 5, 3, er)
    hurt = _hurt(fam, m, ids)
    rebuilt = fam.rebuilt(ecl, er, hurt)
    v = m.recs[ids["victim"]]
    assert (rebuilt[v[1] + FI:v[1] + v[2]] != fam.members[1][v[1] + FI:v[1] + v[2]]).any()
    cases = _status_cases(m, ids, fam)
    jobs, cap = _lay(cases)
    rc, out, res, before, nbad = E.run_device(gpu_ctx, dec, fam, er, jobs, cap, hurt)
    assert rc == 0
    assert nbad == E.check(oracle, rebuilt, jobs, fam.size, out, res, cap, before)
    assert res["status"].tolist() == [st for _, st in cases]
    k = [i for i, (s, _) in enumerate(cases) if s["file_id"] == v[0]][0]
    assert int(res[k]["file_crc"]) == E.zcrc(0, rebuilt[v[1] + FI:v[1] + v[2]].tobytes())   # as recomputed
    _verify_error_frames(gpu_ctx, out, jobs, res)
    for i in range(len(cases)):          # each alone
        j1, c1 = _lay(cases[i:i + 1], start=i % 16)
        rc, out, res, before, nbad = E.run_device(gpu_ctx, dec, fam, er, j1, c1, hurt)
        assert rc == 0 and int(res[0]["status"]) == cases[i][1], i
        assert nbad == E.check(oracle, rebuilt, j1, fam.size, out, res, c1, before)
    dec.free()


def test_call_level(gpu_ctx, oracle):
    from tfs_amd.ec import ErasureCode
    m, ids, fam = _status_family(gpu_ctx, oracle)
    er = fam.erased()
    dec = coder(gpu_ctx, 5, 3, er)
    fid, off, size = m.recs[ids["good"]]
    one = dict(src_offset=off, frame_offset=0, file_id=fid, size=size)
    j1 = E.make_jobs([one])
    c1 = E.cap_of(j1[0])
    ms = fam.survivors(er)
    out = np.zeros(c1 + 64, np.uint8)
    enc_only = ErasureCode(gpu_ctx, 5, 3)
    assert enc_only.read_reply(ms, fam.size, 1, j1, out)[2] == E.MATRIX_INVALID
    enc_only.free()
    assert dec.read_reply(ms, fam.size + 100, 1, j1, out)[2] == E.SIZE_INVALID
    assert dec.read_reply(ms, -1024, 1, j1, out)[2] == E.SIZE_INVALID
    for target in (0, 5, -1):                                       # alive, parity, none
        assert dec.read_reply(ms, fam.size, target, j1, out)[2] == PARAM
    hole = list(ms)
    hole[3] = None
    assert dec.read_reply(hole, fam.size, 1, j1, out)[2] == E.DATA_INVALID
    assert dec.read_reply(ms, fam.size, 1, j1, out, sizes=[fam.size] * 3 + [fam.size - 1024] + [fam.size] * 4)[2] \
        == E.DATA_INVALID
    # the order: a bad size wins over a bad target, a bad target over a NULL source
    assert dec.read_reply(hole, fam.size + 1, 0, j1, out)[2] == E.SIZE_INVALID
    assert dec.read_reply(hole, fam.size, 0, j1, out)[2] == PARAM
    assert E.run_device(gpu_ctx, dec, fam, er, j1, c1, stream=2)[0] == PARAM   # hipStreamPerThread
    hole_fam_members = [a if i != 3 else None for i, a in enumerate(fam.members)]
    import tfs_amd.crc as crc
    d = [None if a is None or er[i] else crc.DeviceBuffer(gpu_ctx, a.size).upload(a)
         for i, a in enumerate(hole_fam_members)]
    d_out, d_res = crc.DeviceBuffer(gpu_ctx, c1 + 16), crc.DeviceBuffer(gpu_ctx, 16)
    assert dec.read_reply_device(d, fam.size, 1, j1, d_out, c1, d_res) == E.DATA_INVALID
    assert dec.read_reply_device(d, fam.size, 1, j1[:0], d_out, c1, d_res) == E.DATA_INVALID   # before n == 0
    # overlapping spans: refused, nothing launched, nothing written
    two = E.make_jobs([one, dict(one, frame_offset=c1 - 1)])
    before = E.prefill(2 * c1)
    rc, o, res, _, _ = E.run_device(gpu_ctx, dec, fam, er, two, 2 * c1)
    assert rc == PARAM
    o2 = before.copy()
    assert dec.read_reply(ms, fam.size, 1, two, o2)[2] == PARAM and (o2 == before).all()
    two["frame_offset"][1] = c1                                       # touching spans are served
    rc, o, res, _, nbad = E.run_device(gpu_ctx, dec, fam, er, two, 2 * c1)
    assert rc == 0 and nbad == 0
    # a refused job's span does not count
    two["frame_offset"][1], two["pcode"][1] = 0, 9
    rc, o, res, _, nbad = E.run_device(gpu_ctx, dec, fam, er, two, 2 * c1)
    assert rc == 0 and res["status"].tolist() == [OK, PARAM] and nbad == 1
    # the plan reads members 0, 2, 3, 4 and the first parity: the other parity members may be missing
    lean = list(ms)
    lean[6] = lean[7] = None
    res, nbad, rc = dec.read_reply(lean, fam.size, 1, j1, out)
    assert rc == 0 and nbad == 0 and int(res[0]["status"]) == OK
    dec.free()


def test_grid_stride_5000_one_tile_jobs(gpu_ctx, oracle):
    """More jobs than the 4,096 workgroups of a launch: they stride."""
    m = E.Member(oracle, seed=41)
    for i in range(5000):
        m.add(1 + (i * 37) % 160)
    img = m.image()
    assert img.size <= 1 << 20
    fam = E.Family(gpu_ctx, 5, 3, 4, img)
    er = fam.erased((1,))
    dec = coder(gpu_ctx, 5, 3, er)
    jobs, cap = E.packed(m.recs, pcode=[E.PCODES[i % 3] for i in range(5000)])
    res = E.check_device(gpu_ctx, oracle, dec, fam, er, jobs, cap)
    assert (res["status"] == OK).all()
    dec.free()


def test_host_form(gpu_ctx, oracle, ecl, eq_member):
    """Pageable and page-locked out give identical bytes; only the covering sets go up and the frames come down."""
    import tfs_amd.crc as crc
    m, img = eq_member
    fam = E.Family(gpu_ctx, 5, 3, 2, img)
    er = fam.erased()
    dec = coder(gpu_ctx, 5, 3, er)
    ms = fam.survivors(er)
    recs = m.recs + [m.recs[-1], m.recs[-1], m.recs[3]]
    ro = [0] * len(m.recs) + [50000, 100, 0]
    rl = [r[2] for r in m.recs] + [3000, 0, 1 << 20]
    jobs, cap = E.packed(recs, start=9, read_offset=ro, read_len=rl, pcode=[E.PCODES[i % 3] for i in range(len(recs))])
    jobs["size"][5] = 20                                            # a short record: an error frame
    jobs["pcode"][6] = 7                                            # a refused job
    before = E.prefill(cap)
    out = before.copy()
    res, nbad, rc = dec.read_reply(ms, fam.size, 2, jobs, out)
    assert rc == CRC_ERR and nbad == 2 == E.check(oracle, img, jobs, fam.size, out, res, cap, before)
    assert res["status"].tolist()[5:7] == [SIZE_ERR, PARAM]
    up, down = dec.read_traffic()
    units = set()
    for j, r in zip(jobs, res):
        if r["status"] in (PARAM, SIZE_ERR):
            continue
        h, d0 = int(j["src_offset"]), int(j["src_offset"]) + FI + int(j["read_offset"])
        n = E.cap_of(j) - 28 - (0 if j["pcode"] == 8 else 40 if j["read_offset"] == 0 else 4)
        units |= set(range(h // 1024, (h + FI + 1023) // 1024))
        if n:
            units |= set(range(d0 // 1024, (d0 + n + 1023) // 1024))
    assert up == 5 * 1024 * len(units) and up < 5 * fam.size
    flen = int(res["frame_len"].astype(np.int64).sum())
    assert flen <= down < flen + 16 * len(jobs)
    pin = crc.PinnedBuffer(gpu_ctx, cap)
    pin.array[:] = before
    res2, nbad2, rc2 = dec.read_reply(ms, fam.size, 2, jobs, pin)
    assert (rc2, nbad2) == (rc, nbad) and res2.tobytes() == res.tobytes()
    assert (pin.array == out).all()
    assert dec.read_traffic() == (up, flen)
    pin.free()
    # a corrupt survivor under the host form: the sealed error frame
    hurt = [a.copy() for a in fam.members]
    hurt[0][m.recs[-1][1] + 40000] ^= 1
    rebuilt = fam.rebuilt(ecl, er, hurt)
    out = before.copy()
    res, nbad, rc = dec.read_reply(fam.survivors(er, hurt), fam.size, 2, jobs, out)
    assert rc == CRC_ERR and nbad == E.check(oracle, rebuilt, jobs, fam.size, out, res, cap, before) == 3
    assert int(res[len(m.recs) - 1]["status"]) == CRC_ERR
    dec.free()
