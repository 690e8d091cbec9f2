"""Task chunk calls of the reinstate session (include/tfs_ec_fetch.h): one
call takes every survivor's chunk -- data and parity members alike -- as the
RespReadRawDataMessage frames it arrived in, checks each frame, decodes the chunk from the
frames' data bytes (zeros behind a short data member's), verifies every record and leaves
every dead member's WriteRawDataMessage frames sealed.

Expected frames come from the oracles (jerasure's decode of the survivors as they are,
oracle_crc over each incoming and outgoing frame body); the plain reinstate session is the
second witness for CRCs and statuses."""
import pytest

import ec_fetch_expect as F
import ec_frames_expect as X
from test_ec_fetch import MORE
from test_ec_frames import bids, pids
from test_marshal import chunks_of, family, up
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode and decode)
from test_reinstate import encode_family, erased_of, expected, plan_of
from test_reinstate import run as plain_run

pytestmark = pytest.mark.gpu

ERROR, CRC_ERR = -1, -1010


def build(oracle, ec_oracle, k, m, dead, seed, lens=MORE):
    imgs, metas = family(oracle, k, seed, lens)
    total = up(max(a.size for a in imgs), 1024)
    fam = encode_family(ec_oracle, k, m, imgs, total)
    erased = erased_of(k, m, dead)
    sizes = [total if erased[i] else imgs[i].size for i in range(k)]
    return imgs, metas, total, fam, erased, sizes


def session(ctx, oracle, k, m, erased, fam, metas, sizes, total, frame_len, fpc, stride=0, **kw):
    """The survivors' frames carry block_len bytes of a data member and `total` bytes of a parity member."""
    from tfs_amd.ec import ErasureCode, ReinstateSession, frames_cfg
    ec = ErasureCode(ctx, k, m, erased)
    ses = ReinstateSession(ec, metas, sizes, total)
    assert ec.rc == 0 and ses.rc == 0
    src, out = plan_of(k, m, erased)
    cfg = frames_cfg(frame_len, bids(k + m), pids(k + m), stride)
    sources = {i: fam[i][:sizes[i]] if i < k else fam[i] for i in src}
    try:
        return F.run(ctx, oracle, ses, k + m, sources, out, total, frame_len, fpc, cfg, stride=stride,
                     padded={i: fam[i] for i in src}, **kw)
    finally:
        ses.free()
        ec.free()


def frames_of(oracle, ems, k, m, out, frame_len):
    return {i: X.member_frames(oracle, ems[i], frame_len, bids(k + m)[i], pids(k + m)[i], i >= k) for i in out}


@pytest.mark.parametrize("k,m,dead", [(5, 3, [2, 6]), (5, 3, [0, 3, 5]), (6, 6, [0, 1, 2, 3, 4])])
def test_dead_sets(gpu_ctx, oracle, ec_oracle, k, m, dead):
    """A dead data member plus a dead parity member; two data and one parity; five dead of (6, 6): two output
    groups, a rebuilt data member in the second.  Data and parity survivors are the sources."""
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, k, m, dead, 100 * k + len(dead))
    ems, ecrc, est = expected(oracle, ec_oracle, k, m, erased, fam, metas, sizes, total)
    _, pres = plain_run(gpu_ctx, k, m, erased, fam, metas, sizes, total, chunks_of(total, 16384))
    src, out = plan_of(k, m, erased)
    assert sorted(out) == sorted(dead) and any(i >= k for i in src) and (est == 0).all()
    for frame_len, fpc, in_stride, form in [(4096, 3, 0, "device"), (8192, 1, 8192 + 40, "device"), (4096, 4, 0, "host")]:
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, k, m, erased, fam, metas, sizes, total, frame_len, fpc,
                                                in_stride=in_stride, form=form, null_unread=True)
        assert all(c[5] == 0 for c in calls)
        F.check_calls(gpu_ctx, calls, frames_of(oracle, ems, k, m, out, frame_len), frame_len)
        assert rc == 0 and (crc == pres[0]).all() and (st == pres[1]).all() and nbad == pres[2]
        assert (crc == ecrc).all() and (st == est).all()
    for i in dead:
        assert (ems[i] == fam[i]).all()


def test_mixed_chunks(gpu_ctx, oracle, ec_oracle):
    """Task, frames and plain chunks in one session give the same frames, members and verdicts."""
    dead = [2, 6]
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, 5, 3, dead, 532)
    ems, ecrc, est = expected(oracle, ec_oracle, 5, 3, erased, fam, metas, sizes, total)
    out = plan_of(5, 3, erased)[1]
    calls, others, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, erased, fam, metas, sizes, total, 8192, 2,
                                                 kinds={0: "frames", 3: "plain"})
    F.check_calls(gpu_ctx, calls, frames_of(oracle, ems, 5, 3, out, 8192), 8192)
    assert sorted(others) == [0, 3]
    for c, mem in others.items():
        for i in out:
            assert (mem[i] == ems[i][c * 16384:c * 16384 + mem[i].size]).all()
    assert rc == 0 and (crc == ecrc).all() and (st == est).all() and nbad == 0


# (what, source member, frame of the member, [(byte of the frame, xor)], status)
DAMAGE = [("a parity source's data", 5, 1, [(28 + 100, 0x04)], CRC_ERR),
          ("a parity source's trailer", 5, 0, [(-1, 0x01)], CRC_ERR),
          ("a parity source's pcode", 5, 2, [(8, 0x02)], ERROR),
          ("a data source's last byte", 4, 2, [(28 + 1026, 0x80)], CRC_ERR)]


@pytest.mark.parametrize("what,member,frame,hits,status", DAMAGE, ids=[d[0].replace(" ", "_").replace("'", "") for d in DAMAGE])
def test_damage(gpu_ctx, oracle, ec_oracle, what, member, frame, hits, status):
    """One survivor's frame damaged in flight: that result alone fails, frame j of every dead member is void and every
    other frame is sealed and accepted; the record walk runs over what arrived."""
    dead = [0, 6]
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, 5, 3, dead, 535, [20001, 12288, 2000, 16384, 9219])
    ems, ecrc, est = expected(oracle, ec_oracle, 5, 3, erased, fam, metas, sizes, total)
    src, out = plan_of(5, 3, erased)
    assert src == [1, 2, 3, 4, 5] and member in src and total == 20480
    hurt = [a.copy() for a in fam]
    for pos, x in hits:
        if pos >= 28:
            hurt[member][frame * 4096 + pos - 28] ^= x
    _, hcrc, hst = expected(oracle, ec_oracle, 5, 3, erased, hurt, metas, sizes, total)
    calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, erased, fam, metas, sizes, total, 4096, 3,
                                            damage={(member, frame): hits})
    assert all(c[5] == 0 for c in calls)
    F.check_calls(gpu_ctx, calls, frames_of(oracle, ems, 5, 3, out, 4096), 4096, bad=[(src.index(member), frame, status)])
    assert rc == 0 and (st == hst).all() and (crc == hcrc).all()
    if what == "a parity source's data":  # the rebuilt member's record over those bytes fails, as in the plain session
        assert (hst != est).any()
