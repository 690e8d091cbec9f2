"""Task chunk calls of the marshalling session (include/tfs_ec_fetch.h):
one call takes every data member's chunk as the RespReadRawDataMessage frames it arrived
in, checks each frame, encodes the chunk from the frames' data bytes (zeros behind them),
verifies the records and leaves every parity member's WriteRawDataMessage frames sealed.

Expected values come from the oracles (tests/ec_fetch_expect.py and ec_frames_expect.py:
jerasure's parity over the zero-padded members, oracle_crc over each incoming and outgoing
frame body); the plain marshalling session is the second witness for the record verdicts.
Every in buffer is garbage behind each trailer, in every gap and where an unread frame
would lie; every out buffer is prefilled and compared whole, with 64 bytes before the first
frame and behind the call's capacity."""
import numpy as np
import pytest

import ec_fetch_expect as F
import ec_frames_expect as X
from test_ec_frames import LENS, bids, pids
from test_marshal import Image, chunks_of, expected, family, padded, up
from test_marshal import run as plain_run
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode)

pytestmark = pytest.mark.gpu

OK, ERROR, CRC_ERR, PARAM = 0, -1, -1010, -1016
DATA_INVALID, SIZE_INVALID = -16001, -16002
# test_ec_frames' lengths (n % 8 of the last frames: 1, 0, 0, 1), a member that ends on a tile's end inside an 8 KiB
# frame, one shorter than the first frame, and last frames with n % 8 = 2 .. 7
MORE = [70001, 36864, 2000, 98304, 65536 + 1024, 81920 - 7, 40962, 40963, 40964, 40965, 40966, 40967]
assert set(LENS) <= set(MORE)


def session(ctx, oracle, k, m, imgs, metas, total, frame_len, fpc, stride=0, version=2, **kw):
    from tfs_amd.ec import ErasureCode, MarshalSession, frames_cfg
    ec = ErasureCode(ctx, k, m)
    ses = MarshalSession(ec, metas, [a.size for a in imgs], total)
    assert ec.rc == 0 and ses.rc == 0
    cfg = frames_cfg(frame_len, bids(k + m), pids(k + m), stride, version)
    try:
        return F.run(ctx, oracle, ses, k + m, {i: imgs[i] for i in range(k)}, list(range(k, k + m)), total, frame_len, fpc,
                     cfg, stride=stride, version=version, padded=dict(enumerate(padded(imgs, total))), **kw)
    finally:
        ses.free()
        ec.free()


def frames_of(oracle, epar, k, m, frame_len, version=2):
    return {k + p: X.member_frames(oracle, epar[p], frame_len, bids(k + m)[k + p], pids(k + m)[k + p], True, version)
            for p in range(m)}


@pytest.fixture(scope="module")
def fam53(oracle, ec_oracle):
    imgs, metas = family(oracle, 5, 53, MORE)
    total = up(max(a.size for a in imgs), 1024)
    return imgs, metas, total, expected(oracle, ec_oracle, 5, 3, imgs, metas, total)


@pytest.fixture(scope="module")
def small(oracle, ec_oracle):
    """Five short members for the damage cases: 5 frames of 4096; member 4's last frame carries 1027 bytes."""
    imgs, metas = family(oracle, 5, 530, [20001, 12288, 2000, 16384, 9219])
    total = up(max(a.size for a in imgs), 1024)
    assert total == 20480 and len(metas[0]) >= 1
    return imgs, metas, total, expected(oracle, ec_oracle, 5, 3, imgs, metas, total)


@pytest.mark.parametrize("k,m", [(2, 1), (5, 3), (8, 4), (6, 6)])
def test_coders(gpu_ctx, oracle, ec_oracle, k, m):
    """(6, 6) takes two output groups.  Frame lengths 4096 and 8192, one and three frames per call, default and wide
    in_stride; NULL for a member whose whole call lies past its end."""
    imgs, metas = family(oracle, k, 10 * k + m, MORE[:max(k, 6)] if k != 8 else MORE)
    total = up(max(a.size for a in imgs), 1024)
    epar, ecrc, est = expected(oracle, ec_oracle, k, m, imgs, metas, total)
    ppar, pres = plain_run(gpu_ctx, k, m, imgs, metas, total, chunks_of(total, 16384), reuse=False)
    for frame_len, fpc, in_stride, null in [(4096, 1, 0, True), (4096, 3, 4096 + 48, False), (8192, 3, 0, True),
                                            (8192, 1, 16384, False)]:
        frames = frames_of(oracle, epar, k, m, frame_len)
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, k, m, imgs, metas, total, frame_len, fpc,
                                                in_stride=in_stride, null_unread=null)
        assert all(c[5] == 0 for c in calls)
        F.check_calls(gpu_ctx, calls, frames, frame_len)
        assert rc == 0 and (crc == pres[0]).all() and (st == pres[1]).all() and nbad == pres[2]
        assert (crc == ecrc).all() and (st == est).all()
        # frames that must not be read: SUCCESS with n = 0, whatever lay there
        assert any((c[4]["n"] == 0).any() for c in calls)


@pytest.mark.parametrize("form", ["pinned", "host"])
def test_host_forms(gpu_ctx, oracle, fam53, form):
    """Page-locked (read and written in place) and pageable (frames at any address), wide strides included."""
    imgs, metas, total, (epar, ecrc, est) = fam53
    frames = frames_of(oracle, epar, 5, 3, 4096)
    for stride, in_stride in ((0, 0), (4096 + 128, 4096 + 56)):
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, imgs, metas, total, 4096, 5, stride=stride,
                                                in_stride=in_stride, form=form, null_unread=stride == 0)
        assert all(c[5] == 0 for c in calls)
        F.check_calls(gpu_ctx, calls, frames, 4096, stride)
        assert rc == 0 and (crc == ecrc).all() and (st == est).all() and nbad == 0


@pytest.mark.parametrize("units", [1, 2, 3])
def test_short_last_tile(gpu_ctx, oracle, ec_oracle, units):
    """total = 4096 k + 1024 u: the last frame ends in a short tile; a record up to the longest member's last byte."""
    total = 32768 + 1024 * units
    b = Image(oracle, 40 + units).fill(total - 12000)
    b.rec(total - b.pos - 36)
    img, mt = b.image()
    imgs, metas = family(oracle, 2, 50 + units, [total - 1024 * units - 3, 30000])
    imgs, metas = imgs + [img], metas + [mt]
    epar, ecrc, est = expected(oracle, ec_oracle, 3, 2, imgs, metas, total)
    for frame_len, fpc in ((4096, 5), (8192, 1), (8192, 1 << 10)):
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 3, 2, imgs, metas, total, frame_len, fpc)
        F.check_calls(gpu_ctx, calls, frames_of(oracle, epar, 3, 2, frame_len), frame_len)
        assert rc == 0 and (crc == ecrc).all() and (st == est).all() and (st == 0).all()


@pytest.mark.parametrize("total,frame_len", [(3072, 4096), (1024, 8192), (8192, 8192)])
def test_totals_up_to_one_frame(gpu_ctx, oracle, ec_oracle, total, frame_len):
    b = Image(oracle, total)
    b.rec(500, at=17)
    img, mt = b.image(total - 5)
    imgs, metas = [img, img[:900].copy()], [mt, mt]
    epar, ecrc, est = expected(oracle, ec_oracle, 2, 2, imgs, metas, total)
    calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 2, 2, imgs, metas, total, frame_len, 1)
    assert len(calls) == 1 and list(calls[0][4]["n"][:, 0]) == [total - 5, 900]
    F.check_calls(gpu_ctx, calls, frames_of(oracle, epar, 2, 2, frame_len), frame_len)
    assert rc == 0 and (crc == ecrc).all() and (st == est).all()


def test_version0_no_records_and_mixed_chunks(gpu_ctx, oracle, fam53):
    imgs, metas, total, (epar, ecrc, est) = fam53
    # version 0 in and out: no CRC judged (the field is 0 and wrong), the CRC field of the outputs is 0
    f0 = frames_of(oracle, epar, 5, 3, 8192, version=0)
    calls, _, (crc, st, _, rc) = session(gpu_ctx, oracle, 5, 3, imgs, metas, total, 8192, 2, version=0)
    F.check_calls(gpu_ctx, calls, f0, 8192, verify=False)
    assert all(f[20:24] == b"\0\0\0\0" for f in f0[5]) and rc == 0 and (crc == ecrc).all() and (st == est).all()
    # a session with no records still checks the frames and yields the parity's
    f2 = frames_of(oracle, epar, 5, 3, 8192)
    none = [np.zeros(0, metas[0].dtype)] * 5
    calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, imgs, none, total, 8192, 2)
    F.check_calls(gpu_ctx, calls, f2, 8192)
    assert rc == 0 and len(crc) == 0 and nbad == 0
    # task, frames and plain chunks in one session: the same frames, parity and verdicts
    nch = len(chunks_of(total, 16384))
    calls, others, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, imgs, metas, total, 8192, 2,
                                                 kinds={1: "plain", 2: "frames", nch - 1: "frames"})
    F.check_calls(gpu_ctx, calls, f2, 8192)
    assert len(others) == 3 and len(calls) == nch - 3
    for c, par in others.items():
        for p in range(3):
            assert (par[5 + p] == epar[p][c * 16384:c * 16384 + par[5 + p].size]).all()
    assert rc == 0 and (crc == ecrc).all() and (st == est).all() and nbad == 0


# (what, source member, frame of the member, [(byte of the frame, xor)], status); n of (4, 2) is 1027, of (0, 4) 3617
DAMAGE = [("data first", 0, 1, [(28, 0x01)], CRC_ERR),
          ("data last", 0, 1, [(28 + 4095, 0x80)], CRC_ERR),
          ("data last of a short frame", 0, 4, [(28 + 3616, 0x10)], CRC_ERR),
          ("data in the straddling piece", 4, 2, [(28 + 1025, 0x02)], CRC_ERR),
          ("body le32", 3, 3, [(24, 0x01)], ERROR),
          ("trailer", 1, 2, [(-2, 0x40)], CRC_ERR),
          ("header crc", 2, 0, [(21, 0x08)], CRC_ERR),
          ("flag", 4, 0, [(3, 0x01)], ERROR),
          ("pcode", 1, 0, [(8, 0x01)], ERROR),
          ("header body length", 0, 0, [(5, 0x02)], ERROR),
          ("data and pcode: the lower-numbered check wins", 3, 1, [(28 + 7, 0xFF), (8, 0x40)], ERROR)]


@pytest.mark.parametrize("what,member,frame,hits,status", DAMAGE, ids=[d[0].replace(" ", "_") for d in DAMAGE])
def test_damage(gpu_ctx, oracle, ec_oracle, small, what, member, frame, hits, status):
    """One frame damaged in flight: exactly that result fails, frame j of every output is void, every other frame
    is sealed and accepted; a data flip inside a record also shows in that record's verdict at finish."""
    imgs, metas, total, (epar, ecrc, est) = small
    assert F.expect_n(imgs[4].size, 8192, 4096) == 1027 and F.expect_n(imgs[0].size, 16384, 4096) == 3617
    hurt = [a.copy() for a in imgs]
    for pos, x in hits:
        if 28 <= pos and frame * 4096 + pos - 28 < imgs[member].size:
            hurt[member][frame * 4096 + pos - 28] ^= x
    _, hcrc, hst = expected(oracle, ec_oracle, 5, 3, hurt, metas, total)  # the record walk runs over what arrived
    frames = frames_of(oracle, epar, 5, 3, 4096)
    for fpc in (3, 1):
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, imgs, metas, total, 4096, fpc,
                                                damage={(member, frame): hits})
        assert all(c[5] == 0 for c in calls)  # the device form is queued whatever the frames hold
        F.check_calls(gpu_ctx, calls, frames, 4096, bad=[(member, frame, status)])
        assert rc == 0 and (st == hst).all() and (crc == hcrc).all()


def test_damage_in_a_record_and_the_host_form(gpu_ctx, oracle, ec_oracle, small):
    """A flip in a record's payload: the frame fails and the record fails; the host form returns the CRC error."""
    imgs, metas, total, (epar, ecrc, est) = small
    x = metas[0][0]
    pos = int(x["offset"]) + 36 + 5
    frame, byte = pos // 4096, pos % 4096
    for form in ("device", "host", "pinned"):
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, oracle, 5, 3, imgs, metas, total, 4096, 2, form=form,
                                                damage={(0, frame): [(28 + byte, 0x20)]})
        F.check_calls(gpu_ctx, calls, frames_of(oracle, epar, 5, 3, 4096), 4096, bad=[(0, frame, CRC_ERR)])
        want_rc = [CRC_ERR if form != "device" and c[0] <= frame * 4096 < c[0] + c[1] else 0 for c in calls]
        assert [c[5] for c in calls] == want_rc
        assert rc == 0 and st[0] == CRC_ERR and nbad == 1 and (st[1:] == est[1:]).all()


def test_second_stream_of_the_callers(gpu_ctx, oracle, fam53):
    imgs, metas, total, (epar, ecrc, est) = fam53
    s = gpu_ctx.stream_create()
    try:
        calls, _, (crc, st, _, rc) = session(gpu_ctx, oracle, 5, 3, imgs, metas, total, 8192, 3, stream=s)
    finally:
        gpu_ctx.stream_destroy(s)
    F.check_calls(gpu_ctx, calls, frames_of(oracle, epar, 5, 3, 8192), 8192)
    assert rc == 0 and (crc == ecrc).all() and (st == est).all()


def test_refused_calls(gpu_ctx, oracle, small):
    """Every refused call returns its code, launches nothing, leaves out and results untouched, and the session
    reaches a correct end."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import FETCH_RESULT_DTYPE, ErasureCode, MarshalSession, fetch_cfg, frames_cfg
    imgs, metas, total, (epar, ecrc, est) = small
    k, m, fl = 5, 3, 4096
    ec = ErasureCode(gpu_ctx, k, m)
    ses = MarshalSession(ec, metas, [a.size for a in imgs], total)
    good, fgood = frames_cfg(fl, bids(8), pids(8)), fetch_cfg()
    ins = F.Bufs(gpu_ctx, range(k), F.IN_LEAD + 5 * (fl + 32) + 72, "device")
    outs = F.Bufs(gpu_ctx, range(k, k + m), F.OUT_LEAD + X.need(fl, total) + 64, "device")
    d_res = crc.DeviceBuffer(gpu_ctx, 16 * k * 5)
    s1, s2 = gpu_ctx.stream_create(), gpu_ctx.stream_create()

    def load(o, n):
        want = np.zeros((k, (n + fl - 1) // fl), FETCH_RESULT_DTYPE)
        for i in range(k):
            img, want[i] = F.in_image(oracle, imgs[i], i, o, n, fl)
            ins.load(i, img)
        for i in range(k, k + m):
            outs.load(i, np.full(outs.size, X.PREFILL, np.uint8))
        d_res.upload(np.full(16 * k * 5, 0xEE, np.uint8))
        return want

    def call(cfg=good, fcfg=fgood, inl="default", out="default", cap=None, res="default", o=0, n=8192, stream=s1,
             shift=0, oshift=0):
        inl = [ins.at(i, F.IN_LEAD + shift) for i in range(k)] + [None] * m if inl == "default" else inl
        out = [None] * k + [outs.at(i, F.OUT_LEAD + oshift) for i in range(k, k + m)] if out == "default" else out
        cap = X.need(fl, n) if cap is None else cap
        return ses.task_device(cfg, fcfg, inl, out, cap, d_res if res == "default" else res, o, n, stream=stream)

    def refusals(o):
        load(o, 8192)
        inl = [ins.at(i, F.IN_LEAD) for i in range(k)] + [None] * m
        assert call(o=o, stream=2) == PARAM                                  # hipStreamPerThread
        assert call(o=o + 4096) == PARAM                                     # not the next chunk
        assert call(o=o, n=5120) == PARAM                                    # len % 4096 before the end
        for kw in ({"cfg": None}, {"fcfg": None}, {"inl": None}, {"out": None}, {"res": None}):
            assert call(o=o, **kw) == PARAM                                  # 2
        assert call(cfg=frames_cfg(1024, bids(8), pids(8)), fcfg=fetch_cfg(8, 1), o=o) == SIZE_INVALID   # 3 before 4
        assert call(cfg=frames_cfg(1024, bids(8), pids(8)), res=None, o=o) == PARAM                      # 2 before 3
        assert call(o=o, oshift=4) == PARAM and call(o=o, cap=X.need(fl, 8192) - 1) == PARAM             # the frames call's 4
        for st in (4096 + 24, 4096 + 28, 4096 + 36, 8):
            assert call(fcfg=fetch_cfg(st), o=o) == PARAM
        assert call(fcfg=fetch_cfg(0, 1), o=o) == PARAM
        for shift in (-4, 1, 4):
            assert call(o=o, shift=shift) == PARAM                           # in[i] % 8 != 4
        assert call(inl=[None] + [a + 1 for a in inl[1:k]] + [None] * m, o=o) == PARAM   # 4 before 5
        assert call(inl=[None] + inl[1:], o=o) == DATA_INVALID               # a NULL source with a frame to read
        assert call(out=[None] * (k + m), o=o) == DATA_INVALID
        gpu_ctx.stream_sync(s1)
        for i in range(k, k + m):
            assert (outs.image(i) == X.PREFILL).all()
        assert (d_res.download(np.uint8, 16 * k * 5) == 0xEE).all()

    try:
        frames = frames_of(oracle, epar, 5, 3, fl)
        refusals(0)
        want = load(0, 8192)
        assert call(o=0) == 0 and call(o=0) == PARAM                         # repeated
        assert call(o=8192, stream=s2) == PARAM                              # a second stream
        gpu_ctx.stream_sync(s1)
        got = d_res.download(FETCH_RESULT_DTYPE, k * 2).reshape(k, 2)
        F.check_calls(gpu_ctx, [(0, 8192, {i: outs.image(i) for i in range(k, k + m)}, got, want, 0)], frames, fl)
        refusals(8192)
        # member 2 (2000 bytes) has nothing to read from 8192 on: NULL and a misaligned address both pass
        want = load(8192, total - 8192)
        inl = [ins.at(i, F.IN_LEAD) for i in range(k)] + [None] * m
        inl[2] = None
        assert call(inl=inl, o=8192, n=total - 8192) == 0
        gpu_ctx.stream_sync(s1)
        got = d_res.download(FETCH_RESULT_DTYPE, k * 3).reshape(k, 3)
        F.check_calls(gpu_ctx, [(8192, total - 8192, {i: outs.image(i) for i in range(k, k + m)}, got, want, 0)], frames, fl)
        c, st, nbad, rc = ses.finish()
        assert rc == 0 and (c == ecrc).all() and (st == est).all() and nbad == 0
    finally:
        ses.free()
        ec.free()
        gpu_ctx.stream_destroy(s1)
        gpu_ctx.stream_destroy(s2)
        for b in (ins, outs):
            b.free()
        d_res.free()
