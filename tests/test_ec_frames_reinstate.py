"""Frame-emitting chunk calls of the reinstate session (include/tfs_ec_frames.h, DESIGN.md
§3.23): one call decodes the chunk, verifies every record -- the survivors' from the bytes
read, the rebuilt members' from the bytes made -- and leaves every dead member's
WriteRawDataMessage frames sealed in a buffer of its own: TFS_RAW_NORMAL_DATA on the first
frame of a rebuilt data member, TFS_RAW_PARITY_DATA on that of a rebuilt parity member.

Expected frames come from the oracles (jerasure's decode of the survivors as they are,
oracle_crc over each frame's body); the plain reinstate session is the second witness for
CRCs and statuses."""
import numpy as np
import pytest

import ec_frames_expect as X
from test_ec_frames import LEAD, LENS, bids, pids
from test_marshal import chunks_of, family, up
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode and decode)
from test_reinstate import encode_family, erased_of, expected, plan_of
from test_reinstate import run as plain_run

pytestmark = pytest.mark.gpu

CRC_ERR = -1010


def session(ctx, k, m, erased, fam, metas, sizes, total, frame_len, fpc, form="device", stride=0):
    """One whole session in calls of `fpc` frames: [(offset, len, {dead member: image})], finish()."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, ReinstateSession, frames_cfg
    ec = ErasureCode(ctx, k, m, erased)
    ses = ReinstateSession(ec, metas, sizes, total)
    assert ec.rc == 0 and ses.rc == 0
    src, out = plan_of(k, m, erased)
    n = k + m
    cfg = frames_cfg(frame_len, bids(n), pids(n), stride)
    step = frame_len * fpc
    size = LEAD + X.need(frame_len, min(step, total), stride) + 64
    dev = form == "device"
    d_src = {i: crc.DeviceBuffer(ctx, total).upload(fam[i]) for i in src} if dev else {}
    bufs = {i: crc.DeviceBuffer(ctx, size) if dev else np.zeros(size, np.uint8) for i in out}
    fill = np.full(size, X.PREFILL, np.uint8)
    calls = []
    for o, ln in chunks_of(total, step):
        cap = X.need(frame_len, ln, stride)
        if dev:
            for b in bufs.values():
                b.upload(fill)
            mem = [d_src[i].ptr + o if i in d_src else None for i in range(n)]
            outl = [bufs[i].ptr + LEAD if i in bufs else None for i in range(n)]
            assert ses.frames_device(cfg, mem, outl, cap, o, ln) == 0
            ctx.sync()
            calls.append((o, ln, {i: b.download(np.uint8, size) for i, b in bufs.items()}))
        else:
            for b in bufs.values():
                b[:] = fill
            mem = [fam[i][o:o + ln].copy() if i in src else None for i in range(n)]
            outl = [bufs[i].ctypes.data + LEAD if i in bufs else None for i in range(n)]
            assert ses.frames(cfg, mem, outl, cap, o, ln) == 0
            calls.append((o, ln, {i: b.copy() for i, b in bufs.items()}))
    res = ses.finish()
    ses.free()
    ec.free()
    if dev:
        for b in list(d_src.values()) + list(bufs.values()):
            b.free()
    return calls, res


def check_calls(calls, frames, frame_len, stride=0):
    st = X.stride_of(frame_len, stride)
    for o, ln, images in calls:
        nf = (ln + frame_len - 1) // frame_len
        cap = X.need(frame_len, ln, stride)
        for i, img in images.items():
            exp = np.full(img.size, X.PREFILL, np.uint8)
            exp[LEAD:LEAD + cap] = X.call_image(frames[i], o // frame_len, nf, st, cap)
            bad = np.nonzero(img != exp)[0]
            assert bad.size == 0, (o, ln, i, int(bad[0]) - LEAD, int(bad.size))


def build(oracle, ec_oracle, k, m, dead, seed):
    imgs, metas = family(oracle, k, seed, LENS)
    total = up(max(a.size for a in imgs), 1024)
    fam = encode_family(ec_oracle, k, m, imgs, total)
    erased = erased_of(k, m, dead)
    sizes = [total if erased[i] else imgs[i].size for i in range(k)]
    return imgs, metas, total, fam, erased, sizes


def run_case(ctx, oracle, ec_oracle, k, m, dead, fam, metas, sizes, total, erased, shapes):
    ems, ecrc, est = expected(oracle, ec_oracle, k, m, erased, fam, metas, sizes, total)
    _, pres = plain_run(ctx, k, m, erased, fam, metas, sizes, total, chunks_of(total, 16384))
    assert (pres[0] == ecrc).all() and (pres[1] == est).all()
    out = plan_of(k, m, erased)[1]
    assert sorted(out) == sorted(dead)
    for frame_len, fpc in shapes:
        frames = {i: X.member_frames(oracle, ems[i], frame_len, bids(k + m)[i], pids(k + m)[i], i >= k) for i in out}
        for i in out:  # F: NORMAL for rebuilt data, PARITY for rebuilt parity, on the first frame only
            flags = [int.from_bytes(f[-4:], "little") for f in frames[i]]
            assert flags == [X.PARITY if i >= k else X.NORMAL] + [0] * (len(flags) - 1)
        calls, (crc, st, nbad, rc) = session(ctx, k, m, erased, fam, metas, sizes, total, frame_len, fpc)
        check_calls(calls, frames, frame_len)
        assert rc == 0 and (crc == pres[0]).all() and (st == pres[1]).all() and nbad == pres[2]
        for _, ln, images in calls:
            nf = (ln + frame_len - 1) // frame_len
            offs = [LEAD + j * (frame_len + 64) for j in range(nf)]
            lens = [X.OVERHEAD + min(frame_len, ln - j * frame_len) for j in range(nf)]
            for img in images.values():
                _, s, bad, prc = ctx.packet_verify(img, offs, lens)
                assert prc == 0 and bad == 0 and (s == 0).all()
    return ems, est


@pytest.mark.parametrize("dead", [[1], [2, 6], [0, 3, 5]])
def test_dead_sets_5_3(gpu_ctx, oracle, ec_oracle, dead):
    """One data member; one data and one parity; two data and one parity."""
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, 5, 3, dead, 530 + len(dead))
    ems, est = run_case(gpu_ctx, oracle, ec_oracle, 5, 3, dead, fam, metas, sizes, total, erased,
                        [(4096, 1), (4096, 3), (16384, 2)])
    assert (est == 0).all()
    for i in dead:
        assert (ems[i] == fam[i]).all()
    # a rebuilt data member's frames cover the zero padding up to total
    short = [i for i in dead if i < 5 and imgs[i].size + 4096 < total]
    if dead != [1]:
        assert short
    for i in short:
        assert not ems[i][imgs[i].size:].any()


def test_five_dead_6_6(gpu_ctx, oracle, ec_oracle):
    """Two output groups, a rebuilt data member in the second."""
    dead = [0, 1, 2, 3, 4]
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, 6, 6, dead, 66)
    ems, est = run_case(gpu_ctx, oracle, ec_oracle, 6, 6, dead, fam, metas, sizes, total, erased, [(4096, 3), (16384, 1)])
    assert (est == 0).all() and plan_of(6, 6, erased)[1][4] == 4
    for i in dead:
        assert (ems[i] == fam[i]).all()


def test_corrupt_survivor_fails_a_rebuilt_record(gpu_ctx, oracle, ec_oracle):
    """A corrupt survivor: the rebuilt member's record over the same bytes fails, as in the plain session; the
    frames are the sealed code of the bytes as read."""
    dead = [0, 3, 5]
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, 5, 3, dead, 533)
    x = metas[0][2]
    fam = [a.copy() for a in fam]
    fam[6][int(x["offset"]) + 36 + 5] ^= 0x21  # a surviving parity member, under a record of dead member 0
    ems, est = run_case(gpu_ctx, oracle, ec_oracle, 5, 3, dead, fam, metas, sizes, total, erased, [(4096, 3)])
    assert (est == CRC_ERR).sum() >= 1 and est[2] == CRC_ERR


def test_host_form_equals_device_form(gpu_ctx, oracle, ec_oracle):
    dead = [2, 6]
    imgs, metas, total, fam, erased, sizes = build(oracle, ec_oracle, 5, 3, dead, 532)
    for stride in (0, 4096 + 136):
        dev, dres = session(gpu_ctx, 5, 3, erased, fam, metas, sizes, total, 4096, 4, stride=stride)
        host, hres = session(gpu_ctx, 5, 3, erased, fam, metas, sizes, total, 4096, 4, form="host", stride=stride)
        for (_, _, a), (_, _, b) in zip(dev, host):
            assert all((a[i] == b[i]).all() for i in a)
        assert (dres[0] == hres[0]).all() and (dres[1] == hres[1]).all() and hres[3] == 0
