"""One family and one coder through the calls in the order a dataserver makes them (include/tfs_ec.h):
marshal, scrub, update on unlink, scrub again, damage, scrub, locate, and on a coder with the erasure
vector reinstate, plain decode and degraded read -- at sizes that differ from call to call, so that the
coder's staging, locate and update buffers are grown and reused by every host form in turn.

The families come from tests/ec_family.py, one per seed of its SEEDS: geometry, hand-laid members,
chunk sequences whose lengths are drawn per chunk (the kernels take a chunk's place only through
tile0 = offset >> 12 and units = len / 1024, and here the two vary independently), erasure vector,
change list and damage list.  Every expected byte, CRC, status, map bit and locate field is composed
there from the oracles and from what the generator did; the judges name the first difference.
Everything is byte-exact; members that a call must not write are downloaded and compared.
"""
import numpy as np
import pytest

import ec_family as F
from ec_family import FILL, UNIT
from test_degraded_read import expected as read_expected
from test_ec_update import units_of
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode and decode)
from test_reinstate import plan_of, sizes_of
from test_scrub import encode

pytestmark = pytest.mark.gpu

PARAM = -1016


class Bufs:
    """Device buffers kept for the life of a case and handed out by size."""

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def new(self, nbytes, fill=None):
        import tfs_amd.crc as crc
        b = crc.DeviceBuffer(self.ctx, max(int(nbytes), 1024))
        self.all.append(b)
        if fill is not None:
            b.upload(np.full(max(int(nbytes), 1024), fill, np.uint8) if np.isscalar(fill) else fill)
        return b

    def free(self):
        for b in self.all:
            b.free()


def marshal(ctx, ec, f, data, chunks, form, bufs, stream=None):
    """(parity, finish's result) of one session on `ec`; the data chunks are checked unchanged."""
    from tfs_amd.ec import MarshalSession
    ses = MarshalSession(ec, f.metas, f.sizes, f.total)
    assert ses.rc == 0
    parity = [np.full(f.total, FILL, np.uint8) for _ in range(f.pn)]
    if form == "host":
        for o, n in chunks:
            given = [a[o:o + n].copy() for a in data]
            assert ses.encode(given + [p[o:o + n] for p in parity], o, n) == 0
            assert all((g == a[o:o + n]).all() for g, a in zip(given, data)), o
    else:
        d = [bufs.new(max(n for _, n in chunks)) for _ in range(f.dn + f.pn)]
        for o, n in chunks:
            for b, a in zip(d, data):
                b.upload(a[o:o + n])
            for b in d[f.dn:]:
                b.upload(np.full(n, FILL, np.uint8))
            assert ses.encode_device(d, o, n, stream=stream) == 0
            ctx.stream_sync(stream) if stream else ctx.sync()
            for i, (b, a) in enumerate(zip(d, data)):
                assert (b.download(np.uint8, n) == a[o:o + n]).all(), (i, o)
            for p in range(f.pn):
                parity[p][o:o + n] = d[f.dn + p].download(np.uint8, n)
    res = ses.finish()
    ses.free()
    return parity, res


def scrub(ctx, ec, f, members, chunks, form, bufs, stream=None):
    """finish's result of one session on `ec`; no member chunk is written."""
    from tfs_amd.ec import ScrubSession
    ses = ScrubSession(ec, f.metas, f.sizes, f.total)
    assert ses.rc == 0
    if form == "host":
        for o, n in chunks:
            given = [a[o:o + n].copy() for a in members]
            assert ses.check(given, o, n) == 0
            assert all((g == a[o:o + n]).all() for g, a in zip(given, members)), o
    else:
        d = [bufs.new(max(n for _, n in chunks)) for _ in members]
        for o, n in chunks:
            for b, a in zip(d, members):
                b.upload(a[o:o + n])
            assert ses.check_device(d, o, n, stream=stream) == 0
            ctx.stream_sync(stream) if stream else ctx.sync()
            for i, (b, a) in enumerate(zip(d, members)):
                assert (b.download(np.uint8, n) == a[o:o + n]).all(), (i, o)
    res = ses.finish()
    ses.free()
    return res


def judge_scrub(what, f, res, want):
    crc, st, nbad, units, tmap, rc = res
    assert rc == 0, (what, rc)
    F.judge_records(what, F.flat(f), crc, st, nbad, want[0], want[1])
    F.judge_map(what, units, tmap, want[2], want[3])


def reinstate(ctx, dec, f, fam, sizes, chunks, form, bufs):
    """({output member: bytes}, finish's result) of one session on `dec`; the sources are checked unchanged."""
    from tfs_amd.ec import ReinstateSession
    ses = ReinstateSession(dec, f.metas, sizes, f.total)
    assert ses.rc == 0
    src, out = plan_of(f.dn, f.pn, f.erased)
    got = {o: np.full(f.total, FILL, np.uint8) for o in out}
    n = f.dn + f.pn
    if form == "host":
        for o, ln in chunks:
            mem = [fam[i][o:o + ln].copy() if i in src else got[i][o:o + ln] if i in got else None for i in range(n)]
            assert ses.decode(mem, o, ln) == 0
            assert all((mem[i] == fam[i][o:o + ln]).all() for i in src), o
    else:
        d = {i: bufs.new(max(ln for _, ln in chunks)) for i in src + out}
        for o, ln in chunks:
            for i in src:
                d[i].upload(fam[i][o:o + ln])
            for i in out:
                d[i].upload(np.full(ln, FILL, np.uint8))
            assert ses.decode_device([d.get(i) for i in range(n)], o, ln) == 0
            ctx.sync()
            for i in src:
                assert (d[i].download(np.uint8, ln) == fam[i][o:o + ln]).all(), (i, o)
            for i in out:
                got[i][o:o + ln] = d[i].download(np.uint8, ln)
    res = ses.finish()
    ses.free()
    return got, res


@pytest.mark.parametrize("seed", F.SEEDS)
def test_life_cycle(gpu_ctx, oracle, ec_oracle, seed):  # noqa: F811
    from tfs_amd.ec import LOCATE_RESULT_DTYPE, ErasureCode
    ctx = gpu_ctx
    f = F.make(oracle, seed)
    dn, pn, total = f.dn, f.pn, f.total
    names = F.flat(f)
    bufs = Bufs(ctx)
    enc = ErasureCode(ctx, dn, pn)
    dec = ErasureCode(ctx, dn, pn, f.erased)
    assert enc.rc == 0 and dec.rc == 0
    try:
        # 1. marshal, device form through reused chunk buffers, then host form, the seed's sequence
        parity0 = encode(ec_oracle, dn, pn, f.data, total)
        crc0, st0 = F.records(oracle, f, f.data)
        assert (st0 == 0).all()
        for form in ("device", "host"):
            par, (crc, st, nbad, rc) = marshal(ctx, enc, f, f.data, f.chunks, form, bufs)
            assert rc == 0, (form, rc)
            F.judge_bytes("marshal, %s form" % form, par, parity0)
            F.judge_records("marshal, %s form" % form, names, crc, st, nbad, crc0, st0)

        # 2. scrub of the clean family, another sequence
        want = F.scrub(oracle, ec_oracle, f, f.data, parity0)
        assert not want[3].any() and not want[2].any()
        judge_scrub("scrub of the clean family", f, scrub(ctx, enc, f, f.data + parity0, f.chunks2, "device", bufs), want)

        # 3. update: the unlink-like change of one data member carried into the parity
        c = f.change
        j, units, nu = c.member, c.units, len(c.units)
        parity1 = encode(ec_oracle, dn, pn, f.new_data, total)
        old_u, new_u = units_of(f.data[j], units), units_of(f.new_data[j], units)
        a, b = (old_u, new_u) if seed % 2 == 0 else (old_u ^ new_u, None)
        d_par = [bufs.new(total, p) for p in parity0]
        d_a, d_b = bufs.new(a.size, a), None if b is None else bufs.new(b.size, b)
        assert enc.update_device(d_par, total, j, d_a, d_b, units, nu) == 0
        ctx.sync()
        F.judge_bytes("update, device form", [d.download(np.uint8, total) for d in d_par], parity1)
        assert (d_a.download(np.uint8, a.size) == a).all() and (b is None or (d_b.download(np.uint8, b.size) == b).all())
        hpar = [p.copy() for p in parity0]
        assert enc.update(hpar, total, j, a, b, units=units) == 0
        F.judge_bytes("update, host form", hpar, parity1)
        crc1, st1 = F.records(oracle, f, f.new_data)
        want = F.scrub(oracle, ec_oracle, f, f.new_data, parity1)
        assert not want[3].any() and (want[0] == crc1).all() and (want[1] == st1).all()
        judge_scrub("scrub after the update", f, scrub(ctx, enc, f, f.new_data + hpar, f.chunks, "host", bufs), want)

        # 4. damage, then scrub with the seed's sequence
        hurt = F.apply_damages(f.new_data + parity1, f.damages)
        want = F.scrub(oracle, ec_oracle, f, hurt[:dn], hurt[dn:])
        assert want[3].any()
        judge_scrub("scrub of the damaged family", f, scrub(ctx, enc, f, hurt, f.chunks, "device", bufs), want)

        # 5. locate over the units the map names, unsorted, as its rows yield them
        listed = F.flagged(want[3])
        assert sorted(listed) == sorted(d.unit for d in f.damages)
        n = len(listed)
        d_mem = [bufs.new(total, a) for a in hurt]
        d_res, d_fix = bufs.new(8 * n, FILL), bufs.new(UNIT * n, FILL)
        rc = enc.locate_device(d_mem, total, listed, n, d_res, d_fix)
        ctx.sync()
        res = d_res.download(LOCATE_RESULT_DTYPE, n)
        fixed = d_fix.download(np.uint8, UNIT * n).reshape(n, UNIT)
        for i, (d, a) in enumerate(zip(d_mem, hurt)):
            assert (d.download(np.uint8, total) == a).all(), i
        given = [a.copy() for a in hurt]
        assert enc.L.tfs_ec_locate_set_piece(enc.h, 3) == 0
        try:
            hres, hfixed, hrc = enc.locate(given, total, units=listed)
        finally:
            assert enc.L.tfs_ec_locate_set_piece(enc.h, 0) == 0
        assert all((g == a).all() for g, a in zip(given, hurt))
        if pn == 1:
            assert rc == PARAM and hrc == PARAM
            assert (res.view(np.uint8) == FILL).all() and (fixed == FILL).all() and not hfixed.any()
        else:
            assert rc == 0 and hrc == 0
            wants = F.locate_wants(f, f.new_data, listed, want[3])
            F.judge_locate("locate, device form", res, fixed, wants, pn)
            F.judge_locate("locate, host form", hres, hfixed, wants, pn, untouched=0)

        # 6. reinstate from the undamaged family as it was marshalled, then the plain decode, on the decode coder
        fam = f.data + parity0
        src, out = plan_of(dn, pn, f.erased)
        sizes = sizes_of(dn, f.erased, f.imgs, total)
        for form in ("device", "host"):
            got, (crc, st, nbad, rc) = reinstate(ctx, dec, f, fam, sizes, f.chunks, form, bufs)
            assert rc == 0, (form, rc)
            F.judge_bytes("reinstate, %s form" % form, got, {i: fam[i] for i in out})
            F.judge_records("reinstate, %s form" % form, names, crc, st, nbad, crc0, st0)
        d_fam = [bufs.new(total, fam[i] if i in src else FILL) for i in range(dn + pn)]
        assert dec.decode_device(d_fam, total) == 0
        ctx.sync()
        back = [d.download(np.uint8, total) for d in d_fam]
        F.judge_bytes("decode_device", {i: back[i] for i in out}, {i: fam[i] for i in out})
        F.judge_bytes("decode_device, sources", {i: back[i] for i in src}, {i: fam[i] for i in src})

        # 7. degraded read of one dead data member: its records, and three ranges
        dead = [i for i in range(dn) if f.erased[i] == 1]
        if dead:
            t = dead[seed % len(dead)]
            mid = total // UNIT // 2 * UNIT
            rj, rbytes = ErasureCode.read_jobs(ranges=[(0, 1), (total - 1, 1), (mid - 5, 11)])
            jobs, cap = ErasureCode.read_jobs(metas=f.metas[t])
            rj["out_offset"] += cap
            jobs, cap = np.concatenate([jobs, rj]), cap + rbytes
            ecrc, est, eout = read_expected(oracle, f.data[t], jobs, total, cap)
            assert (est == 0).all()
            what = ["degraded read of member %d" % t, [(t, tuple(x)) for x in jobs]]
            dj, dout = bufs.new(jobs.nbytes, jobs), bufs.new(cap, FILL)
            dc, ds, db = bufs.new(4 * len(jobs), 0x5A), bufs.new(4 * len(jobs), 0x5A), bufs.new(4, np.zeros(1, np.uint32))
            mem = [d_fam[i] if i in src else None for i in range(dn + pn)]
            assert dec.read_degraded_device(mem, total, t, dj, len(jobs), dout, cap, dc, ds, db) == 0
            ctx.sync()
            F.judge_records(what[0] + ", device form", what[1], dc.download(np.uint32, len(jobs)),
                            ds.download(np.int32, len(jobs)), int(db.download(np.uint32, 1)[0]), ecrc, est)
            F.judge_bytes(what[0] + ", device form", [dout.download(np.uint8, cap)], [eout])
            hout = np.full(cap, FILL, np.uint8)
            given = [fam[i].copy() if i in src else None for i in range(dn + pn)]
            crc, st, nbad, rc = dec.read_degraded(given, total, t, jobs, hout)
            assert rc == 0
            F.judge_records(what[0] + ", host form", what[1], crc, st, nbad, ecrc, est)
            F.judge_bytes(what[0] + ", host form", [hout], [eout])
            assert all((given[i] == fam[i]).all() for i in src)
    finally:
        bufs.free()
        dec.free()
        enc.free()


def test_two_sessions_interleaved_on_one_coder(gpu_ctx, oracle, ec_oracle):  # noqa: F811
    """A marshal of family A and a scrub of family B (the same geometry, another total, damaged) on one coder, their
    chunks alternating: device form on one caller stream, then host form through the coder's staging buffers.  Each
    session's result is what it is alone, and what the oracles say."""
    from tfs_amd.ec import ErasureCode, MarshalSession, ScrubSession
    ctx = gpu_ctx
    fa = F.make(oracle, 1006, geometry=(5, 3), units=23)
    fb = F.make(oracle, 1002, geometry=(5, 3), units=38)
    assert len(fa.chunks) > 1 and len(fb.chunks) > 1 and fa.chunks != fb.chunks
    dn, pn = 5, 3
    want_a = (encode(ec_oracle, dn, pn, fa.data, fa.total),) + F.records(oracle, fa, fa.data)
    hurt_b = F.apply_damages(fb.data + encode(ec_oracle, dn, pn, fb.data, fb.total), fb.damages)
    want_b = F.scrub(oracle, ec_oracle, fb, hurt_b[:dn], hurt_b[dn:])
    assert want_b[3].any()
    bufs = Bufs(ctx)
    ec = ErasureCode(ctx, dn, pn)
    stream = ctx.stream_create()
    try:
        alone_a = marshal(ctx, ec, fa, fa.data, fa.chunks, "device", bufs, stream=stream)
        alone_b = scrub(ctx, ec, fb, hurt_b, fb.chunks, "device", bufs, stream=stream)
        for form in ("device", "host"):
            sa, sb = MarshalSession(ec, fa.metas, fa.sizes, fa.total), ScrubSession(ec, fb.metas, fb.sizes, fb.total)
            assert sa.rc == 0 and sb.rc == 0
            par = [np.full(fa.total, FILL, np.uint8) for _ in range(pn)]
            da = [bufs.new(max(n for _, n in fa.chunks)) for _ in range(dn + pn)]
            db = [bufs.new(max(n for _, n in fb.chunks)) for _ in range(dn + pn)]
            for k in range(max(len(fa.chunks), len(fb.chunks))):
                ca = fa.chunks[k] if k < len(fa.chunks) else None
                cb = fb.chunks[k] if k < len(fb.chunks) else None
                if form == "host":
                    if ca:
                        o, n = ca
                        assert sa.encode([a[o:o + n] for a in fa.data] + [p[o:o + n] for p in par], o, n) == 0
                    if cb:
                        o, n = cb
                        assert sb.check([a[o:o + n] for a in hurt_b], o, n) == 0
                    continue
                if ca:
                    o, n = ca
                    for d, a in zip(da, fa.data + [np.full(fa.total, FILL, np.uint8)] * pn):
                        d.upload(a[o:o + n])
                if cb:
                    o, n = cb
                    for d, a in zip(db, hurt_b):
                        d.upload(a[o:o + n])
                if ca:                              # both launched before either is waited for
                    assert sa.encode_device(da, ca[0], ca[1], stream=stream) == 0
                if cb:
                    assert sb.check_device(db, cb[0], cb[1], stream=stream) == 0
                ctx.stream_sync(stream)
                if ca:
                    for p in range(pn):
                        par[p][ca[0]:ca[0] + ca[1]] = da[dn + p].download(np.uint8, ca[1])
                if cb:
                    for i, (d, a) in enumerate(zip(db, hurt_b)):
                        assert (d.download(np.uint8, cb[1]) == a[cb[0]:cb[0] + cb[1]]).all(), (i, cb)
            ra, rb = sa.finish(), sb.finish()
            sa.free(), sb.free()
            what = "interleaved, %s form: " % form
            assert ra[3] == 0
            F.judge_bytes(what + "marshal of A", par, want_a[0])
            F.judge_records(what + "marshal of A", F.flat(fa), ra[0], ra[1], ra[2], want_a[1], want_a[2])
            judge_scrub(what + "scrub of B", fb, rb, want_b)
            F.judge_bytes(what + "marshal of A against the session alone", par, alone_a[0])
            assert all((x == y).all() for x, y in zip(ra[:2], alone_a[1][:2])) and ra[2] == alone_a[1][2]
            assert all(np.array_equal(x, y) for x, y in zip(rb, alone_b))
    finally:
        ctx.stream_destroy(stream)
        bufs.free()
        ec.free()
