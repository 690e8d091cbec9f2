"""Device forms with 64-bit offsets, at the places where a 32-bit narrowing would show: every path that forms
base + u64 on the device gets one placement with byte 2^32 of its large buffer inside one chosen record or
frame (`straddle`: what comes before lies below 4 GiB, what comes after above) and one with everything past
5 GiB (`past`).  Where the path takes a declared length, that length is over 4 GiB too, one job ends exactly
on it (served) and, in a second call, one byte past it (that path's range status, nothing of it written).

The large allocations are never filled: only a window of a few hundred KiB at their tail is uploaded and
downloaded (Window), at most two of them are alive at a time, and each has SLACK bytes behind the declared
length, so that a kernel that is wrong by a byte stays inside the test's memory.  Expectations are computed as
each path's own test file computes them -- the oracle, Python frame construction, zlib -- over the same bytes
with the offsets shifted back; everything is bit-exact, and every byte of a downloaded window outside the
expected spans must still hold what was uploaded.

The wrapped ranges at the end (src_offset + size passes 2^64) use small ordinary buffers laid out so that not
even a library without the check can leave them."""
import numpy as np
import pytest

import degraded_reply_expect as E
import test_degraded_read as DR
import test_gpu_parity as P
import test_mirror as M
import test_packet as TP
import test_read_reply as RR
import test_receive as R
import test_write_frames as TW
from conftest import ocrc
from ec_family import GEOMETRIES
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

GIB4 = 1 << 32
PAST = 5 * (1 << 30) + 4096       # a multiple of 1024; the byte-granular paths add a residue of 1..15
SLACK = 4096
PARAM = -1016
EDGE = 1                          # TFS_COMPACT_JOB_EDGE
PLACES = ["straddle", "past"]


def straddle_base(at, residue):
    """The base, congruent to `residue` mod 16, that puts local byte `at` (or one of the 15 after it) on 2^32."""
    b = GIB4 - at
    return b - (b - residue) % 16


class Window:
    """The tail of one large device allocation: `base` bytes that are never touched, then the window, which
    starts out as `fill` (the bytes the library is told about and SLACK more)."""

    def __init__(self, ctx, base, fill):
        import tfs_amd.crc as crc
        self.base, self.fill = base, np.ascontiguousarray(fill, dtype=np.uint8)
        self.buf = crc.DeviceBuffer(ctx, base + self.fill.size)
        self.put()

    def put(self):
        self.buf.upload(self.fill, offset=self.base)

    def get(self):
        return self.buf.download(np.uint8, self.fill.size, offset=self.base)

    def unchanged(self):
        return bool((self.get() == self.fill).all())

    def free(self):
        self.buf.free()


class Pool:
    """Small device buffers of one test, and its windows: all freed together."""

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def buf(self, nbytes, data=None):
        import tfs_amd.crc as crc
        b = crc.DeviceBuffer(self.ctx, max(int(nbytes), 16))
        self.all.append(b)
        if data is not None:
            b.upload(data)
        else:
            b.zero()
        return b

    def window(self, base, fill):
        assert sum(isinstance(b, Window) for b in self.all) < 2, "at most two large allocations at a time"
        w = Window(self.ctx, base, fill)
        self.all.append(w)
        return w

    def free(self):
        for b in self.all:
            b.free()
        self.all = []


@pytest.fixture
def pool(gpu_ctx):
    p = Pool(gpu_ctx)
    try:
        yield p
    finally:
        gpu_ctx.sync()
        p.free()


def with_slack(data, byte=0xE7):
    return np.concatenate([np.ascontiguousarray(data, dtype=np.uint8), np.full(SLACK, byte, np.uint8)])


def assert_straddles(base, lo, hi, before, after):
    """Byte 2^32 lies strictly inside [base + lo, base + hi); the (lo, hi) ranges of `before` end at or below
    it and those of `after` begin above it."""
    assert base + lo < GIB4 < base + hi - 1, (base, lo, hi)
    assert all(base + b <= GIB4 for _, b in before) and all(base + a > GIB4 for a, _ in after)
    assert before and base > GIB4 - (1 << 24)


def assert_past(base, ranges):
    assert base >= 5 * (1 << 30) + 4096 and all(base + a >= 5 * (1 << 30) for a, _ in ranges)


# ---- tfs_mirror_frames_device: src_offset, frame_offset ------------------------------------------------------

MIRROR = {"a": dict(first=1024 - 36, frame=1024, lens=[17, 988, 3000, 989], chosen=2, ds=(0, 2, 27)),
          "b": dict(first=40000, frame=32768, lens=[39999, 90000], chosen=1, ds=(2, 27, 0))}


def mirror_layout(oracle, geo, place):
    """(cfg, image, jobs, ds, src_len, out_cap, src_base, out_base): the last record ends on src_len and the
    last span on out_cap."""
    import tfs_amd.crc as crc
    g = MIRROR[geo]
    cfg = crc.mirror_cfg(g["first"], g["frame"], is_server=1, version=2)
    n = len(g["lens"])
    img, recs = M.build_source(oracle, g["lens"], [(5 * i + 3) % 16 for i in range(n)], seed=23)
    ds = (np.arange(40, dtype=np.uint64) * np.uint64(0x0101010101010101)) ^ np.uint64(0xD5D5000000000000)
    jobs, _ = M.make_jobs(cfg, recs, g["ds"], len(ds), [(7 * i + 2) % 16 for i in range(n)])
    # geometry a has all three ds counts, 27 on the chosen file; b has two jobs, so two of them
    assert {int(c) for c in jobs["ds_count"]} == ({0, 2, 27} if geo == "a" else {2, 27})
    counts = [crc.mirror_frame_count(cfg, s) for _, _, s in recs]
    assert counts == ([1, 1, 3, 2] if geo == "a" else [1, 3])      # 17: copy_unaligned; the chosen one: three frames
    spans = [(int(j["frame_offset"]), int(j["frame_offset"]) + crc.mirror_span(cfg, jobs[i:i + 1]))
             for i, j in enumerate(jobs)]
    srcs = [(o, o + s) for _, o, s in recs]
    src_len, out_cap = srcs[-1][1], spans[-1][1]
    assert src_len == max(b for _, b in srcs) and out_cap == max(b for _, b in spans)
    c = g["chosen"]
    if place == "straddle":
        sb = straddle_base(srcs[c][0] + 36 + g["lens"][c] // 2, 5)
        ob = straddle_base((spans[c][0] + spans[c][1]) // 2, 11)
        assert_straddles(sb, srcs[c][0] + 36, srcs[c][1], srcs[:c], srcs[c + 1:])
        assert_straddles(ob, spans[c][0], spans[c][1], spans[:c], spans[c + 1:])
    else:
        sb, ob = PAST + 5, PAST + 11
        assert_past(sb, srcs), assert_past(ob, spans)
    assert sb % 16 != ob % 16 and sb + src_len > GIB4 and ob + out_cap > GIB4
    return cfg, img, jobs, ds, src_len, out_cap, sb, ob


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("geo", ["a", "b"])
def test_mirror_frames(gpu_ctx, oracle, pool, geo, place):
    import tfs_amd.crc as crc
    cfg, img, jobs, ds, src_len, out_cap, sb, ob = mirror_layout(oracle, geo, place)
    simg = with_slack(img[:src_len])
    src = pool.window(sb, simg)
    out = pool.window(ob, M.prefill(out_cap + SLACK))
    d_res, d_nbad = pool.buf(16 * len(jobs)), pool.buf(4)
    far = jobs.copy()
    far["src_offset"] += np.uint64(sb)
    far["frame_offset"] += np.uint64(ob)
    for sl, oc, last in ((src_len, out_cap, 0), (src_len - 1, out_cap, PARAM), (src_len, out_cap - 1, PARAM)):
        out.put()
        d_nbad.zero()
        gpu_ctx.mirror_frames_device(cfg, src.buf, sb + sl, far, ds, out.buf, ob + oc, d_res, d_nbad)
        gpu_ctx.sync()
        got = out.get()
        res = d_res.download(crc.MIRROR_RESULT_DTYPE, len(jobs))
        nbad = int(d_nbad.download(np.uint32, 1)[0])
        assert res["status"].tolist() == [0] * (len(jobs) - 1) + [last], (sl, oc)
        M.check_call(oracle, simg, cfg, jobs, ds, got[:oc], out.fill[:oc], res, nbad, src_len=sl)
        assert (got[oc:] == out.fill[oc:]).all(), "a byte past out_cap was written"
    assert src.unchanged()


# ---- tfs_read_reply_device: src_offset, frame_offset -----------------------------------------------------------
# tests/test_read_reply.py::test_offsets_past_4_gib has this path's `past` placement; this is its straddle, and
# its range rows against lengths over 4 GiB.

def test_read_reply_straddle(gpu_ctx, oracle, pool):
    import tfs_amd.crc as crc
    img, recs = RR.build_image(oracle, [5000, 70001, 100], seed=27)
    jobs, cap = RR.packed(recs, pcode=[39, 63, 8])
    srcs = [(o, o + s) for _, o, s in recs]
    spans = [(int(j["frame_offset"]), int(j["frame_offset"]) + RR.cap_of(j)) for j in jobs]
    src_len = srcs[-1][1]
    assert src_len == img.size and spans[-1][1] == cap
    sb = straddle_base(srcs[1][0] + 36 + 35000, 5)
    ob = straddle_base(spans[1][0] + 28 + 20000, 11)
    assert_straddles(sb, srcs[1][0] + 36, srcs[1][1], srcs[:1], srcs[2:])
    assert_straddles(ob, spans[1][0] + 28, spans[1][0] + 28 + 70001, spans[:1], spans[2:])
    assert sb % 16 != ob % 16
    simg = with_slack(img)
    src = pool.window(sb, simg)
    out = pool.window(ob, RR.prefill(cap + SLACK))
    d_res, d_bad = pool.buf(16 * len(jobs)), pool.buf(4)
    far = jobs.copy()
    far["src_offset"] += np.uint64(sb)
    far["frame_offset"] += np.uint64(ob)
    for sl, oc, last in ((src_len, cap, 0), (src_len - 1, cap, PARAM), (src_len, cap - 1, PARAM)):
        out.put()
        d_bad.zero()
        gpu_ctx.read_reply_device(src.buf, sb + sl, far, out.buf, ob + oc, d_res, d_bad)
        gpu_ctx.sync()
        got = out.get()
        res = d_res.download(crc.READ_RESULT_DTYPE, len(jobs))
        assert res["status"].tolist() == [0, 0, last], (sl, oc)
        nbad = RR.check(oracle, simg[:sl], jobs, got[:oc], res, oc, out.fill[:oc])
        assert nbad == int(d_bad.download(np.uint32, 1)[0]) == (1 if last else 0)
        assert (got[oc:] == out.fill[oc:]).all(), "a byte past out_cap was written"
    assert src.unchanged()


# ---- tfs_compact_jobs_device, tfs_blocks_verify_device: src_offset, dest_offset ------------------------------

COMPACT_SIZES, COMPACT_CHOSEN = [1, 33, 1024, 70001, 8193], 3


def compact_layout(oracle, place):
    """(image, metas, odest, doff, src_len, src_base, dest_base); every record is live, the last ends on src_len."""
    img, metas = P._block_image(oracle, COMPACT_SIZES, seed=61)
    odest, doff, ook = P._oracle_compact(oracle, img, metas, np.zeros(len(metas), np.int32))
    assert (ook == 1).all()
    srcs = [(int(m["offset"]), int(m["offset"]) + int(m["size"])) for m in metas]
    dsts = [(int(d), int(d) + int(m["size"])) for d, m in zip(doff, metas)]
    src_len = srcs[-1][1]
    assert src_len == odest.size == sum(36 + s for s in COMPACT_SIZES)
    c = COMPACT_CHOSEN
    if place == "straddle":
        sb = straddle_base(srcs[c][0] + 36 + 35000, 3)
        db = straddle_base(dsts[c][0] + 36 + 20000, 9)
        assert_straddles(sb, srcs[c][0] + 36, srcs[c][1], srcs[:c], srcs[c + 1:])
        assert_straddles(db, dsts[c][0], dsts[c][1], dsts[:c], dsts[c + 1:])
    else:
        sb, db = PAST + 3, PAST + 9
        assert_past(sb, srcs), assert_past(db, dsts)
    assert sb % 16 != db % 16 and sb + src_len > GIB4
    return img, metas, odest, doff, src_len, sb, db


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("edge", [0, EDGE])
@pytest.mark.parametrize("seg", [1, 8192], ids=["whole", "segmented"])
def test_compact_and_verify_jobs(gpu_ctx, oracle, pool, seg, edge, place):
    import tfs_amd.crc as crc
    img, metas, odest, doff, src_len, sb, db = compact_layout(oracle, place)
    n = len(metas)
    j = np.zeros(n, crc.COMPACT_JOB_DTYPE)
    j["src_offset"], j["dest_offset"] = metas["offset"].astype(np.uint64) + np.uint64(sb), doff.astype(np.uint64) + np.uint64(db)
    j["file_id"], j["size"], j["new_offset"], j["reserved"] = metas["file_id"], metas["size"], doff, edge
    crcs = [ocrc(oracle, 0, img[int(m["offset"]) + 36:int(m["offset"]) + int(m["size"])].tobytes()) for m in metas]
    src = pool.window(sb, with_slack(img[:src_len]))
    dst = pool.window(db, M.prefill(odest.size + SLACK))
    d_j = pool.buf(j.nbytes, j)
    d_c, d_s, d_b = pool.buf(4 * n), pool.buf(4 * n), pool.buf(4)
    gpu_ctx.set_compact_segment(seg)
    try:
        for sl, last in ((src_len, 0), (src_len - 1, PARAM)):
            want = [0] * (n - 1) + [last]
            exp = dst.fill.copy()
            for k in range(n):
                if want[k] == 0:
                    o, sz = int(doff[k]), int(metas[k]["size"])
                    exp[o:o + sz] = odest[o:o + sz]
            for call in ("compact", "verify"):
                dst.put()
                for b in (d_c, d_s, d_b):
                    b.zero()
                if call == "compact":
                    gpu_ctx.compact_jobs_device(src.buf, sb + sl, d_j, n, dst.buf, d_c, d_s, d_b)
                else:
                    gpu_ctx.blocks_verify_device(src.buf, sb + sl, d_j, n, d_c, d_s, d_b)
                gpu_ctx.sync()
                assert d_s.download(np.int32, n).tolist() == want, (call, sl)
                assert int(d_b.download(np.uint32, 1)[0]) == (1 if last else 0)
                got_c = d_c.download(np.uint32, n)
                assert [int(got_c[k]) for k in range(n) if want[k] == 0] == [crcs[k] for k in range(n) if want[k] == 0]
                got = dst.get()
                diff = np.nonzero(got != (exp if call == "compact" else dst.fill))[0]
                assert diff.size == 0, (call, sl, int(diff[0]), int(diff.size))
    finally:
        gpu_ctx.set_compact_segment(1)
    assert src.unchanged()


# ---- tfs_packet_verify_device, tfs_packet_seal_device, tfs_packet_verify_write_device: tfs_packet_desc.offset --
# These take no declared length (each frame brings its own `len`), so there is no range row.

def packet_stream(oracle, sealed, pad):
    """(bytes, [(offset, avail)], [data or None], chosen): bodies of 0, 20, 1,000 and 70,000 bytes -- the two
    long ones WriteDataMessages with 0 and with 27 ds entries -- and the 1,000-byte one again with a flipped body
    byte, `pad` 20-byte frames before and after them.  `chosen` is the 70,000-byte frame."""
    def frame(body, pid):
        return pk.frame_v1(body, pid=pid, crc=ocrc(oracle, TW.FLAG, body) if sealed else 0)
    d964, d69748 = synth_bytes(7001, 964).tobytes(), synth_bytes(7002, 69748).tobytes()
    b1000 = pk.write_data_body(3, 4, 0, d964)
    b70000 = pk.write_data_body(5, 6, 4096, d69748, ds=list(range(100, 127)))
    assert (len(TW.SHORT_BODY), len(b1000), len(b70000)) == (20, 1000, 70000)
    flipped = bytearray(frame(b1000, 9))
    flipped[24 + 500] ^= 0x10
    short = (frame(TW.SHORT_BODY, 1), None)
    core = [short, (frame(b1000, 2), d964), (frame(b70000, 3), d69748), (frame(b"", 4), None),
            (bytes(flipped), None)]
    items = [short] * pad + core + [short] * pad
    parts, frames, pos = [], [], 0
    for i, (raw, _) in enumerate(items):
        gap = (3 * i + 1) % 8
        parts.append(b"\xAA" * gap + raw)
        frames.append((pos + gap, len(raw)))
        pos += gap + len(raw)
    return b"".join(parts), frames, [d for _, d in items], pad + 2


def packet_base(frames, chosen, place, residue):
    o, a = frames[chosen]
    spans = [(f, f + n) for f, n in frames]
    if place == "past":
        base = PAST + residue
        assert_past(base, spans)
        return base
    if place == "crc":                                     # byte 2^32 is the second of the header's crc field
        base, lo, hi = GIB4 - (o + 21), o + 20, o + 24
    else:
        base, lo, hi = straddle_base(o + 24 + 35000, residue), o + 24, o + a
    assert_straddles(base, lo, hi, spans[:chosen], spans[chosen + 1:])
    return base


def packet_descs(pool, frames, base):
    import tfs_amd.crc as crc
    d = np.zeros(len(frames), crc.PACKET_DESC_DTYPE)
    d["offset"] = np.array([f[0] for f in frames], np.uint64) + np.uint64(base)
    d["len"] = [f[1] for f in frames]
    n = len(frames)
    return pool.buf(d.nbytes, d), pool.buf(4 * n), pool.buf(4 * n), pool.buf(16 * n), pool.buf(4)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("pad", [0, 150], ids=["latency", "throughput"])
def test_packet_verify_and_verify_write(gpu_ctx, oracle, pool, pad, place):
    """Both launch sizes (at most 256 frames and more).  Nothing may be written into the frames."""
    import tfs_amd.crc as crc
    buf, frames, datas, chosen = packet_stream(oracle, True, pad)
    n = len(frames)
    base = packet_base(frames, chosen, place, 13)
    win = pool.window(base, with_slack(np.frombuffer(buf, np.uint8), 0xAA))
    d_desc, d_crc, d_st, d_parts, d_bad = packet_descs(pool, frames, base)
    ocrc_, ost, obad = TP.o_verify(oracle, buf, frames)
    assert sorted(set(ost.tolist())) == [-1010, -1, 0] and obad == 2
    gpu_ctx.packet_verify_device(d_desc, n, win.buf, d_crc, d_st, d_bad)
    gpu_ctx.sync()
    assert np.array_equal(d_st.download(np.int32, n), ost) and np.array_equal(d_crc.download(np.uint32, n), ocrc_)
    assert int(d_bad.download(np.uint32, 1)[0]) == obad
    for b in (d_crc, d_st, d_bad):
        b.zero()
    gpu_ctx.packet_verify_write_device(d_desc, n, win.buf, d_crc, d_st, d_parts, d_bad)
    gpu_ctx.sync()
    ndata = TW.check(oracle, buf, frames, datas, d_crc.download(np.uint32, n), d_st.download(np.int32, n),
                     d_parts.download(crc.WRITE_PART_DTYPE, n), int(d_bad.download(np.uint32, 1)[0]))
    assert ndata == 2
    assert win.unchanged()


@pytest.mark.parametrize("place", ["straddle", "crc", "past"])
@pytest.mark.parametrize("pad", [0, 150], ids=["latency", "throughput"])
def test_packet_seal(gpu_ctx, oracle, pool, pad, place):
    """`straddle` puts byte 2^32 inside the 70,000-byte body that is read, `crc` inside the four bytes of that
    frame's header that are written."""
    buf, frames, _, chosen = packet_stream(oracle, False, pad)
    n = len(frames)
    base = packet_base(frames, chosen, place, 6)
    win = pool.window(base, with_slack(np.frombuffer(buf, np.uint8), 0xAA))
    d_desc, d_crc, d_st, _, _ = packet_descs(pool, frames, base)
    ob, ocrc_, ost = TP.o_seal(oracle, buf, frames)
    o = frames[chosen][0]
    assert ob[o + 20:o + 24].any() and not buf[o + 20:o + 24].strip(b"\0")     # the oracle wrote that field
    gpu_ctx.packet_seal_device(d_desc, n, win.buf, d_crc, d_st)
    gpu_ctx.sync()
    assert np.array_equal(d_st.download(np.int32, n), ost) and np.array_equal(d_crc.download(np.uint32, n), ocrc_)
    got = win.get()
    assert np.array_equal(got[:ob.size], ob), "the sealed bytes differ"
    assert (got[ob.size:] == win.fill[ob.size:]).all()


# ---- tfs_receive_frames_device: frame_off into d_base ---------------------------------------------------------
# The device form takes no length of d_base (each desc brings `avail`): no range row.  The image is an ordinary
# allocation, the frames lie far.

@pytest.mark.parametrize("place", PLACES)
def test_receive_frames(gpu_ctx, oracle, pool, place):
    import tfs_amd.crc as crc
    G = crc.receive_granule()
    img, metas = R.build_block(oracle, [("rec", 100), ("at", G - 36), ("rec", 500), ("at", 2 * G - 20),
                                        ("rec", 2 * G + 700), ("rec", 3000), ("at", 6 * G + 333 - 186), ("rec", 150)],
                               seed=29)
    assert img.size == 6 * G + 333
    lens, k = [], 0
    while sum(lens) < img.size:
        lens.append(min((1024, 4096)[k % 2], img.size - sum(lens)))
        k += 1
    frames = R.hand_frames(oracle, img, lens)
    base_bytes, descs = R.lay_out(frames, shift=3)
    spans = [(int(d["frame_off"]), int(d["frame_off"]) + f.size) for d, f in zip(descs, frames)]
    c = 5
    assert lens[c] == 4096 and {1024, 4096} <= set(lens)
    if place == "straddle":
        fb = straddle_base(spans[c][0] + 60 + 2000, 7)
        assert_straddles(fb, spans[c][0] + 56, spans[c][1] - 4, spans[:c], spans[c + 1:])
    else:
        fb = PAST + 7
        assert_past(fb, spans)
    descs = descs.copy()
    descs["frame_off"] += np.uint64(fb)
    n, cap = len(frames), img.size + 100
    win = pool.window(fb, with_slack(base_bytes, 0x3C))
    before = R.prefill(cap + 64)
    d_img = pool.buf(cap + 64, before)
    d_parts, d_bad = pool.buf(16 * n), pool.buf(4)
    r = R.Landed()
    with crc.ReceiveSession(gpu_ctx, crc.receive_cfg(cap, R.BLOCK), d_img.ptr) as s:
        s.frames_device(win.buf, descs, d_parts, d_bad)
        r.crc, r.st, r.rbad, r.total = s.finish(metas)
    r.image = d_img.download(np.uint8, cap + 64)
    r.parts = d_parts.download(crc.RECEIVE_PART_DTYPE, n)
    r.nbad = int(d_bad.download(np.uint32, 1)[0])
    r.base_same, r.before = win.unchanged(), before
    R.check_landed(r, img, frames)
    R.check_verdicts(oracle, r, img, metas)


# ---- tfs_ec_read_degraded_device (out_offset, out_cap), tfs_ec_read_reply_device (read.frame_offset) ----------

@pytest.fixture(scope="module")
def ec_case(gpu_ctx, oracle):
    """One family at the smallest geometry tests/ec_family.py offers, the data member lost."""
    from tfs_amd.ec import ErasureCode
    k, m = min(GEOMETRIES)
    mem = E.Member(oracle, seed=77)
    mem.at(1024, 100, 3000)
    mem.at(1024, 900, 5000)
    mem.at(128, 60, 70001)
    mem.at(1024, 1000, 700)
    fam = E.Family(gpu_ctx, k, m, 0, mem.image())
    er = fam.erased()
    dec = ErasureCode(gpu_ctx, k, m, er)
    assert dec.rc == 0
    rebuilt = fam.rebuilt(E.ec_lib(), er)
    assert (rebuilt == fam.members[0]).all()
    yield mem, fam, er, dec, rebuilt
    dec.free()


def upload_survivors(pool, fam, er):
    return [None if a is None else pool.buf(a.size, a) for a in fam.survivors(er)]


@pytest.mark.parametrize("place", PLACES)
def test_ec_read_degraded(gpu_ctx, oracle, pool, ec_case, place):
    """Three jobs: one whose covering units end below byte 2^32 of out, one whose covering units cross it, one
    past it (`past`: the same layout from 5 GiB + 4 KiB).  The last one ends on out_cap."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode
    mem, fam, er, dec, rebuilt = ec_case
    metas = np.array([mem.recs[0], mem.recs[1], mem.recs[3]], dtype=crc.META_DTYPE)
    jobs, _ = ErasureCode.read_jobs(metas)
    cover = [DR.up1k(int(j["offset"]) + int(j["size"])) - int(j["offset"]) // 1024 * 1024 for j in jobs]
    assert cover[1] >= 4096
    wb = GIB4 - 16384 if place == "straddle" else PAST
    local = [0, 16384 - 2048, 16384 + 8192]
    assert wb % 1024 == 0 and local[0] + cover[0] <= local[1] and local[1] + cover[1] <= local[2]
    if place == "straddle":
        assert wb + local[0] + cover[0] <= GIB4 and wb + local[1] < GIB4 < wb + local[1] + cover[1] - 1024
        assert wb + local[2] > GIB4
    else:
        assert wb >= 5 * (1 << 30) + 4096
    cap = local[2] + cover[2]
    jobs["out_offset"] = local
    far = jobs.copy()
    far["out_offset"] += np.uint64(wb)
    d = upload_survivors(pool, fam, er)
    out = pool.window(wb, np.full(cap + SLACK, DR.FILL, np.uint8))
    n = len(jobs)
    dj, dc, ds, db = pool.buf(far.nbytes, far), pool.buf(4 * n), pool.buf(4 * n), pool.buf(4)
    for oc, last in ((cap, 0), (cap - 1, PARAM)):
        out.put()
        db.zero()
        assert dec.read_degraded_device(d, fam.size, fam.target, dj, n, out.buf, wb + oc, dc, ds, db) == 0
        gpu_ctx.sync()
        ecrc, est, eout = DR.expected(oracle, rebuilt, jobs, fam.size, oc)
        assert est.tolist() == [0, 0, last]
        assert ds.download(np.int32, n).tolist() == est.tolist()
        assert dc.download(np.uint32, n)[est == 0].tolist() == ecrc[est == 0].tolist()
        assert int(db.download(np.uint32, 1)[0]) == (1 if last else 0)
        got = out.get()
        diff = np.nonzero(got[:oc] != eout)[0]
        assert diff.size == 0, (oc, int(diff[0]), int(diff.size))
        assert (got[oc:] == DR.FILL).all(), "a byte past out_cap was written"


@pytest.mark.parametrize("place", PLACES)
def test_ec_read_reply(gpu_ctx, oracle, pool, ec_case, place):
    """The 70,001-byte record's frame lies across byte 2^32 of out; at least one frame has frame + 28 not
    congruent mod 8 with its slice (the unaligned store path).  The last frame ends on out_cap."""
    import tfs_amd.crc as crc
    mem, fam, er, dec, rebuilt = ec_case
    jobs, cap = E.packed(mem.recs, start=3, pcode=[8, 39, 63, 39])
    spans = [(int(j["frame_offset"]), int(j["frame_offset"]) + E.cap_of(j)) for j in jobs]
    assert spans[-1][1] == cap
    c = 2
    if place == "straddle":
        ob = straddle_base(spans[c][0] + 28 + 35000, 2)
        assert_straddles(ob, spans[c][0] + 28, spans[c][0] + 28 + 70001, spans[:c], spans[c + 1:])
    else:
        ob = PAST + 2
        assert_past(ob, spans)
    assert any((ob + int(j["frame_offset"]) + 28 - (int(j["src_offset"]) + 36)) % 8 for j in jobs)
    far = jobs.copy()
    far["frame_offset"] += np.uint64(ob)
    d = upload_survivors(pool, fam, er)
    out = pool.window(ob, E.prefill(cap + SLACK))
    d_res, d_bad = pool.buf(16 * len(jobs)), pool.buf(4)
    for oc, last in ((cap, 0), (cap - 1, PARAM)):
        out.put()
        d_bad.zero()
        assert dec.read_reply_device(d, fam.size, fam.target, far, out.buf, ob + oc, d_res, d_bad) == 0
        gpu_ctx.sync()
        got = out.get()
        res = d_res.download(crc.READ_RESULT_DTYPE, len(jobs))
        assert res["status"].tolist() == [0] * (len(jobs) - 1) + [last]
        nbad = E.check(oracle, rebuilt, jobs, fam.size, got[:oc], res, oc, out.fill[:oc])
        assert nbad == int(d_bad.download(np.uint32, 1)[0]) == (1 if last else 0)
        assert (got[oc:] == out.fill[oc:]).all(), "a byte past out_cap was written"


# ---- ranges that wrap: src_offset + size passes 2^64 -----------------------------------------------------------

def wrapped_case(oracle):
    """(buffer bytes, src_skip, src_len, jobs, expected dest bytes of the two good jobs, dest_cap).

    d_src is the buffer + 4096.  A 20,000-byte record B begins 3,000 bytes before d_src, and inside its payload
    lies a whole valid 300-byte record A that begins 200 bytes before d_src: both are sound records that end
    inside [d_src, d_src + src_len), so a library that adds src_offset + size in 64 bits and compares the wrapped
    sum serves them, reading only this buffer.  C (2^64 - 1, 37 bytes) has no record behind it.  G1 and G2 are
    ordinary records between and after them in job order."""
    import tfs_amd.crc as crc

    def record(fid, pay):
        fi = np.zeros(1, crc.FILEINFO_DTYPE)
        fi["id_"], fi["size_"], fi["usize_"], fi["crc_"] = fid, pay.size + 36, pay.size + 36, ocrc(oracle, 0, pay.tobytes())
        return np.concatenate([fi.view(np.uint8), pay])
    skip = 4096
    a = record(2001, synth_bytes(811, 264))
    pay_b = synth_bytes(812, 19964).copy()
    at_b, at_a = skip - 3000, skip - 200
    pay_b[at_a - (at_b + 36):at_a - (at_b + 36) + a.size] = a
    b = record(2002, pay_b)
    assert (a.size, b.size) == (300, 20000)
    gimg, gmetas = P._block_image(oracle, [1000, 5000], seed=63)
    godest, gdoff, gok = P._oracle_compact(oracle, gimg, gmetas, np.zeros(2, np.int32))
    gsize = int(gmetas["size"].astype(np.int64).sum())
    at_g = at_b + b.size + 8
    buf = np.full(at_g + gsize + SLACK, 0xEE, np.uint8)
    buf[at_b:at_b + b.size] = b
    buf[at_g:at_g + gsize] = gimg[:gsize]
    assert (buf[at_a:at_a + 300] == a).all() and at_a + 300 > skip and at_b + b.size > skip
    src_len = buf.size - skip
    j = np.zeros(5, crc.COMPACT_JOB_DTYPE)
    #         G1                                   A              B              C            G2
    j["src_offset"] = np.array([at_g - skip + int(gmetas[0]["offset"]), 2**64 - 200, 2**64 - 3000, 2**64 - 1,
                                at_g - skip + int(gmetas[1]["offset"])], dtype=np.uint64)
    j["file_id"] = [int(gmetas[0]["file_id"]), 2001, 2002, 2003, int(gmetas[1]["file_id"])]
    j["size"] = [int(gmetas[0]["size"]), 300, 20000, 37, int(gmetas[1]["size"])]
    j["dest_offset"] = [16, 2000, 4000, 30000, 31001]
    j["new_offset"] = [int(gdoff[0]), 0, 0, 0, int(gdoff[1])]
    good = {k: godest[int(gdoff[g]):int(gdoff[g]) + int(gmetas[g]["size"])] for k, g in ((0, 0), (4, 1))}
    crcs = {k: ocrc(oracle, 0, gimg[int(gmetas[g]["offset"]) + 36:int(gmetas[g]["offset"]) + int(gmetas[g]["size"])].tobytes())
            for k, g in ((0, 0), (4, 1))}
    for k in range(5):  # whatever a library makes of a job, it stays inside the two buffers
        first = (int(j["src_offset"][k]) + skip) % 2**64
        assert 0 <= first and first + int(j["size"][k]) + 256 <= buf.size
        assert int(j["dest_offset"][k]) + int(j["size"][k]) <= 40000
    return buf, skip, src_len, j, good, crcs, 40000


@pytest.mark.parametrize("form", ["whole", "segmented", "verify"])
def test_wrapped_ranges_are_refused(gpu_ctx, oracle, pool, form):
    """A, B and C get TFS_EXIT_PARAMETER_ERROR and nothing of them is written; their neighbours are exact.  With
    8 KiB segments B, when it is not refused, is split by the plan kernel, whose own range check is the second
    place the sum was formed."""
    buf, skip, src_len, j, good, crcs, dest_cap = wrapped_case(oracle)
    d_buf = pool.buf(buf.size, buf)
    before = M.prefill(dest_cap + SLACK)
    d_dst = pool.buf(before.size, before)
    d_j, d_c, d_s, d_b = pool.buf(j.nbytes, j), pool.buf(4 * 5), pool.buf(4 * 5), pool.buf(4)
    gpu_ctx.set_compact_segment(8192 if form == "segmented" else 1)
    try:
        if form == "verify":
            gpu_ctx.blocks_verify_device(d_buf.ptr + skip, src_len, d_j, 5, d_c, d_s, d_b)
        else:
            gpu_ctx.compact_jobs_device(d_buf.ptr + skip, src_len, d_j, 5, d_dst, d_c, d_s, d_b)
        gpu_ctx.sync()
    finally:
        gpu_ctx.set_compact_segment(1)
    st = d_s.download(np.int32, 5).tolist()
    assert st == [0, PARAM, PARAM, PARAM, 0], "statuses of G1, A, B, C, G2"
    assert int(d_b.download(np.uint32, 1)[0]) == 3
    c = d_c.download(np.uint32, 5)
    assert {k: int(c[k]) for k in crcs} == crcs
    exp = before.copy()
    if form != "verify":
        for k, rec in good.items():
            o = int(j["dest_offset"][k])
            exp[o:o + rec.size] = rec
    got = d_dst.download(np.uint8, before.size)
    diff = np.nonzero(got != exp)[0]
    assert diff.size == 0, (int(diff[0]), int(diff.size))
    assert (d_buf.download(np.uint8, buf.size) == buf).all()
