"""File repair (include/tfs_repair.h) on the GPU: reply frames built in Python
(tfs_amd.packet.read_reply_frame, sealed with the oracle's CRC) go in; every outgoing frame is held
byte for byte against a WriteDataMessage frame built in Python, every byte of out outside the
spans against the prefill, the source against its copy, and every result field against a model of
the header's rules that reads the frames' own bytes -- through the device form, the host form with
pageable buffers and the host form with page-locked buffers -- and the loop is closed with the
receiver, tfs_packet_verify_write.  Everything is bit-exact."""
import struct
import zlib

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

PARAM, SIZE_ERR, SYNC_ERR, CRC_ERR, TFS_ERROR = -1016, -8034, -8038, -1010, -1
FLAG = pk.TFS_PACKET_FLAG_V1
NONE = 0xFFFFFFFF
M64 = 2**64 - 1
IN_LENS = (700, 1024, 1500)
A_LENS = (1, 2, 15, 16, 17, 699, 700, 701, 1023, 1024, 1025, 2048, 2049, 3000)
A_DS = (0, 1, 3, 27)
PCODES = (8, 39, 63)


def zcrc(seed, data):
    return zlib.crc32(bytes(data), seed ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def prefill(n):
    return ((np.arange(n, dtype=np.uint64) * 131 + 7) % 251).astype(np.uint8)


def cut(n, lens, start=0):
    """The data lengths of the reply frames that carry n bytes, cycling through `lens`."""
    out, k = [], start
    while n > 0:
        out.append(min(n, lens[k % len(lens)]))
        n -= out[-1]
        k += 1
    return out


class Batch:
    """A source of reply frames and the jobs over it.  add() appends one file; the tamper hooks
    change the source or the declarations afterwards."""

    def __init__(self, oracle, cfg, ds, seed=5):
        self.oracle, self.cfg, self.ds, self.seed = oracle, cfg, ds, seed
        self.parts, self.pos, self.nframes = [], 0, 0
        self.ins, self.jobs, self.pays = [], [], []
        self.out_at = 0

    def add(self, n, in_lens, pcode, in_version, ds_count, out_residue, gap=9):
        import tfs_amd.crc as crc
        i = len(self.jobs)
        pay = synth_bytes(self.seed * 1000 + i, n).tobytes()
        fcrc = ocrc(self.oracle, 0, pay)
        fi = struct.pack("<QiiiiiiI", 0x5EED00000000 + 977 * i, 64 + i, n + 36, n + 36, 1700000000 + i, 1600000000 + i,
                         0, fcrc)
        in_first, at = len(self.ins), 0
        for k, nk in enumerate(in_lens):
            r = (5 * self.nframes + 1) % 16  # every residue mod 16 over 16 consecutive frames
            g = (r - self.pos) % 16 or (16 if self.nframes % 3 == 0 else 0)
            self.parts.append(((np.arange(g, dtype=np.uint64) * 37 + self.pos) % 253).astype(np.uint8))
            self.pos += g
            body = pk.read_reply_body(pay[at:at + nk], pcode, fi if k == 0 else None)
            c = ocrc(self.oracle, FLAG, body) if in_version >= 1 else 0
            assert in_version < 1 or c == zcrc(FLAG, body)
            f = np.frombuffer(pk.frame_v1(body, pcode, in_version, 7000 + self.nframes, c), np.uint8)
            rc, d = crc.repair_parse(f, pcode, k == 0, frame_off=self.pos)
            assert rc == 0 and int(d["avail"][0]) == f.size == 28 + nk + int(d["trailer"][0])
            self.ins.append(d[0].copy())
            self.parts.append(f)
            self.pos += f.size
            self.nframes += 1
            at += nk
        j = np.zeros(1, crc.REPAIR_JOB_DTYPE)
        j["file_id"], j["stat_size"] = 0x5EED00000000 + 977 * i, sum(in_lens)
        j["file_number"] = 0xF11E000000000000 + 31 * i
        j["packet_id"] = (0xFFFFFFFFFFFFFFF0 + 3 * i) & M64  # (some ids wrap: the header id is mod 2^64)
        j["block_id"] = 0x00C0FFEE + i
        j["in_first"], j["in_count"] = in_first, len(in_lens)
        j["ds_count"] = ds_count
        j["ds_first"] = (7 * i) % (len(self.ds) - ds_count + 1)
        j["stat_crc"] = j["check_crc"] = fcrc
        self.out_at += gap + (out_residue - (self.out_at + gap)) % 16
        j["frame_offset"] = self.out_at
        self.out_at += crc.repair_span(self.cfg, j)
        self.jobs.append(j[0].copy())
        self.pays.append(pay)
        return i

    def finish(self):
        import tfs_amd.crc as crc
        self.parts.append(np.full(5, 0xA5, np.uint8))
        self.src = np.concatenate(self.parts)
        self.ins = np.array(self.ins, crc.REPAIR_IN_DTYPE)
        self.jobs = np.array(self.jobs, crc.REPAIR_JOB_DTYPE)
        self.cap = self.out_at + 40
        return self

    def frame(self, job, k):
        """(offset, declaration) of incoming frame k of a job."""
        d = self.ins[int(self.jobs["in_first"][job]) + k]
        return int(d["frame_off"]), d

    def reseal(self, job, k):
        """The header CRC of the frame's bytes as they now lie (a tamper that is not to show as a CRC error)."""
        o, d = self.frame(job, k)
        blen = 4 + int(d["data_len"]) + int(d["trailer"])
        struct.pack_into("<I", self.src, o + 20, ocrc(self.oracle, FLAG, self.src[o + 24:o + 24 + blen].tobytes()))


def expected_frames(oracle, b, i):
    """[frame bytes] of job i, by the header's rules, from the payload the frames declare."""
    c, j = b.cfg[0], b.jobs[i]
    fl, ver, cnt = int(c["frame_len"]), int(c["version"]), int(j["ds_count"])
    pay = declared_payload(b, i)
    frames, off, k = [], 0, 0
    while off < len(pay):
        ln = min(fl, len(pay) - off)
        body = pk.write_data_body(int(j["block_id"]), int(j["file_id"]), off, pay[off:off + ln], int(c["is_server"]),
                                  int(j["file_number"]), [int(d) for d in b.ds[int(j["ds_first"]):][:cnt]])
        assert len(body) == 36 + 8 * cnt + ln
        crc = ocrc(oracle, FLAG, body) if ver >= 1 else 0
        assert ver < 1 or crc == zcrc(FLAG, body)
        frames.append(np.frombuffer(pk.frame_v1(body, 9, ver, (int(j["packet_id"]) + k) & M64, crc), np.uint8))
        off += ln
        k += 1
    return frames


def declared_payload(b, i):
    j = b.jobs[i]
    return b"".join(b.src[int(d["frame_off"]) + 28:int(d["frame_off"]) + 28 + int(d["data_len"])].tobytes()
                    for d in b.ins[int(j["in_first"]):int(j["in_first"]) + int(j["in_count"])])


def expected_result(oracle, b, i, src_len=None, out_cap=None):
    """(status, n_frames, span_len, file_crc, bad_in, flags) of job i: include/tfs_repair.h's rows in order."""
    import tfs_amd.crc as crc
    src_len = b.src.size if src_len is None else src_len
    out_cap = b.cap if out_cap is None else out_cap
    j = b.jobs[i]
    cnt, n0, nin = int(j["ds_count"]), int(j["in_first"]), int(j["in_count"])
    refused = lambda s: (s, 0, 0, 0, NONE, 0)
    if cnt > 27 or int(j["ds_first"]) + cnt > len(b.ds) or nin == 0 or n0 + nin > len(b.ins):
        return refused(PARAM)
    ins = b.ins[n0:n0 + nin]
    for d in ins:
        need = 28 + int(d["data_len"]) + int(d["trailer"])
        good_trailer = int(d["trailer"]) == 0 if int(d["pcode"]) == 8 else int(d["trailer"]) in (4, 40)
        if int(d["data_len"]) < 0 or int(d["avail"]) < need or int(d["frame_off"]) + int(d["avail"]) > src_len or \
                int(d["pcode"]) not in PCODES or not good_trailer or int(d["reserved"]):
            return refused(PARAM)
    span = crc.repair_span(b.cfg, b.jobs[i:i + 1])
    if (span and (int(j["frame_offset"]) + span > out_cap or span > 0xFFFFFFFF)) or int(j["reserved"]):
        return refused(PARAM)
    if int(j["stat_size"]) <= 0:
        return refused(SIZE_ERR)
    if sum(int(d["data_len"]) for d in ins) != int(j["stat_size"]):
        return refused(SYNC_ERR)
    pay = declared_payload(b, i)
    fcrc = ocrc(oracle, 0, pay)
    assert fcrc == zcrc(0, pay)
    for k, d in enumerate(ins):
        o, n, t = int(d["frame_off"]), int(d["data_len"]), int(d["trailer"])
        flag, blen, pcode, ver, _, hcrc = struct.unpack_from("<IihhQI", b.src, o)
        body = b.src[o + 24:o + 28 + n + t].tobytes()
        lead = struct.unpack_from("<i", body, 4 + n)[0] if t else None
        if flag != FLAG or blen != 4 + n + t or pcode != int(d["pcode"]) or struct.unpack_from("<i", body)[0] != n or \
                (t == 40 and lead != 36) or (t == 4 and lead != 0):
            return TFS_ERROR, 0, 0, fcrc, k, 0
        if ver >= 1 and hcrc != ocrc(oracle, FLAG, body):
            return CRC_ERR, 0, 0, fcrc, k, 0
    flags = (1 if fcrc != int(j["stat_crc"]) else 0) | (2 if fcrc != int(j["check_crc"]) else 0)
    if flags:
        return CRC_ERR, 0, 0, fcrc, NONE, flags
    return 0, crc.repair_frame_count(b.cfg, int(j["stat_size"])), span, fcrc, NONE, 0


def check_call(oracle, b, out, before, results, nbad, src_len=None):
    """Frames, untouched bytes and every result field of one call."""
    touched = np.zeros(out.size, bool)
    want_bad, all_frames = 0, []
    for i in range(len(b.jobs)):
        want = expected_result(oracle, b, i, src_len, out.size)
        got = tuple(int(results[i][k]) for k in ("status", "n_frames", "span_len", "file_crc", "bad_in", "flags"))
        assert got == want, (i, got, want)
        want_bad += want[0] != 0
        if want[0] in (PARAM, SIZE_ERR, SYNC_ERR):
            all_frames.append([])
            continue
        frames = expected_frames(oracle, b, i)
        o = o0 = int(b.jobs["frame_offset"][i])
        if want[0] != 0:  # no usable frame: every flag word zero, the rest of the span unspecified
            for f in frames:
                assert not out[o:o + 4].any(), (i, o)
                o += f.size
            touched[o0:o] = True
            all_frames.append([])
            continue
        assert sum(f.size for f in frames) == want[2] and len(frames) == want[1]
        for k, f in enumerate(frames):
            g = out[o:o + f.size]
            if not (g == f).all():
                raise AssertionError("job %d frame %d differs at byte %d of %d" % (i, k, int(np.nonzero(g != f)[0][0]), f.size))
            touched[o:o + f.size] = True
            o += f.size
        all_frames.append(frames)
    assert (out[~touched] == before[~touched]).all(), "a byte outside the spans was written"
    assert nbad == want_bad
    return all_frames


def run_device(ctx, b, src_len=None, d_nbad=None, stream=None, sync=None):
    import tfs_amd.crc as crc
    before = prefill(b.cap)
    d_src = crc.DeviceBuffer(ctx, b.src.size + 256).upload(b.src)
    d_out = crc.DeviceBuffer(ctx, b.cap + 16).upload(before)
    d_res = crc.DeviceBuffer(ctx, max(len(b.jobs), 1) * 24)
    own = d_nbad is None
    if own:
        d_nbad = crc.DeviceBuffer(ctx, 4)
        d_nbad.zero()
    assert ctx.L.tfs_crc32_sync(ctx.handle) == 0
    ctx.repair_frames_device(b.cfg, d_src, b.src.size if src_len is None else src_len, b.ins, b.jobs, b.ds, d_out, b.cap,
                             d_res, d_nbad, stream=stream)
    if sync is None:
        assert ctx.L.tfs_crc32_sync(ctx.handle) == 0
    else:
        sync()
    out = d_out.download(np.uint8, b.cap)
    res = d_res.download(crc.REPAIR_RESULT_DTYPE, len(b.jobs))
    nbad = int(d_nbad.download(np.uint32, 1)[0])
    assert (d_src.download(np.uint8, b.src.size) == b.src).all(), "the source was written"
    d_src.free(), d_out.free(), d_res.free()
    if own:
        d_nbad.free()
    return out, before, res, nbad


def run_host(ctx, b, pin_src, pin_out):
    import tfs_amd.crc as crc
    before = prefill(b.cap)
    src, out, bufs = b.src.copy(), before.copy(), []
    if pin_src:
        src = crc.PinnedBuffer(ctx, b.src.size)
        src.array[:] = b.src
        bufs.append(src)
    if pin_out:
        out = crc.PinnedBuffer(ctx, b.cap)
        out.array[:] = before
        bufs.append(out)
    res, nbad, rc = ctx.repair_frames(b.cfg, src, b.ins, b.jobs, b.ds, out)
    got = (out.array if pin_out else out).copy()
    assert ((src.array if pin_src else src) == b.src).all(), "the source was written"
    for x in bufs:
        x.free()
    return got, before, res, nbad, rc


def geometry_a(oracle, version):
    """Cuts below one segment: frame_len 1024, reply frames of 700, 1024 and 1500 data bytes."""
    import tfs_amd.crc as crc
    cfg = crc.repair_cfg(1024, is_server=version // 2, version=version)
    ds = (np.arange(40, dtype=np.uint64) * np.uint64(0x0101010101010101)) ^ np.uint64(0xD5D5000000000000)
    b = Batch(oracle, cfg, ds)
    for i in range(3 * len(A_LENS)):
        n = A_LENS[i % len(A_LENS)]
        b.add(n, cut(n, IN_LENS, start=i), PCODES[i % 3], 2 * ((i // 3) % 2), A_DS[i % 4], (5 * i + 3) % 16)
    b.finish()
    assert {int(f) % 16 for f in b.ins["frame_off"]} == set(range(16))
    assert {int(f) % 16 for f in b.jobs["frame_offset"]} == set(range(16))
    assert {int(c) for c in b.jobs["ds_count"]} == set(A_DS) and {int(p) for p in b.ins["pcode"]} == set(PCODES)
    first = b.ins[b.jobs["in_first"]]
    assert all(int(t) == (0 if int(p) == 8 else 40) for t, p in zip(first["trailer"], first["pcode"]))
    later = np.delete(b.ins, b.jobs["in_first"])
    assert len(later) and all(int(t) == (0 if int(p) == 8 else 4) for t, p in zip(later["trailer"], later["pcode"]))
    versions = {(int(p), struct.unpack_from("<h", b.src, int(o) + 10)[0]) for p, o in zip(b.ins["pcode"], b.ins["frame_off"])}
    assert versions == {(p, v) for p in PCODES for v in (0, 2)}
    counts = {n: crc.repair_frame_count(cfg, n) for n in A_LENS}
    assert (counts[1023], counts[1024], counts[1025], counts[2048], counts[2049], counts[3000]) == (1, 1, 2, 2, 3, 3)
    return b


@pytest.fixture(scope="module")
def geo_a(oracle):
    return {v: geometry_a(oracle, v) for v in (0, 2)}


@pytest.fixture(scope="module")
def geo_b(oracle):
    """All three kinds of cut, a call each (frame_len belongs to the call)."""
    import tfs_amd.crc as crc
    ds = np.arange(1, 30, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    out = []
    for n, in_len, frame_len, pcode, cnt, nf in ((50001, 20000, 18000, 39, 2, 3), (50000, 50000, 50000, 8, 27, 1),
                                                 (33000, 16384, 16384, 63, 0, 3)):
        cfg = crc.repair_cfg(frame_len, is_server=1, version=2)
        b = Batch(oracle, cfg, ds, seed=9 + len(out))
        b.add(n, cut(n, (in_len,)), pcode, 2, cnt, 3 + 5 * len(out))
        b.finish()
        assert crc.repair_frame_count(cfg, n) == nf == -(-n // frame_len)
        assert crc.repair_span(cfg, b.jobs[:1]) == nf * (60 + 8 * cnt) + n
        assert int(b.jobs["in_count"][0]) == -(-n // in_len)
        out.append(b)
    return out


# ---- 1. both geometries, the three forms ---------------------------------------------------

@pytest.mark.parametrize("version", [0, 2])
def test_geometry_a_device_form(gpu_ctx, oracle, geo_a, version):
    b = geo_a[version]
    out, before, res, nbad = run_device(gpu_ctx, b)
    frames = check_call(oracle, b, out, before, res, nbad)
    assert nbad == 0 and (res["status"] == 0).all()
    if version == 0:
        assert all(struct.unpack_from("<I", f, 20)[0] == 0 for fs in frames for f in fs)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_geometry_b_device_form(gpu_ctx, oracle, geo_b, which):
    b = geo_b[which]
    out, before, res, nbad = run_device(gpu_ctx, b)
    check_call(oracle, b, out, before, res, nbad)
    assert res["n_frames"].tolist() == [(3, 1, 3)[which]] and nbad == 0


@pytest.mark.parametrize("pin_src,pin_out", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("which", ["a", "b0", "b1", "b2"])
def test_host_forms_equal_device_form(gpu_ctx, oracle, geo_a, geo_b, which, pin_src, pin_out):
    b = geo_a[2] if which == "a" else geo_b[int(which[1])]
    dev_out, _, dev_res, _ = run_device(gpu_ctx, b)
    out, before, res, nbad, rc = run_host(gpu_ctx, b, pin_src, pin_out)
    assert rc == 0
    check_call(oracle, b, out, before, res, nbad)
    assert (out == dev_out).all() and (res == dev_res).all()


def test_host_form_in_pieces(gpu_ctx, oracle, geo_a):
    """A staging piece smaller than the batch: the host form goes in several launches."""
    b = geo_a[2]
    gpu_ctx.read_set_piece(4096)
    try:
        out, before, res, nbad, rc = run_host(gpu_ctx, b, False, False)
    finally:
        gpu_ctx.read_set_piece(0)
    assert rc == 0
    check_call(oracle, b, out, before, res, nbad)


# ---- 2. the loop closed with the receiver --------------------------------------------------

@pytest.mark.parametrize("which", ["a", "b0", "b1", "b2"])
def test_frames_pass_the_receivers_check(gpu_ctx, oracle, geo_a, geo_b, which):
    import tfs_amd.crc as crc
    b = geo_a[2] if which == "a" else geo_b[int(which[1])]
    out, before, res, nbad = run_device(gpu_ctx, b)
    offs, lens, owner = [], [], []
    for i, j in enumerate(b.jobs):
        o = int(j["frame_offset"])
        for k in range(int(res[i]["n_frames"])):
            body_len = struct.unpack_from("<I", out, o + 4)[0]
            offs.append(o), lens.append(24 + body_len), owner.append(i)
            o += 24 + body_len
        assert o == int(j["frame_offset"]) + int(res[i]["span_len"])
    fcrc, st, bad, rc, parts = gpu_ctx.packet_verify_write(out, offs, lens)
    assert rc == 0 and bad == 0 and (st == 0).all()
    for i, j in enumerate(b.jobs):
        acc, data = 0, b""
        for k in [k for k, w in enumerate(owner) if w == i]:
            assert int(parts[k]["data_len"]) >= 1 and int(parts[k]["data_off"]) == 36 + 8 * int(j["ds_count"])
            acc = crc.combine(acc, int(parts[k]["data_crc"]), int(parts[k]["data_len"]))
            at = offs[k] + 24 + int(parts[k]["data_off"])
            data += out[at:at + int(parts[k]["data_len"])].tobytes()
        assert data == b.pays[i]
        assert acc == int(res[i]["file_crc"]) == int(j["stat_crc"])


# ---- 3. failures, their neighbours untouched and correct -----------------------------------

def failure_batch(oracle):
    import tfs_amd.crc as crc
    cfg = crc.repair_cfg(1024, version=2)
    ds = np.arange(3, 40, dtype=np.uint64) * np.uint64(0xABCDEF0123456789)
    b = Batch(oracle, cfg, ds, seed=11)
    #        pcode, incoming version
    plan = [(8, 2),    # 0 good
            (8, 2),    # 1 a data byte flipped in frame 1 of 3
            (39, 0),   # 2 the same in version-0 frames: only the file CRC can tell
            (63, 2),   # 3 stat_crc wrong
            (39, 2),   # 4 good
            (8, 0),    # 5 check_crc wrong
            (39, 2),   # 6 a trailer FileInfo byte flipped
            (8, 2),    # 7 a wrong flag word
            (63, 2),   # 8 header body length off by one (frame 2)
            (63, 0),   # 9 good
            (39, 2),   # 10 header pcode 63, declared 39
            (8, 2),    # 11 body le32 != the declared length (frame 1), resealed
            (63, 2),   # 12 trailer le32 35, resealed
            (8, 2),    # 13 lengths sum to stat_size - 1
            (39, 2),   # 14 stat_size 0
            (8, 2)]    # 15 good
    for i, (pcode, ver) in enumerate(plan):
        b.add(3000, cut(3000, IN_LENS, start=i), pcode, ver, (2, 0, 27, 1)[i % 4], (7 * i + 2) % 16)
    b.finish()
    assert all(int(c) == 3 for c in b.jobs["in_count"])
    b.src[b.frame(1, 1)[0] + 28 + 300] ^= 0x10
    b.src[b.frame(2, 1)[0] + 28 + 300] ^= 0x10
    b.jobs["stat_crc"][3] ^= 1
    b.jobs["check_crc"][5] ^= 0x80000000
    o, d = b.frame(6, 0)
    b.src[o + 28 + int(d["data_len"]) + 4 + 20] ^= 0x01
    struct.pack_into("<I", b.src, b.frame(7, 0)[0], pk.TFS_PACKET_FLAG_V0)
    o, d = b.frame(8, 2)
    struct.pack_into("<i", b.src, o + 4, 4 + int(d["data_len"]) + int(d["trailer"]) + 1)
    struct.pack_into("<h", b.src, b.frame(10, 0)[0] + 8, 63)
    o, d = b.frame(11, 1)
    struct.pack_into("<i", b.src, o + 24, int(d["data_len"]) - 1)
    b.reseal(11, 1)
    o, d = b.frame(12, 0)
    struct.pack_into("<i", b.src, o + 28 + int(d["data_len"]), 35)
    b.reseal(12, 0)
    b.jobs["stat_size"][13] += 1
    b.jobs["stat_size"][14] = 0
    want = [0, CRC_ERR, CRC_ERR, CRC_ERR, 0, CRC_ERR, CRC_ERR, TFS_ERROR, TFS_ERROR, 0, TFS_ERROR, TFS_ERROR, TFS_ERROR,
            SYNC_ERR, SIZE_ERR, 0]
    bad_in = [NONE, 1, NONE, NONE, NONE, NONE, 0, 0, 2, NONE, 0, 1, 0, NONE, NONE, NONE]
    flags = [0, 0, 3, 1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    return b, want, bad_in, flags


@pytest.fixture(scope="module")
def failures(oracle):
    return failure_batch(oracle)


@pytest.mark.parametrize("form", ["device", "pageable", "pinned"])
def test_failures_in_one_batch(gpu_ctx, oracle, failures, form):
    b, want, bad_in, flags = failures
    if form == "device":
        out, before, res, nbad = run_device(gpu_ctx, b)
    else:
        out, before, res, nbad, rc = run_host(gpu_ctx, b, form == "pinned", form == "pinned")
        assert rc == CRC_ERR
    assert res["status"].tolist() == want
    assert res["bad_in"].tolist() == bad_in and res["flags"].tolist() == flags
    check_call(oracle, b, out, before, res, nbad)  # also file_crc, the flag words and the neighbours
    assert nbad == sum(1 for w in want if w)
    bad = res["status"] != 0
    assert not res["n_frames"][bad].any() and not res["span_len"][bad].any()
    for i in (1, 2, 3, 5, 6, 7, 8, 10, 11, 12):  # three frames each, every flag word zero; file_crc as computed
        o = int(b.jobs["frame_offset"][i])
        head = 60 + 8 * int(b.jobs["ds_count"][i])
        for ln in (1024, 1024, 952):
            assert not out[o:o + 4].any()
            o += head + ln
        assert int(res["file_crc"][i]) == ocrc(oracle, 0, declared_payload(b, i))
    for i in (13, 14):
        assert int(res["file_crc"][i]) == 0


def test_two_failing_frames_report_the_lower(gpu_ctx, oracle):
    import tfs_amd.crc as crc
    cfg = crc.repair_cfg(1024, version=2)
    b = Batch(oracle, cfg, np.arange(4, dtype=np.uint64), seed=13)
    for i in range(3):
        b.add(3000, cut(3000, IN_LENS, start=i), 39, 2, 1, 4 * i)
    b.finish()
    b.src[b.frame(0, 1)[0] + 28 + 5] ^= 0x40                                  # frame 1: CRC; frame 2: shape
    struct.pack_into("<I", b.src, b.frame(0, 2)[0], 0)
    struct.pack_into("<I", b.src, b.frame(2, 0)[0], 0)                        # frame 0: shape; frame 2: CRC
    b.src[b.frame(2, 2)[0] + 28 + 5] ^= 0x40
    out, before, res, nbad = run_device(gpu_ctx, b)
    check_call(oracle, b, out, before, res, nbad)
    assert res["status"].tolist() == [CRC_ERR, 0, TFS_ERROR] and res["bad_in"].tolist() == [1, NONE, 0]


# ---- 4. counters, refusals, streams --------------------------------------------------------

def test_n_bad_accumulates_across_calls(gpu_ctx, oracle, failures):
    import tfs_amd.crc as crc
    b, want, _, _ = failures
    d_nbad = crc.DeviceBuffer(gpu_ctx, 4)
    d_nbad.zero()
    per = sum(1 for w in want if w)
    _, _, _, n1 = run_device(gpu_ctx, b, d_nbad=d_nbad)
    _, _, _, n2 = run_device(gpu_ctx, b, d_nbad=d_nbad)
    d_nbad.free()
    assert (n1, n2) == (per, 2 * per)
    # the host form adds to the caller's word
    res = np.zeros(len(b.jobs), crc.REPAIR_RESULT_DTYPE)
    nbad = np.array([100], np.uint32)
    out = prefill(b.cap)
    for k in (1, 2):
        rc = gpu_ctx.L.tfs_repair_frames(gpu_ctx.handle, b.cfg.ctypes.data, b.src.ctypes.data, b.src.size,
                                         b.ins.ctypes.data, len(b.ins), b.jobs.ctypes.data, len(b.jobs), b.ds.ctypes.data,
                                         len(b.ds), out.ctypes.data, b.cap, res.ctypes.data, nbad.ctypes.data)
        assert rc == CRC_ERR and int(nbad[0]) == 100 + k * per


def test_per_job_refusals_before_reading(gpu_ctx, oracle, geo_a):
    """Each host-decided PARAMETER_ERROR row on one job of a sound batch: that job alone is refused."""
    import copy
    base = geo_a[2]
    cases = []

    def case(fn):
        b = copy.copy(base)
        b.ins, b.jobs = base.ins.copy(), base.jobs.copy()
        fn(b)
        cases.append(b)
    case(lambda b: b.jobs["ds_count"].__setitem__(5, 28))
    case(lambda b: b.jobs["ds_first"].__setitem__(5, len(b.ds)))
    case(lambda b: b.jobs["in_count"].__setitem__(5, 0))
    case(lambda b: b.jobs["in_first"].__setitem__(5, len(b.ins)))
    case(lambda b: b.jobs["reserved"].__setitem__(5, 1))
    case(lambda b: b.jobs["frame_offset"].__setitem__(5, b.cap - 10))
    k = int(base.jobs["in_first"][5])
    case(lambda b: b.ins["data_len"].__setitem__(k, -1))
    case(lambda b: b.ins["avail"].__setitem__(k, int(b.ins["avail"][k]) - 1))
    case(lambda b: b.ins["frame_off"].__setitem__(k, b.src.size - 10))
    case(lambda b: b.ins["pcode"].__setitem__(k, 9))
    case(lambda b: b.ins["trailer"].__setitem__(k, 4 if int(b.ins["pcode"][k]) == 8 else 0))
    case(lambda b: b.ins["reserved"].__setitem__(k, 7))
    for n, b in enumerate(cases):
        out, before, res, nbad = run_device(gpu_ctx, b)
        assert [i for i, s in enumerate(res["status"]) if s != 0] == [5] and int(res["status"][5]) == PARAM, n
        check_call(oracle, b, out, before, res, nbad)


@pytest.mark.parametrize("form", ["device", "host"])
def test_overlapping_spans_refuse_the_call(gpu_ctx, oracle, geo_a, form):
    import copy
    import tfs_amd.crc as crc
    b = copy.copy(geo_a[2])
    b.jobs = b.jobs.copy()
    b.jobs["frame_offset"][20] = int(b.jobs["frame_offset"][19]) + crc.repair_span(b.cfg, b.jobs[19:20]) - 1
    with pytest.raises(crc.TfsCrcError) as e:
        if form == "device":
            run_device(gpu_ctx, b)
        else:
            run_host(gpu_ctx, b, False, False)
    assert e.value.code == PARAM
    # nothing launched, nothing written
    before = prefill(b.cap)
    out = before.copy()
    res = np.zeros(len(b.jobs), crc.REPAIR_RESULT_DTYPE)
    nbad = np.zeros(1, np.uint32)
    rc = gpu_ctx.L.tfs_repair_frames(gpu_ctx.handle, b.cfg.ctypes.data, b.src.ctypes.data, b.src.size, b.ins.ctypes.data,
                                     len(b.ins), b.jobs.ctypes.data, len(b.jobs), b.ds.ctypes.data, len(b.ds),
                                     out.ctypes.data, b.cap, res.ctypes.data, nbad.ctypes.data)
    assert rc == PARAM and (out == before).all() and not res.view(np.uint8).any() and nbad[0] == 0


def test_call_level_refusals(gpu_ctx, geo_a):
    import tfs_amd.crc as crc
    b = geo_a[2]
    L, h = gpu_ctx.L, gpu_ctx.handle
    out = prefill(b.cap)
    before = out.copy()
    res = np.zeros(len(b.jobs), crc.REPAIR_RESULT_DTYPE)
    good = dict(cfg=b.cfg.ctypes.data, src=b.src.ctypes.data, ins=b.ins.ctypes.data, jobs=b.jobs.ctypes.data,
                ds=b.ds.ctypes.data, out=out.ctypes.data, res=res.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return L.tfs_repair_frames(h, a["cfg"], a["src"], b.src.size, a["ins"], len(b.ins), a["jobs"], len(b.jobs),
                                   a["ds"], len(b.ds), a["out"], b.cap, a["res"], None)
    for k in ("cfg", "ins", "jobs", "ds", "out", "res", "src"):
        assert call(**{k: None}) == PARAM, k
    for bad in (crc.repair_cfg(0), crc.repair_cfg(-1), crc.repair_cfg(1024, reserved=1)):
        assert call(cfg=bad.ctypes.data) == PARAM
    assert (out == before).all() and not res.view(np.uint8).any()
    # n == 0 with no frames and an empty ds array are legal
    assert L.tfs_repair_frames(h, b.cfg.ctypes.data, b.src.ctypes.data, b.src.size, None, 0, None, 0, None, 0,
                               out.ctypes.data, b.cap, res.ctypes.data, None) == 0
    assert (out == before).all()


def test_a_callers_stream(gpu_ctx, oracle, failures):
    """On a stream of the caller's the results are complete after that stream's sync; hipStreamPerThread is refused."""
    import tfs_amd.crc as crc
    b, want, _, _ = failures
    s = gpu_ctx.stream_create()
    try:
        out, before, res, nbad = run_device(gpu_ctx, b, stream=s, sync=lambda: gpu_ctx.stream_sync(s))
        assert res["status"].tolist() == want
        check_call(oracle, b, out, before, res, nbad)
    finally:
        gpu_ctx.stream_destroy(s)
    with pytest.raises(crc.TfsCrcError) as e:
        run_device(gpu_ctx, b, stream=2)  # hipStreamPerThread
    assert e.value.code == PARAM
