"""Read replies (include/tfs_read.h) on the GPU: every frame byte for byte
against a frame built in Python from the block image's bytes -- the status from
oracle_verify_file (and the id / short-record / parameter checks that come before it), the
body laid out as the header specifies, the CRC written by oracle_packet_seal and
cross-checked with ~zlib.crc32 -- and every result word, through the device form, the
zero-copy host form and the staged host forms."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

PARAM, SIZE_ERR, INFO_ERR, SYNC_ERR, CRC_ERR = -1016, -8034, -8016, -8038, -1010
PCODES = (8, 39, 63)
FLAG = pk.TFS_PACKET_FLAG_V1


def build_image(oracle, sizes, pay_mod=None, seed=5, tail=0):
    """FileInfo|payload records; record k's payload starts at an offset congruent to pay_mod[k]
    mod 16 (None: packed).  Returns (image, [(file_id, offset, size)]); `tail` bytes follow."""
    import tfs_amd.crc as crc
    recs, parts, o = [], [], 0
    for k, s in enumerate(sizes):
        if pay_mod is not None:
            gap = (pay_mod[k] - (o + 36)) % 16
            parts.append(np.full(gap, 0xEE, np.uint8))
            o += gap
        pay = synth_bytes(seed * 1000 + k, s)
        fi = np.zeros(1, crc.FILEINFO_DTYPE)
        fi["id_"], fi["offset_"], fi["size_"], fi["usize_"] = 5000 + k, o & 0x7FFFFFFF, s + 36, s + 36
        fi["modify_time_"], fi["create_time_"], fi["flag_"] = 1700000000 + k, 1600000000 + k, 0
        fi["crc_"] = ocrc(oracle, 0, pay.tobytes())
        parts += [fi.view(np.uint8).copy(), pay]
        recs.append((5000 + k, o, s + 36))
        o += 36 + s
    parts.append(np.full(tail, 0xEE, np.uint8))
    return np.concatenate(parts), recs


def make_jobs(specs):
    """specs: dicts with src_offset, frame_offset, file_id, size and optional read fields."""
    import tfs_amd.crc as crc
    j = np.zeros(len(specs), crc.READ_JOB_DTYPE)
    for k, s in enumerate(specs):
        j[k]["src_offset"], j[k]["frame_offset"], j[k]["file_id"] = s["src_offset"], s["frame_offset"], s["file_id"]
        j[k]["packet_id"] = s.get("packet_id", 0x1122334455660000 + k)
        j[k]["size"], j[k]["read_offset"] = s["size"], s.get("read_offset", 0)
        j[k]["read_len"] = s.get("read_len", max(s["size"] - 36, 0))
        j[k]["pcode"], j[k]["version"] = s.get("pcode", 39), s.get("version", 2)
    return j


def cap_of(job):
    import tfs_amd.crc as crc
    return crc.read_frame_cap(job)


def zcrc(seed, data):
    return zlib.crc32(bytes(data), seed ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def seal(oracle, frame):
    b = np.frombuffer(bytes(frame), np.uint8).copy()
    off, av = np.zeros(1, np.uint64), np.array([b.size], np.uint32)
    c, st = np.zeros(1, np.uint32), np.zeros(1, np.int32)
    oracle.oracle_packet_seal(b.ctypes.data, off.ctypes.data, av.ctypes.data, 1, c.ctypes.data, st.ctypes.data)
    assert st[0] == 0
    assert struct.unpack_from("<I", b, 20)[0] == zcrc(FLAG, b[24:].tobytes())
    return b


def expect(oracle, img, job, out_cap):
    """(status, frame bytes or None, file_crc, frame_crc) of one job by the header's rules."""
    so, fo, fid = int(job["src_offset"]), int(job["frame_offset"]), int(job["file_id"])
    size, ro, rl = int(job["size"]), int(job["read_offset"]), int(job["read_len"])
    pcode, ver = int(job["pcode"]), int(job["version"])
    if pcode not in PCODES or ro < 0 or rl < 0 or ro > max(size - 36, 0) or so + max(size, 0) > img.size \
            or fo + cap_of(job) > out_cap:
        return PARAM, None, 0, 0
    status, file_crc, n = 0, 0, 0
    if size < 36:
        status = SIZE_ERR
    else:
        n = min(rl, size - 36 - ro)
        whole = ro == 0 and n == size - 36
        info = img[so:so + 36].tobytes()
        id_, _, size_ = struct.unpack_from("<Qii", info)
        pay_crc = ocrc(oracle, 0, img[so + 36:so + size].tobytes())
        file_crc = pay_crc if whole else 0
        oc = ctypes.c_uint32()
        code = oracle.oracle_verify_file(img.ctypes.data, img.size, so, size, ctypes.byref(oc)) if size > 36 else \
            (SYNC_ERR if size_ != size else (CRC_ERR if struct.unpack_from("<I", info, 32)[0] != 0 else 0))
        if size > 36:
            assert oc.value == pay_crc
        if id_ != fid:
            status = INFO_ERR            # the id check comes before the oracle's helper's
        elif code == SYNC_ERR:
            status = SYNC_ERR
        elif whole and code == CRC_ERR:
            status = CRC_ERR             # a slice cannot be checked against crc_
    if status:
        body = struct.pack("<i", status) + (b"" if pcode == 8 else struct.pack("<i", 0))
    else:
        body = struct.pack("<i", n) + img[so + 36 + ro:so + 36 + ro + n].tobytes()
        if pcode != 8:
            if ro == 0:
                fi = bytearray(img[so:so + 36].tobytes())
                struct.pack_into("<i", fi, 12, struct.unpack_from("<i", fi, 12)[0] - 36)
                body += struct.pack("<i", 36) + bytes(fi)
            else:
                body += struct.pack("<i", 0)
    frame = pk.frame_v1(body, pcode, ver, int(job["packet_id"]))
    if ver >= 1:
        frame = seal(oracle, frame).tobytes()
    return status, frame, file_crc, struct.unpack_from("<I", frame, 20)[0]


def prefill(n):
    return ((np.arange(n, dtype=np.uint64) * 131 + 7) % 251).astype(np.uint8)


def check(oracle, img, jobs, out, res, out_cap, before):
    """Frames, results and every byte the call may not have touched."""
    touched = np.zeros(out_cap, bool)
    nbad = 0
    for k, job in enumerate(jobs):
        st, frame, fcrc, hcrc = expect(oracle, img, job, out_cap)
        r = res[k]
        assert int(r["status"]) == st, (k, int(r["status"]), st)
        nbad += st != 0
        if frame is None:
            assert int(r["frame_len"]) == 0 and int(r["file_crc"]) == 0 and int(r["frame_crc"]) == 0, k
            continue
        fo = int(job["frame_offset"])
        assert int(r["frame_len"]) == len(frame), (k, int(r["frame_len"]), len(frame))
        if st:
            assert len(frame) == (28 if int(job["pcode"]) == 8 else 32)
        assert int(r["file_crc"]) == fcrc and int(r["frame_crc"]) == hcrc, (k, hex(int(r["frame_crc"])), hex(hcrc))
        got = out[fo:fo + len(frame)].tobytes()
        if got != frame:
            bad = next(i for i in range(len(frame)) if got[i] != frame[i])
            raise AssertionError("job %d: frame differs at byte %d of %d" % (k, bad, len(frame)))
        touched[fo:fo + cap_of(job)] = True
    assert (out[~touched] == before[~touched]).all(), "a byte outside every span was written"
    return nbad


def run_device(ctx, img, jobs, out_cap, src_pad=0):
    import tfs_amd.crc as crc
    d_src = crc.DeviceBuffer(ctx, img.size + src_pad + 16).upload(img)
    before = prefill(out_cap)
    d_out = crc.DeviceBuffer(ctx, out_cap + 16).upload(before)
    d_res = crc.DeviceBuffer(ctx, 16 * len(jobs))
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.upload(np.array([3], np.uint32))      # n_bad is increased, not set
    ctx.read_reply_device(d_src, img.size, jobs, d_out, out_cap, d_res, d_bad)
    ctx.sync()
    return d_out.download(np.uint8, out_cap), d_res.download(crc.READ_RESULT_DTYPE, len(jobs)), before, \
        int(d_bad.download(np.uint32, 1)[0]) - 3


def run_host(ctx, img, jobs, out_cap, pin_src=False, pin_out=False):
    import tfs_amd.crc as crc
    before = prefill(out_cap)
    src, out, bufs = img, before.copy(), []
    if pin_src:
        src = crc.PinnedBuffer(ctx, img.size)
        src.array[:] = img
        bufs.append(src)
    if pin_out:
        out = crc.PinnedBuffer(ctx, out_cap)
        out.array[:] = before
        bufs.append(out)
    res, nbad, rc = ctx.read_reply(src, jobs, out)
    got = out.array.copy() if pin_out else out
    for b in bufs:
        b.free()
    return got, res, before, nbad, rc


def both_forms(ctx, oracle, img, jobs, out_cap):
    out, res, before, nbad = run_device(ctx, img, jobs, out_cap)
    want = check(oracle, img, jobs, out, res, out_cap, before)
    assert nbad == want
    out, res, before, nbad, rc = run_host(ctx, img, jobs, out_cap, True, True)
    assert check(oracle, img, jobs, out, res, out_cap, before) == want
    assert nbad == want and rc == (CRC_ERR if want else 0)
    return want


def packed(recs, **kw):
    """One job per record, frames packed back to back from a ragged start; returns (jobs, out_cap):
    the last frame ends at the last byte of out."""
    specs, fo = [], kw.pop("start", 3)
    for k, (fid, off, size) in enumerate(recs):
        s = dict(src_offset=off, frame_offset=fo, file_id=fid, size=size, **{a: (v[k] if isinstance(v, list) else v)
                                                                            for a, v in kw.items()})
        specs.append(s)
        fo += cap_of(make_jobs([s])[0])
    return make_jobs(specs), fo


LENGTHS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 5119, 5120, 5121, 6145, 65536, 65557,
           (1 << 20) + 13]


@pytest.fixture(scope="module")
def length_image(oracle):
    return build_image(oracle, LENGTHS, seed=11)


@pytest.mark.parametrize("pcode", PCODES)
def test_lengths(gpu_ctx, oracle, length_image, pcode):
    img, recs = length_image
    jobs, cap = packed(recs, pcode=pcode)
    assert both_forms(gpu_ctx, oracle, img, jobs, cap) == 0


@pytest.mark.parametrize("nbytes", [40, 3000])
def test_alignment_all_256_pairs(gpu_ctx, oracle, nbytes):
    """Every source payload address mod 16 against every frame_offset + 28 mod 16."""
    img, recs = build_image(oracle, [nbytes] * 16, pay_mod=list(range(16)), seed=13)
    specs, fo = [], 0
    for a, (fid, off, size) in enumerate(recs):
        assert (off + 36) % 16 == a
        for b in range(16):
            fo += (b - (fo + 28)) % 16
            specs.append(dict(src_offset=off, frame_offset=fo, file_id=fid, size=size, pcode=PCODES[(a + b) % 3]))
            fo += cap_of(make_jobs([specs[-1]])[0])
    assert both_forms(gpu_ctx, oracle, img, make_jobs(specs), fo) == 0


def test_alignment_long_payload(gpu_ctx, oracle):
    """65,557 bytes: source mod 4 against destination mod 16."""
    img, recs = build_image(oracle, [65557] * 4, pay_mod=[0, 5, 10, 15], seed=14)
    specs, fo = [], 0
    for a, (fid, off, size) in enumerate(recs):
        for b in range(16):
            fo += (b - (fo + 28)) % 16
            specs.append(dict(src_offset=off, frame_offset=fo, file_id=fid, size=size, pcode=PCODES[b % 3]))
            fo += cap_of(make_jobs([specs[-1]])[0])
    assert both_forms(gpu_ctx, oracle, img, make_jobs(specs), fo) == 0


def test_guards_at_the_ends_of_src_and_out(gpu_ctx, oracle):
    """Frames back to back, the last ending at the last byte of out; the last record ends at the
    last byte of src and the one before it fewer than 128 bytes earlier (the destination-anchored
    grid's guard); a refused job's span keeps the prefill."""
    img, recs = build_image(oracle, [5000, 70001, 3000, 2048, 60], seed=15)
    assert recs[-1][1] + recs[-1][2] == img.size and img.size - (recs[-2][1] + recs[-2][2]) < 128
    jobs, cap = packed(recs, pcode=[8, 39, 63, 39, 8])
    jobs[2]["src_offset"] = img.size - 100       # the record passes src_len: refused, span untouched
    assert both_forms(gpu_ctx, oracle, img, jobs, cap) == 1
    # and with src_len one byte short of the last record
    out, res, before, nbad = run_device(gpu_ctx, img[:-1].copy(), jobs, cap)
    assert check(oracle, img[:-1].copy(), jobs, out, res, cap, before) == 2 and nbad == 2


def _status_cases(oracle):
    """(image, jobs, out_cap, expected statuses) with one job per failure kind among good ones."""
    sizes = [3000, 100, 65536, 2000, 40, 5000, 900, 64, 1500, 700, 3100, 800, 0, 2100, 333, 50]
    img, recs = build_image(oracle, sizes, seed=16, tail=200)
    jobs, cap = packed(recs, pcode=[PCODES[k % 3] for k in range(len(recs))])
    want = [0] * len(recs)

    def pay(k):
        return recs[k][1] + 36

    jobs[1]["file_id"] = 77
    want[1] = INFO_ERR
    img[recs[3][1] + 12] ^= 1                     # FileInfo.size_
    want[3] = SYNC_ERR
    img[pay(2)] ^= 0x10                           # first payload byte
    img[pay(5) + 2500] ^= 0x01                    # a middle one
    img[pay(6) + 899] ^= 0x80                     # the last
    img[recs[8][1] + 32] ^= 0x04                  # crc_
    for k in (2, 5, 6, 8):
        want[k] = CRC_ERR
    jobs[7]["size"] = 35
    want[7] = SIZE_ERR
    jobs[12]["size"] = 36                         # an empty file is served
    jobs[9]["src_offset"] = img.size - 10
    jobs[10]["frame_offset"] = cap - 5            # span past out_cap
    jobs[11]["pcode"] = 9
    jobs[13]["read_offset"] = -1
    jobs[14]["read_offset"] = 334
    for k in (9, 10, 11, 13, 14):
        want[k] = PARAM
    return img, jobs, cap, want


def test_statuses_mixed_in_one_launch(gpu_ctx, oracle):
    img, jobs, cap, want = _status_cases(oracle)
    nb = both_forms(gpu_ctx, oracle, img, jobs, cap)
    assert nb == sum(1 for w in want if w)
    out, res, before, nbad = run_device(gpu_ctx, img, jobs, cap)
    assert [int(s) for s in res["status"]] == want


def test_statuses_each_alone(gpu_ctx, oracle):
    img, jobs, cap, want = _status_cases(oracle)
    for k in range(len(jobs)):
        one = jobs[k:k + 1].copy()
        out, res, before, nbad = run_device(gpu_ctx, img, one, cap)
        assert check(oracle, img, one, out, res, cap, before) == (1 if want[k] else 0)
        assert int(res[0]["status"]) == want[k] and nbad == (1 if want[k] else 0), k
        out, res, before, nbad, rc = run_host(gpu_ctx, img, one, cap)
        check(oracle, img, one, out, res, cap, before)
        assert int(res[0]["status"]) == want[k] and rc == (CRC_ERR if want[k] else 0), k


def test_slices(gpu_ctx, oracle):
    """read_offset in {1, 3, 36, 1000}, read_len short of, at and past the end; no CRC check, even on a
    record corrupt inside or outside the slice."""
    img, recs = build_image(oracle, [4000, 4000, 70001], seed=17)
    img[recs[1][1] + 36 + 2] ^= 1                 # record 1: corrupt at payload byte 2 (outside ro >= 3 slices)
    img[recs[1][1] + 36 + 1500] ^= 1              # ... and at byte 1500 (inside most)
    specs, fo = [], 1
    for r, (fid, off, size) in enumerate(recs):
        for ro in (1, 3, 36, 1000):
            left = size - 36 - ro
            for rl in (left - 7, left, left + 100, 0):
                specs.append(dict(src_offset=off, frame_offset=fo, file_id=fid, size=size, read_offset=ro,
                                  read_len=rl, pcode=PCODES[(r + ro + rl) % 3]))
                fo += cap_of(make_jobs([specs[-1]])[0])
    jobs = make_jobs(specs)
    assert both_forms(gpu_ctx, oracle, img, jobs, fo) == 0
    out, res, before, nbad = run_device(gpu_ctx, img, jobs, fo)
    assert (res["file_crc"] == 0).all()
    for k, job in enumerate(jobs):
        if int(job["pcode"]) != 8:                # the V2 trailer of a slice is le32(0)
            end = int(job["frame_offset"]) + int(res[k]["frame_len"])
            assert out[end - 4:end].tobytes() == b"\0\0\0\0"


def test_version_0(gpu_ctx, oracle):
    img, recs = build_image(oracle, [2000, 2000, 40], seed=18)
    img[recs[1][1] + 36 + 5] ^= 2
    jobs, cap = packed(recs, version=0, pcode=[8, 39, 63])
    assert both_forms(gpu_ctx, oracle, img, jobs, cap) == 1
    out, res, before, nbad = run_device(gpu_ctx, img, jobs, cap)
    assert (res["frame_crc"] == 0).all() and int(res[1]["status"]) == CRC_ERR
    for job in jobs:
        fo = int(job["frame_offset"])
        assert out[fo + 20:fo + 24].tobytes() == b"\0\0\0\0"


def test_round_trip_through_verify_and_decoder(gpu_ctx, oracle):
    import tfs_amd.crc as crc
    import tfs_amd.dataserver as ds
    img, recs = build_image(oracle, [0, 1, 100, 4097, 65536, 33], seed=19)
    jobs, cap = packed(recs, start=0, pcode=[39, 8, 63, 39, 8, 39])
    out, res, before, nbad = run_device(gpu_ctx, img, jobs, cap)
    assert nbad == 0 and (res["status"] == 0).all()
    offs = [int(j["frame_offset"]) for j in jobs]
    lens = [int(r["frame_len"]) for r in res]
    c, st, bad, rc = gpu_ctx.packet_verify(out, offs, lens)
    assert rc == 0 and bad == 0 and (st == 0).all() and (c == res["frame_crc"]).all()
    rc, doff, dst, dcrc, consumed = ds.decode_stream(gpu_ctx, out[:cap].tobytes())
    assert rc == 0 and list(doff) == offs and (dst == 0).all() and consumed == cap
    assert (dcrc == res["frame_crc"]).all()
    for k, (fid, off, size) in enumerate(recs):
        if int(jobs[k]["pcode"]) == 8:
            continue
        end = offs[k] + lens[k]
        fi = np.frombuffer(out[end - 36:end].tobytes(), crc.FILEINFO_DTYPE)[0]
        stored = np.frombuffer(img[off:off + 36].tobytes(), crc.FILEINFO_DTYPE)[0]
        assert int(fi["size_"]) == int(stored["size_"]) - 36 == size - 36
        for f in ("id_", "offset_", "usize_", "modify_time_", "create_time_", "flag_", "crc_"):
            assert fi[f] == stored[f], f
        assert struct.unpack_from("<i", out, end - 40)[0] == 36


def test_tickets_5000_short_jobs(gpu_ctx, oracle):
    """Past 4,096 jobs: the cursor and the cross-job pipeline wrap.  Mixed lengths, 0 to 3,000."""
    rng = np.random.default_rng(20)
    sizes = [int(x) for x in rng.integers(0, 3001, 5000)]
    sizes[:8] = [0, 1, 31, 32, 33, 3000, 1024, 1025]
    img, recs = build_image(oracle, sizes, seed=20, tail=64)
    img[recs[4321][1] + 36] ^= 1
    jobs, cap = packed(recs, pcode=[PCODES[k % 3] for k in range(5000)])
    out, res, before, nbad = run_device(gpu_ctx, img, jobs, cap)
    assert check(oracle, img, jobs, out, res, cap, before) == 1 and nbad == 1
    assert int(res[4321]["status"]) == CRC_ERR


def test_offsets_past_4_gib(gpu_ctx, oracle):
    """src_offset and frame_offset past 4 GiB: only the tails of the two allocations are touched."""
    import tfs_amd.crc as crc
    base = (4 << 30) + 4096
    img, recs = build_image(oracle, [70001, 100, 5000], seed=21, tail=256)
    jobs, cap = packed(recs, pcode=[39, 8, 63])
    jobs["src_offset"] += base
    jobs["frame_offset"] += base
    d_src = crc.DeviceBuffer(gpu_ctx, base + img.size)
    d_out = crc.DeviceBuffer(gpu_ctx, base + cap)
    d_src.upload(img, offset=base)
    before = prefill(cap)
    d_out.upload(before, offset=base)
    d_res = crc.DeviceBuffer(gpu_ctx, 16 * len(jobs))
    gpu_ctx.read_reply_device(d_src, base + img.size, jobs, d_out, base + cap, d_res)
    gpu_ctx.sync()
    out = d_out.download(np.uint8, cap, offset=base)
    res = d_res.download(crc.READ_RESULT_DTYPE, len(jobs))
    d_src.free()
    d_out.free()
    jobs["src_offset"] -= base
    jobs["frame_offset"] -= base
    assert check(oracle, img, jobs, out, res, cap, before) == 0


def test_host_paths_give_identical_bytes(gpu_ctx, oracle):
    """Page-locked and pageable src / out in all four combinations, and the staged path in small pieces."""
    img, jobs, cap, want = _status_cases(oracle)
    ref = None
    try:
        for piece in (0, 4096):
            gpu_ctx.read_set_piece(piece)
            for pin_src in (True, False):
                for pin_out in (True, False):
                    out, res, before, nbad, rc = run_host(gpu_ctx, img, jobs, cap, pin_src, pin_out)
                    assert check(oracle, img, jobs, out, res, cap, before) == nbad == sum(1 for w in want if w)
                    assert rc == CRC_ERR
                    # a span's bytes past frame_len are unspecified: compare frames and results
                    frames = [out[int(j["frame_offset"]):int(j["frame_offset"]) + int(r["frame_len"])].tobytes()
                              for j, r in zip(jobs, res)]
                    if ref is None:
                        ref = (frames, res.tobytes())
                    assert (frames, res.tobytes()) == ref, (piece, pin_src, pin_out)
    finally:
        gpu_ctx.read_set_piece(0)


def test_staged_pieces_with_long_records(gpu_ctx, oracle, length_image):
    img, recs = length_image
    jobs, cap = packed(recs, pcode=63)
    try:
        gpu_ctx.read_set_piece(8192)             # most records are a piece of their own; short ones share
        out, res, before, nbad, rc = run_host(gpu_ctx, img, jobs, cap)
        assert check(oracle, img, jobs, out, res, cap, before) == 0 and rc == 0
    finally:
        gpu_ctx.read_set_piece(0)


def test_overlapping_spans_are_refused(gpu_ctx, oracle):
    import tfs_amd.crc as crc
    img, recs = build_image(oracle, [500, 500], seed=22)
    jobs, cap = packed(recs, pcode=8)
    jobs[1]["frame_offset"] -= 1
    before = prefill(cap)
    out = before.copy()
    res = np.zeros(2, crc.READ_RESULT_DTYPE)
    L = crc.lib()
    rc = L.tfs_read_reply(gpu_ctx.handle, img.ctypes.data, img.size, jobs.ctypes.data, 2, out.ctypes.data, cap,
                          res.ctypes.data, None)
    assert rc == PARAM and (out == before).all()
    d_src = crc.DeviceBuffer(gpu_ctx, img.size).upload(img)
    d_out = crc.DeviceBuffer(gpu_ctx, cap).upload(before)
    d_res = crc.DeviceBuffer(gpu_ctx, 32)
    rc = L.tfs_read_reply_device(gpu_ctx.handle, d_src.ptr, img.size, jobs.ctypes.data, 2, d_out.ptr, cap, d_res.ptr,
                                 None, None)
    gpu_ctx.sync()
    assert rc == PARAM and (d_out.download(np.uint8, cap) == before).all()


def test_call_level(gpu_ctx, oracle):
    import tfs_amd.crc as crc
    img, recs = build_image(oracle, [500], seed=23)
    jobs, cap = packed(recs)
    L, h = crc.lib(), gpu_ctx.handle
    out = prefill(cap)
    res = np.zeros(1, crc.READ_RESULT_DTYPE)
    a = (img.ctypes.data, img.size, jobs.ctypes.data)
    assert L.tfs_read_reply(h, *a, 0, None, 0, None, None) == 0                                  # n == 0
    assert L.tfs_read_reply(h, img.ctypes.data, img.size, None, 1, out.ctypes.data, cap, res.ctypes.data, None) == PARAM
    assert L.tfs_read_reply(h, *a, 1, None, cap, res.ctypes.data, None) == PARAM
    assert L.tfs_read_reply(h, *a, 1, out.ctypes.data, cap, None, None) == PARAM
    assert L.tfs_read_reply_device(h, *a, 0, None, 0, None, None, None) == 0
    per_thread = ctypes.c_void_p(2)              # hipStreamPerThread
    d = crc.DeviceBuffer(gpu_ctx, max(img.size, cap) + 64)
    assert L.tfs_read_reply_device(h, d.ptr, img.size, jobs.ctypes.data, 1, d.ptr, cap, d.ptr, None, per_thread) == PARAM
    before = gpu_ctx.L.tfs_crc32_stats
    st0 = crc.CrcStats()
    before(h, ctypes.byref(st0))
    gpu_ctx.read_reply(img, jobs, out)
    st1 = crc.CrcStats()
    before(h, ctypes.byref(st1))
    assert st1.host_calls == st0.host_calls + 1 and st1.host_files == st0.host_files + 1
