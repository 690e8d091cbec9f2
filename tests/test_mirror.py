"""Mirror sync (include/tfs_mirror.h) on the GPU: every frame byte for byte
against a WriteDataMessage frame built in Python from the image's bytes (struct for H and V,
tfs_amd.packet.frame_v1, the CRC written by oracle_packet_seal and cross-checked with
~zlib.crc32), every byte of out outside the spans, every result field (verdicts from
oracle_verify_file plus the id and before-reading checks) -- through the device form, the host
form with pageable buffers and the host form with page-locked buffers -- and the loop closed
with the receiver, tfs_packet_verify_write.  Everything is bit-exact."""
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
FLAG = pk.TFS_PACKET_FLAG_V1
M64 = 2**64 - 1
A_LENS = (1, 3, 4, 15, 16, 17, 987, 988, 989, 2011, 2012, 2013, 3000)
A_DS = (0, 1, 2, 27)
B_LENS = (39999, 40001, 90000)


def zcrc(seed, data):
    return zlib.crc32(bytes(data), seed ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def build_source(oracle, lens, residues, seed=5):
    """Records of the payload lengths `lens`, record i at a source offset congruent to residues[i]
    mod 16, gaps of other bytes between them.  Returns (image, [(file_id, offset, size)])."""
    import tfs_amd.crc as crc
    parts, recs, o = [], [], 0
    for k, (v, r) in enumerate(zip(lens, residues)):
        gap = (r - o) % 16 or (16 if k % 3 == 0 else 0)
        parts.append(((np.arange(gap, dtype=np.uint64) * 37 + o) % 253).astype(np.uint8))
        o += gap
        assert o % 16 == r % 16
        pay = synth_bytes(seed * 1000 + k, v)
        fi = np.zeros(1, crc.FILEINFO_DTYPE)
        fi["id_"], fi["offset_"], fi["size_"], fi["usize_"] = (0x5EED00000000 + 977 * k) | (k << 56), o, v + 36, v + 36
        fi["modify_time_"], fi["create_time_"] = 1700000000 + k, 1600000000 + k
        fi["crc_"] = ocrc(oracle, 0, pay.tobytes())
        parts += [fi.view(np.uint8).copy(), pay]
        recs.append((int(fi["id_"][0]), o, v + 36))
        o += 36 + v
    parts.append(np.full(5, 0xA5, np.uint8))
    return np.concatenate(parts), recs


def make_jobs(cfg, recs, ds_counts, ds_n, out_residues, gap=9):
    """One job per record: spans in record order, job i's frame_offset congruent to
    out_residues[i] mod 16.  Returns (jobs, out_cap)."""
    import tfs_amd.crc as crc
    jobs = np.zeros(len(recs), crc.MIRROR_JOB_DTYPE)
    at = 0
    for i, (fid, off, size) in enumerate(recs):
        j = jobs[i]
        j["src_offset"], j["file_id"], j["size"] = off, fid, size
        j["file_number"] = 0xF11E000000000000 + 31 * i
        j["packet_id"] = (0xFFFFFFFFFFFFFFF0 + 3 * i) & M64  # (some ids wrap: the header id is mod 2^64)
        j["block_id"] = 0x00C0FFEE + i
        j["ds_count"] = ds_counts[i % len(ds_counts)]
        j["ds_first"] = (7 * i) % (ds_n - int(j["ds_count"]) + 1)
        at += gap + (out_residues[i % len(out_residues)] - (at + gap)) % 16
        j["frame_offset"] = at
        at += crc.mirror_span(cfg, jobs[i:i + 1])
    return jobs, at + 40


def expected_frames(oracle, img, cfg, job, ds):
    """[frame bytes] of one job, by the header's rules."""
    import tfs_amd.crc as crc
    c = cfg[0]
    first, fl, ver = int(c["first_len"]), int(c["frame_len"]), int(c["version"])
    so, size, cnt = int(job["src_offset"]), int(job["size"]), int(job["ds_count"])
    pay = img[so + 36:so + size].tobytes()
    V = struct.pack("<i", cnt) + b"".join(struct.pack("<Q", int(d)) for d in ds[int(job["ds_first"]):][:cnt])
    frames, off, k = [], 0, 0
    while off < len(pay):
        ln = min(first if k == 0 else fl, len(pay) - off)
        H = struct.pack("<IQiiiQ", int(job["block_id"]), int(job["file_id"]), off, ln, int(c["is_server"]),
                        int(job["file_number"]))
        body = H + V + pay[off:off + ln]
        assert len(body) == 36 + 8 * cnt + ln
        f = np.frombuffer(pk.frame_v1(body, 9, ver, (int(job["packet_id"]) + k) & M64), np.uint8).copy()
        if ver >= 1:
            o, av = np.zeros(1, np.uint64), np.array([f.size], np.uint32)
            cc, st = np.zeros(1, np.uint32), np.zeros(1, np.int32)
            oracle.oracle_packet_seal(f.ctypes.data, o.ctypes.data, av.ctypes.data, 1, cc.ctypes.data, st.ctypes.data)
            assert st[0] == 0 and struct.unpack_from("<I", f, 20)[0] == zcrc(FLAG, body)
        else:
            assert struct.unpack_from("<I", f, 20)[0] == 0
        frames.append(f)
        off += ln
        k += 1
    assert len(frames) == crc.mirror_frame_count(cfg, size)
    return frames


def expected_result(oracle, img, cfg, job, ds_n, out_cap, src_len=None):
    """(status, file_crc) of one job: the before-reading rules, the id check, oracle_verify_file."""
    import tfs_amd.crc as crc
    src_len = img.size if src_len is None else src_len
    j = job[0]
    so, fo, size, cnt = int(j["src_offset"]), int(j["frame_offset"]), int(j["size"]), int(j["ds_count"])
    span = crc.mirror_span(cfg, job) if cnt <= 27 else 0
    if cnt > 27 or int(j["ds_first"]) + cnt > ds_n or so + max(size, 0) > src_len or \
            (span and fo + span > out_cap) or int(j["reserved"]) != 0:
        return PARAM, 0
    if size <= 36:
        return SIZE_ERR, 0
    oc = ctypes.c_uint32()
    code = oracle.oracle_verify_file(img.ctypes.data, img.size, so, size, ctypes.byref(oc))
    assert oc.value == ocrc(oracle, 0, img[so + 36:so + size].tobytes()) == zcrc(0, img[so + 36:so + size])
    if struct.unpack_from("<Q", img, so)[0] != int(j["file_id"]):
        code = INFO_ERR
    return code, oc.value


def prefill(n):
    return ((np.arange(n, dtype=np.uint64) * 131 + 7) % 251).astype(np.uint8)


def check_call(oracle, img, cfg, jobs, ds, out, before, results, nbad, src_len=None):
    """Frames, untouched bytes and every result field of one call."""
    import tfs_amd.crc as crc
    touched = np.zeros(out.size, bool)
    want_bad = 0
    all_frames = []
    for i in range(len(jobs)):
        job, r = jobs[i:i + 1], results[i]
        status, fcrc = expected_result(oracle, img, cfg, job, len(ds), out.size, src_len)
        got = (int(r["status"]), int(r["n_frames"]), int(r["span_len"]), int(r["file_crc"]))
        want_bad += status != 0
        if status in (PARAM, SIZE_ERR):
            assert got == (status, 0, 0, 0), (i, got)
            all_frames.append([])
            continue
        frames = expected_frames(oracle, img, cfg, job[0], ds)
        o = int(job["frame_offset"][0])
        span = sum(f.size for f in frames)
        assert span == crc.mirror_span(cfg, job)
        if status != 0:  # no usable frame: every flag word zero, the rest of the span unspecified
            assert got == (status, 0, 0, fcrc), (i, got, status)
            for f in frames:
                assert not out[o:o + 4].any(), (i, o)
                o += f.size
            touched[int(job["frame_offset"][0]):o] = True
            all_frames.append([])
            continue
        assert got == (0, len(frames), span, fcrc), (i, got, len(frames), span, hex(fcrc))
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


def run_device(ctx, cfg, img, jobs, ds, cap, src_len=None, d_nbad=None):
    import tfs_amd.crc as crc
    before = prefill(cap)
    d_src = crc.DeviceBuffer(ctx, img.size + 256).upload(img)
    d_out = crc.DeviceBuffer(ctx, cap + 16).upload(before)
    d_res = crc.DeviceBuffer(ctx, max(len(jobs), 1) * 16)
    own = d_nbad is None
    if own:
        d_nbad = crc.DeviceBuffer(ctx, 4)
        d_nbad.zero()
    ctx.mirror_frames_device(cfg, d_src, img.size if src_len is None else src_len, jobs, ds, d_out, cap, d_res, d_nbad)
    assert ctx.L.tfs_crc32_sync(ctx.handle) == 0
    out = d_out.download(np.uint8, cap)
    res = d_res.download(crc.MIRROR_RESULT_DTYPE, len(jobs))
    nbad = int(d_nbad.download(np.uint32, 1)[0])
    d_src.free(), d_out.free(), d_res.free()
    if own:
        d_nbad.free()
    return out, before, res, nbad


def run_host(ctx, cfg, img, jobs, ds, cap, pin_src, pin_out):
    import tfs_amd.crc as crc
    before = prefill(cap)
    src, out, bufs = img.copy(), before.copy(), []
    if pin_src:
        src = crc.PinnedBuffer(ctx, img.size)
        src.array[:] = img
        bufs.append(src)
    if pin_out:
        out = crc.PinnedBuffer(ctx, cap)
        out.array[:] = before
        bufs.append(out)
    res, nbad, rc = ctx.mirror_frames(cfg, src, jobs, ds, out)
    got = (out.array if pin_out else out).copy()
    for b in bufs:
        b.free()
    return got, before, res, nbad, rc


def geometry_a(oracle, version, is_server=0):
    import tfs_amd.crc as crc
    cfg = crc.mirror_cfg(1024 - 36, 1024, is_server=is_server, version=version)
    lens = [A_LENS[i % len(A_LENS)] for i in range(32)]
    img, recs = build_source(oracle, lens, [i % 16 for i in range(32)])
    assert {o % 16 for _, o, _ in recs} == set(range(16))
    ds = (np.arange(40, dtype=np.uint64) * np.uint64(0x0101010101010101)) ^ np.uint64(0xD5D5000000000000)
    jobs, cap = make_jobs(cfg, recs, A_DS, len(ds), [(5 * i + 3) % 16 for i in range(32)])
    assert {int(f) % 16 for f in jobs["frame_offset"]} == set(range(16))
    assert {int(c) for c in jobs["ds_count"]} == set(A_DS)
    counts = {n: crc.mirror_frame_count(cfg, n + 36) for n in A_LENS}
    assert (counts[988], counts[989], counts[2012], counts[2013], counts[3000]) == (1, 2, 2, 3, 3)
    return cfg, img, jobs, ds, cap


@pytest.fixture(scope="module")
def geo_a(oracle):
    return {v: geometry_a(oracle, v, is_server=v // 2) for v in (0, 2)}


@pytest.fixture(scope="module")
def geo_b(oracle):
    import tfs_amd.crc as crc
    cfg = crc.mirror_cfg(40000, 32768, is_server=1, version=2)
    img, recs = build_source(oracle, B_LENS, (3, 8, 13), seed=9)
    ds = np.arange(1, 30, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    jobs, cap = make_jobs(cfg, recs, (2, 27, 0), len(ds), (1, 6, 11))
    assert [crc.mirror_frame_count(cfg, n + 36) for n in B_LENS] == [1, 2, 3]
    return cfg, img, jobs, ds, cap


# ---- 1. both geometries, the three forms ---------------------------------------------------

@pytest.mark.parametrize("version", [0, 2])
def test_geometry_a_device_form(gpu_ctx, oracle, geo_a, version):
    cfg, img, jobs, ds, cap = geo_a[version]
    out, before, res, nbad = run_device(gpu_ctx, cfg, img, jobs, ds, cap)
    frames = check_call(oracle, img, cfg, jobs, ds, out, before, res, nbad)
    assert nbad == 0 and (res["status"] == 0).all()
    if version == 0:
        assert all(struct.unpack_from("<I", f, 20)[0] == 0 for fs in frames for f in fs)


def test_geometry_b_device_form(gpu_ctx, oracle, geo_b):
    cfg, img, jobs, ds, cap = geo_b
    out, before, res, nbad = run_device(gpu_ctx, cfg, img, jobs, ds, cap)
    check_call(oracle, img, cfg, jobs, ds, out, before, res, nbad)
    assert res["n_frames"].tolist() == [1, 2, 3]


@pytest.mark.parametrize("pin_src,pin_out", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("which", ["a", "b"])
def test_host_forms_equal_device_form(gpu_ctx, oracle, geo_a, geo_b, which, pin_src, pin_out):
    cfg, img, jobs, ds, cap = geo_a[2] if which == "a" else geo_b
    dev_out, _, dev_res, _ = run_device(gpu_ctx, cfg, img, jobs, ds, cap)
    out, before, res, nbad, rc = run_host(gpu_ctx, cfg, img, jobs, ds, cap, pin_src, pin_out)
    assert rc == 0
    check_call(oracle, img, cfg, jobs, ds, out, before, res, nbad)
    assert (out == dev_out).all() and (res == dev_res).all()


def test_host_form_in_pieces(gpu_ctx, oracle, geo_a):
    """A staging piece smaller than the batch: the host form goes in several launches."""
    cfg, img, jobs, ds, cap = geo_a[2]
    gpu_ctx.read_set_piece(4096)
    try:
        out, before, res, nbad, rc = run_host(gpu_ctx, cfg, img, jobs, ds, cap, False, False)
    finally:
        gpu_ctx.read_set_piece(0)
    assert rc == 0
    check_call(oracle, img, cfg, jobs, ds, out, before, res, nbad)


# ---- 2. the loop closed with the receiver --------------------------------------------------

@pytest.mark.parametrize("which", ["a", "b"])
def test_frames_pass_the_receivers_check(gpu_ctx, oracle, geo_a, geo_b, which):
    import tfs_amd.crc as crc
    cfg, img, jobs, ds, cap = geo_a[2] if which == "a" else geo_b
    out, before, res, nbad = run_device(gpu_ctx, cfg, img, jobs, ds, cap)
    offs, lens, owner = [], [], []
    for i, j in enumerate(jobs):
        o = int(j["frame_offset"])
        for k in range(int(res[i]["n_frames"])):
            body_len = struct.unpack_from("<I", out, o + 4)[0]
            offs.append(o), lens.append(24 + body_len), owner.append(i)
            o += 24 + body_len
        assert o == int(j["frame_offset"]) + int(res[i]["span_len"])
    fcrc, st, bad, rc, parts = gpu_ctx.packet_verify_write(out, offs, lens)
    assert rc == 0 and bad == 0 and (st == 0).all()
    for i, j in enumerate(jobs):
        acc, total = 0, 0
        for k in [k for k, w in enumerate(owner) if w == i]:
            assert int(parts[k]["data_len"]) >= 1 and int(parts[k]["data_off"]) == 36 + 8 * int(j["ds_count"])
            acc = crc.combine(acc, int(parts[k]["data_crc"]), int(parts[k]["data_len"]))
            total += int(parts[k]["data_len"])
        so = int(j["src_offset"])
        assert total == int(j["size"]) - 36
        assert acc == int(res[i]["file_crc"]) == struct.unpack_from("<I", img, so + 32)[0]


# ---- 3. failures, their neighbours untouched and correct -----------------------------------

def failure_batch(oracle):
    import tfs_amd.crc as crc
    cfg = crc.mirror_cfg(1024 - 36, 1024, version=2)
    #        0 good, 1-3 flips, 4 good, 5 id, 6 size_, 7 both, 8 good, 9-10 short, 11 ds 28, 12 past src, 13 past out, 14 good
    lens = [3000, 3000, 3000, 3000, 17, 2013, 989, 3000, 988, 100, 100, 50, 50, 50, 2012]
    img, recs = build_source(oracle, lens, [(3 * i + 1) % 16 for i in range(len(lens))], seed=11)
    ds = np.arange(3, 40, dtype=np.uint64) * np.uint64(0xABCDEF0123456789)
    jobs, cap = make_jobs(cfg, recs, (2, 0, 27, 1), len(ds), [(7 * i + 2) % 16 for i in range(len(lens))])
    img = img.copy()
    for i, at in ((1, 500), (2, 988 + 512), (3, 988 + 1024 + 400)):  # first, middle and last frame of three
        img[recs[i][1] + 36 + at] ^= 0x10
    struct.pack_into("<Q", img, recs[5][1], recs[5][0] ^ 1)          # id_
    struct.pack_into("<i", img, recs[6][1] + 12, recs[6][2] + 1)     # size_
    struct.pack_into("<Q", img, recs[7][1], recs[7][0] + 2)          # both: the id is checked first
    struct.pack_into("<i", img, recs[7][1] + 12, recs[7][2] - 1)
    jobs["size"][9], jobs["size"][10] = 36, 20
    jobs["ds_count"][11] = 28
    jobs["src_offset"][12] = img.size - 10
    jobs["frame_offset"][13] = cap - 10
    want = [0, CRC_ERR, CRC_ERR, CRC_ERR, 0, INFO_ERR, SYNC_ERR, INFO_ERR, 0, SIZE_ERR, SIZE_ERR, PARAM, PARAM, PARAM, 0]
    return cfg, img, jobs, ds, cap, want


@pytest.fixture(scope="module")
def failures(oracle):
    return failure_batch(oracle)


@pytest.mark.parametrize("form", ["device", "pageable", "pinned"])
def test_failures_in_one_batch(gpu_ctx, oracle, failures, form):
    cfg, img, jobs, ds, cap, want = failures
    if form == "device":
        out, before, res, nbad = run_device(gpu_ctx, cfg, img, jobs, ds, cap)
    else:
        out, before, res, nbad, rc = run_host(gpu_ctx, cfg, img, jobs, ds, cap, form == "pinned", form == "pinned")
        assert rc == CRC_ERR
    assert res["status"].tolist() == want
    check_call(oracle, img, cfg, jobs, ds, out, before, res, nbad)
    assert nbad == sum(1 for w in want if w)
    bad = res["status"] != 0
    assert not res["n_frames"][bad].any() and not res["span_len"][bad].any()
    for i in (1, 2, 3):  # three frames each, every flag word zero
        o = int(jobs["frame_offset"][i])
        head = 60 + 8 * int(jobs["ds_count"][i])
        for ln in (988, 1024, 988):
            assert not out[o:o + 4].any()
            o += head + ln


def test_n_bad_accumulates_across_calls(gpu_ctx, oracle, failures):
    import tfs_amd.crc as crc
    cfg, img, jobs, ds, cap, want = failures
    d_nbad = crc.DeviceBuffer(gpu_ctx, 4)
    d_nbad.zero()
    per = sum(1 for w in want if w)
    _, _, _, n1 = run_device(gpu_ctx, cfg, img, jobs, ds, cap, d_nbad=d_nbad)
    _, _, _, n2 = run_device(gpu_ctx, cfg, img, jobs, ds, cap, d_nbad=d_nbad)
    d_nbad.free()
    assert (n1, n2) == (per, 2 * per)
    # the host form adds to the caller's word
    res = np.zeros(len(jobs), crc.MIRROR_RESULT_DTYPE)
    nbad = np.array([100], np.uint32)
    out = prefill(cap)
    for k in (1, 2):
        rc = gpu_ctx.L.tfs_mirror_frames(gpu_ctx.handle, cfg.ctypes.data, img.ctypes.data, img.size, jobs.ctypes.data,
                                         len(jobs), ds.ctypes.data, len(ds), out.ctypes.data, cap, res.ctypes.data,
                                         nbad.ctypes.data)
        assert rc == CRC_ERR and int(nbad[0]) == 100 + k * per


def test_record_past_a_shorter_src_len(gpu_ctx, oracle, failures):
    """src_len cut inside the last record: that job alone is refused, nothing of it is written."""
    cfg, img, jobs, ds, cap, want = failures
    cut = int(jobs["src_offset"][14]) + int(jobs["size"][14]) - 1
    out, before, res, nbad = run_device(gpu_ctx, cfg, img, jobs, ds, cap, src_len=cut)
    assert res["status"].tolist() == want[:14] + [PARAM]
    check_call(oracle, img, cfg, jobs, ds, out, before, res, nbad, src_len=cut)


@pytest.mark.parametrize("form", ["device", "host"])
def test_overlapping_spans_refuse_the_call(gpu_ctx, oracle, geo_a, form):
    import tfs_amd.crc as crc
    cfg, img, jobs, ds, cap = geo_a[2]
    jobs = jobs.copy()
    jobs["frame_offset"][20] = int(jobs["frame_offset"][19]) + crc.mirror_span(cfg, jobs[19:20]) - 1
    with pytest.raises(crc.TfsCrcError) as e:
        if form == "device":
            out, before, res, nbad = run_device(gpu_ctx, cfg, img, jobs, ds, cap)
        else:
            out, before, res, nbad, rc = run_host(gpu_ctx, cfg, img, jobs, ds, cap, False, False)
    assert e.value.code == PARAM
    # nothing launched, nothing written
    before = prefill(cap)
    out = before.copy()
    res = np.zeros(len(jobs), crc.MIRROR_RESULT_DTYPE)
    nbad = np.zeros(1, np.uint32)
    rc = gpu_ctx.L.tfs_mirror_frames(gpu_ctx.handle, cfg.ctypes.data, img.ctypes.data, img.size, jobs.ctypes.data,
                                     len(jobs), ds.ctypes.data, len(ds), out.ctypes.data, cap, res.ctypes.data,
                                     nbad.ctypes.data)
    assert rc == PARAM and (out == before).all() and not res.view(np.uint8).any() and nbad[0] == 0


def test_call_level_refusals(gpu_ctx, geo_a):
    import tfs_amd.crc as crc
    cfg, img, jobs, ds, cap = geo_a[2]
    L, h = gpu_ctx.L, gpu_ctx.handle
    out = prefill(cap)
    before = out.copy()
    res = np.zeros(len(jobs), crc.MIRROR_RESULT_DTYPE)
    good = dict(cfg=cfg.ctypes.data, src=img.ctypes.data, jobs=jobs.ctypes.data, ds=ds.ctypes.data, out=out.ctypes.data,
                res=res.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return L.tfs_mirror_frames(h, a["cfg"], a["src"], img.size, a["jobs"], len(jobs), a["ds"], len(ds), a["out"],
                                   cap, a["res"], None)
    for k in ("cfg", "jobs", "ds", "out", "res", "src"):
        assert call(**{k: None}) == PARAM, k
    for bad in (crc.mirror_cfg(0, 1024), crc.mirror_cfg(988, 0), crc.mirror_cfg(-1, 1024), crc.mirror_cfg(988, 1024, reserved=1)):
        assert call(cfg=bad.ctypes.data) == PARAM
    assert (out == before).all() and not res.view(np.uint8).any()
    # n == 0 and an empty ds array are legal
    assert L.tfs_mirror_frames(h, cfg.ctypes.data, img.ctypes.data, img.size, None, 0, None, 0, out.ctypes.data, cap,
                               res.ctypes.data, None) == 0
