"""Replicate sessions (include/tfs_replicate.h) on the GPU: every frame byte
for byte against a WriteRawDataMessage frame built in Python from the image's bytes (struct
for header and body, the CRC written by oracle_packet_seal and cross-checked with
~zlib.crc32), every byte of out outside the frames, every frame CRC, and every record's
verdict against oracle_verify_file plus the id and begin-time checks -- through the device
form in one call and in chunks, and the host forms.  Everything is bit-exact."""
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
DATA_INVALID, SIZE_INVALID = -16001, -16002
FLAG = pk.TFS_PACKET_FLAG_V1
PID = 0x1122334455667000
BLOCK = 0x00C0FFEE


def zcrc(seed, data):
    return zlib.crc32(bytes(data), seed ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def build_block(oracle, layout, seed=3):
    """layout: ("gap", n) | ("rec", payload_len) | ("at", offset): a gap up to `offset`.
    Returns (image, metas)."""
    import tfs_amd.crc as crc
    parts, metas, o, k = [], [], 0, 0
    for kind, v in layout:
        if kind == "at":
            assert v >= o, (v, o)
            kind, v = "gap", v - o
        if kind == "gap":
            parts.append(((np.arange(v, dtype=np.uint64) * 37 + o) % 253).astype(np.uint8))
            o += v
            continue
        pay = synth_bytes(seed * 1000 + k, v)
        fi = np.zeros(1, crc.FILEINFO_DTYPE)
        fi["id_"], fi["offset_"], fi["size_"], fi["usize_"] = 7000 + k, o, v + 36, v + 36
        fi["modify_time_"], fi["create_time_"] = 1700000000 + k, 1600000000 + k
        fi["crc_"] = ocrc(oracle, 0, pay.tobytes())
        parts += [fi.view(np.uint8).copy(), pay]
        metas.append((7000 + k, o, v + 36))
        o += 36 + v
        k += 1
    img = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return img, np.array(metas, dtype=crc.META_DTYPE) if metas else np.zeros(0, crc.META_DTYPE)


# frame_len 1024: tiny records, a record over four frames ending on a cut, a payload starting
# on a cut, FileInfos split after k bytes, a whole-frame gap, a trailing gap, a ragged total.
SPLITS = (1, 4, 8, 31, 32, 35)
GEOMETRY = ([("rec", 1), ("rec", 1), ("gap", 10), ("rec", 4096 - 84 - 36), ("at", 5120 - 36), ("rec", 100)] +
            [item for i, k in enumerate(SPLITS) for item in (("at", 6144 + 1024 * i - k), ("rec", 200))] +
            [("at", 13400), ("rec", 3000), ("gap", 335)])


@pytest.fixture(scope="module")
def geometry(oracle):
    img, metas = build_block(oracle, GEOMETRY)
    assert img.size == 16771 and img.size % 4 and img.size % 1024
    offs = [int(m["offset"]) for m in metas]
    assert offs[2] + int(metas[2]["size"]) == 4096 and offs[3] + 36 == 5120
    for i, k in enumerate(SPLITS):
        assert (offs[4 + i] + k) % 1024 == 0
    assert not any(o < 13312 and o + int(s) > 12288 for o, s in zip(offs, metas["size"]))  # frame 12: all gap
    return img, metas


def expected_frames(oracle, img, cfg):
    """[frame bytes] of the block, by the header's rules."""
    import tfs_amd.crc as crc
    c = cfg[0]
    total, fl, ver = int(c["total"]), int(c["frame_len"]), int(c["version"])
    frames = []
    for k in range(crc.replicate_frame_count(cfg)):
        off = k * fl
        data = img[off:min(off + fl, total)].tobytes()
        body = struct.pack("<IQiiiQ", int(c["block_id"]), 0, off, len(data), 0, 0) + data + \
            struct.pack("<i", int(c["new_block"]) if k == 0 else 0)
        assert len(body) == 36 + len(data)
        f = np.frombuffer(pk.frame_v1(body, 35, ver, (int(c["packet_id"]) + k) & (2**64 - 1)), np.uint8).copy()
        if ver >= 1:
            o, av = np.zeros(1, np.uint64), np.array([f.size], np.uint32)
            cc, st = np.zeros(1, np.uint32), np.zeros(1, np.int32)
            oracle.oracle_packet_seal(f.ctypes.data, o.ctypes.data, av.ctypes.data, 1, cc.ctypes.data, st.ctypes.data)
            assert st[0] == 0 and struct.unpack_from("<I", f, 20)[0] == zcrc(FLAG, body)
        frames.append(f)
    return frames


def expected_verdicts(oracle, img, metas, total):
    """(crc, status) per meta: the begin-time rule, then the id check, then oracle_verify_file."""
    crcs, sts = [], []
    for m in metas:
        fid, off, size = int(m["file_id"]), int(m["offset"]), int(m["size"])
        if off < 0 or off + size > total:
            crcs.append(0), sts.append(PARAM)
            continue
        if size <= 36:
            crcs.append(0), sts.append(SIZE_ERR)
            continue
        oc = ctypes.c_uint32()
        code = oracle.oracle_verify_file(img.ctypes.data, img.size, off, size, ctypes.byref(oc))
        assert oc.value == ocrc(oracle, 0, img[off + 36:off + size].tobytes())
        if struct.unpack_from("<Q", img, off)[0] != fid:
            code = INFO_ERR
        crcs.append(oc.value), sts.append(code)
    return np.array(crcs, np.uint32), np.array(sts, np.int32)


def prefill(n):
    return ((np.arange(n, dtype=np.uint64) * 131 + 7) % 251).astype(np.uint8)


def check_out(out, before, frames, stride, base=0):
    touched = np.zeros(out.size, bool)
    for k, f in enumerate(frames):
        o = base + k * stride
        got = out[o:o + f.size]
        if not (got == f).all():
            bad = int(np.nonzero(got != f)[0][0])
            raise AssertionError("frame %d differs at byte %d of %d" % (k, bad, f.size))
        touched[o:o + f.size] = True
    assert (out[~touched] == before[~touched]).all(), "a byte outside the frames was written"


def whole_call(total):
    return [(0, total)]


def run_device(ctx, img, metas, cfg, calls=None, shift=0, slack=64):
    """The block through the device form; frame k of the block lies at out + shift + k * stride."""
    import tfs_amd.crc as crc
    total, fl = int(cfg[0]["total"]), int(cfg[0]["frame_len"])
    nfr = crc.replicate_frame_count(cfg)
    with crc.ReplicateSession(ctx, cfg, metas) as s:
        stride = s.stride
        cap = shift + nfr * stride + slack
        before = prefill(cap)
        d_src = crc.DeviceBuffer(ctx, total + 256)
        if total:
            d_src.upload(img)
        d_out = crc.DeviceBuffer(ctx, cap + 16).upload(before)
        for off, ln in (calls or whole_call(total)):
            o = shift + (off // fl) * stride
            s.frames_device(d_src.ptr + off if total else None, off, ln, d_out.ptr + o, cap - o)
        res = s.finish()
        out = d_out.download(np.uint8, cap)
        d_src.free(), d_out.free()
    return out, before, stride, res


def check_block(oracle, img, metas, cfg, out, before, stride, res, shift=0):
    frames = expected_frames(oracle, img, cfg)
    check_out(out, before, frames, stride, shift)
    crcv, st, nbad, fcrc = res
    ecrc, est = expected_verdicts(oracle, img, metas, int(cfg[0]["total"]))
    assert (st == est).all(), (st.tolist(), est.tolist())
    assert (crcv == ecrc).all()
    assert nbad == int((est != 0).sum())
    assert fcrc.tolist() == [struct.unpack_from("<I", f, 20)[0] for f in frames]
    return frames


def cfg_for(img, fl, **kw):
    import tfs_amd.crc as crc
    return crc.replicate_cfg(img.size, fl, block_id=kw.pop("block_id", BLOCK), packet_id=kw.pop("packet_id", PID), **kw)


# ---- 1. geometry, device form, one call -----------------------------------------------------

@pytest.mark.parametrize("fl", [1024, 4096])
@pytest.mark.parametrize("pad,version,new_block", [(0, 2, 1), (0, 0, 2), (37, 2, 2), (1, 1, 1)])
def test_geometry_one_call(gpu_ctx, oracle, geometry, fl, pad, version, new_block):
    img, metas = geometry
    cfg = cfg_for(img, fl, version=version, new_block=new_block, frame_stride=(fl + 60 + pad) if pad else 0)
    out, before, stride, res = run_device(gpu_ctx, img, metas, cfg)
    assert stride == fl + 60 + pad
    frames = check_block(oracle, img, metas, cfg, out, before, stride, res)
    assert res[2] == 0 and len(frames) == -(-img.size // fl)
    if version == 0:
        assert all(struct.unpack_from("<I", f, 20)[0] == 0 for f in frames)


@pytest.mark.parametrize("shift", range(16))
def test_every_source_to_destination_shift(gpu_ctx, oracle, geometry, shift):
    img, metas = geometry
    cfg = cfg_for(img, 1024)
    out, before, stride, res = run_device(gpu_ctx, img, metas, cfg, shift=shift)
    check_block(oracle, img, metas, cfg, out, before, stride, res, shift)


def test_explicit_packed_stride_equals_default(gpu_ctx, oracle, geometry):
    img, metas = geometry
    cfg = cfg_for(img, 1024, frame_stride=1024 + 60)
    out, before, stride, res = run_device(gpu_ctx, img, metas, cfg)
    check_block(oracle, img, metas, cfg, out, before, stride, res)


@pytest.mark.parametrize("new_block", [1, 2])
def test_empty_block_is_one_empty_frame(gpu_ctx, oracle, new_block):
    img = np.zeros(0, np.uint8)
    cfg = cfg_for(img, 4096, new_block=new_block)
    out, before, stride, res = run_device(gpu_ctx, img, None, cfg)
    frames = check_block(oracle, img, np.zeros(0, "u1"), cfg, out, before, stride, res)
    assert len(frames) == 1 and frames[0].size == 60 and struct.unpack_from("<i", frames[0], 56)[0] == new_block


@pytest.mark.parametrize("total", [1, 37, 1000, 4095])
def test_block_shorter_than_a_frame(gpu_ctx, oracle, total):
    layout = [("rec", total - 36)] if total == 37 else ([("gap", 3), ("rec", 500), ("gap", total - 539)]
                                                        if total >= 1000 else [("gap", total)])
    img, metas = build_block(oracle, layout)
    assert img.size == total
    cfg = cfg_for(img, 4096)
    out, before, stride, res = run_device(gpu_ctx, img, metas, cfg)
    assert len(check_block(oracle, img, metas, cfg, out, before, stride, res)) == 1


@pytest.mark.parametrize("fl", [1024, 4096])
def test_no_records_only_copies_and_seals(gpu_ctx, oracle, geometry, fl):
    img, _ = geometry
    cfg = cfg_for(img, fl, new_block=2)
    out, before, stride, res = run_device(gpu_ctx, img, None, cfg)
    check_block(oracle, img, np.zeros(0, "u1"), cfg, out, before, stride, res)
    assert res[0].size == 0 and res[2] == 0


# ---- 2. chunking ----------------------------------------------------------------------------

def split_calls(total, fl, frames_per_call):
    calls, off, i = [], 0, 0
    while off < total:
        ln = min(frames_per_call[i % len(frames_per_call)] * fl, total - off)
        calls.append((off, ln))
        off += ln
        i += 1
    return calls


@pytest.mark.parametrize("per", [(1,), (2,), (3, 1, 5, 2)])
def test_chunked_calls_equal_one_call(gpu_ctx, oracle, geometry, per):
    img, metas = geometry
    cfg = cfg_for(img, 1024, frame_stride=1100)
    one = run_device(gpu_ctx, img, metas, cfg)
    calls = split_calls(img.size, 1024, per)
    # FileInfos and payloads split by call cuts: every frame cut is one with one frame per call; the
    # uneven split cuts the four-frame record's payload at 3072 and the FileInfo at 9216 - 31
    assert per != (3, 1, 5, 2) or {3072, 9216} <= {o for o, _ in calls}
    out, before, stride, res = run_device(gpu_ctx, img, metas, cfg, calls=calls)
    check_block(oracle, img, metas, cfg, out, before, stride, res)
    assert (out == one[0]).all()
    for a, b in zip(res, one[3]):
        assert np.array_equal(a, b)


def test_bad_calls_change_nothing(gpu_ctx, oracle, geometry):
    import tfs_amd.crc as crc
    img, metas = geometry
    fl, total = 1024, img.size
    cfg = cfg_for(img, fl)
    frames = expected_frames(oracle, img, cfg)
    with crc.ReplicateSession(gpu_ctx, cfg, metas) as s:
        stride = s.stride
        cap = len(frames) * stride + 32
        before = prefill(cap)
        d_src = crc.DeviceBuffer(gpu_ctx, total + 256).upload(img)
        d_out = crc.DeviceBuffer(gpu_ctx, cap + 16).upload(before)

        def call(off, ln, cap_=None, src=True, out=True):
            o = (off // fl) * stride if off >= 0 else 0
            s.frames_device(d_src.ptr + max(off, 0) if src else None, off, ln, d_out.ptr + o if out else None,
                            cap - o if cap_ is None else cap_)

        def refused(code, *a, **kw):
            with pytest.raises(crc.TfsCrcError) as e:
                call(*a, **kw)
            assert e.value.code == code
            assert (d_out.download(np.uint8, cap) == state).all()

        state = before.copy()
        refused(PARAM, fl, fl)                      # skipped: the first call is at 0
        refused(PARAM, 0, 0)                        # len 0 with total > 0
        refused(PARAM, 0, 1000)                     # not whole frames
        refused(PARAM, 0, total + 1)                # overlong
        refused(PARAM, 0, 2 * fl, cap_=stride + 60 + fl - 1)  # out_cap one byte short
        refused(DATA_INVALID, 0, fl, src=False)
        refused(DATA_INVALID, 0, fl, out=False)
        with pytest.raises(crc.TfsCrcError) as e:
            s.finish()                              # nothing covered yet
        assert e.value.code == PARAM
        call(0, 2 * fl, cap_=stride + 60 + fl)      # exactly enough
        gpu_ctx.sync()
        state = d_out.download(np.uint8, cap)
        check_out(state, before, frames[:2], stride)
        refused(PARAM, 0, 2 * fl)                   # repeated
        refused(PARAM, 3 * fl, fl)                  # skipped
        refused(PARAM, 2 * fl + 512, 512)           # misaligned
        refused(PARAM, 2 * fl - 1024, 2048)         # overlaps what is covered
        refused(PARAM, 2 * fl, total - 2 * fl + 1)  # overlong
        with pytest.raises(crc.TfsCrcError) as e:
            s.finish()
        assert e.value.code == PARAM
        call(2 * fl, total - 2 * fl)                # the next correct call still works
        res = s.finish()
        out = d_out.download(np.uint8, cap)
        refused_after = pytest.raises(crc.TfsCrcError)
        with refused_after:
            call(total, fl)                         # past the end
        d_src.free(), d_out.free()
    check_block(oracle, img, metas, cfg, out, before, stride, res)


def test_begin_checks_in_order(gpu_ctx):
    import tfs_amd.crc as crc
    L, h = gpu_ctx.L, ctypes.c_void_p()
    good = crc.replicate_cfg(4096, 1024)
    m = np.array([(1, 0, 100), (2, 50, 100)], dtype=crc.META_DTYPE)

    def begin(cfg, metas=None, n=0, ctx=gpu_ctx.handle, out=ctypes.byref(h)):
        return L.tfs_replicate_begin(ctx, cfg.ctypes.data if cfg is not None else None,
                                     metas.ctypes.data if metas is not None else None, n, out)

    bad_all = crc.replicate_cfg(-1, 1000, new_block=7, reserved=1, frame_stride=5)
    assert begin(bad_all, None, 2, ctx=None) == PARAM
    assert begin(None) == PARAM and begin(good, out=None) == PARAM
    assert begin(bad_all, None, 2) == SIZE_INVALID
    assert begin(crc.replicate_cfg(4096, 0, new_block=7)) == SIZE_INVALID
    assert begin(crc.replicate_cfg(4096, 1000)) == SIZE_INVALID
    assert begin(crc.replicate_cfg(4096, 1024, frame_stride=1083), None, 2) == PARAM
    assert begin(crc.replicate_cfg(4096, 1024, new_block=0)) == PARAM
    assert begin(crc.replicate_cfg(4096, 1024, new_block=3)) == PARAM
    assert begin(crc.replicate_cfg(4096, 1024, reserved=1)) == PARAM
    assert begin(good, None, 2) == PARAM
    assert begin(good, m, 2) == PARAM               # overlap
    assert begin(good, m[::-1].copy(), 2) == PARAM  # not ascending
    assert h.value is None
    assert begin(good, m, 1) == 0 and h.value
    assert L.tfs_replicate_free(h) == 0
    assert L.tfs_replicate_free(None) == PARAM and L.tfs_replicate_finish(None, None, None, None, None) == PARAM
    for total, want in ((0, 1), (1, 1), (1023, 1), (1024, 1), (1025, 2)):
        assert crc.replicate_frame_count(crc.replicate_cfg(total, 1024)) == want


def test_per_thread_stream_and_second_stream_are_refused(gpu_ctx, oracle, geometry):
    import tfs_amd.crc as crc
    img, metas = geometry
    cfg = cfg_for(img, 1024)
    with crc.ReplicateSession(gpu_ctx, cfg, metas) as s:
        d_src = crc.DeviceBuffer(gpu_ctx, img.size + 256).upload(img)
        d_out = crc.DeviceBuffer(gpu_ctx, 17 * s.stride + 16)
        with pytest.raises(crc.TfsCrcError) as e:
            s.frames_device(d_src, 0, 1024, d_out, d_out.nbytes, stream=2)  # hipStreamPerThread
        assert e.value.code == PARAM
        st = gpu_ctx.stream_create()
        s.frames_device(d_src, 0, 1024, d_out, d_out.nbytes, stream=st)
        with pytest.raises(crc.TfsCrcError) as e:
            s.frames_device(d_src.ptr + 1024, 1024, 1024, d_out, d_out.nbytes)
        assert e.value.code == PARAM
        s.frames_device(d_src.ptr + 1024, 1024, img.size - 1024, d_out.ptr + s.stride, d_out.nbytes - s.stride, stream=st)
        res = s.finish()
        assert res[2] == 0
    gpu_ctx.stream_destroy(st)
    d_src.free(), d_out.free()


# ---- 3. findings ----------------------------------------------------------------------------

def flipped(img, at):
    b = img.copy()
    b[at] ^= 0x40
    return b


def test_findings(gpu_ctx, oracle, geometry):
    img, metas = geometry
    fl = 1024
    cfg = cfg_for(img, fl)
    clean = run_device(gpu_ctx, img, metas, cfg)
    clean_fcrc = clean[3][3]
    long_rec = 2                                   # the record over frames 0..3
    cases = {
        "payload": (2048 + 100, {long_rec: CRC_ERR}),           # a middle frame of the long record
        "id": (int(metas[5]["offset"]) + 3, {5: INFO_ERR}),
        "size": (int(metas[6]["offset"]) + 13, {6: SYNC_ERR}),
        "crc": (int(metas[0]["offset"]) + 33, {0: CRC_ERR}),
        "gap": (12288 + 500, {}),
    }
    for name, (at, want) in cases.items():
        bad = flipped(img, at)
        out, before, stride, res = run_device(gpu_ctx, bad, metas, cfg)
        check_block(oracle, bad, metas, cfg, out, before, stride, res)  # faithful sealed copies, right verdicts
        st = res[1]
        assert {i: int(v) for i, v in enumerate(st) if v} == want, name
        changed = [k for k in range(len(clean_fcrc)) if res[3][k] != clean_fcrc[k]]
        assert changed == [at // fl], name


def test_records_rejected_at_begin_still_travel(gpu_ctx, oracle, geometry):
    import tfs_amd.crc as crc
    img, metas = geometry
    extra = np.array([(1, 100, 36), (2, img.size - 10, 100), (3, -5, 50), (4, 5000, 0)], dtype=crc.META_DTYPE)
    mixed = np.concatenate([metas[:3], extra[:2], metas[3:], extra[2:]])
    cfg = cfg_for(img, 1024)
    out, before, stride, res = run_device(gpu_ctx, img, mixed, cfg, calls=split_calls(img.size, 1024, (4,)))
    check_block(oracle, img, mixed, cfg, out, before, stride, res)
    assert res[2] == 4 and sorted(res[1][res[1] != 0].tolist()) == sorted([SIZE_ERR, PARAM, PARAM, SIZE_ERR])


# ---- 4. agreement with what exists ----------------------------------------------------------

def test_agrees_with_block_verify_packet_verify_and_lands_whole(gpu_ctx, oracle, geometry):
    import tfs_amd.crc as crc
    img, metas = geometry
    bad = flipped(flipped(img, 3000), int(metas[7]["offset"]) + 2)
    fl = 1024
    cfg = cfg_for(bad, fl, frame_stride=1096)
    out, before, stride, res = run_device(gpu_ctx, bad, metas, cfg)
    n = len(metas)
    d_img = crc.DeviceBuffer(gpu_ctx, bad.size + 256).upload(bad)
    d_m = crc.DeviceBuffer(gpu_ctx, 16 * n).upload(metas)
    d_c, d_s = crc.DeviceBuffer(gpu_ctx, 4 * n), crc.DeviceBuffer(gpu_ctx, 4 * n)
    gpu_ctx.block_verify_device(d_img, bad.size, d_m, n, d_c, d_s)
    gpu_ctx.sync()
    assert (d_s.download(np.int32, n) == res[1]).all() and (d_c.download(np.uint32, n) == res[0]).all()
    assert sorted(res[1][res[1] != 0].tolist()) == sorted([CRC_ERR, INFO_ERR])
    nfr = len(res[3])
    lens = [60 + min(fl, bad.size - k * fl) for k in range(nfr)]
    desc = np.zeros(nfr, crc.PACKET_DESC_DTYPE)
    desc["offset"], desc["len"] = np.arange(nfr) * stride, lens
    d_f = crc.DeviceBuffer(gpu_ctx, out.size + 16).upload(out)
    d_d = crc.DeviceBuffer(gpu_ctx, 16 * nfr).upload(desc)
    d_pc, d_ps = crc.DeviceBuffer(gpu_ctx, 4 * nfr), crc.DeviceBuffer(gpu_ctx, 4 * nfr)
    gpu_ctx.packet_verify_device(d_d, nfr, d_f, d_pc, d_ps)
    gpu_ctx.sync()
    assert (d_ps.download(np.int32, nfr) == 0).all()
    assert (d_pc.download(np.uint32, nfr) == res[3]).all()
    landed = np.zeros(bad.size, np.uint8)
    for k in range(nfr):
        f = out[k * stride:k * stride + lens[k]]
        block_id, _, off, ln = struct.unpack_from("<IQii", f, 24)
        assert block_id == BLOCK
        landed[off:off + ln] = f[56:56 + ln]
    assert (landed == bad).all()
    for b in (d_img, d_m, d_c, d_s, d_f, d_d, d_pc, d_ps):
        b.free()


# ---- 5. the reference's geometry ------------------------------------------------------------

@pytest.fixture(scope="module")
def reference_block(oracle):
    layout = [("rec", 65536)] * 40 + [("at", (5 << 19) + 37376), ("rec", 3 << 20), ("gap", 5)]
    return build_block(oracle, layout, seed=9)


def run_host(ctx, img, metas, cfg, pin_src, pin_out, calls=None):
    import tfs_amd.crc as crc
    total, fl = int(cfg[0]["total"]), int(cfg[0]["frame_len"])
    nfr = crc.replicate_frame_count(cfg)
    bufs = []
    with crc.ReplicateSession(ctx, cfg, metas) as s:
        stride = s.stride
        cap = nfr * stride + 40
        before = prefill(cap)
        src, out = img, before.copy()
        if pin_src:
            src = crc.PinnedBuffer(ctx, max(total, 1))
            src.array[:total] = img
            bufs.append(src)
        if pin_out:
            out = crc.PinnedBuffer(ctx, cap)
            out.array[:] = before
            bufs.append(out)
        sp = src.ptr if pin_src else (src.ctypes.data if total else None)
        op = out.ptr if pin_out else out.ctypes.data
        for off, ln in (calls or whole_call(total)):
            o = (off // fl) * stride
            ctx._check(ctx.L.tfs_replicate_frames(s.handle, sp + off if sp else None, off, ln, op + o, cap - o),
                       "replicate_frames")
        res = s.finish()
        got = out.array.copy() if pin_out else out
    for b in bufs:
        b.free()
    return got, before, stride, res


def test_reference_geometry_device_and_host(gpu_ctx, oracle, reference_block):
    img, metas = reference_block
    bad = flipped(img, int(metas[40]["offset"]) + 36 + (1 << 20) + 77)   # inside the 3 MiB record
    cfg = cfg_for(bad, 1 << 20, frame_stride=0)
    out, before, stride, res = run_device(gpu_ctx, bad, metas, cfg)
    check_block(oracle, bad, metas, cfg, out, before, stride, res)
    assert res[2] == 1 and int(res[1][40]) == CRC_ERR
    for pin_src, pin_out, calls in ((True, True, None), (False, False, split_calls(bad.size, 1 << 20, (2, 1)))):
        h = run_host(gpu_ctx, bad, metas, cfg, pin_src, pin_out, calls)
        check_block(oracle, bad, metas, cfg, *h)
        assert (h[0][:out.size - 24] == out[:out.size - 24]).all()
        for a, b in zip(h[3], res):
            assert np.array_equal(a, b)


# ---- 6. host forms --------------------------------------------------------------------------

@pytest.mark.parametrize("pin_src,pin_out", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("piece", [0, 3 * (1024 + 64) + 5])
def test_host_forms_equal_device_form(gpu_ctx, oracle, geometry, pin_src, pin_out, piece):
    img, metas = geometry
    cfg = cfg_for(img, 1024, frame_stride=1099)
    dev = run_device(gpu_ctx, img, metas, cfg)
    gpu_ctx.read_set_piece(piece)                  # a staged call of 17 frames goes in pieces of 3
    try:
        calls = None if piece else split_calls(img.size, 1024, (5, 12))
        h = run_host(gpu_ctx, img, metas, cfg, pin_src, pin_out, calls)
    finally:
        gpu_ctx.read_set_piece(0)
    check_block(oracle, img, metas, cfg, *h)
    for a, b in zip(h[3], dev[3]):
        assert np.array_equal(a, b)


def test_host_form_empty_block_and_null_buffers(gpu_ctx, oracle):
    import tfs_amd.crc as crc
    img = np.zeros(0, np.uint8)
    cfg = cfg_for(img, 1024, new_block=2)
    h = run_host(gpu_ctx, img, None, cfg, False, False)
    check_block(oracle, img, np.zeros(0, "u1"), cfg, *h)
    with crc.ReplicateSession(gpu_ctx, crc.replicate_cfg(2048, 1024)) as s:
        out = np.zeros(4096, np.uint8)
        L = gpu_ctx.L
        assert L.tfs_replicate_frames(s.handle, None, 0, 1024, out.ctypes.data, out.size) == DATA_INVALID
        assert L.tfs_replicate_frames(s.handle, out.ctypes.data, 0, 1024, None, out.size) == DATA_INVALID
        assert L.tfs_replicate_frames(s.handle, out.ctypes.data, 1024, 1024, out.ctypes.data, out.size) == PARAM
        assert L.tfs_replicate_frames(None, out.ctypes.data, 0, 1024, out.ctypes.data, out.size) == PARAM
        assert not out.any()
