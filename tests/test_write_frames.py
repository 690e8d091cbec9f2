"""Write frames that yield the file CRC (include/tfs_write.h) on
the GPU: the write-data form of the packet check in its throughput and small
forms, the general-length shift, DataFile's combined CRC and the queue loopback
with WRITE and CLOSE as separate items.  Every expectation comes from the oracle
(oracle_crc / oracle_packet_verify / oracle_datafile_get_crc), never from the
library."""
import struct

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

FLAG = pk.TFS_PACKET_FLAG_V1
FILEINFO = 36
DATA_LENS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 65536, 131073]
DS_COUNTS = [0, 3, 6, 27]


@pytest.fixture(scope="module")
def ds():
    import tfs_amd.dataserver as ds
    ds.lib()
    return ds


def o_verify(oracle, buf, frames):
    off = np.array([f[0] for f in frames], np.uint64)
    av = np.array([f[1] for f in frames], np.uint32)
    crc = np.zeros(len(frames), np.uint32)
    st = np.zeros(len(frames), np.int32)
    b = np.frombuffer(bytes(buf), np.uint8).copy()
    bad = oracle.oracle_packet_verify(b.ctypes.data, off.ctypes.data, av.ctypes.data, len(frames), crc.ctypes.data,
                                      st.ctypes.data)
    return crc, st, bad


def sealed(oracle, body, pcode=pk.WRITE_DATA_MESSAGE, version=pk.TFS_PACKET_VERSION_V2, pid=7):
    return pk.frame_v1(body, pcode=pcode, version=version, pid=pid, crc=ocrc(oracle, FLAG, body))


def raw_body(length_, count, nds, data, offset=0):
    """A WriteDataMessage body with length_ and count written as given (malformed prefixes)."""
    info = struct.pack("<IQiiiQ", 5, 6, offset, length_, 0, 0)
    return info + struct.pack("<i", count) + b"".join(struct.pack("<Q", 100 + v) for v in range(nds)) + bytes(data)


def frame_makers(oracle, big):
    """(maker, data-or-None) pairs: data is D for a frame that must come back with
    its data CRC, None for one that must come back with data_len -1."""
    out = []
    k = 0
    for nd in DATA_LENS + ([2 << 20] if big else []):
        for cnt in (DS_COUNTS if nd < (2 << 20) else [3]):
            k += 1
            data = synth_bytes(9000 + k, nd).tobytes()
            body = pk.write_data_body(k, 77 + k, 4096 * k, data, ds=list(range(cnt)))
            out.append((sealed(oracle, body, pid=k), data))
    d100 = synth_bytes(5, 100).tobytes()
    good = pk.write_data_body(1, 2, 0, d100, ds=[1, 2, 3])
    out.append((sealed(oracle, good, pcode=pk.WRITE_DATA_MESSAGE + 1), None))            # another pcode
    out.append((sealed(oracle, good, pcode=-9), None))                                    # negative pcode
    out.append((pk.frame_v1(good, version=0, crc=0xDEAD), None))                          # version 0: no CRC
    out.append((pk.header_v0(len(good), pk.WRITE_DATA_MESSAGE) + good, None))             # V0 flag
    out.append((sealed(oracle, raw_body(-1, 3, 3, d100)), None))                          # length_ < 0
    out.append((sealed(oracle, raw_body(101, 3, 3, d100)), None))                         # length_ past the body
    out.append((sealed(oracle, raw_body(99, 3, 3, d100)), None))                          # hlen + length_ != body
    out.append((sealed(oracle, raw_body(100, -1, 3, d100)), None))                        # count < 0
    out.append((sealed(oracle, raw_body(100, 28, 28, d100)), None))                       # count = 28
    out.append((sealed(oracle, raw_body(100, 27, 27, d100)), d100))                       # count = 27: the last that counts
    out.append((sealed(oracle, raw_body(100, 0x10000003, 3, d100)), None))                # 8 * count wraps
    bad_h = bytearray(sealed(oracle, good))
    bad_h[24 + 9] ^= 0x04                                                                  # corrupted in H
    out.append((bytes(bad_h), None))
    bad_d = bytearray(sealed(oracle, good))
    bad_d[24 + 60 + 50] ^= 0x80                                                            # corrupted in D
    out.append((bytes(bad_d), None))
    out.append((sealed(oracle, good)[:70], None))                                          # body cut: incomplete
    return out


SHORT_BODY = b"s" * 20  # a WRITE_DATA body shorter than WriteDataInfo + count


def build_mix(oracle, rng, n, big=False):
    """n frames packed at arbitrary byte offsets; the last one is a sealed WRITE_DATA
    frame whose body is shorter than 36 bytes and ends the buffer.  Returns
    (bytes, [(offset, avail)], [data or None])."""
    makers = frame_makers(oracle, big)
    parts, frames, datas, pos = [], [], [], 0
    for i in range(n - 1):
        raw, data = makers[i % len(makers)]
        gap = int(rng.integers(0, 8))
        parts.append(b"\xAA" * gap + raw)
        frames.append((pos + gap, len(raw)))
        datas.append(data)
        pos += gap + len(raw)
    lone = makers[DATA_LENS.index(65536) * len(DS_COUNTS) + 1]  # a batch of one: a 64 KiB write, 3 ds entries
    last = sealed(oracle, SHORT_BODY) if n > 1 else lone[0]
    gap = int(rng.integers(0, 8))
    parts.append(b"\xAA" * gap + last)
    frames.append((pos + gap, len(last)))
    datas.append(None if n > 1 else lone[1])
    return b"".join(parts), frames, datas


def check(oracle, buf, frames, datas, crc, st, parts, nbad=None):
    ocrc_, ost, obad = o_verify(oracle, buf, frames)
    assert np.array_equal(st, ost)
    assert np.array_equal(crc, ocrc_)
    if nbad is not None:
        assert nbad == obad
    ndata = 0
    for i, data in enumerate(datas):
        if data is None:
            assert parts["data_len"][i] == -1, (i, parts[i])
            continue
        ndata += 1
        assert ost[i] == 0, i
        assert parts["data_len"][i] == len(data), (i, parts[i])
        o = frames[i][0] + 24 + int(parts["data_off"][i])
        assert buf[o:o + len(data)] == data, i
        assert parts["data_crc"][i] == ocrc(oracle, 0, data), (i, len(data), hex(parts["data_crc"][i]))
    return ndata


def device_run(ctx, buf, frames, write=True):
    import tfs_amd.crc as crc_mod
    n = len(frames)
    d = np.zeros(n, crc_mod.PACKET_DESC_DTYPE)
    d["offset"] = [f[0] for f in frames]
    d["len"] = [f[1] for f in frames]
    b = np.frombuffer(buf, np.uint8)
    d_base = crc_mod.DeviceBuffer(ctx, len(b)).upload(b)  # the last frame ends the allocation
    d_desc = crc_mod.DeviceBuffer(ctx, d.nbytes).upload(d)
    d_crc = crc_mod.DeviceBuffer(ctx, 4 * n)
    d_st = crc_mod.DeviceBuffer(ctx, 4 * n)
    d_parts = crc_mod.DeviceBuffer(ctx, 16 * n)
    d_bad = crc_mod.DeviceBuffer(ctx, 4)
    d_bad.zero()
    if write:
        ctx.packet_verify_write_device(d_desc, n, d_base, d_crc, d_st, d_parts, d_bad)
    else:
        ctx.packet_verify_device(d_desc, n, d_base, d_crc, d_st, d_bad)
    ctx.sync()
    out = (d_crc.download(np.uint32, n), d_st.download(np.int32, n),
           d_parts.download(crc_mod.WRITE_PART_DTYPE, n) if write else None, int(d_bad.download(np.uint32, 1)[0]))
    for x in (d_base, d_desc, d_crc, d_st, d_parts, d_bad):
        x.free()
    return out


@pytest.fixture(scope="module")
def mix300(oracle):
    return build_mix(oracle, np.random.default_rng(41), 300, big=True)


def test_throughput_form_device(gpu_ctx, oracle, mix300):
    """One launch of 300 frames (packet_write_kernel + packet_data_fold_kernel):
    statuses and CRCs equal tfs_packet_verify_device's and the oracle's, every
    frame with data brings Func::crc(0, D), every other one data_len -1."""
    buf, frames, datas = mix300
    crc, st, parts, nbad = device_run(gpu_ctx, buf, frames)
    ndata = check(oracle, buf, frames, datas, crc, st, parts, nbad)
    assert ndata >= len(DATA_LENS) * len(DS_COUNTS) + 1
    crc0, st0, _, nbad0 = device_run(gpu_ctx, buf, frames, write=False)
    assert np.array_equal(crc, crc0) and np.array_equal(st, st0) and nbad == nbad0
    assert (parts["reserved"] == 0).all()


def test_throughput_form_host(gpu_ctx, oracle, mix300):
    """The same launch from a pageable host buffer (staged)."""
    buf, frames, datas = mix300
    crc, st, nbad, rc, parts = gpu_ctx.packet_verify_write(buf, [f[0] for f in frames], [f[1] for f in frames])
    check(oracle, buf, frames, datas, crc, st, parts, nbad)
    assert rc == -1010


@pytest.mark.parametrize("n", [1, 8, 200])
@pytest.mark.parametrize("path", ["device", "pinned", "pageable"])
def test_small_batches(gpu_ctx, oracle, n, path):
    """<= 256 frames: the device latency form (parse, bodies, H units, finish,
    fold), the host small-batch path over a page-locked buffer (H rides in the same
    batch, the fold is host arithmetic) and over a pageable one."""
    import tfs_amd.crc as crc_mod
    buf, frames, datas = build_mix(oracle, np.random.default_rng(50 + n), n)
    offs, lens = [f[0] for f in frames], [f[1] for f in frames]
    if path == "device":
        crc, st, parts, nbad = device_run(gpu_ctx, buf, frames)
    elif path == "pinned":
        pin = crc_mod.PinnedBuffer(gpu_ctx, len(buf))
        pin.array[:] = np.frombuffer(buf, np.uint8)
        crc, st, nbad, _, parts = gpu_ctx.packet_verify_write(pin.array, offs, lens)
        pin.free()
    else:
        crc, st, nbad, _, parts = gpu_ctx.packet_verify_write(buf, offs, lens)
    ndata = check(oracle, buf, frames, datas, crc, st, parts, nbad)
    assert ndata >= min(n, 1)


def test_small_batch_launched_host_path(oracle, monkeypatch):
    """The launched host path for a small batch (the measurement build's
    TFS_CRC_VARIANT=20 keeps parse / CRC / finish launches): same results."""
    import tfs_amd.crc as crc_mod
    monkeypatch.setenv("TFS_CRC_VARIANT", "20")
    ctx = crc_mod.Context(0)
    monkeypatch.setenv("TFS_CRC_VARIANT", "0")
    try:
        buf, frames, datas = build_mix(oracle, np.random.default_rng(60), 64)
        crc, st, nbad, _, parts = ctx.packet_verify_write(buf, [f[0] for f in frames], [f[1] for f in frames])
        check(oracle, buf, frames, datas, crc, st, parts, nbad)
    finally:
        ctx.close()


def test_decoder_returns_parts_for_a_whole_read(gpu_ctx, ds, oracle):
    """PacketDecoder::decode with a parts vector: one tfs_packet_verify_write over a
    received stream; each WRITE_DATA frame's part names its data and Func::crc(0, data),
    the other frames and a frame that fails its check get data_len -1."""
    datas, stream = [], []
    for i in range(12):
        data = synth_bytes(700 + i, 1 + 977 * i).tobytes()
        body = pk.write_data_body(9, 100 + i, 0, data, ds=list(range(i % 5)), lease=(2, 50 + i) if i % 2 else None)
        pcode = pk.WRITE_DATA_MESSAGE if i != 4 else pk.WRITE_DATA_MESSAGE + 2
        datas.append(data if i != 4 else None)
        stream.append(bytearray(sealed(oracle, body, pcode=pcode, pid=i)))
    stream[7][24 + 40] ^= 0x01  # frame 7 fails its check
    datas[7] = None
    raw = b"".join(bytes(s) for s in stream)
    rc, off, st, crc, parts, consumed = ds.decode_stream_write(gpu_ctx, raw)
    assert rc == -1010 and consumed == len(raw) and len(st) == 12
    frames = pk.split_frames(raw)
    assert [int(o) for o in off] == [f[0] for f in frames]
    check(oracle, raw, frames, datas, crc, st, parts)


def test_shift_device(gpu_ctx, oracle):
    """tfs_crc32_shift_device: 40 (crc, n) pairs against oracle_crc(c, zeros(n)) --
    every single bit 0..26, all-ones below 2^21, 0 and mixed lengths."""
    import tfs_amd.crc as crc_mod
    ns = [1 << k for k in range(27)] + [(1 << 21) - 1, 0, 3, 1025, 65536 + 17, 131073, (1 << 21) + 1, 5 << 20,
                                         (1 << 24) + (1 << 13) + 1, 12345, 255, 4097, (1 << 27) - 1]
    assert len(ns) == 40
    rng = np.random.default_rng(70)
    cs = rng.integers(0, 1 << 32, len(ns), dtype=np.uint64).astype(np.uint32)
    cs[:4] = [0, 1, 0x80000000, 0xFFFFFFFF]
    d_c = crc_mod.DeviceBuffer(gpu_ctx, 4 * len(ns)).upload(cs)
    d_n = crc_mod.DeviceBuffer(gpu_ctx, 4 * len(ns)).upload(np.array(ns, np.uint32))
    d_o = crc_mod.DeviceBuffer(gpu_ctx, 4 * len(ns))
    gpu_ctx.shift_device(d_c, d_n, len(ns), d_o)
    gpu_ctx.sync()
    got = d_o.download(np.uint32, len(ns))
    zeros = bytes(max(ns))
    for c, n, g in zip(cs, ns, got):
        assert int(g) == oracle.oracle_crc(int(c), zeros, n), (hex(int(c)), n)


def _persisted(blk, df, crc):
    """Close df into blk with `crc` and return the payload bytes that were persisted."""
    assert blk.close_write_file(1, crc, df) == 0
    return blk.raw()[FILEINFO:].tobytes()


DATAFILE_CASES = {
    # name: (fragments [(offset, length, carries a crc)], runs the GPU)
    "one": ([(0, 5000, True)], False),
    "three_in_order": ([(0, 4096, True), (4096, 4096, True), (8192, 777, True)], False),
    "three_out_of_order": ([(8192, 777, True), (0, 4096, True), (4096, 4096, True)], False),
    "overlap": ([(0, 4096, True), (4000, 4096, True)], True),
    "gap": ([(0, 4096, True), (5000, 1000, True)], True),
    "rewrite": ([(0, 4096, True), (4096, 4096, True), (0, 4096, True)], True),
    "one_without_crc": ([(0, 4096, True), (4096, 4096, False), (8192, 100, True)], True),
    "65_fragments": ([(64 * i, 64, True) for i in range(65)], True),
    "spill": ([(0, (2 << 20) + 1, True)], True),
}


@pytest.mark.parametrize("case", sorted(DATAFILE_CASES))
def test_datafile_fragments(gpu_ctx, ds, oracle, tmp_path, case):
    """DataFile::get_crc equals oracle_datafile_get_crc over the staged bytes in
    every case; tfs_crc32_stats.host_calls tells whether the GPU ran: not when
    every fragment carried a CRC and they tile the file, otherwise as before."""
    frags, runs_gpu = DATAFILE_CASES[case]
    df = ds.DataFile(gpu_ctx, 1, str(tmp_path))
    total = max(o + n for o, n, _ in frags)
    image = bytearray(total)
    known = np.zeros(total, bool)
    for k, (o, n, has_crc) in enumerate(frags):
        data = synth_bytes(300 + k, n).tobytes()
        if has_crc:
            assert df.set_data_crc(data, o, ocrc(oracle, 0, data)) == n
        else:
            assert df.set_data(data, o) == n
        image[o:o + n] = data
        known[o:o + n] = True
    assert df.get_length() == total
    before = gpu_ctx.stats()["host_calls"]
    got = df.get_crc()
    calls = gpu_ctx.stats()["host_calls"] - before
    assert (calls > 0) == runs_gpu, (case, calls)
    if total <= 2 << 20:
        # the bytes as staged (a gap holds whatever the buffer held): the persisted payload
        blk = ds.LogicBlock(900)
        payload = _persisted(blk, df, got)
        assert len(payload) == total
        assert np.array_equal(np.frombuffer(payload, np.uint8)[known], np.frombuffer(bytes(image), np.uint8)[known])
        blk.free()
    else:
        assert known.all()
        payload = bytes(image)
    assert got == oracle.oracle_datafile_get_crc(payload, len(payload)), case
    df.free()


def _lease_frames(oracle, n, frags, frag_len=4096):
    """n leases of `frags` sealed WRITE_DATA frames of frag_len data bytes each."""
    parts, off, ln, payloads, pos = [], [], [], [], 0
    for i in range(n):
        data = synth_bytes(4000 + i, frags * frag_len).tobytes()
        payloads.append(data)
        for k in range(frags):
            body = pk.write_data_body(321, i + 1, k * frag_len, data[k * frag_len:(k + 1) * frag_len],
                                      ds=[11, 12, 13][:(i + k) % 4], file_number=i + 1)
            fr = sealed(oracle, body, pid=i * frags + k)
            gap = (i * 7 + k * 3) % 8
            parts.append(b"\0" * gap + fr)
            off.append(pos + gap)
            ln.append(len(fr))
            pos += gap + len(fr)
    return b"".join(parts), off, ln, payloads


def _file_info(raw, off):
    import tfs_amd.crc as crc
    return np.frombuffer(raw[off:off + FILEINFO].tobytes(), crc.FILEINFO_DTYPE)[0]


@pytest.mark.parametrize("frags", [1, 3])
@pytest.mark.parametrize("gap", [0, 8])
def test_queue_loopback(gpu_ctx, ds, oracle, frags, gap):
    """64 leases x frags fragments of 4 KiB through one queue of WRITE and CLOSE
    items, 4 workers: in mode 0 (CRC at close) and mode 1 (data CRCs carried from
    the packet check) every persisted record's crc_ and payload equal the oracle's,
    the two leases with a wrong client CRC return -8013 and persist nothing, and
    mode 1 makes one GPU call less per lease (its closes make none)."""
    import tfs_amd.crc as crc_mod
    n = 64
    raw, off, ln, payloads = _lease_frames(oracle, n, frags)
    pin = crc_mod.PinnedBuffer(gpu_ctx, len(raw))
    pin.array[:] = np.frombuffer(raw, np.uint8)
    client = np.array([ocrc(oracle, 0, p) for p in payloads], np.uint32)
    wrong = {5, 40}
    for i in wrong:
        client[i] ^= 0x10
    calls = {}
    for mode in (0, 1):
        blk = ds.LogicBlock(321)
        before = gpu_ctx.stats()["host_calls"]
        rc, st = ds.loopback_queue(gpu_ctx, pin, off, ln, n, frags, client, 4, gap, mode, blk)
        calls[mode] = gpu_ctx.stats()["host_calls"] - before
        assert rc == len(wrong), (mode, rc)
        assert [i for i in range(n) if st[i] != 0] == sorted(wrong) and all(st[i] == -8013 for i in wrong)
        metas, _ = blk.metas()
        assert sorted(int(x) for x in metas["file_id"]) == [i + 1 for i in range(n) if i not in wrong]
        img = blk.raw()
        for m in metas:
            i = int(m["file_id"]) - 1
            fi = _file_info(img, int(m["offset"]))
            assert fi["crc_"] == ocrc(oracle, 0, payloads[i]), (mode, i)
            assert fi["size_"] == FILEINFO + len(payloads[i])
            o = int(m["offset"]) + FILEINFO
            assert img[o:o + len(payloads[i])].tobytes() == payloads[i], (mode, i)
        blk.free()
    # 4 workers close one lease per batch (CloseBatcher::batch_for): mode 0 makes one
    # verify call per lease, mode 1 none
    assert calls[0] - calls[1] == n, calls
    pin.free()


@pytest.mark.parametrize("mode", [0, 1])
def test_queue_loopback_device_error_at_a_write(gpu_ctx, ds, oracle, mode):
    """An injected device error at a write surfaces as -20001: that lease persists
    nothing (one worker, so the failing submission is lease 0's write)."""
    import tfs_amd.crc as crc_mod
    n = 6
    raw, off, ln, payloads = _lease_frames(oracle, n, 1)
    pin = crc_mod.PinnedBuffer(gpu_ctx, len(raw))
    pin.array[:] = np.frombuffer(raw, np.uint8)
    client = np.array([ocrc(oracle, 0, p) for p in payloads], np.uint32)
    blk = ds.LogicBlock(322)
    gpu_ctx.inject_device_error(0, 1)
    try:
        rc, st = ds.loopback_queue(gpu_ctx, pin, off, ln, n, 1, client, 1, 0, mode, blk)
    finally:
        gpu_ctx.inject_device_error(0, 0)
    assert rc == -20001 and st[0] == -20001 and (st[1:] == 0).all()
    metas, _ = blk.metas()
    assert sorted(int(x) for x in metas["file_id"]) == list(range(2, n + 1))
    blk.free()
    pin.free()
