"""The seeded packet kernels at the stripe-0 seed edge (tests/crc_geometry.py).

A frame's body is checksummed with seed TFS_PACKET_FLAG_V1, whose four bytes are
all non-zero, from `frame offset + 24`.  When that device address is 125, 126 or
127 (mod 128) and the body has one of the edge lengths (913 bytes at least), the
seed's high bytes belong to lane 0's first dword of stripe 1 and the kernels
carry them there.  Here every frame is placed from the device address of the
buffer that holds it -- DeviceBuffer.ptr, or tfs_crc32_host_device_ptr for
page-locked memory read in place -- so that its body takes the wanted residue:
the 135 edge shapes, each with its two neighbours that do not cross, and a sweep
of the ds_ count 0..27 at the three edge residues and three others.  Bodies are
WriteDataMessage bodies (pk.write_data_body), so the write-data form yields a
data CRC too.  Expected values come from the oracle (oracle_packet_verify /
oracle_packet_seal / oracle_crc), the zlib identity is the second witness for
the body CRC, and assert_edge_coverage checks the placements each batch ran.

The prefix H of a write frame (at most 252 bytes) cannot reach the edge
(tests/test_crc_geometry.py), its body can: both ride in the same launch here.
"""
import struct

import numpy as np
import pytest

import crc_geometry as cg
from conftest import ocrc
from test_packet import SEED, o_seal, o_verify, zlib_func_crc
from test_write_frames import check
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

HDR = pk.HEADER_V1_SIZE
SLACK = 128                      # after every frame: the kernels read whole 128-byte lines
TAIL = 1000 + 256                # after the last frame: `avail` may exceed a frame by 1000
SWEEP_RESIDUES = (125, 126, 127, 124, 122, 60)
CRC_ERROR = -1010


def list_items():
    """[(body residue, body length, ds_ count, kind, data seed)]: the edge list with
    neighbours, then the count sweep."""
    items = []
    for i, e in enumerate(cg.edge_cases()):
        items.append((e.residue, e.length, i % 28, "edge", 100 + 3 * i))
        for k, (r, n) in enumerate(cg.neighbours(e)):
            items.append((r, n, (i + 7 + k) % 28, "nbr", 101 + 3 * i + k))
    for r in SWEEP_RESIDUES:
        blen = cg.edge_length(r - 124 if r > 124 else 2, 2, 16, 1)
        for count in range(28):
            items.append((r, blen, count, "sweep", 2000 + 28 * r + count))
    return items


def image_cap(items):
    return sum(HDR + n + SLACK + cg.LINE for _, n, _, _, _ in items) + TAIL + 256


class Image:
    """Sealed frames placed from the absolute device address `addr` of their buffer."""

    def __init__(self, oracle, addr, items, cap=None):
        self.addr, self.items = addr, items
        raw = bytearray()
        self.frames, self.datas, self.counts = [], [], []
        for i, (res, blen, count, _, dseed) in enumerate(items):
            body_off = cg.place(addr + len(raw) + HDR, res) - addr
            raw += b"\xAA" * (body_off - HDR - len(raw))
            data = synth_bytes(dseed, blen - 36 - 8 * count).tobytes()
            body = pk.write_data_body(i + 1, 77 + i, 4096 * i, data, ds=list(range(count)))
            assert len(body) == blen
            self.frames.append((len(raw), HDR + blen))
            self.datas.append(data)
            self.counts.append(count)
            raw += pk.frame_v1(body, pid=i, crc=ocrc(oracle, SEED, body))
            raw += b"\xAA" * SLACK
        raw += b"\xAA" * TAIL
        if cap is not None:
            assert len(raw) <= cap
            raw += b"\xAA" * (cap - len(raw))
        self.raw = raw
        self.kind = np.array([it[3] for it in items])
        self.placed = [(addr + o + HDR, n - HDR) for o, n in self.frames]
        self.crosses = np.array([cg.seed_crosses(a, n) for a, n in self.placed])
        for (a, _), it in zip(self.placed, items):
            assert a % 128 == it[0]

    def sealed(self):
        return bytes(self.raw)

    def unsealed(self):
        b = bytearray(self.raw)
        for o, _ in self.frames:
            struct.pack_into("<I", b, o + 20, 0)
        return bytes(b)

    def body(self, i):
        o, n = self.frames[i]
        return bytes(self.raw[o + HDR:o + n])

    def batches(self, size):
        """Index lists: `small` -- at most 256 frames each (the edge list, the sweep,
        the neighbours); `large` -- everything in one launch of more than 256."""
        if size == "large":
            out = [np.arange(len(self.frames))]
            assert out[0].size > 256
            return out
        nb = np.nonzero(self.kind == "nbr")[0]
        out = [np.nonzero(self.kind == "edge")[0], np.nonzero(self.kind == "sweep")[0]]
        out += [nb[k:k + 200] for k in range(0, nb.size, 200)]
        assert all(0 < b.size <= 256 for b in out)
        return out

    def check_coverage(self, idx):
        """The batch reaches every class of the edge if it carries the edge list; what
        crosses in it is exactly what was built to."""
        kinds = self.kind[idx]
        if (kinds == "edge").any():
            cg.assert_edge_coverage([self.placed[i] for i in idx])
        want = [k == "edge" or (k == "sweep" and self.items[i][0] > 124) for i, k in zip(idx, kinds)]
        assert self.crosses[idx].tolist() == want


def dev_run(ctx, d_base, frames, mode, extra=0):
    """One device launch over `frames` [(offset, len)]; `extra` is added to every len
    (an `avail` that exceeds the frame).  Returns (crc, status, n_bad, parts)."""
    import tfs_amd.crc as crc_mod
    n = len(frames)
    d = np.zeros(n, crc_mod.PACKET_DESC_DTYPE)
    d["offset"] = [f[0] for f in frames]
    d["len"] = [f[1] + extra for f in frames]
    bufs = [crc_mod.DeviceBuffer(ctx, sz) for sz in (d.nbytes, 4 * n, 4 * n, 16 * n, 4)]
    d_desc, d_crc, d_st, d_parts, d_bad = bufs
    d_desc.upload(d)
    d_bad.zero()
    parts = None
    if mode == "verify":
        ctx.packet_verify_device(d_desc, n, d_base, d_crc, d_st, d_bad)
    elif mode == "seal":
        ctx.packet_seal_device(d_desc, n, d_base, d_crc, d_st)
    else:
        ctx.packet_verify_write_device(d_desc, n, d_base, d_crc, d_st, d_parts, d_bad)
    ctx.sync()
    if mode == "write":
        parts = d_parts.download(crc_mod.WRITE_PART_DTYPE, n)
    out = (d_crc.download(np.uint32, n), d_st.download(np.int32, n), int(d_bad.download(np.uint32, 1)[0]), parts)
    for b in bufs:
        b.free()
    return out


@pytest.fixture(scope="module")
def dev_image(gpu_ctx, oracle):
    """The edge list, neighbours and count sweep in device memory, placed from DeviceBuffer.ptr."""
    import tfs_amd.crc as crc_mod
    items = list_items()
    cap = image_cap(items)
    d_base = crc_mod.DeviceBuffer(gpu_ctx, cap)
    img = Image(oracle, d_base.ptr, items, cap)
    yield d_base, img
    d_base.free()


def check_write(oracle, img, idx, crc, st, parts, nbad, extra=0):
    frames = [(img.frames[i][0], img.frames[i][1] + extra) for i in idx]
    datas = [img.datas[i] for i in idx]
    ndata = check(oracle, img.sealed(), frames, datas, crc, st, parts, nbad)
    assert ndata == len(idx) and nbad == 0
    assert parts["data_off"].tolist() == [36 + 8 * img.counts[i] for i in idx]
    assert (parts["reserved"] == 0).all()


@pytest.mark.parametrize("form", ["small", "one_pass", "three"])
def test_verify_and_seal_device_at_the_edge(gpu_ctx, oracle, dev_image, form, monkeypatch):
    """tfs_packet_verify_device and tfs_packet_seal_device at three launch sizes: at
    most 256 frames (parse, latency form, finish), more (the one-pass
    packet_files_kernel, both modes) and the measurement build's three-launch form
    (TFS_CRC_VARIANT=51).  Statuses, CRCs and n_bad equal the oracle's; after the
    seal the whole buffer equals the oracle's sealed bytes: only the four bytes
    at +20 of each frame of the batch change, not the 0xAA gaps nor the bytes of a
    neighbouring frame that share a line with a body's end."""
    import tfs_amd.crc as crc_mod
    d_base, img = dev_image
    ctx = gpu_ctx
    if form == "three":
        monkeypatch.setenv("TFS_CRC_VARIANT", "51")
        ctx = crc_mod.Context(0)
        monkeypatch.setenv("TFS_CRC_VARIANT", "0")
    try:
        sealed, unsealed = img.sealed(), img.unsealed()
        for idx in img.batches("small" if form == "small" else "large"):
            img.check_coverage(idx)
            frames = [img.frames[i] for i in idx]
            d_base.upload(np.frombuffer(sealed, np.uint8))
            crc, st, nbad, _ = dev_run(ctx, d_base, frames, "verify")
            ocrc_, ost, obad = o_verify(oracle, sealed, frames)
            bad = np.nonzero(crc != ocrc_)[0]
            assert bad.size == 0, [(cg.classify(*img.placed[idx[k]]), img.frames[idx[k]]) for k in bad[:8]]
            assert np.array_equal(st, ost) and (st == 0).all() and nbad == obad == 0
            for k, i in enumerate(idx):
                if img.crosses[i]:
                    assert int(crc[k]) == zlib_func_crc(SEED, img.body(i)), img.items[i]
            d_base.upload(np.frombuffer(unsealed, np.uint8))
            crc2, st2, _, _ = dev_run(ctx, d_base, frames, "seal")
            ob, ocrc2, ost2 = o_seal(oracle, unsealed, frames)
            assert np.array_equal(crc2, ocrc2) and np.array_equal(st2, ost2) and np.array_equal(crc2, ocrc_)
            got = d_base.download(np.uint8, len(sealed))
            assert np.array_equal(got, ob)
            diff = np.nonzero(got != np.frombuffer(unsealed, np.uint8))[0]
            allowed = {o + 20 + b for o, _ in frames for b in range(4)}
            assert set(diff.tolist()) <= allowed
            for o, n in frames:
                assert got[o:o + n].tobytes() == sealed[o:o + n]
    finally:
        if form == "three":
            ctx.close()


@pytest.mark.parametrize("size", ["small", "large"])
def test_verify_write_device_at_the_edge_and_every_count(gpu_ctx, oracle, dev_image, size):
    """tfs_packet_verify_write_device (packet_write_kernel for more than 256 frames,
    the latency form below): every frame's data CRC equals oracle_crc(0, D), its
    data_off is 36 + 8 count and data_len the data's, with count swept over 0..27
    at body residues 125, 126, 127 (the edge) and 124, 122, 60."""
    d_base, img = dev_image
    d_base.upload(np.frombuffer(img.sealed(), np.uint8))
    swept = {(img.items[i][0], img.counts[i]) for i in np.nonzero(img.kind == "sweep")[0]}
    assert swept == {(r, c) for r in SWEEP_RESIDUES for c in range(28)}
    for idx in img.batches(size):
        img.check_coverage(idx)
        frames = [img.frames[i] for i in idx]
        crc, st, nbad, parts = dev_run(gpu_ctx, d_base, frames, "write")
        check_write(oracle, img, idx, crc, st, parts, nbad)


def sensitivity_items():
    """One edge frame per s (three stripes, nvalid 63, 15 tail bytes) in 1 + 30 + 1
    copies; flips[k] = (byte position in the frame, bit) for copy k, None: untouched."""
    items, flips = [], []
    for s in cg.EDGE_S:
        e = cg.edge_case(s, 3, 16, 15)
        pos = list(range(8))                                  # the dwords at A and A + 4
        pos += [4 - s, 4 - s + 15]                            # lane 0's run of stripe 1: first and last byte
        pos += [e.length - e.t - 1]                           # the last byte before B16
        pos += list(range(e.length - e.t, e.length))          # the tail
        body_pos = sorted(set(pos))
        assert len(body_pos) == 8 + 1 + 1 + 15 and body_pos[-1] == e.length - 1
        fl = [None] + [(HDR + p, (p * 3 + s) % 8) for p in body_pos] + [(20 + b, (b + s) % 8) for b in range(4)] + [None]
        for f in fl:
            items.append((e.residue, e.length, 3, "edge", 7000 + s))   # the same body in every copy
            flips.append(f)
    return items, flips


@pytest.mark.parametrize("size", ["small", "large"])
def test_single_bit_flips_at_the_edge(gpu_ctx, oracle, size):
    """Copies of one edge frame per s with one bit flipped in the first eight body
    bytes, lane 0's run of stripe 1, the last byte before B16, every tail byte and
    every byte of the header CRC: exactly the flipped copies fail their check,
    every untouched one passes, and the CRC computed is the oracle's.  `large`:
    the same frames three times over in one launch of more than 256."""
    import tfs_amd.crc as crc_mod
    items, flips = sensitivity_items()
    cap = image_cap(items)
    d_base = crc_mod.DeviceBuffer(gpu_ctx, cap)
    try:
        img = Image(oracle, d_base.ptr, items, cap)
        assert img.crosses.all()
        raw = bytearray(img.raw)
        for (o, _), f in zip(img.frames, flips):
            if f is not None:
                raw[o + f[0]] ^= 1 << f[1]
        raw = bytes(raw)
        d_base.upload(np.frombuffer(raw, np.uint8))
        frames = list(img.frames) * (1 if size == "small" else 3)
        want = [0 if f is None else CRC_ERROR for f in flips] * (len(frames) // len(flips))
        assert (len(frames) > 256) == (size == "large") and want.count(0) == 2 * 3 * (len(frames) // len(flips))
        ocrc_, ost, obad = o_verify(oracle, raw, frames)
        assert ost.tolist() == want
        for mode in ("verify", "write"):
            crc, st, nbad, parts = dev_run(gpu_ctx, d_base, frames, mode)
            assert st.tolist() == want, (mode, [k for k in range(len(want)) if st[k] != want[k]][:8])
            assert np.array_equal(crc, ocrc_) and nbad == obad == len(want) - want.count(0)
            if parts is not None:
                assert [p >= 0 for p in parts["data_len"]] == [w == 0 for w in want]
    finally:
        d_base.free()


@pytest.mark.parametrize("size", ["small", "large"])
def test_avail_larger_than_the_frame(gpu_ctx, oracle, dev_image, size):
    """tfs_packet_desc.len is the bytes available, and a streamer's buffer usually
    holds more than one frame: with len = frame + 1 and frame + 1000 (the extra
    bytes inside the buffer, 0xAA or the next frame) verify, the write-data form
    and seal give the CRCs, statuses, parts and sealed bytes of the exact-length
    run and of the oracle."""
    d_base, img = dev_image
    sealed, unsealed = img.sealed(), img.unsealed()
    idx = img.batches(size)[0]
    img.check_coverage(idx)
    frames = [img.frames[i] for i in idx]
    assert max(o + n for o, n in frames) + 1000 + 128 <= len(sealed)
    d_base.upload(np.frombuffer(sealed, np.uint8))
    crc0, st0, nbad0, _ = dev_run(gpu_ctx, d_base, frames, "verify")
    for extra in (1, 1000):
        wide = [(o, n + extra) for o, n in frames]
        ocrc_, ost, obad = o_verify(oracle, sealed, wide)
        crc, st, nbad, _ = dev_run(gpu_ctx, d_base, frames, "verify", extra)
        assert np.array_equal(crc, ocrc_) and np.array_equal(st, ost) and nbad == obad == 0
        assert np.array_equal(crc, crc0) and np.array_equal(st, st0) and nbad == nbad0
        crc, st, nbad, parts = dev_run(gpu_ctx, d_base, frames, "write", extra)
        assert np.array_equal(crc, crc0)
        check_write(oracle, img, idx, crc, st, parts, nbad, extra)
    for extra in (1, 1000):
        wide = [(o, n + extra) for o, n in frames]
        d_base.upload(np.frombuffer(unsealed, np.uint8))
        crc, st, _, _ = dev_run(gpu_ctx, d_base, frames, "seal", extra)
        ob, ocrc2, ost2 = o_seal(oracle, unsealed, wide)
        assert np.array_equal(crc, ocrc2) and np.array_equal(st, ost2) and np.array_equal(crc, crc0)
        assert np.array_equal(d_base.download(np.uint8, len(sealed)), ob)


@pytest.mark.parametrize("where", ["pinned_in_place", "staged"])
def test_host_forms_at_the_edge(gpu_ctx, oracle, where):
    """tfs_packet_verify, tfs_packet_seal and tfs_packet_verify_write from host memory.

    pinned_in_place: at most 256 frames in page-locked memory within 8 MiB -- the
    bodies' CRCs go through the synchronous small-batch path, which reads them in
    place (the resident ring lands bodies of up to 16 KiB in slots of its own only
    while a batch's landed bytes stay within 64 KiB: the edge batch holds more), so
    the frames are placed from tfs_crc32_host_device_ptr.

    staged: more than 256 frames are copied to the device first; span_of rounds the
    span's start down to a multiple of 256 and the staging buffer is a whole
    hipMalloc allocation, so a body's device residue mod 128 is that of its offset
    in the caller's buffer: the frames are placed by their offsets."""
    import tfs_amd.crc as crc_mod
    items = list_items()
    cap = image_cap(items)
    pin = None
    try:
        if where == "pinned_in_place":
            pin = crc_mod.PinnedBuffer(gpu_ctx, cap)
            img = Image(oracle, gpu_ctx.host_device_ptr(pin.ptr), items, cap)
            arr = pin.array
            idx = img.batches("small")[0]
            landable = sum(n - HDR for _, n in (img.frames[i] for i in idx) if n - HDR <= 16384)
            assert landable > 64 << 10 and cap <= 8 << 20
        else:
            img = Image(oracle, 0, items, cap)
            arr = np.zeros(cap, np.uint8)
            idx = img.batches("large")[0]
        img.check_coverage(idx)
        sealed, unsealed = img.sealed(), img.unsealed()
        offs, lens = [img.frames[i][0] for i in idx], [img.frames[i][1] for i in idx]
        frames = list(zip(offs, lens))
        ocrc_, ost, obad = o_verify(oracle, sealed, frames)
        arr[:] = np.frombuffer(sealed, np.uint8)
        crc, st, nbad, rc = gpu_ctx.packet_verify(arr, offs, lens)
        bad = np.nonzero(crc != ocrc_)[0]
        assert bad.size == 0, [(cg.classify(*img.placed[idx[k]]), img.frames[idx[k]]) for k in bad[:8]]
        assert np.array_equal(st, ost) and nbad == obad == 0 and rc == 0
        crc, st, nbad, rc, parts = gpu_ctx.packet_verify_write(arr, offs, lens)
        assert rc == 0 and np.array_equal(crc, ocrc_)
        check_write(oracle, img, idx, crc, st, parts, nbad)
        arr[:] = np.frombuffer(unsealed, np.uint8)
        crc, st = gpu_ctx.packet_seal(arr, offs, lens)
        ob, ocrc2, ost2 = o_seal(oracle, unsealed, frames)
        assert np.array_equal(crc, ocrc2) and np.array_equal(st, ost2) and np.array_equal(arr, ob)
        for o, n in frames:
            assert arr[o:o + n].tobytes() == sealed[o:o + n]
    finally:
        if pin is not None:
            pin.free()
