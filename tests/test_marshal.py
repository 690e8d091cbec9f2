"""Marshalling session (include/tfs_ec.h tfs_ec_marshal_*): the
parity of a family encoded chunk by chunk, with every record of the data members
verified from the bytes that feed the code.

Expected values are composed from what is already pinned: oracle_ec_encode
(jerasure, tests/test_ec.py) for the parity of the zero-extended members,
oracle_crc and the FileInfo fields of the images for every CRC and status;
tfs_ec_encode_device and tfs_block_verify are second witnesses.  The images are
laid out by hand (Image below): records at chosen byte offsets with random bytes
in the gaps between them, which a LogicBlock cannot produce.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, ocrc
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

FI = 36
OK, CRC_ERR, PARAM, INFO_ERR, SIZE_ERR, SYNC_ERR = 0, -1010, -1016, -8016, -8034, -8038
DATA_INVALID, SIZE_INVALID, MATRIX_INVALID = -16001, -16002, -16003
FILL = 0xA5


@pytest.fixture(scope="module")
def ec_oracle():
    so = os.path.join(ROOT, "oracle", "liboracle_ec.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle_ec.so"])
    L = ctypes.CDLL(so)
    L.oracle_ec_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return L


def up(n, q):
    return (n + q - 1) // q * q


class Image:
    """A data member laid out by hand: records at chosen offsets, random bytes between them."""

    def __init__(self, oracle, seed):
        self.oracle, self.seed, self.parts, self.pos, self.metas, self.fid = oracle, seed, [], 0, [], 1

    def gap(self, n):
        if n:
            self.parts.append(synth_bytes(self.seed + 31 * len(self.parts), n))
            self.pos += n

    def rec(self, nbytes, at=None):
        """A record of `nbytes` payload bytes whose FileInfo starts at `at` (default: here)."""
        if at is not None:
            assert at >= self.pos, (at, self.pos)
            self.gap(at - self.pos)
        from tfs_amd.crc import FILEINFO_DTYPE
        p = synth_bytes(self.seed + 1000 + self.fid, nbytes)
        fi = np.zeros(1, FILEINFO_DTYPE)
        fi["id_"], fi["offset_"], fi["size_"], fi["usize_"] = self.fid + (self.seed << 20), self.pos, nbytes + FI, nbytes + FI
        fi["crc_"] = ocrc(self.oracle, 0, p.tobytes())
        self.metas.append((int(fi["id_"][0]), self.pos, nbytes + FI))
        self.parts += [fi.view(np.uint8).copy(), p]
        self.pos += FI + nbytes
        self.fid += 1
        return len(self.metas) - 1

    def payload(self, p0, p1):
        """A record whose payload is exactly [p0, p1)."""
        return self.rec(p1 - p0, at=p0 - FI)

    def fill(self, until, lo=900, hi=9000):
        """Records of varying length, some with gaps before them, up to about `until`."""
        i = 0
        while self.pos + FI + hi + 64 < until:
            self.gap((i * 5) % 23 if i % 3 == 0 else 0)
            self.rec(lo + (i * 2741) % (hi - lo))
            i += 1
        return self

    def image(self, size=None):
        from tfs_amd.crc import META_DTYPE
        img = np.concatenate(self.parts) if self.parts else np.zeros(0, np.uint8)
        if size is not None:
            assert size >= img.size
            img = np.concatenate([img, synth_bytes(self.seed + 5, size - img.size)])
        return img, np.array(self.metas, META_DTYPE)


def padded(imgs, total):
    out = []
    for a in imgs:
        b = np.zeros(total, np.uint8)
        b[:a.size] = a
        out.append(b)
    return out


def expected(oracle, ec_oracle, k, m, imgs, metas, total):
    """(parity list, crc, status) from the oracles."""
    from tfs_amd.crc import FILEINFO_DTYPE
    ms = padded(imgs, total) + [np.zeros(total, np.uint8) for _ in range(m)]
    p = (ctypes.c_void_p * (k + m))(*[a.ctypes.data for a in ms])
    assert ec_oracle.oracle_ec_encode(k, m, p, None, total) == 0
    crc, st = [], []
    for img, mt in zip(imgs, metas):
        for x in mt:
            off, sz = int(x["offset"]), int(x["size"])
            if off < 0 or off + sz > img.size:
                crc.append(0), st.append(PARAM)
            elif sz <= FI:
                crc.append(0), st.append(SIZE_ERR)
            else:
                fi = np.frombuffer(img[off:off + FI].tobytes(), FILEINFO_DTYPE)[0]
                c = ocrc(oracle, 0, img[off + FI:off + sz].tobytes())
                crc.append(c)
                st.append(INFO_ERR if int(fi["id_"]) != int(x["file_id"]) else SYNC_ERR if int(fi["size_"]) != sz else
                          CRC_ERR if int(fi["crc_"]) != c else OK)
    return ms[k:], np.array(crc, np.uint32), np.array(st, np.int32)


def chunks_of(total, clen):
    return [(o, min(clen, total - o)) for o in range(0, total, clen)]


def run(ctx, k, m, imgs, metas, total, chunks, form="device", stream=None, reuse=True):
    """One whole session.  Device form with reuse: every chunk goes through the same
    chunk-sized device buffers, as the reference's loop reuses its 1 MiB buffers."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, MarshalSession
    ec = ErasureCode(ctx, k, m)
    assert ec.rc == 0
    ses = MarshalSession(ec, metas, [a.size for a in imgs], total)
    assert ses.rc == 0
    data = padded(imgs, total)
    parity = [np.full(total, FILL, np.uint8) for _ in range(m)]
    if form == "host":
        for o, n in chunks:
            assert ses.encode([a[o:o + n] for a in data + parity], o, n) == 0
    elif reuse:
        cmax = max(n for _, n in chunks)
        d = [crc.DeviceBuffer(ctx, cmax) for _ in range(k + m)]
        sync = (lambda: ctx.stream_sync(stream)) if stream else ctx.sync
        for o, n in chunks:
            for i in range(k):
                d[i].upload(data[i][o:o + n])
            for i in range(m):
                d[k + i].upload(np.full(n, FILL, np.uint8))
            assert ses.encode_device(d, o, n, stream=stream) == 0
            sync()
            for i in range(m):
                parity[i][o:o + n] = d[k + i].download(np.uint8, n)
    else:
        d = [crc.DeviceBuffer(ctx, total).upload(a) for a in data + parity]
        for o, n in chunks:
            assert ses.encode_device([b.ptr + o for b in d], o, n, stream=stream) == 0
    res = ses.finish()
    if form == "device" and not reuse:
        parity = [d[k + i].download(np.uint8, total) for i in range(m)]
    ses.free()
    ec.free()
    return parity, res


def check(ctx, oracle, ec_oracle, k, m, imgs, metas, total, chunks, **kw):
    epar, ecrc, est = expected(oracle, ec_oracle, k, m, imgs, metas, total)
    par, (crc, st, nbad, rc) = run(ctx, k, m, imgs, metas, total, chunks, **kw)
    assert rc == 0
    for i in range(m):
        diff = np.nonzero(par[i] != epar[i])[0]
        assert diff.size == 0, (i, int(diff[0]), int(diff.size))
    flat = [x for mt in metas for x in mt]
    bad = np.nonzero(st != est)[0]
    assert bad.size == 0, [(int(i), flat[i], int(st[i]), int(est[i])) for i in bad[:5]]
    bad = np.nonzero(crc != ecrc)[0]
    assert bad.size == 0, [(int(i), flat[i], hex(crc[i]), hex(ecrc[i])) for i in bad[:5]]
    assert nbad == int((est != 0).sum())
    return par, crc, st


def family(oracle, k, seed, lens):
    """k filled members of the given block_len."""
    out = [Image(oracle, seed + i).fill(lens[i % len(lens)]).image(lens[i % len(lens)]) for i in range(k)]
    return [a for a, _ in out], [b for _, b in out]


@pytest.mark.parametrize("k,m", [(5, 3), (2, 1), (8, 4), (6, 6)])
def test_coders(gpu_ctx, oracle, ec_oracle, k, m):
    """(6, 6) takes two output groups: the CRC side runs with the first only."""
    from tfs_amd.ec import ErasureCode
    import tfs_amd.crc as crc
    lens = [70001, 98304, 65536 + 1024, 81920 - 7]
    imgs, metas = family(oracle, k, 10 * k + m, lens)
    total = up(max(a.size for a in imgs), 1024)
    par, gcrc, st = check(gpu_ctx, oracle, ec_oracle, k, m, imgs, metas, total, chunks_of(total, 16384))
    assert (st == 0).all() and len(st) > 10 * k
    # second witnesses: the plain encode and the block verify of the library
    d = [crc.DeviceBuffer(gpu_ctx, total).upload(a) for a in padded(imgs, total)] + \
        [crc.DeviceBuffer(gpu_ctx, total) for _ in range(m)]
    ec = ErasureCode(gpu_ctx, k, m)
    assert ec.encode_device(d, total) == 0
    gpu_ctx.sync()
    for i in range(m):
        assert (d[k + i].download(np.uint8, total) == par[i]).all()
    ec.free()
    at = 0
    for a, mt in zip(imgs, metas):
        c2, s2, _, _ = gpu_ctx.block_verify(a, mt)
        assert (c2 == gcrc[at:at + len(mt)]).all() and (s2 == 0).all()
        at += len(mt)


CHUNK = 16384  # the placements below speak of this chunk length


@pytest.fixture(scope="module")
def placements(oracle):
    """One member (of 5) with every placement the kernel takes another path for."""
    b = Image(oracle, 77)
    b.rec(1, at=5)                                   # a 1-byte payload
    pos = 128
    for s in range(8):                               # payload starts and ends at every residue mod 8 ...
        for e in range(8):
            p0 = up(pos + FI, 8) + s
            p1 = p0 + 8 * (2 + (s * 8 + e) % 5) + ((e - s) % 8)
            assert p0 % 8 == s and p1 % 8 == e
            b.payload(p0, p1)
            pos = p1
    # ... and on either side of 128, 1024 and 4096 byte boundaries, start and end
    base = up(b.pos + 200, 4096)
    for q in (128, 1024, 4096):
        for ds in (-1, 0, 1):
            p0 = base + q + ds
            b.payload(p0, p0 + 300 + ds)             # starts around the boundary
            p1 = base + 4096 + q + ds
            b.payload(p1 - 517, p1)                  # ends around the boundary (== q + ds mod 4096)
            base = up(b.pos + 200, 4096)
    C = up(b.pos + 100, CHUNK)                       # a chunk's start
    b.payload(C + 100, C + 128 * 9)                  # ends exactly on a packet's end
    b.payload(C + 1200, C + 2048)                    # ... a unit's end
    b.payload(C + 2100, C + 4096)                    # ... a tile's end
    b.payload(C + 4196, C + CHUNK)                   # ... a chunk's end
    b.rec(3000, at=C + CHUNK + 4096 - 10)            # FileInfo straddling a tile boundary
    b.rec(2000, at=C + 2 * CHUNK - 20)               # FileInfo straddling a chunk boundary
    b.rec(500, at=C + 2 * CHUNK + 8192 - FI)         # FileInfo ends on a tile boundary: the payload starts the next tile
    b.gap(up(b.pos, 4096) + 3 - b.pos)
    t0 = b.pos // 4096
    for i in range(40):                              # 40 records of 37-60 bytes in one tile
        b.rec(1 + (i * 7) % 24)
    assert (b.pos - 1) // 4096 == t0
    b.rec(3 * CHUNK + 777, at=up(b.pos, 4096) + 555)  # a record across at least three chunks, a gap before it
    b.gap(1000)
    b.rec(4096 * 2, at=up(b.pos + FI, 4096) - FI)    # a payload of two whole tiles exactly
    img, metas = b.image()
    others = family(oracle, 4, 300, [img.size - 5000, img.size + 3000, 90000, img.size])
    imgs = [others[0][0], img] + others[0][1:]
    ms = [others[1][0], metas] + others[1][1:]
    total = up(max(a.size for a in imgs), 1024)
    assert 64 << 10 <= total <= 256 << 10
    return imgs, ms, total


def test_placements_equivalences(gpu_ctx, oracle, ec_oracle, placements):
    """One chunk, many chunks (4 KiB, 8 KiB, 16 KiB) and the host form: identical parity, CRCs and statuses,
    all equal to the oracles'."""
    imgs, metas, total = placements
    ref = None
    for chunks, kw in [([(0, total)], {}), (chunks_of(total, 4096), {}), (chunks_of(total, 8192), {}),
                       (chunks_of(total, CHUNK), {}), (chunks_of(total, CHUNK), {"form": "host"}),
                       (chunks_of(total, 65536), {"reuse": False})]:
        par, crc, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, imgs, metas, total, chunks, **kw)
        assert (st == 0).all()
        if ref is None:
            ref = (par, crc, st)
        assert all((a == b).all() for a, b in zip(par, ref[0])) and (crc == ref[1]).all()


@pytest.mark.parametrize("units", [1, 2, 3])
def test_short_last_tile(gpu_ctx, oracle, ec_oracle, units):
    """total a multiple of 1024 but not of 4096; a record ends at the longest member's last byte."""
    total = 65536 + 1024 * units
    b = Image(oracle, 40 + units).fill(total - 12000)
    b.rec(total - b.pos - FI)                            # up to the member's last byte, into the short tile
    img, mt = b.image()
    assert img.size == total
    imgs, metas = family(oracle, 2, 50 + units, [total - 1024 * units - 3, 30000])
    imgs, metas = [imgs[0], img, imgs[1]], [metas[0], mt, metas[1]]
    for clen in (total, 8192):
        _, _, st = check(gpu_ctx, oracle, ec_oracle, 3, 2, imgs, metas, total, chunks_of(total, clen))
        assert (st == 0).all()


def test_big_record(gpu_ctx, oracle, ec_oracle):
    """One 3 MiB record (768 tiles: the fold's lanes chain 12 tiles each) beside small ones; 1 MiB chunks."""
    b = Image(oracle, 90)
    b.rec(5000)
    b.rec(3 << 20, at=6000 + 3)
    b.rec(777)
    img, mt = b.image()
    small = Image(oracle, 91).fill(200000)
    img2, mt2 = small.image()
    total = up(img.size, 1024)
    for reuse in (True, False):
        _, _, st = check(gpu_ctx, oracle, ec_oracle, 2, 1, [img, img2], [mt, mt2], total, chunks_of(total, 1 << 20),
                         reuse=reuse)
        assert (st == 0).all()


def test_corruption(gpu_ctx, oracle, ec_oracle):
    """A flipped payload byte is that record's CRC error alone; the parity is the encode of the bytes as given."""
    b = Image(oracle, 120)
    b.gap(50)
    r_first = b.rec(5000)
    r_mid = b.rec(9000)
    x = up(b.pos + 400, 4096)
    r_tile = b.payload(x - 300, x + 5000)
    r_last = b.rec(3000)
    b.gap(100)
    r_id = b.rec(2000)
    r_size = b.rec(2500)
    r_ok = b.rec(4000)
    b.gap(64)
    r_ok2 = b.rec(1234)
    img, mt = b.image()
    imgs, metas = family(oracle, 4, 130, [img.size + 2000, 70000])
    imgs, metas = [imgs[0], imgs[1], img, imgs[2], imgs[3]], [metas[0], metas[1], mt, metas[2], metas[3]]
    total = up(max(a.size for a in imgs), 1024)
    at = len(metas[0]) + len(metas[1])

    def o(r):
        return int(mt[r]["offset"])
    hurt = img.copy()
    hurt[o(r_first) + FI] ^= 1                                             # a payload's first byte
    hurt[o(r_mid) + FI + 4500] ^= 0x80                                     # interior
    hurt[up(o(r_tile) + FI, 4096)] ^= 2                                    # the first byte of the payload's second tile
    hurt[o(r_last) + int(mt[r_last]["size"]) - 1] ^= 0x10                  # a payload's last byte
    hurt[o(r_id) + 3] ^= 4                                                 # FileInfo.id_
    hurt[o(r_size) + 12] ^= 1                                              # FileInfo.size_
    hurt[o(r_ok2) - 10] ^= 0xFF                                            # a gap
    hurt[o(r_ok) + 20] ^= 0xFF                                             # another field of r_ok's own header
    want = {r_first: CRC_ERR, r_mid: CRC_ERR, r_tile: CRC_ERR, r_last: CRC_ERR, r_id: INFO_ERR, r_size: SYNC_ERR,
            r_ok: OK, r_ok2: OK}
    imgs[2] = hurt
    for clen in (total, 8192):
        par, crc, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, imgs, metas, total, chunks_of(total, clen))
        assert {r: int(st[at + r]) for r in want} == want
        assert int((st != 0).sum()) == 6                                   # nobody else; n_bad is checked by check()
    # a flipped byte in another record's header leaves the neighbours alone
    hurt2 = img.copy()
    hurt2[o(r_mid) + 33] ^= 1                                              # r_mid's crc_ field
    imgs[2] = hurt2
    _, _, st = check(gpu_ctx, oracle, ec_oracle, 5, 3, imgs, metas, total, chunks_of(total, 16384))
    assert st[at + r_mid] == CRC_ERR and int((st != 0).sum()) == 1 and st[at + r_first] == OK and st[at + r_tile] == OK


def test_rejected_before_the_pass(gpu_ctx, oracle, ec_oracle):
    """size <= 36, a record past sizes[i], a negative offset: reported, and the neighbours still verified."""
    from tfs_amd.crc import META_DTYPE
    imgs, metas = family(oracle, 2, 200, [80000, 66000])
    mt = metas[0].tolist()
    n = len(mt)
    last = mt[-1]
    mt.insert(3, (999, mt[3][1] - 40, 36))                    # size == 36, overlapping its neighbours' bytes
    mt.insert(1, (998, -5, 100))                              # negative offset
    mt.insert(6, (997, 100, 20))                              # size < 36, out of order
    mt.append((996, imgs[0].size - 100, 101))                 # one byte past block_len
    mt.append((995, imgs[0].size + 4096, 50))                 # wholly past block_len
    metas[0] = np.array(mt, META_DTYPE)
    total = 80896
    _, _, st = check(gpu_ctx, oracle, ec_oracle, 2, 1, imgs, metas, total, chunks_of(total, 8192))
    got = st[:len(mt)].tolist()
    assert got[1] == PARAM and got[4] == SIZE_ERR and got[6] == SIZE_ERR and got[-2:] == [PARAM, PARAM]
    assert got.count(0) == n and last[2] > FI


def test_no_records(gpu_ctx, oracle, ec_oracle):
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode
    imgs = [synth_bytes(900 + i, n) for i, n in enumerate((70000, 65536, 1))]
    metas = [np.zeros(0, crc.META_DTYPE)] * 3
    total = 70656
    par, c, st = check(gpu_ctx, oracle, ec_oracle, 3, 2, imgs, metas, total, chunks_of(total, 4096))
    assert len(st) == 0
    d = [crc.DeviceBuffer(gpu_ctx, total).upload(a) for a in padded(imgs, total)] + \
        [crc.DeviceBuffer(gpu_ctx, total) for _ in range(2)]
    ec = ErasureCode(gpu_ctx, 3, 2)
    assert ec.encode_device(d, total) == 0
    gpu_ctx.sync()
    assert all((d[3 + i].download(np.uint8, total) == par[i]).all() for i in range(2))
    ec.free()


def test_call_level_errors(gpu_ctx, oracle):
    """Every refused call launches nothing: the parity buffers keep their fill."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, MarshalSession
    imgs, metas = family(oracle, 2, 400, [66000, 70000])
    sizes = [a.size for a in imgs]
    total = 70656
    ec = ErasureCode(gpu_ctx, 2, 1)

    def begin(mt=metas, sz=sizes, tot=total, coder=ec):
        s = MarshalSession(coder, mt, sz, tot)
        rc = s.rc
        if rc:
            assert not s.h.value
        s.free()
        return rc
    assert begin() == 0
    assert begin(tot=total + 100) == SIZE_INVALID and begin(tot=0) == SIZE_INVALID and begin(tot=-1024) == SIZE_INVALID
    assert begin(sz=[sizes[0], total + 1]) == DATA_INVALID and begin(sz=[-1, sizes[1]]) == DATA_INVALID
    swapped = metas[0].copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    assert begin(mt=[swapped, metas[1]]) == PARAM                       # unsorted
    over = metas[1].copy()
    over["size"][1] += 1
    assert begin(mt=[metas[0], over]) == PARAM                          # overlapping
    assert begin(tot=total + 100, sz=[total + 200, 0]) == SIZE_INVALID  # the size check comes before the members'
    L = ec.L
    h = ctypes.c_void_p()
    assert L.tfs_ec_marshal_begin(None, None, None, None, total, ctypes.byref(h)) == PARAM
    # the chunk rules
    ses = MarshalSession(ec, metas, sizes, total)
    d = [crc.DeviceBuffer(gpu_ctx, total).upload(a) for a in padded(imgs, total)] + \
        [crc.DeviceBuffer(gpu_ctx, total).upload(np.full(total, FILL, np.uint8))]

    def at(o):
        return [b.ptr + o for b in d]
    s1, s2 = gpu_ctx.stream_create(), gpu_ctx.stream_create()
    try:
        assert ses.encode_device(at(4096), 4096, 4096, stream=s1) == PARAM      # the first chunk is at 0
        assert ses.encode_device(at(0), 0, 8192, stream=2) == PARAM             # hipStreamPerThread
        assert ses.encode_device(at(0), 0, 1000, stream=s1) == PARAM            # len % 1024
        assert ses.encode_device(at(0), 0, 5120, stream=s1) == PARAM            # len % 4096 before the end
        assert ses.encode_device(at(0), 0, 0, stream=s1) == PARAM
        assert ses.encode_device(at(0), 0, total + 1024, stream=s1) == PARAM    # past total
        assert ses.encode_device(at(0)[:2] + [None], 0, 8192, stream=s1) == DATA_INVALID
        assert ses.finish()[3] == PARAM                                         # nothing covered yet
        gpu_ctx.sync()
        assert (d[2].download(np.uint8, total) == FILL).all()
        assert ses.encode_device(at(0), 0, 8192, stream=s1) == 0
        assert ses.encode_device(at(0), 0, 8192, stream=s1) == PARAM            # repeated
        assert ses.encode_device(at(12288), 12288, 4096, stream=s1) == PARAM    # skipped
        assert ses.encode_device(at(8192), 8192, 4096, stream=s2) == PARAM      # another stream
        assert ses.encode_device(at(8192), 8192, 4096, stream=None) == PARAM    # the context's stream is another one too
        assert ses.encode([np.zeros(4096, np.uint8)] * 3, 8192, 4096) == PARAM  # and so is the host form's
        assert ses.finish()[3] == PARAM                                         # before the last chunk
        gpu_ctx.stream_sync(s1)
        assert (d[2].download(np.uint8, total)[8192:] == FILL).all()
        assert ses.encode_device(at(8192), 8192, 2048, stream=s1) == PARAM      # offset + len != total
        assert ses.encode_device(at(8192), 8192, total - 8192, stream=s1) == 0  # 62,464 bytes: 1 KiB units to the end
        crc_, st, nbad, rc = ses.finish()
        assert rc == 0 and (st == 0).all() and nbad == 0 and len(st) == len(metas[0]) + len(metas[1])
        assert ses.encode_device(at(0), 0, 8192, stream=s1) == PARAM            # a finished session takes no chunk
    finally:
        ses.free()
        gpu_ctx.stream_destroy(s1)
        gpu_ctx.stream_destroy(s2)
        ec.free()
