"""Receive sessions (include/tfs_receive.h) on the GPU: frames sealed by a
replicate session or built by hand land in a block image byte for byte, every frame's outcome
against the oracle's seal, every record's verdict at finish against oracle_verify_file, the
replicate session's own verdicts and tfs_block_verify_device of the landed image -- through
the device form in one call, frame by frame and in ragged groups, at every shift, and the
host forms.  Everything is bit-exact.

The grid geometry is 12 G + 333 bytes, not 5 G: a FileInfo cut after each of six byte counts
needs six granule boundaries of its own."""
import ctypes
import struct

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from test_replicate import (BLOCK, GEOMETRY, PID, SPLITS, build_block, cfg_for, expected_verdicts, prefill, run_device,
                            zcrc)

pytestmark = pytest.mark.gpu

PARAM, SIZE_ERR, INFO_ERR, SYNC_ERR, CRC_ERR, ERR = -1016, -8034, -8016, -8038, -1010, -1
SIZE_INVALID = -16002
FLAG = pk.TFS_PACKET_FLAG_V1


def granule():
    import tfs_amd.crc as crc
    return crc.receive_granule()


def grid_layout(G):
    return ([("rec", 100),                                   # inside granule 0
             ("at", G - 36), ("rec", 500),                   # payload starts on a boundary
             ("at", 2 * G - 336), ("rec", 300)] +            # payload ends on one
            [item for i, k in enumerate(SPLITS) for item in (("at", (3 + i) * G - k), ("rec", 200))] +
            [("at", 9 * G - 50), ("rec", 2 * G + 700),       # whole granules 9 and 10
             ("at", 12 * G + 333 - 186), ("rec", 150)])      # ends at the last byte of a ragged tail


@pytest.fixture(scope="module")
def blocks(oracle):
    G = granule()
    rep = build_block(oracle, GEOMETRY)
    grid = build_block(oracle, grid_layout(G))
    img, metas = grid
    assert img.size == 12 * G + 333
    offs = [int(m["offset"]) for m in metas]
    assert offs[1] + 36 == G and offs[2] + int(metas[2]["size"]) == 2 * G
    for i, k in enumerate(SPLITS):
        assert (offs[3 + i] + k) % G == 0
    assert offs[-1] + int(metas[-1]["size"]) == img.size
    return {"rep": rep, "grid": grid}


def sealed(ctx, img, metas, fl, **kw):
    """The block's frames as a replicate session seals them, and its finish()."""
    cfg = cfg_for(img, fl, **kw)
    out, _, stride, res = run_device(ctx, img, metas, cfg)
    frames = [out[k * stride:k * stride + 60 + min(fl, img.size - k * fl)].copy()
              for k in range(max(1, -(-img.size // fl)))]
    return frames, res


def hand_frames(oracle, img, lens, block_id=BLOCK, version=2, new_block=1):
    """Frames of any lengths over img, sealed by the oracle."""
    frames, off = [], 0
    for k, n in enumerate(lens):
        data = img[off:off + n].tobytes()
        body = struct.pack("<IQiiiQ", block_id, 0, off, n, 0, 0) + data + struct.pack("<i", new_block if k == 0 else 0)
        f = np.frombuffer(pk.frame_v1(body, 35, version, PID + k), np.uint8).copy()
        if version >= 1:
            o, av = np.zeros(1, np.uint64), np.array([f.size], np.uint32)
            cc, st = np.zeros(1, np.uint32), np.zeros(1, np.int32)
            oracle.oracle_packet_seal(f.ctypes.data, o.ctypes.data, av.ctypes.data, 1, cc.ctypes.data, st.ctypes.data)
            assert st[0] == 0 and struct.unpack_from("<I", f, 20)[0] == zcrc(FLAG, body)
        frames.append(f)
        off += n
    assert off == img.size
    return frames


def lay_out(frames, shift=0, pad=5):
    """(base, descs): the frames in one buffer, `pad` bytes of filler between them."""
    import tfs_amd.crc as crc
    size = shift + sum(f.size + pad for f in frames) + 64
    base = prefill(size)
    descs = np.zeros(len(frames), crc.RECEIVE_DESC_DTYPE)
    o = shift
    for j, f in enumerate(frames):
        base[o:o + f.size] = f
        rc, d = crc.receive_parse(base[o:o + f.size], frame_off=o)
        assert rc == 0
        descs[j] = d[0]
        o += f.size + pad
    return base, descs


def groups_of(n, sizes):
    out, j, k = [], 0, 0
    while j < n:
        m = min(sizes[k % len(sizes)], n - j)
        out.append((j, j + m))
        j, k = j + m, k + 1
    return out


class Landed:
    pass


def receive(ctx, frames, metas, groups=None, cap=None, shift=0, ishift=0, block_id=BLOCK, before_finish=None,
            descs_edit=None):
    """The frames through the device form; returns what landed and every outcome."""
    import tfs_amd.crc as crc
    total = sum(f.size - 60 for f in frames)
    cap = total + 100 if cap is None else cap
    base, descs = lay_out(frames, shift)
    if descs_edit:
        descs_edit(descs)
    n = len(frames)
    before = prefill(cap + 64)
    d_base = crc.DeviceBuffer(ctx, base.size).upload(base)
    d_img = crc.DeviceBuffer(ctx, ishift + cap + 64)
    d_img.upload(before, offset=ishift)
    d_parts = crc.DeviceBuffer(ctx, n * 16)
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.zero()
    r = Landed()
    with crc.ReceiveSession(ctx, crc.receive_cfg(cap, block_id), d_img.ptr + ishift) as s:
        for a, b in (groups or [(0, n)]):
            s.frames_device(d_base, descs[a:b], d_parts.ptr + 16 * a, d_bad)
        if before_finish:
            ctx.sync()
            before_finish(d_img, ishift)
        r.crc, r.st, r.rbad, r.total = s.finish(metas)
    r.image = d_img.download(np.uint8, cap + 64, offset=ishift)
    r.parts = d_parts.download(crc.RECEIVE_PART_DTYPE)
    r.nbad = int(d_bad.download(np.uint32)[0])
    r.base_same = bool((d_base.download(np.uint8) == base).all())
    r.before = before
    for d in (d_base, d_img, d_parts, d_bad):
        d.free()
    return r


def check_landed(r, img, frames):
    total = img.size
    assert r.total == total
    assert (r.image[:total] == img).all(), "the landed image differs from the source"
    assert (r.image[total:] == r.before[total:]).all(), "a byte beyond total was written"
    assert r.base_same, "a byte of the frame buffer was written"
    assert r.parts["status"].tolist() == [0] * len(frames) and r.nbad == 0
    assert r.parts["crc"].tolist() == [struct.unpack_from("<I", f, 20)[0] for f in frames]
    assert r.parts["flag"][0] in (1, 2) and not r.parts["flag"][1:].any() and not r.parts["reserved"].any()


def check_verdicts(oracle, r, img, metas):
    ecrc, est = expected_verdicts(oracle, img, metas, img.size)
    assert r.st.tolist() == est.tolist()
    assert r.crc.tolist() == ecrc.tolist()
    assert r.rbad == int((est != 0).sum())


# ---- 1. round trip ---------------------------------------------------------------------------

@pytest.mark.parametrize("grouping", ["one", "each", "ragged"])
@pytest.mark.parametrize("fl", [1024, 4096])
@pytest.mark.parametrize("name", ["rep", "grid"])
def test_round_trip(gpu_ctx, oracle, blocks, name, fl, grouping):
    import tfs_amd.crc as crc
    img, metas = blocks[name]
    frames, rep_res = sealed(gpu_ctx, img, metas, fl, new_block=1 if name == "rep" else 2)
    n = len(frames)
    groups = {"one": None, "each": groups_of(n, (1,)), "ragged": groups_of(n, (3, 1, 5, 2))}[grouping]
    r = receive(gpu_ctx, frames, metas, groups)
    check_landed(r, img, frames)
    assert r.parts["crc"].tolist() == rep_res[3].tolist()        # the replicate session's out_frame_crc
    check_verdicts(oracle, r, img, metas)
    assert r.crc.tolist() == rep_res[0].tolist() and r.st.tolist() == rep_res[1].tolist()
    # tfs_block_verify_device of what landed
    d_img = crc.DeviceBuffer(gpu_ctx, img.size + 256).upload(r.image[:img.size])
    d_m = crc.DeviceBuffer(gpu_ctx, metas.nbytes).upload(metas)
    d_c, d_s = crc.DeviceBuffer(gpu_ctx, 4 * len(metas)), crc.DeviceBuffer(gpu_ctx, 4 * len(metas))
    gpu_ctx.block_verify_device(d_img, img.size, d_m, len(metas), d_c, d_s)
    gpu_ctx.sync()
    assert d_c.download(np.uint32).tolist() == r.crc.tolist() and d_s.download(np.int32).tolist() == r.st.tolist()
    for d in (d_img, d_m, d_c, d_s):
        d.free()


# ---- 2. frame cuts off the grid ----------------------------------------------------------------

def off_grid_lens(total, G):
    lens = [1, G - 1, 17, 2 * G + 5, 3, 5, G - 30, G, 1000, 2, 1, G + 1]
    assert sum(lens) < total
    return lens + [total - sum(lens)]


@pytest.mark.parametrize("grouping", ["one", "each", "pairs"])
def test_frame_cuts_off_the_grid(gpu_ctx, oracle, blocks, grouping):
    """Granules assembled from two and three frames (17 + 3 + 5 bytes share granules with their
    neighbours), within one call and across calls."""
    img, metas = blocks["grid"]
    frames = hand_frames(oracle, img, off_grid_lens(img.size, granule()))
    n = len(frames)
    r = receive(gpu_ctx, frames, metas, {"one": None, "each": groups_of(n, (1,)), "pairs": groups_of(n, (2, 3))}[grouping])
    check_landed(r, img, frames)
    check_verdicts(oracle, r, img, metas)


# ---- 3. every shift ------------------------------------------------------------------------------

def short_lens(total, G):
    return [1, G - 1, 17, 2 * G + 5, total - 3 * G - 22]


@pytest.mark.parametrize("shift", range(16))
def test_every_frame_shift(gpu_ctx, oracle, blocks, shift):
    img, metas = blocks["rep"]
    frames = hand_frames(oracle, img, short_lens(img.size, granule()))
    r = receive(gpu_ctx, frames, metas, shift=shift)
    check_landed(r, img, frames)
    check_verdicts(oracle, r, img, metas)


@pytest.mark.parametrize("ishift", range(16))
def test_every_image_shift(gpu_ctx, oracle, blocks, ishift):
    img, metas = blocks["rep"]
    frames = hand_frames(oracle, img, short_lens(img.size, granule()))
    r = receive(gpu_ctx, frames, metas, ishift=ishift)
    check_landed(r, img, frames)
    check_verdicts(oracle, r, img, metas)


# ---- 4. findings: each is one flipped byte -----------------------------------------------------

LONG = 9  # the grid block's record over whole granules 9 and 10


def frame_of(frames, pos):
    off = 0
    for k, f in enumerate(frames):
        if pos < off + f.size - 60:
            return k, 56 + pos - off
        off += f.size - 60
    raise AssertionError(pos)


@pytest.mark.parametrize("where", ["edge", "whole"])
def test_damage_after_sealing(gpu_ctx, oracle, blocks, where):
    img, metas = blocks["grid"]
    G = granule()
    assert int(metas[LONG]["size"]) == 2 * G + 736
    pos = int(metas[LONG]["offset"]) + 36 + 3 if where == "edge" else 9 * G + 1234
    frames, _ = sealed(gpu_ctx, img, metas, 1024)
    k, at = frame_of(frames, pos)
    frames[k][at] ^= 0x40
    r = receive(gpu_ctx, frames, metas)
    bad = img.copy()
    bad[pos] ^= 0x40
    assert (r.image[:img.size] == bad).all()
    est = [0] * len(frames)
    est[k] = CRC_ERR
    assert r.parts["status"].tolist() == est and r.nbad == 1
    rst = [0] * len(metas)
    rst[LONG] = CRC_ERR
    assert r.st.tolist() == rst and r.rbad == 1
    assert r.crc.tolist() == expected_verdicts(oracle, bad, metas, img.size)[0].tolist()


@pytest.mark.parametrize("where", ["edge", "whole"])
def test_rot_before_sealing(gpu_ctx, oracle, blocks, where):
    """The case the session exists for: a record that rotted on the source travels under valid
    frame CRCs, and only its own verdict names it."""
    img, metas = blocks["grid"]
    G = granule()
    pos = int(metas[LONG]["offset"]) + int(metas[LONG]["size"]) - 2 if where == "edge" else 10 * G + 77
    bad = img.copy()
    bad[pos] ^= 0x01
    frames, _ = sealed(gpu_ctx, bad, metas, 4096)
    r = receive(gpu_ctx, frames, metas)
    check_landed(r, bad, frames)
    rst = [0] * len(metas)
    rst[LONG] = CRC_ERR
    assert r.st.tolist() == rst and r.rbad == 1
    check_verdicts(oracle, r, bad, metas)


def test_damage_in_a_gap(gpu_ctx, oracle, blocks):
    img, metas = blocks["grid"]
    pos = 200                                  # between record 0 and the record at G - 36
    assert int(metas[0]["offset"]) + int(metas[0]["size"]) <= pos < int(metas[1]["offset"])
    frames, _ = sealed(gpu_ctx, img, metas, 1024)
    k, at = frame_of(frames, pos)
    frames[k][at] ^= 0x80
    r = receive(gpu_ctx, frames, metas)
    est = [0] * len(frames)
    est[k] = CRC_ERR
    assert r.parts["status"].tolist() == est and r.nbad == 1
    assert not r.st.any() and r.rbad == 0


@pytest.mark.parametrize("at,want", [(24, ERR), (36, ERR), (40, ERR), (8, ERR), (4, ERR), (0, ERR), (-1, CRC_ERR),
                                     (20, CRC_ERR)])
def test_frame_field_findings(gpu_ctx, oracle, blocks, at, want):
    """block_id_, offset_, length_, the pcode, the body length and the flag: TFS_ERROR; F and the
    header's crc field: TFS_EXIT_CHECK_CRC_ERROR.  Frame 1 of three; the others stay clean and
    every frame still lands in its declared range."""
    import tfs_amd.crc as crc
    img, metas = blocks["rep"]
    frames = hand_frames(oracle, img, [5000, 6000, img.size - 11000])
    base, descs = lay_out(frames)
    frames[1][at] ^= 0x04
    r = receive(gpu_ctx, frames, metas, descs_edit=lambda d: d.__setitem__(slice(None), descs))
    assert r.parts["status"].tolist() == [0, want, 0] and r.nbad == 1
    assert (r.image[:img.size] == img).all() and r.total == img.size
    if want == CRC_ERR:
        assert int(r.parts["crc"][1]) == zcrc(FLAG, frames[1][24:].tobytes())
    check_verdicts(oracle, r, img, metas)


def test_version_0_is_not_checked(gpu_ctx, oracle, blocks):
    img, metas = blocks["rep"]
    frames = hand_frames(oracle, img, [5000, img.size - 5000], version=0)
    frames[1][100] ^= 0xFF
    r = receive(gpu_ctx, frames, metas)
    assert r.parts["status"].tolist() == [0, 0] and r.parts["crc"].tolist() == [0, 0] and r.nbad == 0


def test_wrong_block_id(gpu_ctx, oracle, blocks):
    img, metas = blocks["rep"]
    frames = hand_frames(oracle, img, [img.size])
    r = receive(gpu_ctx, frames, metas, block_id=BLOCK + 1)
    assert r.parts["status"].tolist() == [ERR] and r.nbad == 1


def test_record_statuses_in_order(gpu_ctx, oracle, blocks):
    """FileInfo id_, size_ and crc_ damaged before sealing, metas out of range and size <= 36."""
    import tfs_amd.crc as crc
    img, metas = blocks["grid"]
    bad = img.copy()
    o = [int(m["offset"]) for m in metas]
    bad[o[3]] ^= 1                  # id_
    bad[o[4] + 12] ^= 1             # size_
    bad[o[5] + 32] ^= 1             # crc_
    bad[o[6]] ^= 1                  # id_ and size_: the id is checked first
    bad[o[6] + 12] ^= 1
    extra = np.array([(1, -4, 100), (2, img.size - 50, 51), (3, 10, 36), (4, 10, 0), (5, 2**31 - 10, 100)], crc.META_DTYPE)
    m2 = np.concatenate([metas, extra])
    frames, _ = sealed(gpu_ctx, bad, metas, 4096)
    r = receive(gpu_ctx, frames, m2)
    check_landed(r, bad, frames)
    assert r.st[3:7].tolist() == [INFO_ERR, SYNC_ERR, CRC_ERR, INFO_ERR]
    assert r.st[len(metas):].tolist() == [PARAM, PARAM, SIZE_ERR, SIZE_ERR, PARAM]
    assert not r.crc[len(metas):].any()
    check_verdicts(oracle, r, bad, m2)


# ---- 5. metas in any order -----------------------------------------------------------------------

def test_metas_any_order(gpu_ctx, oracle, blocks):
    import tfs_amd.crc as crc
    img, metas = blocks["grid"]
    frames = hand_frames(oracle, img, [img.size])
    rng = np.random.default_rng(5)
    overlap = np.array([(int(metas[LONG]["file_id"]), int(metas[LONG]["offset"]), int(metas[LONG]["size"])),
                        (7, int(metas[LONG]["offset"]) + 100, 5000)], crc.META_DTYPE)  # the second lies inside the first
    for m in (metas[::-1].copy(), metas[rng.permutation(len(metas))], np.concatenate([metas, metas[2:3]]),
              np.concatenate([metas[:4], overlap])):
        r = receive(gpu_ctx, frames, m)
        check_verdicts(oracle, r, img, m)
    assert r.st[-1] == INFO_ERR and r.st[-2] == 0


# ---- 6. finish reads edges only ------------------------------------------------------------------

def test_finish_reads_edges_only(gpu_ctx, oracle, blocks):
    import tfs_amd.crc as crc
    img, metas = blocks["grid"]
    G = granule()
    frames = hand_frames(oracle, img, [img.size])
    good = expected_verdicts(oracle, img, metas, img.size)

    def wipe_whole(d_img, ishift):      # all of granule 10, inside the long record
        d_img.upload(np.full(G, 0xA5, np.uint8), offset=ishift + 10 * G)

    r = receive(gpu_ctx, frames, metas, before_finish=wipe_whole)
    assert r.st.tolist() == good[1].tolist() and r.crc.tolist() == good[0].tolist() and not r.st.any()

    def flip_edge(d_img, ishift):       # one byte of the long record's tail edge
        d_img.upload(img[11 * G + 5:11 * G + 6] ^ 0xFF, offset=ishift + 11 * G + 5)

    r = receive(gpu_ctx, frames, metas, before_finish=flip_edge)
    assert r.st[LONG] == CRC_ERR and r.rbad == 1


# ---- 7. a record longer than 64 granules ---------------------------------------------------------

def test_long_record(gpu_ctx, oracle):
    G = granule()
    img, metas = build_block(oracle, [("gap", 77), ("rec", 70 * G + 123), ("gap", 9)], seed=9)
    frames, rep_res = sealed(gpu_ctx, img, metas, 65536)
    r = receive(gpu_ctx, frames, metas, groups_of(len(frames), (2, 1)))
    check_landed(r, img, frames)
    check_verdicts(oracle, r, img, metas)
    assert not r.st.any() and r.crc.tolist() == rep_res[0].tolist()
    bad = img.copy()
    bad[77 + 36 + 33 * G] ^= 2
    r = receive(gpu_ctx, hand_frames(oracle, bad, [img.size]), metas)
    assert r.st.tolist() == [CRC_ERR]
    check_verdicts(oracle, r, bad, metas)


# ---- 8. the empty block ----------------------------------------------------------------------------

def test_empty_block(gpu_ctx, oracle):
    import tfs_amd.crc as crc
    empty = np.zeros(0, np.uint8)
    frames = hand_frames(oracle, empty, [0], new_block=2)
    r = receive(gpu_ctx, frames, None, cap=0)
    assert r.total == 0 and r.parts["status"].tolist() == [0] and r.parts["flag"].tolist() == [2]
    assert r.parts["crc"][0] == struct.unpack_from("<I", frames[0], 20)[0]
    assert (r.image == r.before).all() and len(r.crc) == 0 and r.rbad == 0
    # image_cap 0 with a NULL image
    base, descs = lay_out(frames)
    d_base = crc.DeviceBuffer(gpu_ctx, base.size).upload(base)
    d_parts = crc.DeviceBuffer(gpu_ctx, 16)
    with crc.ReceiveSession(gpu_ctx, crc.receive_cfg(0, BLOCK), None) as s:
        s.frames_device(d_base, descs, d_parts)
        c, st, nbad, total = s.finish(np.array([(1, 0, 40)], crc.META_DTYPE))
    assert total == 0 and st.tolist() == [PARAM] and c.tolist() == [0] and nbad == 1
    assert d_parts.download(crc.RECEIVE_PART_DTYPE)["status"].tolist() == [0]
    d_base.free(), d_parts.free()


# ---- 9. refused calls change nothing ---------------------------------------------------------------

def test_refused_calls_change_nothing(gpu_ctx, oracle, blocks):
    import tfs_amd.crc as crc
    img, metas = blocks["rep"]
    frames = hand_frames(oracle, img, [4000, 5000, img.size - 9000])
    base, descs = lay_out(frames)
    cap = img.size + 10
    before = prefill(cap + 64)
    d_base = crc.DeviceBuffer(gpu_ctx, base.size).upload(base)
    d_img = crc.DeviceBuffer(gpu_ctx, cap + 64).upload(before)
    pre_parts = np.full(3 * 16, 0x5A, np.uint8)
    d_parts = crc.DeviceBuffer(gpu_ctx, 3 * 16).upload(pre_parts)
    d_bad = crc.DeviceBuffer(gpu_ctx, 4).upload(np.array([7], np.uint32))

    def refused(s, d, **kw):
        with pytest.raises(crc.TfsCrcError) as e:
            s.frames_device(d_base, d, d_parts, d_bad, **kw)
        assert e.value.code == PARAM
        gpu_ctx.sync()
        assert (d_img.download() == before).all() and (d_parts.download() == pre_parts).all()
        assert d_bad.download(np.uint32)[0] == 7

    def edited(j, field, value):
        d = descs.copy()
        d[field][j] = value
        return d

    with crc.ReceiveSession(gpu_ctx, crc.receive_cfg(cap, BLOCK), d_img) as s:
        refused(s, descs[1:])                                  # out of order: not at the cursor
        refused(s, descs[[0, 2]])                              # a hole inside the call
        refused(s, descs[[0, 0]])                              # overlap with the cursor
        refused(s, edited(1, "data_len", -1))
        refused(s, edited(2, "avail", int(descs["avail"][2]) - 1))   # avail short
        refused(s, descs, stream=2)                            # hipStreamPerThread
    with crc.ReceiveSession(gpu_ctx, crc.receive_cfg(8999, BLOCK), d_img) as s:
        refused(s, descs[:2])                                  # past image_cap
        s.frames_device(d_base, descs[:1], d_parts, d_bad)
        c, st, nbad, total = s.finish()
        assert total == 4000
        with pytest.raises(crc.TfsCrcError):
            s.finish()
        with pytest.raises(crc.TfsCrcError):
            s.frames_device(d_base, descs[1:2], d_parts, d_bad)
    d_img.upload(before)
    d_parts.upload(pre_parts)
    d_bad.upload(np.array([7], np.uint32))
    st2 = gpu_ctx.stream_create()
    with crc.ReceiveSession(gpu_ctx, crc.receive_cfg(cap, BLOCK), d_img) as s:
        s.frames_device(d_base, descs[:1], d_parts, d_bad, stream=st2)
        gpu_ctx.stream_sync(st2)
        now_img, now_parts = d_img.download(), d_parts.download()
        with pytest.raises(crc.TfsCrcError) as e:             # a second stream
            s.frames_device(d_base, descs[1:], d_parts.ptr + 16, d_bad)
        assert e.value.code == PARAM
        gpu_ctx.sync()
        assert (d_img.download() == now_img).all() and (d_parts.download() == now_parts).all()
        s.frames_device(d_base, descs[1:], d_parts.ptr + 16, d_bad, stream=st2)   # a correct call still works
        c, st, nbad, total = s.finish(metas)
    gpu_ctx.stream_destroy(st2)
    assert total == img.size and (d_img.download()[:img.size] == img).all()
    assert d_parts.download(crc.RECEIVE_PART_DTYPE)["status"].tolist() == [0, 0, 0] and d_bad.download(np.uint32)[0] == 7
    est = expected_verdicts(oracle, img, metas, img.size)
    assert st.tolist() == est[1].tolist() and c.tolist() == est[0].tolist()
    for d in (d_base, d_img, d_parts, d_bad):
        d.free()


# ---- 10. begin's checks in order ---------------------------------------------------------------------

def test_begin_checks_in_order(gpu_ctx):
    import tfs_amd.crc as crc
    L, h = gpu_ctx.L, ctypes.c_void_p()
    d = crc.DeviceBuffer(gpu_ctx, 4096)

    def begin(cfg, image):
        return L.tfs_receive_begin(gpu_ctx.handle, cfg.ctypes.data if cfg is not None else None, image, ctypes.byref(h))

    assert begin(None, d.ptr) == PARAM
    assert L.tfs_receive_begin(gpu_ctx.handle, crc.receive_cfg(10).ctypes.data, d.ptr, None) == PARAM
    assert begin(crc.receive_cfg(-1, reserved=(1, 0)), None) == SIZE_INVALID      # the size comes first
    assert begin(crc.receive_cfg(10, reserved=(0, 1)), d.ptr) == PARAM
    assert begin(crc.receive_cfg(10, reserved=(1, 0)), d.ptr) == PARAM
    assert begin(crc.receive_cfg(10), None) == PARAM and h.value is None
    assert begin(crc.receive_cfg(0), None) == 0 and h.value
    assert L.tfs_receive_free(h) == 0
    d.free()


# ---- 11. host forms equal the device form ------------------------------------------------------------

@pytest.mark.parametrize("pin_base,pin_image,piece", [(True, False, 0), (False, False, 0), (False, True, 0),
                                                      (True, True, 0), (False, False, 3000)])
def test_host_forms(gpu_ctx, oracle, blocks, pin_base, pin_image, piece):
    import tfs_amd.crc as crc
    img, metas = blocks["grid"]
    frames = hand_frames(oracle, img, off_grid_lens(img.size, granule()))
    frames[3][56 + 10] ^= 1                                  # one finding, so n_bad and the parts say something
    dev = receive(gpu_ctx, frames, metas)
    base, descs = lay_out(frames)
    cap = img.size + 100
    before = prefill(cap + 64)
    bufs = []
    hbase = base.copy()
    if pin_base:
        hbase = crc.PinnedBuffer(gpu_ctx, base.size)
        hbase.array[:] = base
        bufs.append(hbase)
    if pin_image:
        pimg = crc.PinnedBuffer(gpu_ctx, cap + 64)
        pimg.array[:] = before
        bufs.append(pimg)
        image = gpu_ctx.host_device_ptr(pimg.ptr)
    else:
        d_img = crc.DeviceBuffer(gpu_ctx, cap + 64).upload(before)
        image = d_img.ptr
    gpu_ctx.read_set_piece(piece)
    try:
        with crc.ReceiveSession(gpu_ctx, crc.receive_cfg(cap, BLOCK), image) as s:
            parts = np.zeros(0, crc.RECEIVE_PART_DTYPE)
            nbad = 0
            for a, b in groups_of(len(frames), (4, 9)):
                p, nb = s.frames(hbase, descs[a:b])
                parts, nbad = np.concatenate([parts, p]), nbad + nb
            c, st, rbad, total = s.finish(metas)
    finally:
        gpu_ctx.read_set_piece(0)
    landed = pimg.array.copy() if pin_image else d_img.download()
    assert (landed == dev.image).all() and total == dev.total
    assert parts.tolist() == dev.parts.tolist() and nbad == dev.nbad == 1
    assert c.tolist() == dev.crc.tolist() and st.tolist() == dev.st.tolist() and rbad == dev.rbad
    assert ((hbase.array if pin_base else hbase) == base).all()
    for b in bufs:
        b.free()
    if not pin_image:
        d_img.free()
