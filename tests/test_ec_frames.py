"""Frame-emitting chunk calls of the marshalling session (include/tfs_ec_frames.h,
DESIGN.md §3.23): one call encodes the chunk, verifies the records and leaves every
parity member's WriteRawDataMessage frames sealed in a buffer of its own.

Expected frames come from the oracles (tests/ec_frames_expect.py: jerasure's parity,
oracle_crc over each frame's body); the plain marshalling session over the same members
and tfs_packet_verify are second witnesses.  Every out buffer is prefilled and compared
whole, with 64 bytes before the first frame and behind the call's capacity, so a byte
written outside the call's frames fails the comparison."""
import numpy as np
import pytest

import ec_frames_expect as X
from test_marshal import Image, chunks_of, expected, family, padded, up
from test_marshal import run as plain_run
from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode)

pytestmark = pytest.mark.gpu

OK, CRC_ERR, PARAM = 0, -1010, -1016
DATA_INVALID, SIZE_INVALID = -16001, -16002
LEAD = 64
LENS = [70001, 98304, 65536 + 1024, 81920 - 7]


def bids(n):
    return [1000 + 7 * i for i in range(n)]


def pids(n):
    return [((i + 1) << 40) + 7 for i in range(n)]


class Outs:
    """One prefilled out buffer per parity member, LEAD bytes before the address the call gets."""

    def __init__(self, ctx, k, m, cap, form):
        import tfs_amd.crc as crc
        self.ctx, self.k, self.m, self.size, self.form = ctx, k, m, LEAD + cap + 64, form
        if form == "device":
            self.b = [crc.DeviceBuffer(ctx, self.size) for _ in range(m)]
        elif form == "pinned":
            self.b = [crc.PinnedBuffer(ctx, self.size) for _ in range(m)]
        else:
            self.b = [np.zeros(self.size, np.uint8) for _ in range(m)]

    def prefill(self):
        fill = np.full(self.size, X.PREFILL, np.uint8)
        for b in self.b:
            if self.form == "device":
                b.upload(fill)
            elif self.form == "pinned":
                b.array[:] = fill
            else:
                b[:] = fill

    def args(self, shift=0):
        at = [b.ctypes.data if self.form == "host" else b.ptr for b in self.b]
        return [None] * self.k + [a + LEAD + shift for a in at]

    def images(self):
        if self.form == "device":
            return [b.download(np.uint8, self.size) for b in self.b]
        return [np.array(b.array if self.form == "pinned" else b) for b in self.b]

    def free(self):
        if self.form != "host":
            for b in self.b:
                b.free()


def session(ctx, k, m, imgs, metas, total, frame_len, fpc, stride=0, version=2, form="device", stream=None, plain=()):
    """One whole session in calls of `fpc` frames; the chunks whose number is in `plain` go through the plain
    encode call.  Returns ([(offset, len, [image per parity member])], {chunk number: [parity]}, finish())."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, MarshalSession, frames_cfg
    ec = ErasureCode(ctx, k, m)
    ses = MarshalSession(ec, metas, [a.size for a in imgs], total)
    assert ec.rc == 0 and ses.rc == 0
    data = padded(imgs, total)
    cfg = frames_cfg(frame_len, bids(k + m), pids(k + m), stride, version)
    step = frame_len * fpc
    outs = Outs(ctx, k, m, X.need(frame_len, min(step, total), stride), form)
    dev = form == "device"
    d_src = [crc.DeviceBuffer(ctx, total).upload(a) for a in data] if dev else None
    d_par = [crc.DeviceBuffer(ctx, step) for _ in range(m)] if dev and plain else None
    sync = (lambda: ctx.stream_sync(stream)) if stream else ctx.sync
    calls, plains = [], {}
    for c, (o, n) in enumerate(chunks_of(total, step)):
        src = [b.ptr + o for b in d_src] if dev else [a[o:o + n] for a in data]
        if c in plain:
            if dev:
                assert ses.encode_device(src + d_par, o, n, stream=stream) == 0
                sync()
                plains[c] = [b.download(np.uint8, n) for b in d_par]
            else:
                par = [np.zeros(n, np.uint8) for _ in range(m)]
                assert ses.encode(src + par, o, n) == 0
                plains[c] = par
            continue
        outs.prefill()
        cap = X.need(frame_len, n, stride)
        if dev:
            assert ses.frames_device(cfg, src + [None] * m, outs.args(), cap, o, n, stream=stream) == 0
            sync()
        else:
            assert ses.frames(cfg, src + [None] * m, outs.args(), cap, o, n) == 0
        calls.append((o, n, outs.images()))
    res = ses.finish()
    ses.free()
    ec.free()
    outs.free()
    for b in (d_src or []) + (d_par or []):
        b.free()
    return calls, plains, res


def check_calls(calls, frames, frame_len, stride=0):
    """Every call's out buffers, whole: the expected frames at their places, the prefill everywhere else."""
    st = X.stride_of(frame_len, stride)
    for o, n, images in calls:
        nf = (n + frame_len - 1) // frame_len
        cap = X.need(frame_len, n, stride)
        for p, img in enumerate(images):
            exp = np.full(img.size, X.PREFILL, np.uint8)
            exp[LEAD:LEAD + cap] = X.call_image(frames[p], o // frame_len, nf, st, cap)
            bad = np.nonzero(img != exp)[0]
            assert bad.size == 0, (o, n, p, int(bad[0]) - LEAD, int(bad.size))


def data_areas(calls, m, frame_len, stride=0):
    st = X.stride_of(frame_len, stride)
    return [np.concatenate([X.data_of(images[p][LEAD:], frame_len, n, st) for _, n, images in calls]) for p in range(m)]


def verify_frames(ctx, calls, frame_len, stride=0):
    """tfs_packet_verify accepts every frame of every call."""
    st = X.stride_of(frame_len, stride)
    for _, n, images in calls:
        nf = (n + frame_len - 1) // frame_len
        offs = [LEAD + j * st for j in range(nf)]
        lens = [X.OVERHEAD + min(frame_len, n - j * frame_len) for j in range(nf)]
        for img in images:
            _, s, nbad, rc = ctx.packet_verify(img, offs, lens)
            assert rc == 0 and nbad == 0 and (s == 0).all()


@pytest.fixture(scope="module")
def fam53(oracle, ec_oracle):
    """The 5:3 family most cases share, with its oracle parity, CRCs and statuses."""
    imgs, metas = family(oracle, 5, 53, LENS)
    total = up(max(a.size for a in imgs), 1024)
    return imgs, metas, total, expected(oracle, ec_oracle, 5, 3, imgs, metas, total)


@pytest.mark.parametrize("k,m", [(2, 1), (5, 3), (8, 4), (6, 6)])
def test_coders(gpu_ctx, oracle, ec_oracle, k, m):
    """(6, 6) takes two output groups.  One frame and three frames per call, frame lengths 4096 and 16384."""
    imgs, metas = family(oracle, k, 10 * k + m, LENS)
    total = up(max(a.size for a in imgs), 1024)
    epar, ecrc, est = expected(oracle, ec_oracle, k, m, imgs, metas, total)
    ppar, pres = plain_run(gpu_ctx, k, m, imgs, metas, total, chunks_of(total, 16384), reuse=False)
    for frame_len in (4096, 16384):
        frames = [X.member_frames(oracle, epar[p], frame_len, bids(k + m)[k + p], pids(k + m)[k + p], True) for p in range(m)]
        for fpc in (1, 3):
            calls, _, (crc, st, nbad, rc) = session(gpu_ctx, k, m, imgs, metas, total, frame_len, fpc)
            check_calls(calls, frames, frame_len)
            for a, b in zip(data_areas(calls, m, frame_len), ppar):
                assert (a == b).all()
            assert rc == 0 and (crc == pres[0]).all() and (st == pres[1]).all() and nbad == pres[2]
            assert (crc == ecrc).all() and (st == est).all() and len(st) > 10 * k
            verify_frames(gpu_ctx, calls, frame_len)


@pytest.mark.parametrize("units", [1, 2, 3])
def test_short_last_frame(gpu_ctx, oracle, ec_oracle, units):
    """total = 4096 n + 1024 u: the last frame ends in a short tile; one call, and one frame per call."""
    total = 65536 + 1024 * units
    b = Image(oracle, 40 + units).fill(total - 12000)
    b.rec(total - b.pos - 36)  # a record up to the member's last byte, into the short tile
    img, mt = b.image()
    imgs, metas = family(oracle, 2, 50 + units, [total - 1024 * units - 3, 30000])
    imgs, metas = imgs + [img], metas + [mt]
    epar, ecrc, est = expected(oracle, ec_oracle, 3, 2, imgs, metas, total)
    for frame_len in (4096, 8192):
        frames = [X.member_frames(oracle, epar[p], frame_len, bids(5)[3 + p], pids(5)[3 + p], True) for p in range(2)]
        assert len(frames[0][-1]) == X.OVERHEAD + (total % frame_len)
        for fpc in (1, 5, 1 << 20):
            calls, _, (crc, st, nbad, rc) = session(gpu_ctx, 3, 2, imgs, metas, total, frame_len, fpc)
            check_calls(calls, frames, frame_len)
            assert rc == 0 and (crc == ecrc).all() and (st == est).all() and (st == 0).all()
            verify_frames(gpu_ctx, calls, frame_len)


@pytest.mark.parametrize("total,frame_len", [(3072, 4096), (1024, 8192), (8192, 8192), (4096, 4096)])
def test_one_frame_totals(gpu_ctx, oracle, ec_oracle, total, frame_len):
    """A total shorter than one frame, and total == frame_len."""
    b = Image(oracle, total)
    b.rec(500, at=17)
    img, mt = b.image(total - 5)
    imgs, metas = [img, img[:900].copy()], [mt, mt]
    epar, ecrc, est = expected(oracle, ec_oracle, 2, 2, imgs, metas, total)
    frames = [X.member_frames(oracle, epar[p], frame_len, bids(4)[2 + p], pids(4)[2 + p], True) for p in range(2)]
    assert len(frames[0]) == 1
    calls, _, (crc, st, nbad, rc) = session(gpu_ctx, 2, 2, imgs, metas, total, frame_len, 1)
    check_calls(calls, frames, frame_len)
    assert rc == 0 and (crc == ecrc).all() and (st == est).all()
    verify_frames(gpu_ctx, calls, frame_len)


def test_strides(gpu_ctx, oracle, fam53):
    """The explicit stride frame_len + 64 is the default; a wide stride leaves the gaps at their prefill."""
    imgs, metas, total, (epar, ecrc, est) = fam53
    frames = [X.member_frames(oracle, epar[p], 4096, bids(8)[5 + p], pids(8)[5 + p], True) for p in range(3)]
    ref, _, _ = session(gpu_ctx, 5, 3, imgs, metas, total, 4096, 4)
    check_calls(ref, frames, 4096)
    same, _, _ = session(gpu_ctx, 5, 3, imgs, metas, total, 4096, 4, stride=4096 + 64)
    for (_, _, a), (_, _, b) in zip(ref, same):
        assert all((x == y).all() for x, y in zip(a, b))
    for stride in (4096 + 72, 8192 + 8):
        wide, _, (crc, st, _, rc) = session(gpu_ctx, 5, 3, imgs, metas, total, 4096, 4, stride=stride)
        check_calls(wide, frames, 4096, stride)
        verify_frames(gpu_ctx, wide, 4096, stride)
        assert rc == 0 and (crc == ecrc).all() and (st == est).all()


def test_version0_no_records_and_mixed_chunks(gpu_ctx, oracle, fam53):
    imgs, metas, total, (epar, ecrc, est) = fam53
    # version 0: the CRC field is 0
    f0 = [X.member_frames(oracle, epar[p], 8192, bids(8)[5 + p], pids(8)[5 + p], True, version=0) for p in range(3)]
    calls, _, (crc, st, _, rc) = session(gpu_ctx, 5, 3, imgs, metas, total, 8192, 2, version=0)
    check_calls(calls, f0, 8192)
    assert all(f[20:24] == b"\0\0\0\0" for f in f0[0])
    assert rc == 0 and (crc == ecrc).all() and (st == est).all()
    # a session with no records still yields the frames
    f2 = [X.member_frames(oracle, epar[p], 8192, bids(8)[5 + p], pids(8)[5 + p], True) for p in range(3)]
    none = [np.zeros(0, metas[0].dtype)] * 5
    calls, _, (crc, st, nbad, rc) = session(gpu_ctx, 5, 3, imgs, none, total, 8192, 2)
    check_calls(calls, f2, 8192)
    assert rc == 0 and len(crc) == 0 and nbad == 0
    # plain encode chunks mixed into the session: the same frames, the same parity, the same verdicts
    calls, plains, (crc, st, nbad, rc) = session(gpu_ctx, 5, 3, imgs, metas, total, 8192, 2, plain={1, 4})
    check_calls(calls, f2, 8192)
    assert len(plains) == 2 and len(calls) == len(chunks_of(total, 16384)) - 2
    for c, par in plains.items():
        for p in range(3):
            assert (par[p] == epar[p][c * 16384:c * 16384 + par[p].size]).all()
    assert rc == 0 and (crc == ecrc).all() and (st == est).all() and nbad == 0


def test_refused_calls(gpu_ctx, oracle, fam53):
    """Every refused call returns its code, leaves out untouched and lets the session go on to a correct end."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode, MarshalSession, frames_cap, frames_cfg
    imgs, metas, total, (epar, ecrc, est) = fam53
    k, m = 5, 3
    ec = ErasureCode(gpu_ctx, k, m)
    ses = MarshalSession(ec, metas, [a.size for a in imgs], total)
    d_src = [crc.DeviceBuffer(gpu_ctx, total).upload(a) for a in padded(imgs, total)]
    outs = Outs(gpu_ctx, k, m, X.need(4096, total), "device")
    outs.prefill()
    good = frames_cfg(4096, bids(8), pids(8))
    assert frames_cap(good, 8192) == X.need(4096, 8192) and frames_cap(good, total) == X.need(4096, total)
    assert frames_cap(frames_cfg(1024), 8192) == 0 and frames_cap(frames_cfg(4096, frame_stride=4096 + 8), 8192) == 0
    s1, s2 = gpu_ctx.stream_create(), gpu_ctx.stream_create()

    def call(cfg=good, src=None, out="default", cap=None, o=0, n=8192, stream=s1, shift=0):
        src = [b.ptr + o for b in d_src] + [None] * m if src is None else src
        out = outs.args(shift) if out == "default" else out
        cap = X.need(4096, n) if cap is None else cap
        return ses.frames_device(cfg, src, out, cap, o, n, stream=stream)

    def refusals(o):
        n = 8192
        src = [b.ptr + o for b in d_src] + [None] * m
        assert call(o=o, stream=2) == PARAM                                  # hipStreamPerThread
        assert call(o=o + 4096) == PARAM                                     # not the next chunk
        assert call(o=o, n=5120) == PARAM                                    # len % 4096 before the end
        assert call(cfg=None, o=o) == PARAM
        assert call(out=None, o=o) == PARAM
        for fl in (0, -4096, 1024, 6144):
            assert call(cfg=frames_cfg(fl, bids(8), pids(8)), o=o) == SIZE_INVALID
        assert call(cfg=frames_cfg(1024, bids(8), pids(8), reserved=1), o=o) == SIZE_INVALID   # 3 before 4
        for st in (4096 + 56, 4096 + 60, 4096 + 68, 8):
            assert call(cfg=frames_cfg(4096, bids(8), pids(8), frame_stride=st), o=o, cap=1 << 20) == PARAM
        assert call(cfg=frames_cfg(4096, bids(8), pids(8), reserved=1), o=o) == PARAM
        assert call(cfg=frames_cfg(16384, bids(8), pids(8)), o=o, n=8192, cap=1 << 20) == PARAM   # len % frame_len
        for shift in (1, 4):
            assert call(o=o, shift=shift) == PARAM                           # out[i] % 8
        assert call(o=o, cap=X.need(4096, n) - 1) == PARAM
        assert call(o=o, cap=0) == PARAM
        assert call(src=[None] * (k + m), o=o, cap=0) == PARAM               # 4 before 5
        assert ses.frames_device(good, None, outs.args(), X.need(4096, n), o, n, stream=s1) == DATA_INVALID
        assert call(src=src[:2] + [None] + src[3:], o=o) == DATA_INVALID     # a NULL source member
        assert call(out=outs.args()[:-1] + [None], o=o) == DATA_INVALID      # a NULL out of an output member
        gpu_ctx.stream_sync(s1)
        for img in outs.images():
            assert (img == X.PREFILL).all()

    try:
        refusals(0)
        assert call(cfg=frames_cfg(8192, bids(8), pids(8)), o=0, n=8192, cap=1 << 20) == 0
        assert call(o=0) == PARAM                                            # repeated
        assert call(o=8192, stream=s2) == PARAM                              # a second stream
        assert call(cfg=frames_cfg(8192, bids(8), pids(8)), o=8192, n=4096, cap=1 << 20) == PARAM  # the frame rule:
        assert call(o=8192, n=4096) == 0                                     # ... len % frame_len before the end
        assert call(cfg=frames_cfg(8192, bids(8), pids(8)), o=12288, n=8192, cap=1 << 20) == PARAM  # offset % frame_len
        assert call(o=12288, n=4096) == 0
        gpu_ctx.stream_sync(s1)
        outs.prefill()
        refusals(16384)
        frames = [X.member_frames(oracle, epar[p], 4096, bids(8)[5 + p], pids(8)[5 + p], True) for p in range(m)]
        n = total - 16384
        assert call(o=16384, n=n) == 0                                       # the rest in one call
        gpu_ctx.stream_sync(s1)
        check_calls([(16384, n, outs.images())], frames, 4096)
        c, st, nbad, rc = ses.finish()
        assert rc == 0 and (c == ecrc).all() and (st == est).all() and nbad == 0
    finally:
        ses.free()
        ec.free()
        gpu_ctx.stream_destroy(s1)
        gpu_ctx.stream_destroy(s2)
        outs.free()


def test_second_stream_of_the_callers(gpu_ctx, oracle, fam53):
    """A whole session on a stream of the caller's."""
    imgs, metas, total, (epar, ecrc, est) = fam53
    frames = [X.member_frames(oracle, epar[p], 16384, bids(8)[5 + p], pids(8)[5 + p], True) for p in range(3)]
    s = gpu_ctx.stream_create()
    try:
        calls, _, (crc, st, _, rc) = session(gpu_ctx, 5, 3, imgs, metas, total, 16384, 2, stream=s)
    finally:
        gpu_ctx.stream_destroy(s)
    check_calls(calls, frames, 16384)
    assert rc == 0 and (crc == ecrc).all() and (st == est).all()


def test_corrupt_source(gpu_ctx, oracle, ec_oracle, fam53):
    """A data record corrupted before the pass is reported; the frames are the sealed code of the bytes as read,
    as the two-pass form (encode, then seal) gives them."""
    imgs, metas, total, _ = fam53
    bad = [a.copy() for a in imgs]
    x = metas[2][3]
    bad[2][int(x["offset"]) + 36 + 11] ^= 0x40
    epar, ecrc, est = expected(oracle, ec_oracle, 5, 3, bad, metas, total)
    at = len(metas[0]) + len(metas[1]) + 3
    assert est[at] == CRC_ERR and int((est != 0).sum()) == 1
    frames = [X.member_frames(oracle, epar[p], 4096, bids(8)[5 + p], pids(8)[5 + p], True) for p in range(3)]
    calls, _, (crc, st, nbad, rc) = session(gpu_ctx, 5, 3, bad, metas, total, 4096, 3)
    check_calls(calls, frames, 4096)
    verify_frames(gpu_ctx, calls, 4096)
    assert rc == 0 and nbad == 1 and (st == est).all() and (crc == ecrc).all()
    # the two-pass form: the plain session's parity through record-less replicate sessions
    import tfs_amd.crc as C
    ppar, _ = plain_run(gpu_ctx, 5, 3, bad, metas, total, chunks_of(total, 16384), reuse=False)
    for p in range(3):
        cfg = C.replicate_cfg(total, 4096, bids(8)[5 + p], pids(8)[5 + p], C.RAW_PARITY_DATA, 2, frame_stride=4096 + 64)
        out = np.full(X.need(4096, total), X.PREFILL, np.uint8)
        with C.ReplicateSession(gpu_ctx, cfg) as r:
            r.frames(ppar[p], 0, total, out)
            r.finish()
        got = np.concatenate([images[p][LEAD:LEAD + X.need(4096, n)] for _, n, images in calls])
        two = np.concatenate([out[(o // 4096) * 4160:(o // 4096) * 4160 + X.need(4096, n)] for o, n, _ in calls])
        assert (got == two).all()


@pytest.mark.parametrize("form", ["host", "pinned"])
def test_host_forms(gpu_ctx, oracle, fam53, form):
    """Pageable and page-locked host forms equal the device form, wide stride included."""
    imgs, metas, total, (epar, ecrc, est) = fam53
    frames = [X.member_frames(oracle, epar[p], 4096, bids(8)[5 + p], pids(8)[5 + p], True) for p in range(3)]
    for stride in (0, 4096 + 128):
        dev, _, dres = session(gpu_ctx, 5, 3, imgs, metas, total, 4096, 5, stride=stride)
        calls, _, (crc, st, nbad, rc) = session(gpu_ctx, 5, 3, imgs, metas, total, 4096, 5, stride=stride, form=form)
        check_calls(calls, frames, 4096, stride)
        for (_, _, a), (_, _, b) in zip(dev, calls):
            assert all((x == y).all() for x, y in zip(a, b))
        assert rc == 0 and (crc == dres[0]).all() and (st == dres[1]).all() and (crc == ecrc).all()
