"""tfs_read_reply_device and tfs_mirror_frames_device on the caller's streams.  The two calls share a design:
each takes the next of four plan slots, the kernel's scratch lies behind the plan in that slot, the call records
an event on the slot and the slot's next user waits for it.  Here the calls run on the context's stream, on a
stream the context made and on one the runtime made; nine are queued on one stream without a wait in between,
each on its own slice of the jobs, its own region of out, its own results and n_bad word; ten alternate between
two streams; and after every call's return the host arrays it was given are overwritten, as both headers allow.
hipStreamPerThread is refused and nothing is touched.

A slot's memory is allocated in multiples of 64 KiB, so the batches of at most 32 jobs used here never make a
slot grow: a read reply's slot holds 64 bytes a job (growth needs more than 1,024 jobs in one call, which
tests/test_read_reply.py::test_tickets_5000_short_jobs has, though with nothing else in flight), and geometry A
or the failure batch needs about 16 KiB.  test_mirror_slot_grows_while_calls_are_in_flight is the one test that
reaches "wait for the slot's event, free, allocate anew" with other calls queued: files of 500,000 and 1,500,000
bytes under 1 KiB frames need plans of more than 64 KiB and more than 256 KiB.

The images and jobs come from tests/test_read_reply.py and tests/test_mirror.py, whose check functions judge
every call: frames bit-exact against frames built in Python, every result word, every byte outside the spans."""
import ctypes

import numpy as np
import pytest

import test_mirror as M
import test_read_reply as RR
from test_scalar_and_streams import _hip

pytestmark = pytest.mark.gpu

PARAM = -1016
COUNTS = [1, 2, 4, 8, 16, 32, 3, 1, 32]      # nine calls over four slots: every slot is reused, the first twice
PER_THREAD = 2                               # the handle value of hipStreamPerThread


@pytest.fixture(scope="module")
def ctx():
    """A context of this module's own: no other test's calls are queued on its slots."""
    import tfs_amd.crc as crc
    c = crc.Context(0)
    yield c
    c.close()


class Streams:
    """None (the context's stream), one the context made, one hipStreamCreate made."""

    def __init__(self, ctx):
        self.ctx, self.hip = ctx, _hip()
        self.owned = ctx.stream_create()
        s = ctypes.c_void_p()
        assert self.hip.hipStreamCreate(ctypes.byref(s)) == 0
        self.foreign = s.value

    def sync(self, s):
        if s is None:
            self.ctx.sync()
        elif s == self.owned:
            self.ctx.stream_sync(s)
        else:
            assert self.hip.hipStreamSynchronize(s) == 0

    def close(self):
        self.ctx.stream_destroy(self.owned)
        assert self.hip.hipStreamDestroy(self.foreign) == 0


@pytest.fixture
def streams(ctx):
    s = Streams(ctx)
    try:
        yield s
    finally:
        ctx.sync()
        s.close()


def scribble(*arrays):
    for a in arrays:
        a.view(np.uint8).reshape(-1)[:] = 0xFF


# ---- the two paths behind one shape: batches(), launch(), judge() ---------------------------------------------

class ReadPath:
    """32 records of mixed lengths; six of them fail, each in its own way."""
    result_dtype = "READ_RESULT_DTYPE"

    def __init__(self, ctx, oracle):
        import tfs_amd.crc as crc
        self.ctx, self.oracle = ctx, oracle
        sizes = [3000, 100, 0, 2000, 40, 5000, 900, 64, 1500, 700, 3100, 800, 1, 2100, 333, 50] * 2
        sizes[21] = 70001
        self.img, recs = RR.build_image(oracle, sizes, seed=31, tail=200)
        self.img[recs[4][1] + 36 + 7] ^= 0x10                       # payload: CRC_ERR
        self.img[recs[13][1] + 12] ^= 1                             # FileInfo.size_: SYNC_ERR
        self.img[recs[21][1] + 36 + 60000] ^= 0x01                  # deep in the long payload: CRC_ERR
        recs[9] = (77, recs[9][1], recs[9][2])                      # another id: INFO_ERR
        recs[17] = (recs[17][0], recs[17][1], 35)                   # SIZE_ERR
        recs[26] = (recs[26][0], self.img.size - 10, recs[26][2])   # past src_len: PARAM
        self.recs, self.bad = recs, {4, 9, 13, 17, 21, 26}
        self.d_src = crc.DeviceBuffer(ctx, self.img.size + 16).upload(self.img)

    def batches(self, counts):
        """[(host arrays of the call, region bytes)]: call k takes count records from a start of its own."""
        out, start = [], 0
        for k, n in enumerate(counts):
            idx = [(start + i) % 32 for i in range(n)]
            jobs, cap = RR.packed([self.recs[i] for i in idx], start=k % 16, pcode=[RR.PCODES[(i + k) % 3] for i in idx])
            out.append(((jobs,), cap, len(self.bad & set(idx))))
            start += n + 3
        return out

    def launch(self, arrays, d_out, cap, d_res, d_bad, stream):
        self.ctx.read_reply_device(self.d_src, self.img.size, arrays[0], d_out, cap, d_res, d_bad, stream=stream)

    def judge(self, arrays, out, before, res, nbad):
        assert RR.check(self.oracle, self.img, arrays[0], out, res, out.size, before) == nbad

    @staticmethod
    def written(arrays, res):
        """The (first, end) bytes of out that hold a frame, error frames included."""
        return [(int(j["frame_offset"]), int(j["frame_offset"]) + int(r["frame_len"])) for j, r in zip(arrays[0], res)]

    def free(self):
        self.d_src.free()


class MirrorPath:
    """test_mirror's geometry A (32 good files) and its failure batch (15 jobs, 9 of them fail)."""
    result_dtype = "MIRROR_RESULT_DTYPE"

    def __init__(self, ctx, oracle):
        import tfs_amd.crc as crc
        self.ctx, self.oracle = ctx, oracle
        self.good = M.geometry_a(oracle, 2)
        self.fail = M.failure_batch(oracle)
        self.d_src = {id(g[1]): crc.DeviceBuffer(ctx, g[1].size + 256).upload(g[1]) for g in (self.good, self.fail)}

    def batches(self, counts):
        """Counts of 3, 4 and 8 are cut from the failure batch, the others from geometry A; the second batch of
        32 is in reverse order (spans out of job order take the overlap check's other branch)."""
        gcfg, gimg, gjobs, gds, gcap = self.good
        fcfg, fimg, fjobs, fds, fcap, want = self.fail
        out, start, seen32 = [], 0, False
        for n in counts:
            if n in (3, 4, 8):
                a = {8: 0, 4: 8, 3: 12}[n]
                jobs, src = fjobs[a:a + n].copy(), (fcfg.copy(), fimg, fds.copy(), fcap)
                nbad = sum(1 for w in want[a:a + n] if w)
            else:
                a = start % (33 - n)
                jobs, src, nbad = gjobs[a:a + n].copy(), (gcfg.copy(), gimg, gds.copy(), gcap), 0
                if n == 32 and seen32:
                    jobs = jobs[::-1].copy()
                seen32 = seen32 or n == 32
                start += 5
            cfg, img, ds, cap = src
            out.append(((jobs, cfg, ds, img), cap, nbad))
        return out

    def launch(self, arrays, d_out, cap, d_res, d_bad, stream):
        jobs, cfg, ds, img = arrays
        self.ctx.mirror_frames_device(cfg, self.d_src[id(img)], img.size, jobs, ds, d_out, cap, d_res, d_bad, stream=stream)

    def judge(self, arrays, out, before, res, nbad):
        jobs, cfg, ds, img = arrays
        M.check_call(self.oracle, img, cfg, jobs, ds, out, before, res, nbad)

    @staticmethod
    def written(arrays, res):
        """The (first, end) bytes of out that hold the frames of a file that passed."""
        return [(int(j["frame_offset"]), int(j["frame_offset"]) + int(r["span_len"])) for j, r in zip(arrays[0], res)]

    def free(self):
        for d in self.d_src.values():
            d.free()


@pytest.fixture(scope="module", params=["read", "mirror"])
def path(request, ctx, oracle):
    p = (ReadPath if request.param == "read" else MirrorPath)(ctx, oracle)
    yield p
    ctx.sync()
    p.free()


class Calls:
    """The device side of a list of batches: one out buffer with a region per call, results and n_bad words of
    each call's own.  queue(k, stream) launches call k from copies of its host arrays and overwrites the copies
    on return; judge() downloads everything and checks every call against the untouched originals."""

    def __init__(self, ctx, path, batches):
        import tfs_amd.crc as crc
        self.ctx, self.path, self.batches = ctx, path, batches
        self.off, fills, at = [], [], 0
        for _, cap, _ in batches:
            self.off.append(at)
            fills.append(RR.prefill((cap + 64 + 255) // 256 * 256))      # every region starts the pattern anew
            at += fills[-1].size
        self.before = np.concatenate(fills)
        self.d_out = crc.DeviceBuffer(ctx, at + 16).upload(self.before)
        self.d_res = [crc.DeviceBuffer(ctx, 16 * len(b[0][0])) for b in batches]
        self.d_bad = crc.DeviceBuffer(ctx, 4 * len(batches)).upload(np.full(len(batches), 3, np.uint32))
        for d in self.d_res:
            d.upload(np.full(d.nbytes // 4, 0x5A5A5A5A, np.uint32))

    def queue(self, k, stream):
        arrays, cap, _ = self.batches[k]
        mine = tuple(a.copy() if i < 3 else a for i, a in enumerate(arrays))     # (the image is not an argument)
        self.path.launch(mine, self.d_out.ptr + self.off[k], cap, self.d_res[k], self.d_bad.ptr + 4 * k, stream)
        scribble(*mine[:3])                                                      # "may be reused on return"

    def fetch(self):
        import tfs_amd.crc as crc
        out = self.d_out.download(np.uint8, self.before.size)
        res = [d.download(getattr(crc, self.path.result_dtype), len(b[0][0])) for d, b in zip(self.d_res, self.batches)]
        return out, res, self.d_bad.download(np.uint32, len(self.batches)).astype(np.int64) - 3

    def judge(self, only=None):
        out, res, nbad = self.fetch()
        touched = np.zeros(out.size, bool)
        for k, (arrays, cap, want_bad) in enumerate(self.batches):
            if only is not None and k not in only:
                assert (np.frombuffer(res[k].tobytes(), np.uint32) == 0x5A5A5A5A).all() and nbad[k] == 0, k
                continue
            o = self.off[k]
            touched[o:o + cap] = True
            self.path.judge(arrays, out[o:o + cap], self.before[o:o + cap], res[k], int(nbad[k]))
            assert int(nbad[k]) == want_bad, (k, int(nbad[k]), want_bad)
        assert (out[~touched] == self.before[~touched]).all(), "a byte outside every call's region was written"
        return out, res, nbad

    def free(self):
        for d in [self.d_out, self.d_bad] + self.d_res:
            d.free()


@pytest.fixture
def calls(ctx):
    made = []

    def make(path, batches):
        made.append(Calls(ctx, path, batches))
        return made[-1]
    try:
        yield make
    finally:
        ctx.sync()
        for c in made:
            c.free()


# ---- the tests ----------------------------------------------------------------------------------------------------

def test_callers_streams_give_identical_results(ctx, path, streams, calls):
    """The same call (32 jobs, then the batch with the failures) on the context's stream, an owned stream and a
    foreign stream: each exact on its own, and the three identical."""
    for pick in (5, 3):                                  # COUNTS[5] == 32, COUNTS[3] == 8
        batch = path.batches(COUNTS)[pick]
        assert len(batch[0][0]) == COUNTS[pick] and (pick == 5 or batch[2] > 0)
        c = calls(path, [batch] * 3)
        for k, s in enumerate((None, streams.owned, streams.foreign)):
            c.queue(k, s)
            streams.sync(s)
        out, res, nbad = c.judge()
        cap = batch[1]
        spans = path.written(batch[0], res[0])
        assert sum(1 for a, b in spans if b > a) >= len(spans) - batch[2] > 0
        for k in (1, 2):
            assert res[k].tobytes() == res[0].tobytes() and nbad[k] == nbad[0], k
            mine, first = out[c.off[k]:c.off[k] + cap], out[c.off[0]:c.off[0] + cap]
            for a, b in spans:       # every frame that was written; a failed file's span is unspecified but for
                assert (mine[a:b] == first[a:b]).all(), (k, a, b)       # what judge() compared
            if batch[2] == 0:
                assert (mine == first).all(), k


@pytest.mark.parametrize("which", ["context", "owned", "foreign"])
def test_nine_calls_queued_without_a_wait(ctx, path, streams, calls, which):
    """More calls in flight than the ring has slots, on one stream: a slot's next user waits for its event before
    it overwrites the plan and the scratch behind it."""
    s = {"context": None, "owned": streams.owned, "foreign": streams.foreign}[which]
    batches = path.batches(COUNTS)
    assert [len(b[0][0]) for b in batches] == COUNTS and sum(b[2] for b in batches) > 0
    c = calls(path, batches)
    for k in range(len(batches)):
        c.queue(k, s)
    streams.sync(s)
    c.judge()


def test_two_streams_interleaved(ctx, path, streams, calls):
    """Five calls each on an owned and on a foreign stream, alternating, no wait until the end: a slot recorded on
    one stream is waited for by a call on the other."""
    batches = path.batches([32, 1, 8, 16, 3, 32, 4, 2, 16, 8])
    c = calls(path, batches)
    for k in range(len(batches)):
        c.queue(k, streams.owned if k % 2 == 0 else streams.foreign)
    streams.sync(streams.owned)
    streams.sync(streams.foreign)
    c.judge()


def test_stream_per_thread_is_refused(ctx, path, calls):
    """TFS_EXIT_PARAMETER_ERROR, nothing launched: out, results and n_bad keep what they held, and the next
    ordinary call on the context is exact."""
    import tfs_amd.crc as crc
    batches = path.batches([8, 8])
    c = calls(path, batches)
    with pytest.raises(crc.TfsCrcError) as e:
        c.queue(0, PER_THREAD)
    assert e.value.code == PARAM and "PerThread" in str(e.value)
    ctx.sync()
    c.judge(only=())
    c.queue(1, None)
    ctx.sync()
    c.judge(only=(1,))


# ---- a slot that grows while other calls are queued ------------------------------------------------------------

GROW_LENS = [3000, 17, 500000, 989, 1500000, 2013]
GROW_DS = (0, 2, 27, 1, 27, 2)
GROW_CALLS = [[0], [1], [3], [5], [2], [0, 1], [3, 5], [1], [4]]      # calls 0, 4 and 8 share slot 0; 1, 5 slot 1; ...


class GrowingMirror(MirrorPath):
    """Frames of 1 KiB with 27 ds entries: a frame costs the plan its 276 prefix bytes, 32 bytes of frame, 32 of
    its unit and 4 of scratch, so the files of 500,000 and 1,500,000 bytes need far more than a slot's first
    64 KiB."""

    def __init__(self, ctx, oracle):
        import tfs_amd.crc as crc
        self.ctx, self.oracle = ctx, oracle
        self.cfg = crc.mirror_cfg(1024 - 36, 1024, version=2)
        self.img, recs = M.build_source(oracle, GROW_LENS, [(3 * i + 1) % 16 for i in range(len(GROW_LENS))], seed=37)
        self.ds = np.arange(1, 41, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        self.jobs, self.cap = M.make_jobs(self.cfg, recs, GROW_DS, len(self.ds), [(7 * i + 2) % 16 for i in range(len(recs))])
        self.d_src = {id(self.img): crc.DeviceBuffer(ctx, self.img.size + 256).upload(self.img)}

    def plan_bounds(self, idx):
        """(least, most) bytes of slot memory a call over jobs `idx` needs: least counts the frames' prefix bytes
        alone (TFS_MIRROR_FRAME_HEAD + 8 * ds_count each), most every structure with room to spare."""
        import tfs_amd.crc as crc
        least = most = 0
        for i in idx:
            nf = crc.mirror_frame_count(self.cfg, int(self.jobs["size"][i]))
            head = crc.MIRROR_FRAME_HEAD + 8 * int(self.jobs["ds_count"][i])
            least += nf * head
            most += nf * (head + 32 + 2 * 36) + 128
        return least, most + 4096

    def batches(self, calls):
        return [((self.jobs[idx].copy(), self.cfg.copy(), self.ds.copy(), self.img), self.cap, 0) for idx in calls]


@pytest.mark.parametrize("which", ["context", "owned", "foreign"])
def test_mirror_slot_grows_while_calls_are_in_flight(oracle, which):
    """Nine calls queued without a wait on a context of the test's own, whose slots start empty.  Slot 0 serves
    calls 0, 4 and 8: a 3,000-byte file (the first 64 KiB), then 500,000 bytes (more than 64 KiB), then 1,500,000
    bytes (more than whatever the second needed, rounded up to 64 KiB) -- twice the slot's next user must wait
    for the event, free the memory and allocate anew while calls on the other slots are still queued."""
    import tfs_amd.crc as crc
    K = 64 << 10
    ctx = crc.Context(0)
    made = []
    try:
        path = GrowingMirror(ctx, oracle)
        made.append(path)
        b0, b4, b8 = (path.plan_bounds(GROW_CALLS[k]) for k in (0, 4, 8))
        assert b0[1] <= K < b4[0] and (b4[1] + K - 1) // K * K < b8[0], (b0, b4, b8)
        assert all(path.plan_bounds(GROW_CALLS[k])[1] <= K for k in (1, 2, 3, 5, 6, 7))
        streams = Streams(ctx)
        made.append(streams)
        c = Calls(ctx, path, path.batches(GROW_CALLS))
        made.append(c)
        s = {"context": None, "owned": streams.owned, "foreign": streams.foreign}[which]
        for k in range(len(GROW_CALLS)):
            c.queue(k, s)
        streams.sync(s)
        c.judge()
    finally:
        ctx.sync()
        for m in reversed(made):
            m.close() if isinstance(m, Streams) else m.free()
        ctx.close()
