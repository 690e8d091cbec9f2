#!/usr/bin/env python3
"""Reinstate session (include/tfs_ec.h tfs_ec_reinstate_*) against
the fastest route the library offered before it for the same result:
tfs_ec_decode_device over the members, then tfs_blocks_verify_device over the
records of all five data members, surviving and rebuilt, in one launch (the members
share an allocation), on one stream between HIP events.  One process, measurement
only; bench.py and benchlines/ are not involved.

k = 5, m = 3; 64 MiB members, everything device-resident; data members 1 and 3 and
parity member 0 are dead, so the sources are data 0, 2, 4 and parity 1, 2 and the
outputs data 1, 3 and parity 0.

  (a) 1,024 records of 64 KiB per member, one chunk of the whole member   [gated]
  (b) the same members in 64 chunks of 1 MiB, the reference's loop
  (c) members holding one 64 MiB record each: the fold's long chain

The two sides alternate round by round; each round times REPS calls, one by one.
A session's call is its decode call or calls and tfs_ec_reinstate_finish, which
launches the fold, copies the statuses to the host and synchronises: the copy
cannot be kept out of the events, so it is inside the session's time (against the
session), and the time from the last decode to the end of finish is reported
beside it, as are begin (host plan and upload, not timed with the call) and a
device-to-host copy of the statuses' size alone.  Reports median / min / max /
spread of each side, and for (a) whether the session's median is within the old
route's median plus its own round-to-round spread.

  python tools/reinstate_probe.py [ROUNDS [CASES, e.g. "ab"]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
from tfs_amd.ec import ErasureCode, ReinstateSession  # noqa: E402

K, M = 5, 3
FI = 36
SIZE = 64 << 20
DEAD = (1, 3, K)                      # data 1, data 3, parity 0
ERASED = [1 if i in DEAD else 0 for i in range(K + M)]  # five left: every survivor is a source
SOURCES = [i for i in range(K + M) if ERASED[i] == 0][:K]


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med}


def block_image(ctx, nrec, rec, seed):
    """nrec records of `rec` bytes (FileInfo + payload) back to back, CRCs from the file kernel."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, nrec * rec, dtype=np.uint8)
    off = np.arange(nrec, dtype=np.int64) * rec
    crcs = ctx.batch(img, off + FI, np.full(nrec, rec - FI, np.uint32), 0)
    metas = np.zeros(nrec, crc.META_DTYPE)
    metas["file_id"] = np.arange(1, nrec + 1) + (seed << 32)
    metas["offset"] = off
    metas["size"] = rec
    fi = np.zeros(nrec, crc.FILEINFO_DTYPE)
    fi["id_"], fi["offset_"], fi["size_"], fi["usize_"], fi["crc_"] = metas["file_id"], off, rec, rec, crcs
    view = img.reshape(nrec, rec)
    view[:, :FI] = fi.view(np.uint8).reshape(nrec, FI)
    return img, metas


class Case:
    def __init__(self, ctx, nrec, rec, seed):
        assert nrec * rec == SIZE
        self.ctx = ctx
        self.all = crc.DeviceBuffer(ctx, (K + M) * SIZE)   # the members share one allocation
        self.ptr = [self.all.ptr + i * SIZE for i in range(K + M)]
        self.out2 = crc.DeviceBuffer(ctx, len(DEAD) * SIZE)  # the session's rebuilt members
        self.metas = []
        for i in range(K):
            img, mt = block_image(ctx, nrec, rec, seed + i)
            self.all.upload(img, offset=i * SIZE)
            self.metas.append(mt)
        self.n = K * nrec
        jobs = np.zeros(self.n, crc.COMPACT_JOB_DTYPE)
        allm = np.concatenate(self.metas)
        jobs["src_offset"] = allm["offset"].astype(np.uint64) + np.repeat(np.arange(K, dtype=np.uint64) * SIZE, nrec)
        jobs["file_id"], jobs["size"] = allm["file_id"], allm["size"]
        self.d_jobs = crc.DeviceBuffer(ctx, jobs.nbytes).upload(jobs)
        self.d_crc, self.d_st, self.d_bad = (crc.DeviceBuffer(ctx, 4 * self.n), crc.DeviceBuffer(ctx, 4 * self.n),
                                             crc.DeviceBuffer(ctx, 4))
        enc = ErasureCode(ctx, K, M)
        assert enc.rc == 0 and enc.encode_device(self.ptr, SIZE) == 0  # the family as it was marshalled
        ctx.sync()
        enc.free()
        self.orig = {i: self.all.download(np.uint8, SIZE, offset=i * SIZE) for i in DEAD}
        self.dec = ErasureCode(ctx, K, M, ERASED)
        assert self.dec.rc == 0
        self.rec = rec

    def old(self):
        assert self.dec.decode_device(self.ptr, SIZE) == 0   # rebuilds members 1, 3 and 5 where they lie
        self.ctx.blocks_verify_device(self.all, K * SIZE, self.d_jobs, self.n, self.d_crc, self.d_st, self.d_bad)

    def session(self, chunk):
        """(begin s, decode ms, whole call ms, results)."""
        ctx = self.ctx
        t0 = time.perf_counter()
        ses = ReinstateSession(self.dec, self.metas, [SIZE] * K, SIZE)
        t_begin = time.perf_counter() - t0
        assert ses.rc == 0
        e0, e1, e2 = crc.Event(ctx), crc.Event(ctx), crc.Event(ctx)
        e0.record()
        for o in range(0, SIZE, chunk):
            ptrs = [self.out2.ptr + DEAD.index(i) * SIZE + o if i in DEAD else self.ptr[i] + o if i in SOURCES else None
                    for i in range(K + M)]
            assert ses.decode_device(ptrs, o, chunk) == 0
        e1.record()
        res = ses.finish()
        e2.record()
        ctx.sync()
        ses.free()
        return t_begin, e0.elapsed_ms(e1), e0.elapsed_ms(e2), res

    def run(self, name, chunk, rounds, reps=3):
        ctx = self.ctx
        # both sides agree before timing
        self.d_bad.zero()
        for i in DEAD:  # the dead members' bytes are gone before either side runs
            ctx._check(ctx.L.tfs_crc32_memset_device(ctx.handle, self.ptr[i], 0xA5, SIZE, None), "memset")
        self.out2.upload(np.full(len(DEAD) * SIZE, 0x5A, np.uint8))
        self.old()
        ctx.sync()
        _, _, _, (c2, s2, nbad, rc) = self.session(chunk)
        ok = rc == 0 and nbad == 0 and int(self.d_bad.download(np.uint32)[0]) == 0 and (s2 == 0).all() \
            and (self.d_st.download(np.int32, self.n) == 0).all() and (self.d_crc.download(np.uint32, self.n) == c2).all()
        for j, i in enumerate(DEAD):
            a = self.all.download(np.uint8, SIZE, offset=i * SIZE)
            ok = ok and (a == self.out2.download(np.uint8, SIZE, offset=j * SIZE)).all() and (a == self.orig[i]).all()
        if not ok:
            raise SystemExit("reinstate_probe: the two sides disagree (%s)" % name)
        times = {"decode_then_verify": [], "session": [], "session_decode_calls": [], "session_begin": []}
        for r in range(rounds):
            self.old()
            ctx.sync()
            t = []
            for _ in range(reps):
                e0, e1 = crc.Event(ctx), crc.Event(ctx)
                e0.record()
                self.old()
                e1.record()
                ctx.sync()
                t.append(e0.elapsed_ms(e1))
            times["decode_then_verify"].append(sum(t) / reps)
            self.session(chunk)
            tb, te, ta = [], [], []
            for _ in range(reps):
                b, e, a, _ = self.session(chunk)
                tb.append(1e3 * b), te.append(e), ta.append(a)
            times["session"].append(sum(ta) / reps)
            times["session_decode_calls"].append(sum(te) / reps)
            times["session_begin"].append(sum(tb) / reps)
        host = np.zeros(2 * self.n, np.uint32)
        t0 = time.perf_counter()
        for _ in range(20):
            ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, host.ctypes.data, self.d_crc.ptr, min(host.nbytes, 4 * self.n),
                                              None), "memcpy d2h")
        d2h = (time.perf_counter() - t0) / 20 * 1e3
        res = {k: dict(spread(v), unit="ms") for k, v in times.items()}
        o, w, e = res["decode_then_verify"], res["session"], res["session_decode_calls"]
        res["fold_and_statuses_ms"] = w["median"] - e["median"]
        res["statuses_d2h_alone_ms"] = d2h
        res["session_over_old"] = w["median"] / o["median"]
        res["session_GBps_traffic"] = (K + len(DEAD)) * SIZE / (w["median"] / 1e3) / 1e9
        res["old_GBps_traffic"] = (2 * K + len(DEAD)) * SIZE / (o["median"] / 1e3) / 1e9
        res["per_decode_call_ms"] = e["median"] / (SIZE // chunk)
        res["within_old_median_plus_spread"] = bool(w["median"] <= o["median"] + o["spread"])
        return {"records": self.n, "record_bytes": self.rec, "chunk_bytes": chunk, "chunks": SIZE // chunk,
                "rounds": rounds, "reps": reps, "ms": times, "ab": res}

    def free(self):
        self.dec.free()
        for b in (self.all, self.out2, self.d_jobs, self.d_crc, self.d_st, self.d_bad):
            b.free()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    if rounds < 8:
        raise SystemExit("reinstate_probe: at least 8 rounds")
    ctx = crc.Context(0)
    res = {"tool": "reinstate_probe", "k": K, "m": M, "member_bytes": SIZE, "erased": ERASED}
    cases = sys.argv[2] if len(sys.argv) > 2 else "abc"
    if "a" in cases or "b" in cases:
        big = Case(ctx, 1024, 65536, 1)
        if "a" in cases:
            res["a_one_chunk"] = big.run("a", SIZE, rounds)
        if "b" in cases:
            res["b_64_chunks_of_1MiB"] = big.run("b", 1 << 20, rounds)
        big.free()
    if "c" in cases:
        one = Case(ctx, 1, SIZE, 21)
        res["c_one_64MiB_record"] = one.run("c", SIZE, rounds)
        one.free()
    if "a" in cases:
        res["acceptance_a"] = res["a_one_chunk"]["ab"]["within_old_median_plus_spread"]
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
