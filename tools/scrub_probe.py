#!/usr/bin/env python3
"""Scrub session (include/tfs_ec.h tfs_ec_scrub_*) against the nearest
work the library did before it: the marshalling session over the same data members, in
the same process.  Both move dn + pn member-sizes; the marshalling session writes the
parity where the scrub session reads it.  One process, measurement only; bench.py and
benchlines/ are not involved.

k = 5, m = 3; 64 MiB members, everything device-resident.

  (a) 1,024 records of 64 KiB per member, one chunk of the whole member   [gated]
  (b) the same members in 64 chunks of 1 MiB, the dataserver's loop
  (c) members holding one 64 MiB record each

The two sides alternate round by round; each round times REPS calls, one by one, between
HIP events.  A call is the session's chunk call or calls and its finish, which launches
the fold (the scrub session: and the count), copies the results to the host and
synchronises; begin (host plan and upload) is reported beside it and not timed with the
call.  Before timing both sides are checked for equal record CRCs, no failed record and a
zero map.  Reports median / min / max / spread of each side, and for (a) whether the
scrub session's median is within the marshalling session's median plus the marshalling
session's own round-to-round spread (max - min).  Writes profiles/scrub_probe.json.

  python tools/scrub_probe.py [ROUNDS [CASES, e.g. "ab"]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
from tfs_amd.ec import ErasureCode, MarshalSession, ScrubSession  # noqa: E402
from tools.marshal_probe import FI, K, M, SIZE, block_image, spread  # noqa: E402,F401


class Case:
    def __init__(self, ctx, nrec, rec, seed):
        assert nrec * rec == SIZE
        self.ctx = ctx
        self.all = crc.DeviceBuffer(ctx, (K + M) * SIZE)   # the members share one allocation
        self.ptr = [self.all.ptr + i * SIZE for i in range(K + M)]
        self.metas = []
        for i in range(K):
            img, mt = block_image(ctx, nrec, rec, seed + i)
            self.all.upload(img, offset=i * SIZE)
            self.metas.append(mt)
        self.n = K * nrec
        self.enc = ErasureCode(ctx, K, M)
        assert self.enc.rc == 0
        self.rec = rec

    def session(self, kind, chunk):
        """(begin s, chunk calls ms, whole call ms, results)."""
        ctx = self.ctx
        t0 = time.perf_counter()
        ses = (MarshalSession if kind == "marshal" else ScrubSession)(self.enc, self.metas, [SIZE] * K, SIZE)
        t_begin = time.perf_counter() - t0
        assert ses.rc == 0
        call = ses.encode_device if kind == "marshal" else ses.check_device
        e0, e1, e2 = crc.Event(ctx), crc.Event(ctx), crc.Event(ctx)
        e0.record()
        for o in range(0, SIZE, chunk):
            assert call([p + o for p in self.ptr], o, chunk) == 0
        e1.record()
        res = ses.finish()
        e2.record()
        ctx.sync()
        ses.free()
        return t_begin, e0.elapsed_ms(e1), e0.elapsed_ms(e2), res

    def run(self, name, chunk, rounds, reps=3):
        # the marshalling session writes the parity the scrub session reads; both agree before timing
        _, _, _, (c1, s1, bad1, rc1) = self.session("marshal", chunk)
        _, _, _, (c2, s2, bad2, units, tmap, rc2) = self.session("scrub", chunk)
        ok = rc1 == 0 and rc2 == 0 and bad1 == 0 and bad2 == 0 and (s1 == 0).all() and (s2 == 0).all() and \
            (c1 == c2).all() and not tmap.any() and not units.any()
        if not ok:
            raise SystemExit("scrub_probe: the two sides disagree (%s)" % name)
        times = {"marshal": [], "scrub": [], "marshal_chunk_calls": [], "scrub_chunk_calls": [], "marshal_begin": [],
                 "scrub_begin": []}
        for r in range(rounds):
            for kind in ("marshal", "scrub"):
                self.session(kind, chunk)
                tb, te, ta = [], [], []
                for _ in range(reps):
                    b, e, a, _ = self.session(kind, chunk)
                    tb.append(1e3 * b), te.append(e), ta.append(a)
                times[kind].append(sum(ta) / reps)
                times[kind + "_chunk_calls"].append(sum(te) / reps)
                times[kind + "_begin"].append(sum(tb) / reps)
        res = {k: dict(spread(v), unit="ms") for k, v in times.items()}
        o, w = res["marshal"], res["scrub"]
        res["scrub_over_marshal"] = w["median"] / o["median"]
        res["scrub_GBps_traffic"] = (K + M) * SIZE / (w["median"] / 1e3) / 1e9
        res["marshal_GBps_traffic"] = (K + M) * SIZE / (o["median"] / 1e3) / 1e9
        res["scrub_finish_ms"] = w["median"] - res["scrub_chunk_calls"]["median"]
        res["marshal_finish_ms"] = o["median"] - res["marshal_chunk_calls"]["median"]
        res["within_marshal_median_plus_spread"] = bool(w["median"] <= o["median"] + o["spread"])
        return {"records": self.n, "record_bytes": self.rec, "chunk_bytes": chunk, "chunks": SIZE // chunk,
                "rounds": rounds, "reps": reps, "ms": times, "ab": res}

    def free(self):
        self.enc.free()
        self.all.free()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    if rounds < 8:
        raise SystemExit("scrub_probe: at least 8 rounds")
    ctx = crc.Context(0)
    res = {"tool": "scrub_probe", "k": K, "m": M, "member_bytes": SIZE}
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
        res["acceptance_a"] = res["a_one_chunk"]["ab"]["within_marshal_median_plus_spread"]
    out = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scrub_probe.json"), "w") as f:
        f.write(out + "\n")
    print(out)
    ctx.close()


if __name__ == "__main__":
    main()
