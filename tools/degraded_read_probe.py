#!/usr/bin/env python3
"""Degraded read (include/tfs_ec.h tfs_ec_read_degraded_device)
against the two launches the library offered before it for the same job:
tfs_ec_decode_device over the whole member, then tfs_block_verify_device over
the rebuilt member, on one stream between HIP events.  One process, measurement
only; bench.py and benchlines/ are not involved.

k = 5, m = 3; the target is a 64 MiB member of 1,024 records of 64 KiB
(FileInfo + 65,500 payload bytes), everything device-resident.

  (a) every record, the target alone erased
  (b) every record, the target + one data + one parity member erased (the old
      path rebuilds three members, the read one)
  (c) 64 records spread over the member, the target alone erased
  (d) one 8 MiB record read alone: what a single wave sustains

The two sides alternate round by round; each round times REPS calls.  Reports
median / min / max / spread of each side, and for (a) whether the read's median
is within the old path's median plus its own round-to-round spread.

  python tools/degraded_read_probe.py [ROUNDS]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
from tfs_amd.ec import ErasureCode  # noqa: E402

K, M, TARGET = 5, 3, 2
FI = 36


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
    metas["file_id"] = np.arange(1, nrec + 1)
    metas["offset"] = off
    metas["size"] = rec
    fi = np.zeros(nrec, crc.FILEINFO_DTYPE)
    fi["id_"], fi["offset_"], fi["size_"], fi["usize_"], fi["crc_"] = metas["file_id"], off, rec, rec, crcs
    view = img.reshape(nrec, rec)
    view[:, :FI] = fi.view(np.uint8).reshape(nrec, FI)
    return img, metas


class Case:
    def __init__(self, ctx, nrec, rec, seed):
        self.ctx, self.size = ctx, nrec * rec
        self.img, self.metas = block_image(ctx, nrec, rec, seed)
        rng = np.random.default_rng(seed + 1)
        self.d = []
        for i in range(K + M):
            b = crc.DeviceBuffer(ctx, self.size)
            if i == TARGET:
                b.upload(self.img)
            elif i < K:
                b.upload(rng.integers(0, 256, self.size, dtype=np.uint8))
            self.d.append(b)
        enc = ErasureCode(ctx, K, M)
        assert enc.rc == 0 and enc.encode_device(self.d, self.size) == 0
        ctx.sync()
        enc.free()
        self.out = crc.DeviceBuffer(ctx, self.size)

    def run(self, name, also, pick, rounds, reps=3):
        ctx, n = self.ctx, len(pick)
        erased = [1 if i == TARGET or i in also else 0 for i in range(K + M)]
        dec = ErasureCode(ctx, K, M, erased)
        assert dec.rc == 0
        metas = self.metas[pick]
        jobs, cap = ErasureCode.read_jobs(metas)
        d_metas = crc.DeviceBuffer(ctx, metas.nbytes).upload(metas)
        d_jobs = crc.DeviceBuffer(ctx, jobs.nbytes).upload(jobs)
        d_crc, d_st, d_bad = (crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4))
        d_crc2, d_st2 = crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4 * n)
        members = [None if erased[i] else self.d[i] for i in range(K + M)]

        def old():
            assert dec.decode_device(self.d, self.size) == 0
            ctx.block_verify_device(self.d[TARGET], self.size, d_metas, n, d_crc, d_st, d_bad)

        def new():
            assert dec.read_degraded_device(members, self.size, TARGET, d_jobs, n, self.out, cap, d_crc2, d_st2,
                                            d_bad) == 0

        # both sides agree before timing
        for i in range(K + M):
            if erased[i]:
                self.d[i].zero()
        d_bad.zero()
        self.out.zero()
        old()
        new()
        ctx.sync()
        got = self.out.download(np.uint8, cap)
        exp = np.concatenate([self.img[int(m["offset"]):int(m["offset"]) + int(m["size"])] for m in metas])
        if (int(d_bad.download(np.uint32)[0]) != 0 or not (d_st2.download(np.int32, n) == 0).all()
                or not (d_crc.download(np.uint32, n) == d_crc2.download(np.uint32, n)).all()
                or not (got == exp).all()
                or not (self.d[TARGET].download(np.uint8, self.size) == self.img).all()):
            raise SystemExit("degraded_read_probe: the two sides disagree (%s)" % name)
        times = {"decode_then_verify": [], "read_degraded": []}
        for r in range(rounds):
            for k, fn in (("decode_then_verify", old), ("read_degraded", new)):
                fn()
                e0, e1 = crc.Event(ctx), crc.Event(ctx)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                ctx.sync()
                times[k].append(e0.elapsed_ms(e1) / reps)
        res = {k: dict(spread(v), unit="ms") for k, v in times.items()}
        o, w = res["decode_then_verify"], res["read_degraded"]
        res["read_over_old"] = w["median"] / o["median"]
        res["read_GBps_rebuilt"] = cap / (w["median"] / 1e3) / 1e9
        res["read_GBps_traffic"] = (K + 1) * cap / (w["median"] / 1e3) / 1e9
        res["within_old_median_plus_spread"] = bool(w["median"] <= o["median"] + o["spread"])
        for b in (d_metas, d_jobs, d_crc, d_st, d_bad, d_crc2, d_st2):
            b.free()
        dec.free()
        return {"records": n, "record_bytes": int(metas["size"][0]), "erased": erased, "rounds": rounds, "reps": reps,
                "ms": times, "ab": res}

    def free(self):
        for b in self.d + [self.out]:
            b.free()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    if rounds < 8:
        raise SystemExit("degraded_read_probe: at least 8 rounds")
    ctx = crc.Context(0)
    res = {"tool": "degraded_read_probe", "k": K, "m": M, "target": TARGET}
    big = Case(ctx, 1024, 65536, 1)
    res["member_bytes"] = big.size
    res["a_all_records_target_alone"] = big.run("a", (), np.arange(1024), rounds)
    res["b_all_records_three_erased"] = big.run("b", (0, K + 1), np.arange(1024), rounds)
    res["c_64_records"] = big.run("c", (), np.arange(8, 1024, 16), rounds)
    big.free()
    one = Case(ctx, 1, 8 << 20, 9)
    res["d_one_8MiB_record"] = one.run("d", (), np.arange(1), rounds)
    one.free()
    res["acceptance_a"] = res["a_all_records_target_alone"]["ab"]["within_old_median_plus_spread"]
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
