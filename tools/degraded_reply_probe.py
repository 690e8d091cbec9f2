#!/usr/bin/env python3
"""Degraded read replies (include/tfs_ec_read.h tfs_ec_read_reply_device) against what
the library offered before for the same job, in one process, device-resident, 5:3.  Measurement only;
bench.py and benchlines/ are not involved.

  one pass:     tfs_ec_read_reply_device -- rebuild, verify, seal, one launch, no scratch;
  composition:  tfs_ec_read_degraded_device into a scratch buffer, then tfs_read_reply_device from it,
                on one stream (for the slice of case (d): a range job from the FileInfo to the slice's
                end, the least the second call can be given).

Cases: (a) 1,024 whole 64 KiB records of a 64 MiB member, V2 frames, the target alone erased; (b) the
same with the target, one more data member and one parity member erased; (c) one 64 KiB record alone;
(d) one 1 MiB slice at read_offset 3 MiB of an 8 MiB record; (e) case (a) with every frame 3 bytes off
the slice's address mod 16.

The sides alternate round by round, at least 8 rounds.  A round queues one warm-up call and then REPS
calls back to back between two HIP events and divides.  Before timing, every frame of the one pass is
compared byte for byte with the composition's, and every status is 0.  Writes
profiles/degraded_reply_probe.json.

  python tools/degraded_reply_probe.py [ROUNDS]
"""
import json
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
import tfs_amd.ec as ec  # noqa: E402

FI, K, M, TARGET = 36, 5, 3, 2


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med,
            "unit": "ms"}


def member_of_records(size, rec, rng):
    """A member image tiled with records of `rec` bytes (FileInfo included); returns (image, [(id, offset, size)])."""
    img = rng.integers(0, 256, size, dtype=np.uint8)
    recs = []
    for k in range(size // rec):
        o = k * rec
        c = (zlib.crc32(img[o + FI:o + rec].tobytes(), 0xFFFFFFFF) ^ 0xFFFFFFFF) & 0xFFFFFFFF  # Func::crc(0, .)
        img[o:o + FI] = np.frombuffer(struct.pack("<QiiiiiiI", 1 + k, o, rec, rec, 1700000000, 1600000000, 0, c), np.uint8)
        recs.append((1 + k, o, rec))
    return img, recs


class Side:
    """A family on the device, a coder, and the buffers of both forms for one job list."""

    def __init__(self, ctx, members, erased, recs, read_offset, read_len, misalign=0):
        self.ctx, self.size = ctx, members[0].size
        self.dec = ec.ErasureCode(ctx, K, M, erased)
        assert self.dec.rc == 0
        self.d = [None if erased[i] else crc.DeviceBuffer(ctx, members[i].size).upload(members[i]) for i in range(K + M)]
        n = self.n = len(recs)
        off = np.array([r[1] for r in recs], np.int64)
        size = np.array([r[2] for r in recs], np.int64)
        nserve = np.minimum(read_len, size - FI - read_offset)
        cap = 28 + nserve + (40 if read_offset == 0 else 4)
        self.frame_bytes = int(cap.sum())
        d0 = off + FI + read_offset
        # frames one behind the other, each moved up so that frame + 28 = D0 + misalign mod 16
        fo, at = np.zeros(n, np.int64), 0
        for k in range(n):
            at += (int(d0[k]) + misalign - 28 - at) % 16
            fo[k] = at
            at += int(cap[k])
        self.out_cap = at + 16
        rj = np.zeros(n, crc.READ_JOB_DTYPE)
        rj["src_offset"], rj["frame_offset"], rj["file_id"] = off, fo, [r[0] for r in recs]
        rj["packet_id"] = 1000 + np.arange(n)
        rj["size"], rj["read_offset"], rj["read_len"], rj["pcode"], rj["version"] = size, read_offset, read_len, 39, 2
        self.jobs = ec.ErasureCode.reply_jobs(rj)
        self.d_out = crc.DeviceBuffer(ctx, self.out_cap)
        self.d_res = crc.DeviceBuffer(ctx, 16 * n)
        self.d_bad = crc.DeviceBuffer(ctx, 4)
        self.d_bad.zero()
        # the composition: covering units into a scratch, the reply from there
        whole = read_offset == 0 and (nserve == size - FI).all()
        if whole:
            dj, scap = ec.ErasureCode.read_jobs([(r[0], r[1], r[2]) for r in recs])
            self.covered = scap
        else:  # a range job from the FileInfo to the slice's end
            dj, scap = ec.ErasureCode.read_jobs(ranges=[(int(off[k]), int(FI + read_offset + nserve[k])) for k in range(n)])
            self.covered = scap
        self.d_dj = crc.DeviceBuffer(ctx, dj.nbytes).upload(dj)
        # (tfs_read_reply_device wants the whole record inside src_len, rebuilt or not)
        self.scap = scap
        self.src_len = max(scap, int((dj["out_offset"].astype(np.int64) + off % 1024 + size).max()))
        self.d_scratch = crc.DeviceBuffer(ctx, self.src_len + 16)
        self.d_crc, self.d_st = crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4 * n)
        self.cj = rj.copy()
        self.cj["src_offset"] = dj["out_offset"].astype(np.int64) + off % 1024
        self.d_out2 = crc.DeviceBuffer(ctx, self.out_cap)
        self.d_res2 = crc.DeviceBuffer(ctx, 16 * n)
        # the units the one pass reads per source member
        units = set()
        for k in range(n):
            units |= set(range(int(off[k]) // 1024, (int(off[k]) + FI + 1023) // 1024))
            units |= set(range(int(d0[k]) // 1024, (int(d0[k] + nserve[k]) + 1023) // 1024)) if nserve[k] else set()
        self.one_pass_units = len(units)

    def one_pass(self):
        rc = self.dec.read_reply_device(self.d, self.size, TARGET, self.jobs, self.d_out, self.out_cap, self.d_res, self.d_bad)
        assert rc == 0, rc

    def composition(self):
        rc = self.dec.read_degraded_device(self.d, self.size, TARGET, self.d_dj, self.n, self.d_scratch, self.scap,
                                           self.d_crc, self.d_st, self.d_bad)
        assert rc == 0, rc
        self.ctx.read_reply_device(self.d_scratch, self.src_len, self.cj, self.d_out2, self.out_cap, self.d_res2, self.d_bad)

    def check(self):
        self.one_pass()
        self.composition()
        self.ctx.sync()
        r1 = self.d_res.download(crc.READ_RESULT_DTYPE, self.n)
        r2 = self.d_res2.download(crc.READ_RESULT_DTYPE, self.n)
        if int(self.d_bad.download(np.uint32, 1)[0]) or (r1["status"] != 0).any() or r1.tobytes() != r2.tobytes():
            raise SystemExit("degraded_reply_probe: the two sides' results differ, or a clean record did not verify")
        o1, o2 = self.d_out.download(np.uint8, self.out_cap), self.d_out2.download(np.uint8, self.out_cap)
        for j, r in zip(self.jobs, r1):
            a, b = int(j["frame_offset"]), int(j["frame_offset"]) + int(r["frame_len"])
            if o1[a:b].tobytes() != o2[a:b].tobytes():
                raise SystemExit("degraded_reply_probe: a frame of the one pass differs from the composition's")

    def accounted(self):
        """Bytes each side moves through device memory, plans and results included."""
        dn, n = K, self.n
        return {"one_pass": {"read": dn * 1024 * self.one_pass_units + 64 * n, "written": self.frame_bytes + 16 * n},
                "composition": {"read": dn * self.covered + 32 * n + self.covered + 64 * n,
                                "written": self.covered + 8 * n + self.frame_bytes + 16 * n}}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    if rounds < 8:
        raise SystemExit("degraded_reply_probe: at least 8 rounds")
    ctx = crc.Context(0)
    rng = np.random.default_rng(0x5EAD)

    def family(timg):
        ms = [timg if i == TARGET else rng.integers(0, 256, timg.size, dtype=np.uint8) if i < K
              else np.zeros(timg.size, np.uint8) for i in range(K + M)]
        enc = ec.ErasureCode(ctx, K, M)
        assert enc.rc == 0 and enc.encode(ms, timg.size) == 0
        enc.free()
        return ms
    img64, recs64 = member_of_records(64 << 20, 65536, rng)
    fam64 = family(img64)
    big, brecs = member_of_records(8 << 20, 8 << 20, rng)   # one record of 8 MiB, FileInfo included
    fam8 = family(big)
    alone = [1 if i == TARGET else 0 for i in range(K + M)]
    three = [1 if i in (TARGET, 0, K + 1) else 0 for i in range(K + M)]
    cases = {
        "a_1024_whole_64k_records": (Side(ctx, fam64, alone, recs64, 0, 65536 - FI), 3),
        "b_same_three_members_erased": (Side(ctx, fam64, three, recs64, 0, 65536 - FI), 3),
        "c_one_64k_record_alone": (Side(ctx, fam64, alone, recs64[517:518], 0, 65536 - FI), 50),
        "d_1m_slice_at_3m_of_8m_record": (Side(ctx, fam8, alone, brecs, 3 << 20, 1 << 20), 20),
        "e_case_a_frames_3_bytes_off": (Side(ctx, fam64, alone, recs64, 0, 65536 - FI, misalign=3), 3),
    }
    for side, _ in cases.values():
        side.check()
    times = {name: {"one_pass": [], "composition": []} for name in cases}
    e0, e1 = crc.Event(ctx), crc.Event(ctx)
    for _ in range(rounds):
        for name, (side, reps) in cases.items():
            for form in ("one_pass", "composition"):
                call = getattr(side, form)
                call()
                e0.record()
                for _ in range(reps):
                    call()
                e1.record()
                ctx.sync()
                times[name][form].append(e0.elapsed_ms(e1) / reps)
    out = {"tool": "degraded_reply_probe", "geometry": "5:3", "rounds": rounds, "pcode": 39, "cases": {}}
    for name, (side, reps) in cases.items():
        if int(side.d_bad.download(np.uint32, 1)[0]) != 0:
            raise SystemExit("degraded_reply_probe: failed jobs during the timed calls")
        a, b = spread(times[name]["one_pass"]), spread(times[name]["composition"])
        out["cases"][name] = {
            "jobs": side.n, "reps_per_round": reps, "ms": times[name], "one_pass": a, "composition": b,
            "one_pass_over_composition": a["median"] / b["median"],
            "ranges_overlap": bool(a["max"] >= b["min"] and b["max"] >= a["min"]),
            "one_pass_median_no_higher": bool(a["median"] <= b["median"]),
            "bytes": side.accounted(),
        }
    ca, ce = out["cases"]["a_1024_whole_64k_records"], out["cases"]["e_case_a_frames_3_bytes_off"]
    out["e_over_a_one_pass"] = ce["one_pass"]["median"] / ca["one_pass"]["median"]
    out["speed_gate_a_and_c"] = bool(ca["one_pass_median_no_higher"] and
                                     out["cases"]["c_one_64k_record_alone"]["one_pass_median_no_higher"])
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "degraded_reply_probe.json"), "w") as f:
        f.write(text + "\n")
    brief = {k: (round(v["one_pass"]["median"], 4), round(v["composition"]["median"], 4),
                 round(v["one_pass_over_composition"], 3), v["ranges_overlap"]) for k, v in out["cases"].items()}
    print(json.dumps({"brief": brief, "e_over_a": out["e_over_a_one_pass"], "gate": out["speed_gate_a_and_c"]}))
    ctx.close()


if __name__ == "__main__":
    main()
