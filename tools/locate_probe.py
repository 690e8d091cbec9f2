#!/usr/bin/env python3
"""Scrub locate (include/tfs_ec.h tfs_ec_locate_device) against the nearest
calls the library had before it, in the same process.  One process, measurement only;
bench.py and benchlines/ are not involved.

k = 5, m = 3; 64 MiB members, everything device-resident.

  (a) the common case: 64 flagged units scattered over the family, indexed form, with
      repaired units, against tfs_ec_encode_device over a dense 64 KiB per member (the
      nearest prior call of the same launch size).  Rule: the locate median
      at most the yardstick's median plus the yardstick's own spread (max - min).  Beside it,
      as a breakdown: the same 64 units without an output for repaired units, and the dense
      form over 64 units (no list to upload).
  (b) a member rotted throughout: every unit of one data member wrong, dense form over the
      whole family, against the scrub session's chunk call over the same eight members
      (the same dn + pn member-sizes read, the same syndromes).  No bound: the ratio and
      the locate kernel's bytes/s are written down.
  (c) a clean list: (b) over the clean family, against the same yardstick -- the
      wave-uniform skip of the candidate and repair stages.

The two sides alternate round by round; each round times REPS calls, each alone between
HIP events.  Before timing, every case's results are checked against what the probe did
to the family.  Writes profiles/locate_probe.json.

  python tools/locate_probe.py [ROUNDS]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
from tfs_amd.ec import LOCATE_CONFIRMED, LOCATE_RESULT_DTYPE, ErasureCode, ScrubSession  # noqa: E402
from tools.marshal_probe import K, M, SIZE, spread  # noqa: E402

UNITS = SIZE // 1024
REPS = 3


def timed(ctx, call):
    e0, e1 = crc.Event(ctx), crc.Event(ctx)
    e0.record()
    assert call() == 0
    e1.record()
    ctx.sync()
    return e0.elapsed_ms(e1)


def ab(ctx, sides, rounds):
    """sides: {name: call}; the sides alternate round by round, a round is the mean of REPS calls."""
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, call in sides.items():
            timed(ctx, call)
            times[name].append(sum(timed(ctx, call) for _ in range(REPS)) / REPS)
    return times, {name: dict(spread(v), unit="ms") for name, v in times.items()}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    if rounds < 8:
        raise SystemExit("locate_probe: at least 8 rounds")
    ctx = crc.Context(0)
    enc = ErasureCode(ctx, K, M)
    assert enc.rc == 0
    mem = [crc.DeviceBuffer(ctx, SIZE) for _ in range(K + M)]
    for i in range(K):
        ctx.synth_fill_device(mem[i], SIZE, 100 + i)
    assert enc.encode_device(mem, SIZE) == 0
    ctx.sync()
    # (a): member 2 again, with 8 bytes inverted in each of 64 scattered units
    hurt2 = crc.DeviceBuffer(ctx, SIZE)
    ctx.synth_fill_device(hurt2, SIZE, 102)
    rng = np.random.default_rng(7)
    flagged = rng.choice(UNITS, 64, replace=False).astype(np.uint32)
    orig = {}
    for u in flagged:
        at = int(u) * 1024 + 8 * int(rng.integers(0, 128))
        orig[int(u)] = mem[2].download(np.uint8, 1024, offset=int(u) * 1024)
        hurt2.upload(~mem[2].download(np.uint8, 8, offset=at), offset=at)
    fam_a = mem[:2] + [hurt2] + mem[3:]
    # (b): member 1 with other bytes everywhere
    rot1 = crc.DeviceBuffer(ctx, SIZE)
    ctx.synth_fill_device(rot1, SIZE, 901)
    fam_b = mem[:1] + [rot1] + mem[2:]
    d_res = crc.DeviceBuffer(ctx, 8 * UNITS)
    d_fix = crc.DeviceBuffer(ctx, SIZE)
    none = [np.zeros(0, crc.META_DTYPE)] * K

    def locate(fam, units, n, fixed=True):
        return lambda: enc.locate_device(fam, SIZE, units, n, d_res, d_fix if fixed else None)

    def scrub_chunk(fam):
        def call():
            ses = ScrubSession(enc, none, [SIZE] * K, SIZE)
            assert ses.rc == 0
            e0, e1 = crc.Event(ctx), crc.Event(ctx)
            e0.record()
            assert ses.check_device(fam, 0, SIZE) == 0
            e1.record()
            ctx.sync()
            ms = e0.elapsed_ms(e1)
            ses.free()
            return ms
        return call

    def ab_scrub(fam, side, rounds):
        """locate against the scrub session's chunk call (its begin and finish are not timed)."""
        sc = scrub_chunk(fam)
        times = {"scrub_chunk": [], "locate": []}
        for _ in range(rounds):
            sc()
            times["scrub_chunk"].append(sum(sc() for _ in range(REPS)) / REPS)
            timed(ctx, side)
            times["locate"].append(sum(timed(ctx, side) for _ in range(REPS)) / REPS)
        return times, {name: dict(spread(v), unit="ms") for name, v in times.items()}

    res = {"tool": "locate_probe", "k": K, "m": M, "member_bytes": SIZE, "rounds": rounds, "reps": REPS}
    # checks before timing
    assert locate(fam_a, flagged, 64)() == 0
    ctx.sync()
    r = d_res.download(LOCATE_RESULT_DTYPE, 64)
    fx = d_fix.download(np.uint8, 64 * 1024).reshape(64, 1024)
    ok = (r["kind"] == 2).all() and (r["member"] == 2).all() and (r["diff_bytes"] == 8).all() and \
        (r["flags"] == LOCATE_CONFIRMED).all() and all((fx[k] == orig[int(u)]).all() for k, u in enumerate(flagged))
    assert locate(fam_b, None, UNITS)() == 0
    ctx.sync()
    r = d_res.download(LOCATE_RESULT_DTYPE, UNITS)
    ok = ok and (r["kind"] == 2).all() and (r["member"] == 1).all()
    ok = ok and (d_fix.download(np.uint8, 1 << 20) == mem[1].download(np.uint8, 1 << 20)).all()
    assert locate(mem, None, UNITS)() == 0
    ctx.sync()
    r = d_res.download(LOCATE_RESULT_DTYPE, UNITS)
    ok = ok and (r["kind"] == 0).all() and not r["parity"].any()
    if not ok:
        raise SystemExit("locate_probe: a result differs from what the probe did to the family")

    t, s = ab(ctx, {"encode_64KiB": lambda: enc.encode_device(mem, 65536),
                    "locate_64_indexed": locate(fam_a, flagged, 64),
                    "locate_64_indexed_no_fixed": locate(fam_a, flagged, 64, fixed=False),
                    "locate_64_dense": locate(fam_a, None, 64)}, rounds)
    y, w = s["encode_64KiB"], s["locate_64_indexed"]
    res["a_64_scattered_units"] = {
        "ms": t, "ab": s, "locate_over_encode": w["median"] / y["median"],
        "list_upload_ms": w["median"] - s["locate_64_dense"]["median"],
        "repaired_units_ms": w["median"] - s["locate_64_indexed_no_fixed"]["median"],
        "within_encode_median_plus_spread": bool(w["median"] <= y["median"] + y["spread"])}
    res["acceptance_a"] = res["a_64_scattered_units"]["within_encode_median_plus_spread"]
    for name, fam in (("b_member_rotted_throughout", fam_b), ("c_clean_family", mem)):
        t, s = ab_scrub(fam, locate(fam, None, UNITS), rounds)
        y, w = s["scrub_chunk"], s["locate"]
        res[name] = {"ms": t, "ab": s, "locate_over_scrub_chunk": w["median"] / y["median"],
                     "locate_GBps_read": (K + M) * SIZE / (w["median"] / 1e3) / 1e9,
                     "scrub_chunk_GBps_read": (K + M) * SIZE / (y["median"] / 1e3) / 1e9,
                     "within_scrub_median_plus_spread": bool(w["median"] <= y["median"] + y["spread"])}
    out = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "locate_probe.json"), "w") as f:
        f.write(out + "\n")
    print(out)
    enc.free()
    ctx.close()


if __name__ == "__main__":
    main()
