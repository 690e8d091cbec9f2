#!/usr/bin/env python3
"""Parity update (include/tfs_ec.h tfs_ec_update(_device)) against the nearest
calls the library had before it, in the same process.  One process, measurement only;
bench.py and benchlines/ are not involved.

k = 5, m = 3; 64 MiB members, everything device-resident but (d).

  (a) the unlink: one unit, three parity members bound, old and new bytes given, against what
      the library offered for the same bytes where all members are in one place:
      tfs_ec_encode_device over that one unit of the five data members.  Both are one launch.
      Rule: the update's median at most the yardstick's median plus the
      yardstick's own spread (max - min).
  (b) 64 scattered units, the list uploaded, beside the dense form over 64 units (no list) and
      16 units in the launch arguments.  No bound.
  (c) a whole member rewritten, dense: with a and b (8 member-sizes of traffic) and delta-only
      (7), against a full tfs_ec_encode_device of the family (8).  No bound; the traffic rates
      are written down.
  (d) the parity server's call: the host form with one unit and its one parity member bound,
      pageable memory.  Microseconds per call by the host clock (the call is synchronous).

The sides alternate round by round; each round times REPS calls, each alone between HIP events.
An update applied twice is undone, so the timed calls flip the same parity units back and forth.
Before timing, the update's parity is checked against tfs_ec_encode_device of the data with the
new bytes, in every form timed.  Writes profiles/update_probe.json.

  python tools/update_probe.py [ROUNDS]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
from tfs_amd.ec import ErasureCode  # noqa: E402
from tools.locate_probe import REPS, ab  # noqa: E402
from tools.marshal_probe import K, M, SIZE, spread  # noqa: E402

UNITS = SIZE // 1024
J = 2          # the data member that changes
HOST_CALLS = 20


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    if rounds < 8:
        raise SystemExit("update_probe: at least 8 rounds")
    ctx = crc.Context(0)
    enc = ErasureCode(ctx, K, M)
    assert enc.rc == 0
    mem = [crc.DeviceBuffer(ctx, SIZE) for _ in range(K + M)]
    for i in range(K):
        ctx.synth_fill_device(mem[i], SIZE, 100 + i)
    assert enc.encode_device(mem, SIZE) == 0
    new_j = crc.DeviceBuffer(ctx, SIZE)           # member J with other bytes everywhere
    ctx.synth_fill_device(new_j, SIZE, 902)
    want = [crc.DeviceBuffer(ctx, SIZE) for _ in range(M)]   # the parity of the family with new_j, by the encode
    assert enc.encode_device(mem[:J] + [new_j] + mem[J + 1:K] + want, SIZE) == 0
    ctx.sync()
    h_old = [mem[K + p].download(np.uint8, SIZE) for p in range(M)]
    h_want = [w.download(np.uint8, SIZE) for w in want]
    for w in want:
        w.free()
    par = [crc.DeviceBuffer(ctx, SIZE).upload(h) for h in h_old]       # the update's own parity members
    rng = np.random.default_rng(11)
    scattered = rng.choice(UNITS, 64, replace=False).astype(np.uint32)
    one = scattered[:1]

    def slots(buf, units):
        d = crc.DeviceBuffer(ctx, 1024 * len(units))
        d.upload(np.concatenate([buf.download(np.uint8, 1024, offset=int(u) * 1024) for u in units]))
        return d
    a64, b64 = slots(mem[J], scattered), slots(new_j, scattered)
    a_dense, b_dense = slots(mem[J], range(64)), slots(new_j, range(64))
    delta = crc.DeviceBuffer(ctx, SIZE)
    delta.upload(mem[J].download(np.uint8, SIZE) ^ new_j.download(np.uint8, SIZE))

    def update(d_a, d_b, units, n):
        return lambda: enc.update_device(par, SIZE, J, d_a, d_b, units, n)

    def parity_now():
        ctx.sync()
        return [p.download(np.uint8, SIZE) for p in par]

    def expect(units):
        """The parity with the listed units of member J changed: h_want there, h_old elsewhere."""
        out = [h.copy() for h in h_old]
        for o, w in zip(out, h_want):
            for u in units:
                o[1024 * int(u):1024 * int(u) + 1024] = w[1024 * int(u):1024 * int(u) + 1024]
        return out

    def check(call, units):
        """One call gives the encode's bytes in the listed units and leaves the others; a second undoes it."""
        assert call() == 0
        ok = all((g == e).all() for g, e in zip(parity_now(), expect(units)))
        assert call() == 0
        return ok and all((g == e).all() for g, e in zip(parity_now(), h_old))

    forms = {"update_1": (update(a64, b64, one, 1), one),
             "update_16_in_arguments": (update(a64, b64, scattered[:16], 16), scattered[:16]),
             "update_64_indexed": (update(a64, b64, scattered, 64), scattered),
             "update_64_dense": (update(a_dense, b_dense, None, 64), range(64))}
    ok = all(check(call, units) for call, units in forms.values())
    for call in (update(mem[J], new_j, None, UNITS), update(delta, None, None, UNITS)):
        assert call() == 0
        ok = ok and all((g == e).all() for g, e in zip(parity_now(), h_want))
        assert call() == 0
        ok = ok and all((g == e).all() for g, e in zip(parity_now(), h_old))
    if not ok:
        raise SystemExit("update_probe: the update's parity differs from the encode's")

    res = {"tool": "update_probe", "k": K, "m": M, "member_bytes": SIZE, "rounds": rounds, "reps": REPS}
    t, s = ab(ctx, {"encode_1_unit": lambda: enc.encode_device(mem, 1024), "update_1": forms["update_1"][0]}, rounds)
    y, w = s["encode_1_unit"], s["update_1"]
    res["a_unlink_one_unit"] = {"ms": t, "ab": s, "update_over_encode": w["median"] / y["median"],
                                "within_encode_median_plus_spread": bool(w["median"] <= y["median"] + y["spread"])}
    res["acceptance_a"] = res["a_unlink_one_unit"]["within_encode_median_plus_spread"]
    t, s = ab(ctx, {name: forms[name][0] for name in ("update_64_indexed", "update_64_dense", "update_16_in_arguments")}, rounds)
    res["b_64_scattered_units"] = {"ms": t, "ab": s,
                                   "list_upload_ms": s["update_64_indexed"]["median"] - s["update_64_dense"]["median"]}
    t, s = ab(ctx, {"encode_family": lambda: enc.encode_device(mem, SIZE),
                    "update_a_b": update(mem[J], new_j, None, UNITS),
                    "update_delta_only": update(delta, None, None, UNITS)}, rounds)
    sizes = {"encode_family": K + M, "update_a_b": 2 + 2 * M, "update_delta_only": 1 + 2 * M}
    res["c_whole_member_dense"] = {"ms": t, "ab": s, "member_sizes_of_traffic": sizes,
                                   "GBps": {n: sizes[n] * SIZE / (s[n]["median"] / 1e3) / 1e9 for n in sizes},
                                   "update_a_b_over_encode": s["update_a_b"]["median"] / s["encode_family"]["median"],
                                   "update_delta_only_over_encode": s["update_delta_only"]["median"] / s["encode_family"]["median"]}
    # (d) the host form, pageable memory, one parity member bound
    ctx.sync()
    h_par = h_old[1].copy()
    u = int(one[0])
    h_a = mem[J].download(np.uint8, 1024, offset=u * 1024)
    h_b = new_j.download(np.uint8, 1024, offset=u * 1024)
    bound = [None, h_par, None]
    assert enc.update(bound, SIZE, J, h_a, h_b, units=[u]) == 0
    if not (h_par == expect([u])[1]).all():
        raise SystemExit("update_probe: the host form's parity differs from the encode's")
    us = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(HOST_CALLS):
            assert enc.update(bound, SIZE, J, h_a, h_b, units=[u]) == 0
        us.append((time.perf_counter() - t0) / HOST_CALLS * 1e6)
    res["d_host_form_one_unit_one_parity"] = {"us_per_call": us, "calls_per_round": HOST_CALLS, "ab": dict(spread(us), unit="us")}
    out = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "update_probe.json"), "w") as f:
        f.write(out + "\n")
    print(out)
    enc.free()
    ctx.close()


if __name__ == "__main__":
    main()
