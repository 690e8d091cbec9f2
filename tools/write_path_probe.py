#!/usr/bin/env python3
"""Write frames that yield the file CRC (include/tfs_write.h):
what the write-data form costs and what the close gains, in one process
(measurement only; bench.py and benchlines/ are not involved).

  (a) launch   NFRAMES device-resident, sealed WRITE_DATA frames of 64 KiB data
               (6 ds entries): tfs_packet_verify_write_device against plain
               tfs_packet_verify_device over the same frames, alternated round by
               round, each timed with HIP events around REPS launches.  Reports
               both forms' median / min / max and spread.
  (b) queue    tfs_ds_loopback_queue (WRITE and CLOSE as separate queued items,
               8 workers): mode 0 (file CRC computed at close) against mode 1
               (data CRCs carried from the packet check, combined on the host),
               alternated, gap 0 and 8.  Reports close p50 / p99, GiB/s of
               payload, and the H2D copy rate measured in the same run.

  python tools/write_path_probe.py [ROUNDS] [NFRAMES] [NLEASES]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
import tfs_amd.dataserver as ds  # noqa: E402
from tfs_amd import packet as pk  # noqa: E402
from tfs_amd.synth import synth_bytes  # noqa: E402

DATA = 65536
NDS = 6
GROUP = 256  # frames built on the host; the device image repeats them


def host_frames(count, first=0):
    """`count` unsealed WRITE_DATA frames back to back: (bytes, frame size)."""
    out = []
    for i in range(count):
        data = synth_bytes(0x5EED + first + i, DATA).tobytes()
        body = pk.write_data_body(7, first + i + 1, 0, data, ds=list(range(NDS)), file_number=first + i + 1)
        out.append(pk.frame_v1(body, pid=first + i + 1))
    return b"".join(out), len(out[0])


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread_pct": 100.0 * (v[-1] - v[0]) / med}


def launch_ab(ctx, rounds, nframes, reps=3):
    grp, frame = host_frames(GROUP)
    ngroups = max(1, nframes // GROUP)
    n = ngroups * GROUP
    img = crc.DeviceBuffer(ctx, n * frame + 4096)
    g = np.frombuffer(grp, np.uint8)
    for k in range(ngroups):
        img.upload(g, k * len(grp))
    pd = np.zeros(n, crc.PACKET_DESC_DTYPE)
    pd["offset"] = np.arange(n, dtype=np.uint64) * frame
    pd["len"] = frame
    d_pd = crc.DeviceBuffer(ctx, pd.nbytes).upload(pd)
    d_crc = crc.DeviceBuffer(ctx, 4 * n)
    d_st = crc.DeviceBuffer(ctx, 4 * n)
    d_parts = crc.DeviceBuffer(ctx, 16 * n)
    d_bad = crc.DeviceBuffer(ctx, 4)
    ctx.packet_seal_device(d_pd, n, img, d_crc, d_st)
    ctx.sync()
    # both forms agree before timing; every frame brings its data CRC, equal to the
    # file kernel's Func::crc(0, D) over the same bytes
    d_bad.zero()
    ctx.packet_verify_device(d_pd, n, img, d_crc, d_st, d_bad)
    ctx.sync()
    plain = d_crc.download(np.uint32, n)
    ctx.packet_verify_write_device(d_pd, n, img, d_crc, d_st, d_parts, d_bad)
    ctx.sync()
    parts = d_parts.download(crc.WRITE_PART_DTYPE, n)
    fd = np.zeros(n, crc.DESC_DTYPE)
    fd["offset"] = pd["offset"] + 24 + 36 + 8 * NDS
    fd["len"] = DATA
    d_fd = crc.DeviceBuffer(ctx, fd.nbytes).upload(fd)
    d_z = crc.DeviceBuffer(ctx, 4 * n)
    ctx.batch_device(d_fd, n, img, d_z)
    ctx.sync()
    if (int(d_bad.download(np.uint32)[0]) != 0 or not (d_crc.download(np.uint32, n) == plain).all()
            or not (parts["data_len"] == DATA).all() or not (parts["data_off"] == 36 + 8 * NDS).all()
            or not (parts["data_crc"] == d_z.download(np.uint32, n)).all()):
        raise SystemExit("write_path_probe: the two forms disagree")
    cases = {"plain": lambda: ctx.packet_verify_device(d_pd, n, img, d_crc, d_st, d_bad),
             "write": lambda: ctx.packet_verify_write_device(d_pd, n, img, d_crc, d_st, d_parts, d_bad)}
    times = {k: [] for k in cases}
    for r in range(rounds):
        for k, fn in cases.items():
            fn()
            e0, e1 = crc.Event(ctx), crc.Event(ctx)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            ctx.sync()
            times[k].append(e0.elapsed_ms(e1) / reps)
    res = {k: dict(spread(v), unit="ms", GBps=n * frame / (spread(v)["median"] / 1e3) / 1e9) for k, v in times.items()}
    res["write_over_plain"] = res["write"]["median"] / res["plain"]["median"]
    for b in (img, d_pd, d_crc, d_st, d_parts, d_bad, d_fd, d_z):
        b.free()
    return {"frames": n, "frame_bytes": frame, "rounds": rounds, "reps": reps, "ms": times, "ab": res}


def queue_ab(ctx, rounds, nleases, nthreads=8):
    raw, frame = host_frames(nleases, first=100000)
    pin = crc.PinnedBuffer(ctx, len(raw))
    pin.array[:] = np.frombuffer(raw, np.uint8)
    off = np.arange(nleases, dtype=np.uint64) * frame
    ln = np.full(nleases, frame, np.uint32)
    crc_s, st = ctx.packet_seal(pin.array, off, ln)
    assert (st == 0).all()
    # client CRCs: Func::crc(0, data) from the file kernel
    data_off = off + 24 + 36 + 8 * NDS
    client = ctx.batch(pin.array, data_off, np.full(nleases, DATA, np.uint32), 0)
    # the H2D rate of this run: the frames' buffer copied to the device
    dev = crc.DeviceBuffer(ctx, len(raw))
    h2d = []
    for _ in range(5):
        e0, e1 = crc.Event(ctx), crc.Event(ctx)
        e0.record()
        ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, dev.ptr, pin.ptr, len(raw), None), "memcpy h2d")
        e1.record()
        ctx.sync()
        h2d.append(len(raw) / (e0.elapsed_ms(e1) / 1e3) / 2**30)
    dev.free()
    out = {"leases": nleases, "threads": nthreads, "data_bytes": DATA, "h2d_GiBps": spread(h2d), "gaps": {}}
    for gap in (0, 8):
        runs = {0: [], 1: []}
        for r in range(rounds + 1):  # round 0 warms both modes up
            for mode in (0, 1):
                blk = ds.LogicBlock(1000 + r)
                t0 = time.perf_counter()
                rc, lst, us = ds.loopback_queue(ctx, pin, off, ln, nleases, 1, client, nthreads, gap, mode, blk,
                                                close_us=True)
                dt = time.perf_counter() - t0
                blk.free()
                if rc != 0:
                    raise SystemExit("write_path_probe: loopback_queue mode %d returned %d" % (mode, rc))
                if r:
                    runs[mode].append({"GiBps": nleases * DATA / dt / 2**30, "p50_us": float(np.percentile(us, 50)),
                                       "p99_us": float(np.percentile(us, 99))})
        res = {}
        for mode in (0, 1):
            res["mode%d" % mode] = {k: spread([x[k] for x in runs[mode]]) for k in ("GiBps", "p50_us", "p99_us")}
        res["mode1_over_mode0_GiBps"] = res["mode1"]["GiBps"]["median"] / res["mode0"]["GiBps"]["median"]
        res["mode1_GiBps_over_h2d"] = res["mode1"]["GiBps"]["median"] / out["h2d_GiBps"]["median"]
        res["mode0_GiBps_over_h2d"] = res["mode0"]["GiBps"]["median"] / out["h2d_GiBps"]["median"]
        out["gaps"][str(gap)] = res
    pin.free()
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    nframes = int(sys.argv[2]) if len(sys.argv) > 2 else 131072
    nleases = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    if rounds < 4:
        raise SystemExit("write_path_probe: at least 4 rounds")
    ctx = crc.Context(0)
    res = {"tool": "write_path_probe", "launch": launch_ab(ctx, rounds, nframes), "queue": queue_ab(ctx, rounds, nleases)}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
