#!/usr/bin/env python3
"""Mirror sync (include/tfs_mirror.h) against what a caller could compose before
for the same bytes, in one process, device-resident.  Measurement only; bench.py and benchlines/
are not involved.

The workload's own shape: 1,024 files of 64 KiB of one block, the reference's first_len /
frame_len (MAX_READ_SIZE - 36, MAX_READ_SIZE), two ds entries a frame.  Two sanity shapes: one
file of 8 MiB (nine frames) and a Zipf mix of 1 KiB .. 4 MiB files.

  (a) tfs_mirror_frames_device: one call for the batch;
  (b) what the library had: tfs_block_verify_device over the records, one tfs_crc32_memcpy per
      frame's data into frames built beforehand (header, H and V in place, crc 0), then
      tfs_packet_seal_device over the frames (three reads and one write of every payload byte);
  (c) one device copy of the same number of payload bytes (one read, one write: the floor).

The forms alternate round by round; each run is timed with device events on the context's
stream, after warm-up rounds of every form; (a)'s time on the calling thread (checks, plan,
enqueue) is taken beside it, since the device waits for it.  Before timing, (a)'s results are checked (every
status 0, file_crc == the stored crc_), (a)'s out is compared byte for byte with (b)'s sealed
frames, and sampled frames with frames built here (zlib).  Writes profiles/mirror_probe.json.

  python tools/mirror_probe.py [RUNS]
"""
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402

FI = 36
FLAG = 0x4E534654
FIRST, FL = crc.MAX_READ_SIZE - FI, crc.MAX_READ_SIZE
DS = np.array([0x0A0A0A0A00001F90, 0x0A0A0A0B00001F90], np.uint64)
HEAD = 60 + 8 * len(DS)
PEAK = 8e12       # bytes/s of HBM, MI355X
UNIT = 16 << 10   # mirror_plan.h kMirSeg


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med,
            "unit": "ms"}


def frame_ranges(n):
    """(offset, length) of every frame of a payload of n bytes."""
    out, off, k = [], 0, 0
    while off < n:
        ln = min(FIRST if k == 0 else FL, n - off)
        out.append((off, ln))
        off += ln
        k += 1
    return out


def probe_shape(ctx, name, sizes, runs, warm):
    sizes = np.asarray(sizes, np.int64)
    n = len(sizes)
    rec_off = np.concatenate(([0], np.cumsum(sizes + FI)[:-1])).astype(np.uint64)
    total = int((sizes + FI).sum())
    payload = int(sizes.sum())
    img = crc.DeviceBuffer(ctx, total + 4096)
    ctx.synth_fill_device(img, (total + 7) & ~7, 0x5EAD, 0)  # (whole 8-byte words; the buffer has the room)
    desc = np.zeros(n, crc.DESC_DTYPE)
    desc["offset"], desc["len"] = rec_off + FI, sizes
    d_desc = crc.DeviceBuffer(ctx, desc.nbytes).upload(desc)
    d_crc = crc.DeviceBuffer(ctx, 4 * n)
    ctx.batch_device(d_desc, n, img, d_crc)
    d_roff = crc.DeviceBuffer(ctx, rec_off.nbytes).upload(rec_off)
    d_len = crc.DeviceBuffer(ctx, 4 * n).upload(sizes.astype(np.uint32))
    ctx.write_headers_device(img, d_roff, d_len, d_crc, 1, n)  # file id = 1 + index
    ctx.sync()
    stored = d_crc.download(np.uint32, n)
    metas = np.zeros(n, crc.META_DTYPE)
    metas["file_id"], metas["offset"], metas["size"] = 1 + np.arange(n), rec_off, sizes + FI
    d_metas = crc.DeviceBuffer(ctx, metas.nbytes).upload(metas)

    cfg = crc.mirror_cfg()
    jobs = np.zeros(n, crc.MIRROR_JOB_DTYPE)
    jobs["src_offset"], jobs["file_id"], jobs["size"] = rec_off, metas["file_id"], metas["size"]
    jobs["file_number"] = 0x700000 + np.arange(n)
    jobs["packet_id"] = 1000 + 16 * np.arange(n)
    jobs["block_id"], jobs["ds_first"], jobs["ds_count"] = 4711, 0, len(DS)
    frames, at = [], 0   # (job, k, frame offset in out, payload offset, length)
    for i in range(n):
        at += (int(rec_off[i]) + FI - (at + HEAD)) % 16   # the first frame's data on the source's address mod 16
        jobs["frame_offset"][i] = at
        for k, (off, ln) in enumerate(frame_ranges(int(sizes[i]))):
            frames.append((i, k, at, off, ln))
            at += HEAD + ln
        assert at - int(jobs["frame_offset"][i]) == crc.mirror_span(cfg, jobs[i:i + 1])
    cap = at + 64
    nfr = len(frames)
    units = sum(-(-ln // UNIT) for _, _, _, _, ln in frames)
    d_out = crc.DeviceBuffer(ctx, cap)
    d_res = crc.DeviceBuffer(ctx, 16 * n)
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.zero()

    def form_a():
        ctx.mirror_frames_device(cfg, img, total, jobs, DS, d_out, cap, d_res, d_bad)

    # (b): the frames built beforehand, then verify, copy, seal
    pre = np.zeros(cap, np.uint8)
    for i, k, fo, off, ln in frames:
        h = struct.pack("<IihhQI", FLAG, 36 + 8 * len(DS) + ln, 9, 2, int(jobs["packet_id"][i]) + k, 0) + \
            struct.pack("<IQiiiQ", 4711, int(jobs["file_id"][i]), off, ln, 0, int(jobs["file_number"][i])) + \
            struct.pack("<i", len(DS)) + DS.tobytes()
        pre[fo:fo + HEAD] = np.frombuffer(h, np.uint8)
    d_frames = crc.DeviceBuffer(ctx, cap).upload(pre)
    pd = np.zeros(nfr, crc.PACKET_DESC_DTYPE)
    pd["offset"] = [f[2] for f in frames]
    pd["len"] = [HEAD + f[4] for f in frames]
    d_pd = crc.DeviceBuffer(ctx, pd.nbytes).upload(pd)
    d_pcrc, d_pst = crc.DeviceBuffer(ctx, 4 * nfr), crc.DeviceBuffer(ctx, 4 * nfr)
    d_vc, d_st = crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4 * n)
    d_bad_b = crc.DeviceBuffer(ctx, 4)
    d_bad_b.zero()
    st = ctx.stream
    copies = [(d_frames.ptr + fo + HEAD, img.ptr + int(rec_off[i]) + FI + off, ln) for i, k, fo, off, ln in frames]

    def form_b():
        ctx.block_verify_device(img, total, d_metas, n, d_vc, d_st, d_bad_b)
        for dst, src, ln in copies:
            ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, dst, src, ln, st), "memcpy")
        ctx.packet_seal_device(d_pd, nfr, d_frames, d_pcrc, d_pst)

    d_copy = crc.DeviceBuffer(ctx, payload + 4096)

    def form_c():
        ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, d_copy.ptr, img.ptr, payload, st), "memcpy")

    # correctness before the clock
    form_a()
    form_b()
    ctx.sync()
    res = d_res.download(crc.MIRROR_RESULT_DTYPE, n)
    if res["status"].any() or int(d_bad.download(np.uint32, 1)[0]) or int(d_bad_b.download(np.uint32, 1)[0]):
        raise SystemExit("mirror_probe %s: a clean file did not verify" % name)
    if (res["file_crc"] != stored).any() or (d_vc.download(np.uint32, n) != stored).any():
        raise SystemExit("mirror_probe %s: a file CRC differs from the stored one" % name)
    if (d_pst.download(np.int32, nfr) != 0).any():
        raise SystemExit("mirror_probe %s: form (b) did not seal" % name)
    got_a, got_b = d_out.download(np.uint8, at), d_frames.download(np.uint8, at)
    used = np.zeros(at, bool)
    for _, _, fo, _, ln in frames:
        used[fo:fo + HEAD + ln] = True
    if not (got_a[used] == got_b[used]).all():
        raise SystemExit("mirror_probe %s: (a)'s frames differ from (b)'s" % name)
    for i, k, fo, off, ln in [frames[0], frames[nfr // 2], frames[-1]]:
        f = got_a[fo:fo + HEAD + ln].tobytes()
        c = zlib.crc32(f[24:], FLAG ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
        data = img.download(np.uint8, ln, int(rec_off[i]) + FI + off).tobytes()
        if struct.unpack_from("<I", f, 20)[0] != c or f[HEAD:] != data or f[:20] != pre[fo:fo + 20].tobytes():
            raise SystemExit("mirror_probe %s: frame %d of file %d differs from the frame built on the host" % (name, k, i))

    forms = {"a_mirror_frames": form_a, "b_verify_copy_seal": form_b, "c_device_copy_alone": form_c}
    times = {k: [] for k in forms}
    e0, e1 = crc.Event(ctx), crc.Event(ctx)
    host_a = []  # the calling thread's time inside (a): the checks, the plan and the enqueue
    for r in range(warm + runs):
        for key, call in forms.items():
            e0.record()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            e1.record()
            ctx.sync()
            if r >= warm:
                times[key].append(e0.elapsed_ms(e1))
                if key == "a_mirror_frames":
                    host_a.append((t1 - t0) * 1e3)
    ab = {k: spread(v) for k, v in times.items()}
    a, b, c = (ab[k]["median"] for k in forms)
    larger = max(ab["a_mirror_frames"]["spread"], ab["b_verify_copy_seal"]["spread"])
    moved = {
        "a_mirror_frames": {"read": payload + FI * n, "written": payload + HEAD * nfr},
        "b_verify_copy_seal": {"read": 3 * payload + FI * n + HEAD * nfr, "written": payload + 4 * nfr},
        "c_device_copy_alone": {"read": payload, "written": payload},
    }
    out = {
        "files": n, "payload_bytes": payload, "frames": nfr, "units_one_wave_each": units, "runs": runs, "warmup": warm,
        "ms": times, "ab": ab, "a_host_call_ms": spread(host_a), "bytes": moved,
        "payload_GiBps": {k: payload / (ab[k]["median"] / 1e3) / 2**30 for k in forms},
        "fraction_of_8TBps": {k: (moved[k]["read"] + moved[k]["written"]) / (ab[k]["median"] / 1e3) / PEAK for k in forms},
        "a_over_b": a / b, "a_over_c": a / c,
        "a_faster_than_b_by_more_than_the_larger_spread": bool(b - a > larger),
    }
    for buf in (img, d_desc, d_crc, d_roff, d_len, d_metas, d_out, d_res, d_bad, d_frames, d_pd, d_pcrc, d_pst, d_vc,
                d_st, d_bad_b, d_copy):
        buf.free()
    return out


def zipf_sizes(seed=7, count=2048, budget=96 << 20):
    rng = np.random.default_rng(seed)
    s = np.minimum(rng.zipf(1.3, count), 4096).astype(np.int64) * 1024
    keep = np.cumsum(s) <= budget
    return s[keep]


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    if runs < 20:
        raise SystemExit("mirror_probe: at least 20 runs")
    ctx = crc.Context(0)
    shapes = {
        "files_1024_x_64KiB": np.full(1024, 65536),
        "one_file_8MiB": np.array([8 << 20]),
        "zipf_mix": zipf_sizes(),
    }
    out = {"tool": "mirror_probe", "first_len": FIRST, "frame_len": FL, "ds_per_frame": len(DS),
           "shapes": {k: probe_shape(ctx, k, v, runs, 4) for k, v in shapes.items()}}
    out["acceptance_a_faster_than_b_at_64KiB"] = \
        out["shapes"]["files_1024_x_64KiB"]["a_faster_than_b_by_more_than_the_larger_spread"]
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mirror_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
