#!/usr/bin/env python3
"""Read replies (include/tfs_read.h tfs_read_reply_device) against what the
library offered before for the same bytes, in one process, device-resident.  Measurement
only; bench.py and benchlines/ are not involved.

The workload's own shape: N files of 64 KiB (N = 65,536: 4 GiB of payload per launch), every
file read whole as a RESP_READ_DATA_MESSAGE_V2 reply, each frame placed so that frame + 28 is
congruent to the payload's address mod 16.

  (a) tfs_read_reply_device: one launch verifies, copies and seals (the plan of N jobs is built
      on the host and uploaded inside the call);
  (b) what the library had: tfs_compact_jobs_device over the same records (verify and copy),
      then tfs_packet_seal_device over frames of the same sizes (a second read of every byte);
  (c) tfs_compact_jobs_device alone (one read, one write: what (a) should approach).

Beside them, to say where (a)'s time over (c) goes: (a) with every frame on the payload's address
mod 128 (in (c) source and destination lines coincide; mod 16 they do not), and the upload of
(a)'s plan alone (N x 64 bytes from page-locked memory, which (c)'s device-resident job list
does not pay).  The calling thread's time per call is recorded too.

The forms alternate round by round.  A round queues one warm-up call and then REPS calls back
to back between two HIP events and divides: the device form is asynchronous, and the host work
of the next call (the plan) overlaps the kernel of the last as it does in a server.  Before
timing, (a)'s results are checked (every status 0) and sampled frames are compared byte for
byte with frames built here (zlib).  Writes profiles/read_reply_probe.json.

  python tools/read_reply_probe.py [ROUNDS] [N]
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

FI, FILE, REPS = 36, 65536, 3
FLAG = 0x4E534654


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med,
            "unit": "ms"}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    if rounds < 8:
        raise SystemExit("read_reply_probe: at least 8 rounds")
    ctx = crc.Context(0)
    rec = FI + FILE
    total = n * rec
    img = crc.DeviceBuffer(ctx, (total + 4095) // 4096 * 4096 + 4096)
    ctx.synth_fill_device(img, (total + 7) // 8 * 8, 0x5EAD, 0)
    rec_off = np.arange(n, dtype=np.uint64) * rec
    desc = np.zeros(n, crc.DESC_DTYPE)
    desc["offset"], desc["len"] = rec_off + FI, FILE
    d_desc = crc.DeviceBuffer(ctx, desc.nbytes).upload(desc)
    d_crc = crc.DeviceBuffer(ctx, 4 * n)
    ctx.batch_device(d_desc, n, img, d_crc)
    d_roff = crc.DeviceBuffer(ctx, rec_off.nbytes).upload(rec_off)
    d_len = crc.DeviceBuffer(ctx, 4 * n).upload(np.full(n, FILE, np.uint32))
    ctx.write_headers_device(img, d_roff, d_len, d_crc, 1, n)  # file id = 1 + index
    ctx.sync()
    # (a): the frames, each where its data keeps the payload's address mod 16
    frame_len = 24 + 4 + FILE + 4 + FI
    stride = (frame_len + 15 + 15) // 16 * 16
    jobs = np.zeros(n, crc.READ_JOB_DTYPE)
    jobs["src_offset"] = rec_off
    jobs["frame_offset"] = np.arange(n, dtype=np.uint64) * stride + ((rec_off + FI - 28) % 16)
    jobs["file_id"] = 1 + np.arange(n, dtype=np.uint64)
    jobs["packet_id"] = 1000 + np.arange(n, dtype=np.uint64)
    jobs["size"], jobs["read_len"], jobs["pcode"], jobs["version"] = rec, FILE, 39, 2
    out_cap = n * stride + 64
    # the same frames on the payload's address mod 128: source and destination lines coincide, as in (c)
    stride128 = (frame_len + 127 + 127) // 128 * 128
    jobs128 = jobs.copy()
    jobs128["frame_offset"] = np.arange(n, dtype=np.uint64) * stride128 + ((rec_off + FI - 28) % 128)
    out_cap128 = n * stride128 + 128
    d_out = crc.DeviceBuffer(ctx, out_cap128)
    d_res = crc.DeviceBuffer(ctx, 16 * n)
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.zero()
    # (b), (c): the same records compacted (verify + copy), then frames of the same sizes sealed
    cj = np.zeros(n, crc.COMPACT_JOB_DTYPE)
    cj["src_offset"], cj["dest_offset"], cj["file_id"], cj["size"] = rec_off, rec_off, jobs["file_id"], rec
    cj["new_offset"] = (rec_off & 0x7FFFFFFF).astype(np.int32)
    d_cj = crc.DeviceBuffer(ctx, cj.nbytes).upload(cj)
    d_cdst = crc.DeviceBuffer(ctx, total + 4096)
    d_cst = crc.DeviceBuffer(ctx, 4 * n)
    d_frames = crc.DeviceBuffer(ctx, out_cap)
    ctx.synth_fill_device(d_frames, out_cap // 8 * 8, 0xF00D, 0)
    foff = jobs["frame_offset"].astype(np.uint64)
    d_foff = crc.DeviceBuffer(ctx, foff.nbytes).upload(foff)
    d_blen = crc.DeviceBuffer(ctx, 4 * n).upload(np.full(n, frame_len - 24, np.uint32))
    ctx.write_packet_headers_device(d_frames, d_foff, d_blen, n, 39, 2, 1000)
    pd = np.zeros(n, crc.PACKET_DESC_DTYPE)
    pd["offset"], pd["len"] = foff, frame_len
    d_pd = crc.DeviceBuffer(ctx, pd.nbytes).upload(pd)
    d_pcrc = crc.DeviceBuffer(ctx, 4 * n)
    d_pst = crc.DeviceBuffer(ctx, 4 * n)

    def form_a():
        ctx.read_reply_device(img, total, jobs, d_out, out_cap, d_res, d_bad)

    def form_a128():
        ctx.read_reply_device(img, total, jobs128, d_out, out_cap128, d_res, d_bad)

    def form_c():
        ctx.compact_jobs_device(img, total, d_cj, n, d_cdst, None, d_cst, d_bad)

    def form_b():
        form_c()
        ctx.packet_seal_device(d_pd, n, d_frames, d_pcrc, d_pst)

    # correctness before the clock
    form_a()
    form_b()
    ctx.sync()
    res = d_res.download(crc.READ_RESULT_DTYPE, n)
    if int(d_bad.download(np.uint32, 1)[0]) != 0 or (res["status"] != 0).any() or (res["frame_len"] != frame_len).any():
        raise SystemExit("read_reply_probe: a clean file did not verify")
    if (d_pst.download(np.int32, n) != 0).any():
        raise SystemExit("read_reply_probe: the seal of form (b) failed")
    for k in sorted({0, 1, n // 2, n - 1}):
        record = img.download(np.uint8, rec, int(rec_off[k])).tobytes()
        info = bytearray(record[:FI])
        struct.pack_into("<i", info, 12, FILE)
        body = struct.pack("<i", FILE) + record[FI:] + struct.pack("<i", FI) + bytes(info)
        c = zlib.crc32(body, FLAG ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
        want = struct.pack("<IihhQI", FLAG, len(body), 39, 2, 1000 + k, c) + body
        got = d_out.download(np.uint8, frame_len, int(jobs["frame_offset"][k])).tobytes()
        if got != want or int(res["frame_crc"][k]) != c:
            raise SystemExit("read_reply_probe: frame %d differs from the frame built on the host" % k)

    # what (a) has that (c) has not, alone: its plan (N x 64 bytes) from page-locked memory to the device
    h_plan = crc.PinnedBuffer(ctx, 64 * n)
    d_plan = crc.DeviceBuffer(ctx, 64 * n)
    st = ctx.stream

    def upload():
        ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, d_plan.ptr, h_plan.ptr, 64 * n, st), "memcpy")

    forms = {"a_read_reply": form_a, "b_compact_then_seal": form_b, "c_compact_alone": form_c,
             "a_frames_on_the_payload_mod_128": form_a128, "plan_upload_alone": upload}
    times = {name: [] for name in forms}
    host = {name: [] for name in forms}   # the calling thread's time in the REPS calls of a round, per call
    e0, e1 = crc.Event(ctx), crc.Event(ctx)
    for _ in range(rounds):
        for name, call in forms.items():
            call()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            host[name].append((time.perf_counter() - t0) / REPS * 1e3)
            e1.record()
            ctx.sync()
            times[name].append(e0.elapsed_ms(e1) / REPS)
    if int(d_bad.download(np.uint32, 1)[0]) != 0:
        raise SystemExit("read_reply_probe: CRC mismatches during the timed calls")
    ab = {name: spread(v) for name, v in times.items()}
    payload = n * FILE
    bytes_moved = {
        "a_read_reply": {"read": n * rec + n * 64, "written": n * frame_len + n * 16},
        "b_compact_then_seal": {"read": n * rec + n * 40 + n * frame_len + n * 16, "written": n * rec + n * 4 + n * 12},
        "c_compact_alone": {"read": n * rec + n * 40, "written": n * rec + n * 4},
    }
    a, b, c = (ab[k]["median"] for k in ("a_read_reply", "b_compact_then_seal", "c_compact_alone"))
    larger = max(ab["a_read_reply"]["spread"], ab["b_compact_then_seal"]["spread"])
    out = {
        "tool": "read_reply_probe", "files": n, "file_bytes": FILE, "payload_bytes": payload, "rounds": rounds,
        "reps_per_round": REPS, "pcode": 39, "ms": times, "ab": ab, "bytes": bytes_moved,
        "host_ms_per_call": {name: spread(v) for name, v in host.items()},
        "a_minus_c_ms": a - c, "a_mod_128_over_c": ab["a_frames_on_the_payload_mod_128"]["median"] / c, "plan_upload_alone_ms": ab["plan_upload_alone"]["median"],
        "payload_multiples_moved": {k: (v["read"] + v["written"]) / payload for k, v in bytes_moved.items()},
        "GBps_of_bytes_moved": {k: (bytes_moved[k]["read"] + bytes_moved[k]["written"]) / (ab[k]["median"] / 1e3) / 1e9
                                for k in bytes_moved},
        "payload_GiBps": {k: payload / (ab[k]["median"] / 1e3) / 2**30 for k in bytes_moved},
        "a_over_b": a / b, "a_over_c": a / c,
        "a_faster_than_b_by_more_than_the_larger_spread": bool(b - a > larger),
        "a_within_3_pct_of_c": bool(a <= 1.03 * c),
    }
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "read_reply_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
