#!/usr/bin/env python3
"""Replicate sessions (include/tfs_replicate.h) against what a caller could
compose before for the same bytes, in one process, device-resident.  Measurement only;
bench.py and benchlines/ are not involved.

The workload's own shape: a block's data file of 64 MiB holding records of 64 KiB, sent in
frames of MAX_READ_SIZE (1 MiB) by calls of 8 frames, as ReplicateTask::do_replicate's loop
does; B blocks per timed window (B = 16: 1 GiB), one session per block.

  (a) a replicate session per block: begin (the plan, on the host), 8 calls of 8 frames, finish
      (every record's verdict) and free;
  (a1) the same with the whole data file in one call of 64 frames (what the loop's shape costs);
  (b) what the library had: tfs_block_verify_device over the image, a device copy of each 1 MiB
      piece into its frame's place, the frame headers, then tfs_packet_seal_device over the 64
      frames (three reads and one write of every byte; the 36 bytes of WriteDataInfo and flag_
      around the data are not written, so (b) does a little less than the real thing);
  (c) one device copy of the data file (one read, one write: the floor of any form).

The forms alternate round by round.  A round runs one warm-up block and then B blocks back to
back under a host clock that ends in a device synchronise ((a)'s finish synchronises; (b) and
(c) synchronise after each block, as a caller that needs the verdicts before the commit
does).  (a)'s time is also split by the calling thread's clock into begin, the frames calls
and finish + free.  Before timing, (a)'s verdicts are checked (every status 0) and sampled
frames are compared byte for byte with frames built here (zlib).  Writes
profiles/replicate_probe.json.

  python tools/replicate_probe.py [ROUNDS] [BLOCKS]
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

FI, FILE, FL, PER = 36, 65536, 1 << 20, 8
FLAG = 0x4E534654
TOTAL = 64 << 20


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med,
            "unit": "ms"}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    if rounds < 8:
        raise SystemExit("replicate_probe: at least 8 rounds")
    ctx = crc.Context(0)
    rec = FI + FILE
    n = TOTAL // rec                      # records; the rest of the data file is a trailing gap
    img = crc.DeviceBuffer(ctx, TOTAL + 4096)
    ctx.synth_fill_device(img, TOTAL, 0x5EAD, 0)
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
    metas = np.zeros(n, crc.META_DTYPE)
    metas["file_id"], metas["offset"], metas["size"] = 1 + np.arange(n), rec_off, rec
    d_metas = crc.DeviceBuffer(ctx, metas.nbytes).upload(metas)
    cfg = crc.replicate_cfg(TOTAL, FL, block_id=4711, packet_id=1000)
    nfr = crc.replicate_frame_count(cfg)
    stride = FL + 60
    d_out = crc.DeviceBuffer(ctx, nfr * stride + 64)     # a block's frames side by side, so that they can be checked
    split = {"begin": [], "frames": [], "finish_free": []}

    def form_a(keep=None, per=PER):
        t0 = time.perf_counter()
        s = crc.ReplicateSession(ctx, cfg, metas)
        t1 = time.perf_counter()
        for off in range(0, TOTAL, per * FL):
            ln = min(per * FL, TOTAL - off)
            s.frames_device(img.ptr + off, off, ln, d_out.ptr + (off // FL) * stride, per * stride)
        t2 = time.perf_counter()
        res = s.finish()
        s.close()
        t3 = time.perf_counter()
        if keep is not None:
            keep.append((t1 - t0, t2 - t1, t3 - t2))
        return res

    # (b): verify, copy each piece into its frame's place, write the headers, seal
    d_st, d_vc = crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4 * n)
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.zero()
    d_frames = crc.DeviceBuffer(ctx, nfr * stride + 64)
    foff = np.arange(nfr, dtype=np.uint64) * stride
    d_foff = crc.DeviceBuffer(ctx, foff.nbytes).upload(foff)
    d_blen = crc.DeviceBuffer(ctx, 4 * nfr).upload(np.full(nfr, FL + 36, np.uint32))
    pd = np.zeros(nfr, crc.PACKET_DESC_DTYPE)
    pd["offset"], pd["len"] = foff, FL + 60
    d_pd = crc.DeviceBuffer(ctx, pd.nbytes).upload(pd)
    d_pcrc, d_pst = crc.DeviceBuffer(ctx, 4 * nfr), crc.DeviceBuffer(ctx, 4 * nfr)
    st = ctx.stream

    def form_b():
        ctx.block_verify_device(img, TOTAL, d_metas, n, d_vc, d_st, d_bad)
        for k in range(nfr):
            ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, d_frames.ptr + k * stride + 56, img.ptr + k * FL, FL, st), "memcpy")
        ctx.write_packet_headers_device(d_frames, d_foff, d_blen, nfr, 35, 2, 1000)
        ctx.packet_seal_device(d_pd, nfr, d_frames, d_pcrc, d_pst)
        ctx.sync()

    d_copy = crc.DeviceBuffer(ctx, TOTAL + 4096)

    def form_c():
        ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, d_copy.ptr, img.ptr, TOTAL, st), "memcpy")
        ctx.sync()

    # correctness before the clock
    vc, vst, nbad, fcrc = form_a()
    form_b()
    if nbad or vst.any() or int(d_bad.download(np.uint32, 1)[0]) != 0:
        raise SystemExit("replicate_probe: a clean record did not verify")
    if (d_pst.download(np.int32, nfr) != 0).any() or (d_vc.download(np.uint32, n) != vc).any():
        raise SystemExit("replicate_probe: form (b) disagrees")
    for k in sorted({0, 1, nfr // 2, nfr - 1}):
        data = img.download(np.uint8, FL, k * FL).tobytes()
        body = struct.pack("<IQiiiQ", 4711, 0, k * FL, FL, 0, 0) + data + struct.pack("<i", 1 if k == 0 else 0)
        c = zlib.crc32(body, FLAG ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
        want = struct.pack("<IihhQI", FLAG, len(body), 35, 2, 1000 + k, c) + body
        got = d_out.download(np.uint8, FL + 60, k * stride).tobytes()
        if got != want or int(fcrc[k]) != c:
            raise SystemExit("replicate_probe: frame %d differs from the frame built on the host" % k)

    forms = {"a_replicate_session": form_a, "a1_one_call_per_block": lambda: form_a(None, nfr),
             "b_verify_copy_seal": form_b, "c_device_copy_alone": form_c}
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name, call in forms.items():
            call()
            ctx.sync()
            keep = [] if name == "a_replicate_session" else None
            t0 = time.perf_counter()
            for _ in range(blocks):
                call(keep) if keep is not None else call()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / blocks * 1e3)
            if keep:
                for key, col in zip(("begin", "frames", "finish_free"), zip(*keep)):
                    split[key].append(sum(col) / len(col) * 1e3)
    ab = {name: spread(v) for name, v in times.items()}
    a, b, c = (ab[k]["median"] for k in ("a_replicate_session", "b_verify_copy_seal", "c_device_copy_alone"))
    larger = max(ab["a_replicate_session"]["spread"], ab["b_verify_copy_seal"]["spread"])
    bytes_moved = {
        "a_replicate_session": {"read": TOTAL, "written": TOTAL + 60 * nfr},
        "b_verify_copy_seal": {"read": n * rec + TOTAL + TOTAL + 36 * nfr, "written": TOTAL + 24 * nfr},
        "c_device_copy_alone": {"read": TOTAL, "written": TOTAL},
    }
    out = {
        "tool": "replicate_probe", "data_file_bytes": TOTAL, "records": n, "record_bytes": rec, "frame_len": FL,
        "frames_per_call": PER, "blocks_per_window": blocks, "rounds": rounds, "ms_per_block": times, "ab": ab,
        "a_split_ms_per_block": {k: spread(v) for k, v in split.items()}, "bytes_per_block": bytes_moved,
        "data_GiBps": {k: TOTAL / (ab[k]["median"] / 1e3) / 2**30 for k in forms},
        "a_over_b": a / b, "a_over_c": a / c,
        "a_faster_than_b_by_more_than_the_larger_spread": bool(b - a > larger),
    }
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "replicate_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
