#!/usr/bin/env python3
"""File repair (include/tfs_repair.h) against the same work composed from the
calls the library had before it, in one process on one GPU, device-resident.  Measurement only;
bench.py and benchlines/ are not involved.

Two shapes: 1,024 files of 64 KiB, one reply frame and one outgoing frame each; one file of 8 MiB
fetched in 1 MiB reply frames and sent in 1 MiB frames.  Two ds entries a frame, pcode 8, version 2.

  (a) tfs_repair_frames_device: one call for the batch;
  (b) tfs_packet_verify_device over the incoming frames, one device copy per incoming frame that
      gathers each file's data behind a 36-byte FileInfo (prepared beforehand), then
      tfs_mirror_frames_device with first_len = frame_len over that image (three reads and two
      writes of every payload byte).

The forms alternate round by round; each run is timed with device events on the context's
stream, after warm-up rounds of both; (a)'s time on the calling thread (checks, plan, enqueue) is
taken beside it, since the device waits for it.  Before timing, (a)'s results are checked (every
status 0, file_crc == zlib's) and (a)'s out is compared byte for byte with (b)'s.  Writes
profiles/repair_probe.json.

  python tools/repair_probe.py [RUNS]
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
DS = np.array([0x0A0A0A0A00001F90, 0x0A0A0A0B00001F90], np.uint64)
HEAD = 60 + 8 * len(DS)


def zcrc(seed, data):
    return zlib.crc32(data, seed ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med,
            "unit": "ms"}


def probe_shape(ctx, name, sizes, in_len, frame_len, runs, warm):
    n = len(sizes)
    rng = np.random.default_rng(17)
    # the source: sealed reply frames, each frame's data on a 16-byte boundary
    parts, ins, at = [], [], 0
    jobs = np.zeros(n, crc.REPAIR_JOB_DTYPE)
    fcrc = np.zeros(n, np.uint32)
    image_parts, rec_off, img_at = [], np.zeros(n, np.uint64), 0
    gathers = []  # (offset in the image, offset in the source, bytes): form (b)'s copies
    for i, size in enumerate(sizes):
        pay = rng.integers(0, 256, int(size), dtype=np.uint8).tobytes()
        fcrc[i] = zcrc(0, pay)
        jobs["in_first"][i] = len(ins)
        for off in range(0, int(size), in_len):
            data = pay[off:off + in_len]
            body = struct.pack("<i", len(data)) + data
            pad = (16 - (at + 28) % 16) % 16
            parts.append(b"\0" * pad)
            at += pad
            f = struct.pack("<IihhQI", FLAG, len(body), 8, 2, 7000 + len(ins), zcrc(FLAG, body)) + body
            rc, d = crc.repair_parse(np.frombuffer(f, np.uint8), 8, off == 0, frame_off=at)
            assert rc == 0
            ins.append(d[0].copy())
            gathers.append((img_at + FI + off, at + 28, len(data)))
            parts.append(f)
            at += len(f)
        jobs["in_count"][i] = len(ins) - int(jobs["in_first"][i])
        fi = np.zeros(1, crc.FILEINFO_DTYPE)
        fi["id_"], fi["offset_"], fi["size_"], fi["usize_"], fi["crc_"] = 1 + i, img_at, size + FI, size + FI, fcrc[i]
        rec_off[i] = img_at
        image_parts += [fi.tobytes(), b"\0" * (int(size) + (-(int(size) + FI)) % 16)]
        img_at += FI + int(size) + (-(int(size) + FI)) % 16
    src = np.frombuffer(b"".join(parts), np.uint8)
    ins = np.array(ins, crc.REPAIR_IN_DTYPE)
    payload = int(np.sum(sizes))
    cfg = crc.repair_cfg(frame_len)
    jobs["file_id"], jobs["stat_size"], jobs["stat_crc"], jobs["check_crc"] = 1 + np.arange(n), sizes, fcrc, fcrc
    jobs["file_number"] = 0x700000 + np.arange(n)
    jobs["packet_id"] = 1000 + 16 * np.arange(n)
    jobs["block_id"], jobs["ds_first"], jobs["ds_count"] = 4711, 0, len(DS)
    out_at = 0
    for i in range(n):
        out_at += (-(out_at + HEAD)) % 16  # the first frame's data on a 16-byte boundary, as the source's
        jobs["frame_offset"][i] = out_at
        out_at += crc.repair_span(cfg, jobs[i:i + 1])
    cap = out_at + 64
    nfr = sum(crc.repair_frame_count(cfg, int(s)) for s in sizes)

    d_src = crc.DeviceBuffer(ctx, src.size + 4096).upload(src)
    d_out = crc.DeviceBuffer(ctx, cap)
    d_res = crc.DeviceBuffer(ctx, 24 * n)
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.zero()

    def form_a():
        ctx.repair_frames_device(cfg, d_src, src.size, ins, jobs, DS, d_out, cap, d_res, d_bad)

    # (b): verify the incoming frames, gather the data behind the FileInfos, mirror
    pd = np.zeros(len(ins), crc.PACKET_DESC_DTYPE)
    pd["offset"], pd["len"] = ins["frame_off"], ins["avail"]
    d_pd = crc.DeviceBuffer(ctx, pd.nbytes).upload(pd)
    d_pcrc, d_pst = crc.DeviceBuffer(ctx, 4 * len(ins)), crc.DeviceBuffer(ctx, 4 * len(ins))
    d_bad_b = crc.DeviceBuffer(ctx, 4)
    d_bad_b.zero()
    d_img = crc.DeviceBuffer(ctx, img_at + 4096).upload(np.frombuffer(b"".join(image_parts), np.uint8))
    mcfg = crc.mirror_cfg(frame_len, frame_len)
    mjobs = np.zeros(n, crc.MIRROR_JOB_DTYPE)
    for k in ("frame_offset", "file_id", "file_number", "packet_id", "block_id", "ds_first", "ds_count"):
        mjobs[k] = jobs[k]
    mjobs["src_offset"], mjobs["size"] = rec_off, np.asarray(sizes) + FI
    d_out_b = crc.DeviceBuffer(ctx, cap)
    d_res_b = crc.DeviceBuffer(ctx, 16 * n)
    st = ctx.stream
    copies = [(d_img.ptr + io, d_src.ptr + so, ln) for io, so, ln in gathers]

    def form_b():
        ctx.packet_verify_device(d_pd, len(ins), d_src, d_pcrc, d_pst, d_bad_b)
        for dst, s, ln in copies:
            ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, dst, s, ln, st), "memcpy")
        ctx.mirror_frames_device(mcfg, d_img, img_at, mjobs, DS, d_out_b, cap, d_res_b, d_bad_b)

    # correctness before the clock
    d_out.upload(np.zeros(cap, np.uint8))
    d_out_b.upload(np.zeros(cap, np.uint8))
    form_a()
    form_b()
    ctx.sync()
    res = d_res.download(crc.REPAIR_RESULT_DTYPE, n)
    res_b = d_res_b.download(crc.MIRROR_RESULT_DTYPE, n)
    if res["status"].any() or res_b["status"].any() or int(d_bad.download(np.uint32, 1)[0]) or \
            int(d_bad_b.download(np.uint32, 1)[0]) or (d_pst.download(np.int32, len(ins)) != 0).any():
        raise SystemExit("repair_probe %s: a clean file did not verify" % name)
    if (res["file_crc"] != fcrc).any() or (res_b["file_crc"] != fcrc).any():
        raise SystemExit("repair_probe %s: a file CRC differs from zlib's" % name)
    if not (d_out.download(np.uint8, out_at) == d_out_b.download(np.uint8, out_at)).all():
        raise SystemExit("repair_probe %s: (a)'s frames differ from (b)'s" % name)

    forms = {"a_repair_frames": form_a, "b_verify_gather_mirror": form_b}
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
                if key == "a_repair_frames":
                    host_a.append((t1 - t0) * 1e3)
    ab = {k: spread(v) for k, v in times.items()}
    a, b = (ab[k]["median"] for k in forms)
    larger = max(ab["a_repair_frames"]["spread"], ab["b_verify_gather_mirror"]["spread"])
    out = {
        "files": n, "payload_bytes": payload, "incoming_frames": len(ins), "outgoing_frames": nfr, "runs": runs,
        "warmup": warm, "ms": times, "ab": ab, "a_host_call_ms": spread(host_a),
        "payload_GiBps": {k: payload / (ab[k]["median"] / 1e3) / 2**30 for k in forms},
        "a_over_b_median": a / b, "a_over_b_min": ab["a_repair_frames"]["min"] / ab["b_verify_gather_mirror"]["min"],
        "a_faster_than_b_by_more_than_the_larger_spread": bool(b - a > larger),
    }
    for buf in (d_src, d_out, d_res, d_bad, d_pd, d_pcrc, d_pst, d_bad_b, d_img, d_out_b, d_res_b):
        buf.free()
    return out


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    if runs < 20:
        raise SystemExit("repair_probe: at least 20 runs")
    ctx = crc.Context(0)
    mib = 1 << 20
    shapes = {
        "files_1024_x_64KiB": (np.full(1024, 65536), mib, mib),
        "one_file_8MiB_in_1MiB_frames": (np.array([8 * mib]), mib, mib),
    }
    out = {"tool": "repair_probe", "ds_per_frame": len(DS),
           "shapes": {k: probe_shape(ctx, k, s, il, fl, runs, 4) for k, (s, il, fl) in shapes.items()}}
    out["goal_a_faster_than_b"] = {k: v["a_faster_than_b_by_more_than_the_larger_spread"] for k, v in out["shapes"].items()}
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "repair_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
