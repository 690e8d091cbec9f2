#!/usr/bin/env python3
"""Receive sessions (include/tfs_receive.h) against what a caller could compose
before for the same bytes, in one process on the same buffers, device-resident.  Measurement
only; bench.py and benchlines/ are not involved.

The workload's own shape: a block's data file of 64 MiB holding records of 64 KiB, received as
WriteRawDataMessage frames of MAX_READ_SIZE (1 MiB) in calls of 8 frames; B blocks per timed
window (B = 16: 1 GiB), one session per block.  The frames are sealed once, before the clock, by
a replicate session.

  (a) a receive session per block: begin, 8 calls of 8 frames, finish (every record's verdict)
      and free;
  (a1) the same with all 64 frames in one call (what the calls' shape costs);
  (b) what the library had: tfs_packet_verify_device over the 64 frames, a device copy of each
      frame's data into the image, tfs_block_verify_device over the landed image (three reads
      and one write of every byte);
  (c) one device copy of the data file (one read, one write: the floor of any form).

The forms alternate round by round.  A round runs one warm-up block and then B blocks back to
back under a host clock that ends in a device synchronise ((a)'s finish synchronises; (b) and
(c) synchronise after each block, as a caller that needs the verdicts before the commit does).
(a)'s time is also split by the calling thread's clock into begin, the frames calls and
finish + free.  Before timing, (a)'s outcomes are checked: every frame status 0 with the
replicate session's frame CRC, every record status 0 with (b)'s CRC, and the landed image equal
to the source.  Writes profiles/receive_probe.json.

  python tools/receive_probe.py [ROUNDS] [BLOCKS]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402

FI, FILE, FL, PER = 36, 65536, 1 << 20, 8
TOTAL = 64 << 20
BLOCK = 4711


def spread(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return {"median": med, "min": v[0], "max": v[-1], "spread": v[-1] - v[0], "spread_pct": 100.0 * (v[-1] - v[0]) / med,
            "unit": "ms"}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    if rounds < 8:
        raise SystemExit("receive_probe: at least 8 rounds")
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
    # the frames, sealed by a replicate session
    rcfg = crc.replicate_cfg(TOTAL, FL, block_id=BLOCK, packet_id=1000)
    nfr = crc.replicate_frame_count(rcfg)
    stride = FL + 60
    d_frames = crc.DeviceBuffer(ctx, nfr * stride + 64)
    with crc.ReplicateSession(ctx, rcfg, metas) as rs:
        rs.frames_device(img, 0, TOTAL, d_frames, nfr * stride)
        _, rst, _, fcrc = rs.finish()
    if rst.any():
        raise SystemExit("receive_probe: the source block does not verify")
    descs = np.zeros(nfr, crc.RECEIVE_DESC_DTYPE)
    descs["frame_off"], descs["avail"] = np.arange(nfr, dtype=np.uint64) * stride, stride
    descs["data_offset"], descs["data_len"] = np.arange(nfr) * FL, FL
    d_image = crc.DeviceBuffer(ctx, TOTAL + 4096)
    d_parts = crc.DeviceBuffer(ctx, 16 * nfr)
    d_bad = crc.DeviceBuffer(ctx, 4)
    d_bad.zero()
    rx_cfg = crc.receive_cfg(TOTAL, BLOCK)
    split = {"begin": [], "frames": [], "finish_free": []}

    def form_a(keep=None, per=PER):
        t0 = time.perf_counter()
        s = crc.ReceiveSession(ctx, rx_cfg, d_image)
        t1 = time.perf_counter()
        for k in range(0, nfr, per):
            s.frames_device(d_frames, descs[k:k + per], d_parts.ptr + 16 * k, d_bad)
        t2 = time.perf_counter()
        res = s.finish(metas)
        s.close()
        t3 = time.perf_counter()
        if keep is not None:
            keep.append((t1 - t0, t2 - t1, t3 - t2))
        return res

    # (b): verify the frames, copy each frame's data into the image, verify the landed image
    pd = np.zeros(nfr, crc.PACKET_DESC_DTYPE)
    pd["offset"], pd["len"] = descs["frame_off"], stride
    d_pd = crc.DeviceBuffer(ctx, pd.nbytes).upload(pd)
    d_pcrc, d_pst = crc.DeviceBuffer(ctx, 4 * nfr), crc.DeviceBuffer(ctx, 4 * nfr)
    d_st, d_vc = crc.DeviceBuffer(ctx, 4 * n), crc.DeviceBuffer(ctx, 4 * n)
    d_vbad = crc.DeviceBuffer(ctx, 4)
    d_vbad.zero()
    d_image_b = crc.DeviceBuffer(ctx, TOTAL + 4096)
    st = ctx.stream

    def form_b():
        ctx.packet_verify_device(d_pd, nfr, d_frames, d_pcrc, d_pst, d_vbad)
        for k in range(nfr):
            ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, d_image_b.ptr + k * FL, d_frames.ptr + k * stride + 56, FL, st),
                       "memcpy")
        ctx.block_verify_device(d_image_b, TOTAL, d_metas, n, d_vc, d_st, d_vbad)
        ctx.sync()

    d_copy = crc.DeviceBuffer(ctx, TOTAL + 4096)

    def form_c():
        ctx._check(ctx.L.tfs_crc32_memcpy(ctx.handle, d_copy.ptr, img.ptr, TOTAL, st), "memcpy")
        ctx.sync()

    # correctness before the clock
    vc, vst, nbad, total = form_a()
    form_b()
    parts = d_parts.download(crc.RECEIVE_PART_DTYPE)
    if total != TOTAL or nbad or vst.any() or parts["status"].any() or int(d_bad.download(np.uint32, 1)[0]):
        raise SystemExit("receive_probe: a clean frame or record did not verify")
    if (parts["crc"] != fcrc).any() or (d_pcrc.download(np.uint32, nfr) != fcrc).any():
        raise SystemExit("receive_probe: a frame CRC differs from the sender's")
    if (d_vc.download(np.uint32, n) != vc).any() or d_st.download(np.int32, n).any() or d_pst.download(np.int32, nfr).any():
        raise SystemExit("receive_probe: form (b) disagrees")
    for off in range(0, TOTAL, 8 << 20):
        if (d_image.download(np.uint8, 8 << 20, off) != img.download(np.uint8, 8 << 20, off)).any():
            raise SystemExit("receive_probe: the landed image differs from the source")

    forms = {"a_receive_session": form_a, "a1_one_call_per_block": lambda: form_a(None, nfr),
             "b_verify_copy_verify": form_b, "c_device_copy_alone": form_c}
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name, call in forms.items():
            call()
            ctx.sync()
            keep = [] if name == "a_receive_session" else None
            t0 = time.perf_counter()
            for _ in range(blocks):
                call(keep) if keep is not None else call()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / blocks * 1e3)
            if keep:
                for key, col in zip(("begin", "frames", "finish_free"), zip(*keep)):
                    split[key].append(sum(col) / len(col) * 1e3)
    ab = {name: spread(v) for name, v in times.items()}
    a, b, c = (ab[k]["median"] for k in ("a_receive_session", "b_verify_copy_verify", "c_device_copy_alone"))
    larger = max(ab["a_receive_session"]["spread"], ab["b_verify_copy_verify"]["spread"])
    G = crc.receive_granule()
    edge = n * (2 * (G - 1) + FI)          # at most, per record
    bytes_moved = {
        "a_receive_session": {"read": TOTAL + 60 * nfr, "written": TOTAL, "finish_reread_at_most": edge},
        "b_verify_copy_verify": {"read": TOTAL + 60 * nfr + TOTAL + n * rec, "written": TOTAL},
        "c_device_copy_alone": {"read": TOTAL, "written": TOTAL},
    }
    out = {
        "tool": "receive_probe", "granule": G, "data_file_bytes": TOTAL, "records": n, "record_bytes": rec,
        "frame_len": FL, "frames_per_call": PER, "blocks_per_window": blocks, "rounds": rounds, "ms_per_block": times,
        "ab": ab, "a_split_ms_per_block": {k: spread(v) for k, v in split.items()}, "bytes_per_block": bytes_moved,
        "data_GiBps": {k: TOTAL / (ab[k]["median"] / 1e3) / 2**30 for k in forms},
        "a_over_b": a / b, "a_over_c": a / c,
        "a_faster_than_b_by_more_than_the_larger_spread": bool(b - a > larger),
    }
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "receive_probe.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
