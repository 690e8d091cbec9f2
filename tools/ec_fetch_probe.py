#!/usr/bin/env python3
"""Task chunk calls of the marshalling and reinstate sessions (include/tfs_ec_fetch.h,
DESIGN.md §3.24) against the composition the library offered before them for the same
work: tfs_packet_verify over the chunk's incoming RespReadRawDataMessage frames, then the
frames chunk call (include/tfs_ec_frames.h) over their data.  One process, measurement
only; bench.py and benchlines/ are not involved.

k = 5, m = 3; 64 MiB members of 1,024 records of 64 KiB; every member's incoming frames
(1 MiB of data each, frame_len + 32 apart, sealed once before any timing) device-resident.

  (a) marshalling, the task's loop: 64 chunks of 1 MiB, one frame per call
  (b) reinstate, the same loop: data members 0 and 2 and parity member 1 are dead
  (A), (B) the whole member in one call: 64 frames per source; the composition then has
      to gather the frames' data into contiguous chunks (one device copy per frame) first

With full frames of one chunk the composition needs no gather: the frames call reads the
data where it lies in the frame, 8-byte aligned.  The two forms alternate round by round
after a warm-up of each; the loop is timed between two device events, the task whole on
the host clock.  Before timing, the two forms' outgoing frames and verdicts are compared.
The plain and the frames chunk loops are timed too, for comparison with
profiles/ec_frames_probe.json.  No gate: the ratios are reported.

  python tools/ec_fetch_probe.py [ROUNDS [CASES, e.g. "abAB"]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tfs_amd.crc as crc  # noqa: E402
from marshal_probe import block_image, spread  # noqa: E402
from tfs_amd.ec import (FETCH_RESULT_DTYPE, ErasureCode, MarshalSession, ReinstateSession, fetch_cfg,  # noqa: E402
                        frames_cap, frames_cfg)
from tfs_amd.packet import read_raw_reply_frame  # noqa: E402

K, M = 5, 3
N = K + M
SIZE = 64 << 20
FRAME = 1 << 20
NF = SIZE // FRAME
IST = FRAME + 32
BIDS = [5000 + i for i in range(N)]
PIDS = [(i + 1) << 40 for i in range(N)]
DEAD = [0, 2, K + 1]
HBM = 8e12


class Probe:
    def __init__(self, ctx):
        self.ctx = ctx
        self.mem = crc.DeviceBuffer(ctx, N * SIZE)
        self.ptr = [self.mem.ptr + i * SIZE for i in range(N)]
        self.metas = []
        for i in range(K):
            img, mt = block_image(ctx, 1024, 65536, 1 + i)
            self.mem.upload(img, offset=i * SIZE)
            self.metas.append(mt)
        self.enc = ErasureCode(ctx, K, M)
        self.dec = ErasureCode(ctx, K, M, [1 if i in DEAD else 0 for i in range(N)])
        assert self.enc.rc == 0 and self.dec.rc == 0
        assert self.enc.encode_device(self.ptr, SIZE) == 0
        ctx.sync()
        # every member's incoming frames, sealed once: 4 bytes of lead, so that a frame's data is 8-byte aligned
        self.span = NF * IST
        self.inb = crc.DeviceBuffer(ctx, N * (self.span + 64) + 8)
        self.inp = [self.inb.ptr + 4 + i * (self.span + 64) for i in range(N)]
        offs = [j * IST for j in range(NF)]
        for i in range(N):
            member = self.mem.download(np.uint8, SIZE, offset=i * SIZE)
            img = np.zeros(self.span, np.uint8)
            for j in range(NF):
                head = read_raw_reply_frame(b"", SIZE, 2, PIDS[i] + j)
                img[offs[j]:offs[j] + 24] = np.frombuffer(head[:24], np.uint8)
                img[offs[j] + 4:offs[j] + 8] = np.frombuffer(np.uint32(8 + FRAME).tobytes(), np.uint8)
                img[offs[j] + 24:offs[j] + 28] = np.frombuffer(np.uint32(FRAME).tobytes(), np.uint8)
                img[offs[j] + 28:offs[j] + 28 + FRAME] = member[j * FRAME:(j + 1) * FRAME]
                img[offs[j] + 28 + FRAME:offs[j] + 32 + FRAME] = np.frombuffer(np.int32(SIZE).tobytes(), np.uint8)
            ctx.packet_seal(img, offs, [IST] * NF)
            self.inb.upload(img, offset=4 + i * (self.span + 64))
        # the composition's verify descriptors, frame j of member i
        d = np.concatenate([ctx._packet_desc([4 + i * (self.span + 64) + o for o in offs], [IST] * NF) for i in range(N)])
        self.desc_item = d.dtype.itemsize
        self.desc = crc.DeviceBuffer(ctx, d.nbytes).upload(d)
        self.vcrc, self.vst = crc.DeviceBuffer(ctx, 4 * N * NF), crc.DeviceBuffer(ctx, 4 * N * NF)
        self.vbad = crc.DeviceBuffer(ctx, 64)
        self.res = crc.DeviceBuffer(ctx, 16 * K * NF)
        self.gather = crc.DeviceBuffer(ctx, K * SIZE)

    def plan(self, reinstate):
        if not reinstate:
            return list(range(K)), list(range(K, N))
        alive = [i for i in range(N) if i not in DEAD][:K]
        return alive, DEAD

    def begin(self, reinstate):
        cls, ec = (ReinstateSession, self.dec) if reinstate else (MarshalSession, self.enc)
        s = cls(ec, self.metas, [SIZE] * K, SIZE)
        assert s.rc == 0
        return s

    def loop(self, reinstate, form, fpc, outs, cfg, cap):
        """One whole session; form: task | composed | frames | plain.  Returns (loop ms, finish())."""
        ctx = self.ctx
        src, dead = self.plan(reinstate)
        ses = self.begin(reinstate)
        step = fpc * FRAME
        outl = [None] * N
        for b, i in zip(outs, dead):
            outl[i] = b.ptr
        fc = fetch_cfg()
        stream = ctx.L.tfs_crc32_stream(ctx.handle)
        e0, e1 = crc.Event(ctx), crc.Event(ctx)
        e0.record()
        for o in range(0, SIZE, step):
            j0 = o // FRAME
            if form == "task":
                inl = [self.inp[i] + j0 * IST if i in src else None for i in range(N)]
                assert ses.task_device(cfg, fc, inl, outl, cap, self.res, o, step) == 0
                continue
            if form == "composed":
                for i in src:  # the wire check of the chunk's frames
                    at = (i * NF + j0) * self.desc_item
                    ctx.packet_verify_device(self.desc.ptr + at, fpc, self.inb.ptr, self.vcrc.ptr + 4 * (i * NF + j0),
                                             self.vst.ptr + 4 * (i * NF + j0), self.vbad.ptr)
                if fpc == 1:  # the data where it lies in the frame
                    mem = [self.inp[i] + j0 * IST + 28 if i in src else None for i in range(N)]
                else:         # the memcpy out of every frame
                    for s_, i in enumerate(src):
                        for j in range(fpc):
                            ctx.L.tfs_crc32_memcpy(ctx.handle, self.gather.ptr + s_ * SIZE + (j0 + j) * FRAME,
                                                   self.inp[i] + (j0 + j) * IST + 28, FRAME, stream)
                    mem = [self.gather.ptr + src.index(i) * SIZE + o if i in src else None for i in range(N)]
                assert ses.frames_device(cfg, mem, outl, cap, o, step) == 0
                continue
            mem = [self.ptr[i] + o if i in src else None for i in range(N)]
            if form == "frames":
                assert ses.frames_device(cfg, mem, outl, cap, o, step) == 0
            else:
                for b, i in zip(outs, dead):
                    mem[i] = b.ptr
                assert (ses.decode_device if reinstate else ses.encode_device)(mem, o, step) == 0
        e1.record()
        res = ses.finish()
        ses.free()
        ctx.sync()
        return e0.elapsed_ms(e1), res

    def run(self, reinstate, fpc, rounds):
        ctx = self.ctx
        cfg = frames_cfg(FRAME, BIDS, PIDS)
        cap = frames_cap(cfg, fpc * FRAME)
        outs = {f: [crc.DeviceBuffer(ctx, max(cap, fpc * FRAME) + 64) for _ in range(M)] for f in ("task", "composed")}
        got = {}
        for f in ("composed", "task"):  # agreement, on the last chunk's frames and the verdicts
            _, res = self.loop(reinstate, f, fpc, outs[f], cfg, cap)
            got[f] = ([b.download(np.uint8, cap) for b in outs[f]], res)
        for x, y in zip(got["composed"][0], got["task"][0]):
            if not (x == y).all():
                raise SystemExit("ec_fetch_probe: the two forms' frames differ")
        ra, rb = got["composed"][1], got["task"][1]
        r = self.res.download(FETCH_RESULT_DTYPE, K * fpc)
        if not ((ra[0] == rb[0]).all() and (ra[1] == rb[1]).all() and (rb[1] == 0).all() and (r["status"] == 0).all()
                and (r["n"] == FRAME).all()):
            raise SystemExit("ec_fetch_probe: the two forms' verdicts differ")
        if (self.vst.download(np.int32, N * NF) != 0).any():
            raise SystemExit("ec_fetch_probe: the composition's verify refused a frame")
        forms = ["composed", "task", "frames", "plain"]
        t = {f: [] for f in forms}
        t.update({f + "_loop": [] for f in forms})
        for f in forms:
            self.loop(reinstate, f, fpc, outs["task" if f != "composed" else "composed"], cfg, cap)
        for _ in range(rounds):
            for f in forms:
                ctx.sync()
                t0 = time.perf_counter()
                ms, _ = self.loop(reinstate, f, fpc, outs["task" if f != "composed" else "composed"], cfg, cap)
                t[f].append(1e3 * (time.perf_counter() - t0))
                t[f + "_loop"].append(ms)
        for bs in outs.values():
            for b in bs:
                b.free()
        ab = {k: dict(spread(v), unit="ms") for k, v in t.items()}
        ab["task_over_composed"] = ab["task"]["median"] / ab["composed"]["median"]
        ab["task_loop_over_composed_loop"] = ab["task_loop"]["median"] / ab["composed_loop"]["median"]
        ab["task_not_slower"] = bool(ab["task_loop"]["median"] <= ab["composed_loop"]["median"] + ab["composed_loop"]["spread"])
        gather = 0 if fpc == 1 else 2 * K
        moved = {"task": (K + M) * SIZE, "composed": (K + K + gather + M) * SIZE}  # member-sizes read and written
        ab["bytes_moved"] = moved
        ab["fraction_of_8TBps"] = {f: moved[f] / (1e-3 * ab[f + "_loop"]["median"]) / HBM for f in moved}
        return {"rounds": rounds, "frames_per_call": fpc, "calls": NF // fpc, "ms": t, "ab": ab}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    cases = sys.argv[2] if len(sys.argv) > 2 else "abAB"
    ctx = crc.Context(0)
    p = Probe(ctx)
    res = {"tool": "ec_fetch_probe", "k": K, "m": M, "member_bytes": SIZE, "frame_len": FRAME}
    for c, name, reinstate, fpc in (("a", "a_marshalling_loop", False, 1), ("b", "b_reinstate_loop", True, 1),
                                    ("A", "A_marshalling_whole", False, NF), ("B", "B_reinstate_whole", True, NF)):
        if c in cases:
            res[name] = p.run(reinstate, fpc, rounds)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
