#!/usr/bin/env python3
"""Frame-emitting chunk calls of the marshalling and reinstate sessions (include/
tfs_ec_frames.h) against the composition the library offered before
them for the same frames: the session's plain chunk call into chunk buffers, then one
record-less tfs_replicate session per output member that reads the coded chunk again,
copies it into a frame and seals it.  One process, measurement only; bench.py and
benchlines/ are not involved.

k = 5, m = 3; 64 MiB members of 1,024 records of 64 KiB, device-resident; the
reference's loop: 64 chunks of 1 MiB, frames of 1 MiB, the chunk and frame buffers
reused chunk after chunk.

  (a) marshalling: three parity members leave as TFS_RAW_PARITY_DATA frames    [gated]
  (b) reinstate: data members 0 and 2 and parity member 1 are dead             [gated]
  (w) no gate: the whole member in one call (len == total) beside tfs_ec_encode_device
      and one seal session per parity member

A task is timed whole on the host clock, from the first begin to the end of the last
finish and free, the device idle before and after: the composition's 1 + pn begins,
folds and finishes are what the fused form drops, so they belong inside.  The chunk
loop alone is also timed between HIP events.  The two forms alternate round by round
after a warm-up round of each.  Before any timing both forms' frames are compared byte
for byte, chunk by chunk, and the records' verdicts too.  Gate: the fused form's median
is no more than the composition's median plus the composition's own round-to-round
spread.

  python tools/ec_frames_probe.py [ROUNDS [CASES, e.g. "ab"]]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfs_amd.crc as crc  # noqa: E402
from marshal_probe import block_image, spread  # noqa: E402
from tfs_amd.ec import ErasureCode, MarshalSession, ReinstateSession, frames_cap, frames_cfg  # noqa: E402

K, M = 5, 3
N = K + M
SIZE = 64 << 20
CHUNK = 1 << 20
FRAME = 1 << 20
BIDS = [5000 + i for i in range(N)]
PIDS = [(i + 1) << 40 for i in range(N)]
DEAD = [0, 2, K + 1]


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
        erased = [1 if i in DEAD else 0 for i in range(N)]
        self.dec = ErasureCode(ctx, K, M, erased)
        assert self.enc.rc == 0 and self.dec.rc == 0
        assert self.enc.encode_device(self.ptr, SIZE) == 0  # the stored parity the reinstate reads
        ctx.sync()
        self.cfg = frames_cfg(FRAME, BIDS, PIDS)
        self.cap = frames_cap(self.cfg, CHUNK)
        self.chunk = [crc.DeviceBuffer(ctx, CHUNK) for _ in range(M)]       # the composition's coded pieces
        self.out_a = [crc.DeviceBuffer(ctx, self.cap + 64) for _ in range(M)]  # its frames
        self.out_b = [crc.DeviceBuffer(ctx, self.cap + 64) for _ in range(M)]  # the fused form's frames

    def outputs(self, reinstate):
        return DEAD if reinstate else list(range(K, N))

    def begin(self, reinstate):
        if reinstate:
            return ReinstateSession(self.dec, self.metas, [SIZE] * K, SIZE)
        return MarshalSession(self.enc, self.metas, [SIZE] * K, SIZE)

    def members(self, reinstate, o, outs=None):
        """The chunk's member pointers: sources at their place in the members, outputs None or chunk buffers."""
        dead = self.outputs(reinstate)
        p = [None if i in dead else self.ptr[i] + o for i in range(N)]
        for b, i in zip(outs or [], dead):
            p[i] = b.ptr
        return p

    def composed(self, reinstate, each=None):
        """The session's plain chunk call, then one record-less replicate session per output.  (loop ms, res)"""
        ctx, dead = self.ctx, self.outputs(reinstate)
        ses = self.begin(reinstate)
        reps = [crc.ReplicateSession(ctx, crc.replicate_cfg(SIZE, FRAME, BIDS[i], PIDS[i],
                                                            crc.RAW_PARITY_DATA if i >= K else crc.RAW_NORMAL_DATA, 2,
                                                            frame_stride=FRAME + 64)) for i in dead]
        assert ses.rc == 0
        call = ses.decode_device if reinstate else ses.encode_device
        e0, e1 = crc.Event(ctx), crc.Event(ctx)
        e0.record()
        for o in range(0, SIZE, CHUNK):
            assert call(self.members(reinstate, o, self.chunk), o, CHUNK) == 0
            for r, src, out in zip(reps, self.chunk, self.out_a):
                r.frames_device(src, o, CHUNK, out, self.cap)
            if each:
                each(o, self.out_a)
        e1.record()
        res = ses.finish()
        for r in reps:
            r.finish()
            r.close()
        ses.free()
        ctx.sync()
        return e0.elapsed_ms(e1), res

    def fused(self, reinstate, each=None):
        ctx, dead = self.ctx, self.outputs(reinstate)
        ses = self.begin(reinstate)
        assert ses.rc == 0
        outl = [None] * N
        for b, i in zip(self.out_b, dead):
            outl[i] = b.ptr
        e0, e1 = crc.Event(ctx), crc.Event(ctx)
        e0.record()
        for o in range(0, SIZE, CHUNK):
            assert ses.frames_device(self.cfg, self.members(reinstate, o), outl, self.cap, o, CHUNK) == 0
            if each:
                each(o, self.out_b)
        e1.record()
        res = ses.finish()
        ses.free()
        ctx.sync()
        return e0.elapsed_ms(e1), res

    def agree(self, reinstate):
        """Both forms' frames, chunk by chunk, and the verdicts."""
        ctx = self.ctx
        seen = {}

        def keep(tag):
            def f(o, outs):
                ctx.sync()
                seen[(tag, o)] = [b.download(np.uint8, self.cap) for b in outs]
            return f
        _, ra = self.composed(reinstate, keep("a"))
        _, rb = self.fused(reinstate, keep("b"))
        for o in range(0, SIZE, CHUNK):
            for x, y in zip(seen[("a", o)], seen[("b", o)]):
                if not (x == y).all():
                    raise SystemExit("ec_frames_probe: the two forms' frames differ at %d" % o)
        if not ((ra[0] == rb[0]).all() and (ra[1] == rb[1]).all() and (rb[1] == 0).all() and ra[3] == 0 and rb[3] == 0):
            raise SystemExit("ec_frames_probe: the two forms' verdicts differ")

    def run(self, reinstate, rounds):
        self.agree(reinstate)
        t = {"composed": [], "fused": [], "composed_loop": [], "fused_loop": []}
        for form in (self.composed, self.fused):  # warm-up
            form(reinstate)
        for _ in range(rounds):
            for name, form in (("composed", self.composed), ("fused", self.fused)):
                self.ctx.sync()
                t0 = time.perf_counter()
                loop, _ = form(reinstate)
                t[name].append(1e3 * (time.perf_counter() - t0))
                t[name + "_loop"].append(loop)
        res = {k: dict(spread(v), unit="ms") for k, v in t.items()}
        c, f = res["composed"], res["fused"]
        res["fused_over_composed"] = f["median"] / c["median"]
        res["fused_loop_over_composed_loop"] = res["fused_loop"]["median"] / res["composed_loop"]["median"]
        res["per_chunk_us"] = {"composed": 1e3 * res["composed_loop"]["median"] / (SIZE // CHUNK),
                               "fused": 1e3 * res["fused_loop"]["median"] / (SIZE // CHUNK)}
        res["within_composed_median_plus_spread"] = bool(f["median"] <= c["median"] + c["spread"])
        return {"rounds": rounds, "chunks": SIZE // CHUNK, "outputs": self.outputs(reinstate), "ms": t, "ab": res}

    def whole(self, rounds):
        """No gate: len == total in one call beside tfs_ec_encode_device and one seal session per parity member."""
        ctx = self.ctx
        cfg = frames_cfg(FRAME, BIDS, PIDS)
        cap = frames_cap(cfg, SIZE)
        outs = [crc.DeviceBuffer(ctx, cap + 64) for _ in range(M)]
        par = [crc.DeviceBuffer(ctx, SIZE) for _ in range(M)]
        t = {"encode_then_seal": [], "fused": []}

        def old():
            assert self.enc.encode_device(self.ptr[:K] + [b.ptr for b in par], SIZE) == 0
            for j, i in enumerate(range(K, N)):
                with crc.ReplicateSession(ctx, crc.replicate_cfg(SIZE, FRAME, BIDS[i], PIDS[i], crc.RAW_PARITY_DATA, 2,
                                                                 frame_stride=FRAME + 64)) as r:
                    r.frames_device(par[j], 0, SIZE, outs[j], cap)
                    r.finish()
            ctx.sync()

        def new():
            ses = MarshalSession(self.enc, self.metas, [SIZE] * K, SIZE)
            assert ses.frames_device(cfg, self.ptr[:K] + [None] * M, [None] * K + [b.ptr for b in outs], cap, 0, SIZE) == 0
            res = ses.finish()
            ses.free()
            ctx.sync()
            return res
        for b in outs:
            b.zero()
        old()
        a = [b.download(np.uint8, cap) for b in outs]
        for b in outs:
            b.zero()
        res = new()
        if not all((x == b.download(np.uint8, cap)).all() for x, b in zip(a, outs)) or res[2] != 0:
            raise SystemExit("ec_frames_probe: the whole-member forms differ")
        for _ in range(rounds):
            for name, form in (("encode_then_seal", old), ("fused", new)):
                ctx.sync()
                t0 = time.perf_counter()
                form()
                t[name].append(1e3 * (time.perf_counter() - t0))
        for b in outs + par:
            b.free()
        res = {k: dict(spread(v), unit="ms") for k, v in t.items()}
        res["fused_over_encode_then_seal"] = res["fused"]["median"] / res["encode_then_seal"]["median"]
        res["note"] = "the fused form also verifies 5,120 records; encode_then_seal verifies none"
        return {"rounds": rounds, "ms": t, "ab": res}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    if rounds < 5:
        raise SystemExit("ec_frames_probe: at least 5 alternations")
    cases = sys.argv[2] if len(sys.argv) > 2 else "abw"
    ctx = crc.Context(0)
    p = Probe(ctx)
    res = {"tool": "ec_frames_probe", "k": K, "m": M, "member_bytes": SIZE, "chunk_bytes": CHUNK, "frame_len": FRAME}
    if "a" in cases:
        res["a_marshalling"] = p.run(False, rounds)
        res["acceptance_a"] = res["a_marshalling"]["ab"]["within_composed_median_plus_spread"]
    if "b" in cases:
        res["b_reinstate"] = p.run(True, rounds)
        res["acceptance_b"] = res["b_reinstate"]["ab"]["within_composed_median_plus_spread"]
    if "w" in cases:
        res["w_whole_member"] = p.whole(rounds)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
