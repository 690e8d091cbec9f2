"""The algebra of the degraded read reply, restated lane by lane in Python as
ec_read_reply_kernel is built and checked against the byte loop of the CPU restatement and zlib (CPU only).

The workgroup is the degraded read's (tests/test_degraded_math.py: 8 waves, tiles dealt to waves, the per-lane
chain with the 128-byte step and the tile step, one multiplication by xpow[...]), with four differences restated
here: the tiles come from the job's covering set (tile 0 holds the FileInfo; the slice's tiles count from the
slice's first unit when its units are disjoint from the FileInfo's), bytes outside the slice [D0, D1) are masked
out of the chain, pad is taken from D1, and the fold over the 8 waves yields c = crc(0, D), from which

    crc(FLAG, le32(n) || D)      = pre ^ c,   pre = shift(crc(FLAG, le32(n)), n)   (host)
    crc(FLAG, le32(n) || D || T) = the same carried over T's dwords, one slice-by-4 step each
"""
import struct
import zlib

import numpy as np
import pytest

from conftest import ocrc
from test_degraded_math import BIAS, STEP_PACKET, STEP_TILE, W, XPOW, low_bytes, lut4, mult, shift, slice4

FI = 36
FLAG = 0x4E534654


def zcrc(seed, data):
    return zlib.crc32(bytes(data), seed ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def cover(H, D0, n):
    """reply_cover of tfs_amd/csrc/ec_reply_plan.h: (hA, e0, tb1, e1, nt)."""
    hA, hE = H & ~1023, (H + FI + 1023) & ~1023
    sA, sE = D0 & ~1023, (D0 + n + 1023) & ~1023
    if n and sA <= hE:
        return hA, sE, hA, sE, (sE - hA + 4095) >> 12
    if n:
        return hA, hE, sA - 4096, sE, 1 + ((sE - sA + 4095) >> 12)
    return hA, hE, hA, hE, 1


def emulate(mem, H, read_offset, n):
    """(c, the FileInfo bytes caught in tile 0, the units loaded) as one workgroup has them."""
    D0 = H + FI + read_offset
    D1 = D0 + n
    hA, e0, tb1, e1, nt = cover(H, D0, n)
    pad = tb1 + 4096 * nt - D1
    out, info, units = 0, bytearray(FI), []
    for w in range(W):
        crc = [0] * 64
        for t in range(w, nt, W):
            for lane in range(64):
                pu = (hA if t == 0 else tb1 + 4096 * t) + 1024 * (lane >> 4)
                ok = pu < (e0 if t == 0 else e1)
                if ok and lane & 15 == 0:
                    units.append(pu >> 10)
                base = pu + 8 * (lane & 15)
                c = crc[lane]
                for k in range(8):
                    q = base + 128 * k
                    v = int.from_bytes(mem[q:q + 8], "little") if ok else 0
                    if t == 0 and ok:
                        for b in range(8):
                            if 0 <= q + b - H < FI:
                                info[q + b - H] = (v >> (8 * b)) & 255
                    sk, ek = D0 - q, D1 - q
                    if not (sk <= 0 and ek >= 8):
                        v &= 0 if ek <= sk else low_bytes(ek) & ~low_bytes(sk)
                    piece = slice4(slice4(v & 0xFFFFFFFF) ^ (v >> 32))
                    c = lut4(STEP_TILE if k == 0 else STEP_PACKET, c) ^ piece
                crc[lane] = c
        if w >= nt or n == 0:
            continue
        tl = nt - 1 - ((nt - 1 - w) % W)
        part = 0
        for lane in range(64):
            dl = 4096 * (nt - 1 - tl) + 3192 - 1024 * (lane >> 4) - 8 * (lane & 15)
            assert 0 <= BIAS + dl - pad < len(XPOW)
            part ^= mult(XPOW[BIAS + dl - pad], crc[lane])
        out ^= part
    return out, bytes(info), units


def frame_crc(c, n, info, first):
    """The verdict wave's header CRC of a V2 / V3 reply: pre ^ c carried over the trailer's dwords."""
    pre = shift(zcrc(FLAG, struct.pack("<I", n)), n)
    f = pre ^ c
    words = [FI] + list(struct.unpack("<9I", info)) if first else [0]
    if first:
        words[4] = (words[4] - FI) & 0xFFFFFFFF     # size_ less 36
    assert len(words) <= 10
    for w in words:
        f = slice4(f ^ w)
    return f, pre ^ c


@pytest.fixture(scope="module")
def mem():
    return np.random.default_rng(19).integers(0, 256, 160 * 1024, dtype=np.uint8).tobytes()


def check(oracle, mem, H, ro, n):
    assert H + FI + ro + n + 4096 <= len(mem)
    c, info, units = emulate(mem, H, ro, n)
    D0 = H + FI + ro
    data = mem[D0:D0 + n]
    assert c == zcrc(0, data) == ocrc(oracle, 0, data), (H, ro, n)
    assert info == mem[H:H + FI]
    want = set(range(H >> 10, (H + FI + 1023) >> 10)) | (set(range(D0 >> 10, (D0 + n + 1023) >> 10)) if n else set())
    assert sorted(units) == sorted(want), (H, ro, n)            # each covering unit once, no other
    for first in (True, False):
        if first and ro:
            continue
        fi = bytearray(info)
        struct.pack_into("<i", fi, 12, struct.unpack_from("<i", fi, 12)[0] - FI)
        trailer = struct.pack("<i", FI) + bytes(fi) if first else struct.pack("<i", 0)
        f, head = frame_crc(c, n, info, first)
        assert head == zcrc(FLAG, struct.pack("<I", n) + data)      # pcode 8: no trailer
        assert f == zcrc(FLAG, struct.pack("<I", n) + data + trailer), (H, ro, n, first)
        if n <= 4096:
            assert f == ocrc(oracle, FLAG, struct.pack("<I", n) + data + trailer)


@pytest.mark.parametrize("edge", [8, 1024, 4096, 32768])
def test_slices_around_every_edge(oracle, mem, edge):
    """Slices that start, and slices that end, 0..8 bytes around a piece, unit, tile and eight-tile boundary."""
    H = 1000                                    # the FileInfo straddles a unit edge
    for d in range(-8, 9):
        D0 = (H + FI) // edge * edge + 2 * edge + d if edge < 32768 else 32768 + d
        ro = D0 - (H + FI)
        check(oracle, mem, H, ro, 700)                           # starts around the edge
        start = H + FI + (5 if edge < 32768 else 0)
        D1 = (start // edge + (3 if edge == 8 else 1)) * edge + d
        check(oracle, mem, H, start - (H + FI), D1 - start)      # ends around the edge


def test_no_slice_and_header_placements(oracle, mem):
    for H in (0, 100, 988, 989, 1000, 1023, 4090, 5 * 1024 - 36, 5 * 1024 - 35):
        check(oracle, mem, H, 0, 0)                              # n = 0: the FileInfo's units alone
        check(oracle, mem, H, 77, 0)
        check(oracle, mem, H, 0, 1)
        check(oracle, mem, H, 0, 5000)


def test_header_and_slice_disjoint_and_touching(oracle, mem):
    H = 2000                                                     # FileInfo in unit 1, ends at 2036
    for ro, n in ((12, 100),          # the slice starts in the FileInfo's unit: overlapping sets
                  (2048 - 2036, 50),  # the slice starts with the next unit: touching
                  (3071 - 2036, 2),   # ends one byte into the unit after: still touching
                  (3072 - 2036, 10),  # one unit between: disjoint
                  (3072 - 2036, 4096 * 9 + 5), (40000, 1), (40000, 8192), (65536 - 2036 - 3, 40000),
                  (4096 * 8 + 3072 - 2036, 4096 * 8 + 17)):
        check(oracle, mem, H, ro, n)
    check(oracle, mem, 1020, 2048 - 1056, 3)                     # a two-unit FileInfo, the slice touching it
    check(oracle, mem, 1020, 3072 - 1056, 3)                     # and disjoint from it


def test_whole_payloads(oracle, mem):
    """For a whole payload c is also the value checked against crc_."""
    for H, pay in ((100, 0), (100, 1), (92, 988), (1000, 4059), (1000, 4060), (7, 32731 + 8), (3, 70001)):
        check(oracle, mem, H, 0, pay)
