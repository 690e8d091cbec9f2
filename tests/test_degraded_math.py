"""The algebra of the degraded read's in-register CRC, restated
lane by lane in Python as ec_read_kernel is built and checked against the
oracle's byte loop (CPU only).

A workgroup of W = 8 waves walks the covering units [A, E) of a record in tiles of
4 units counted from A; wave w takes tiles w, w + W, ...  Lane l owns 8 bytes at
8 (l & 15) of each of the 8 packets of unit l >> 4.  Its chain runs over its
pieces in address order,

    c' = shift(c, step) ^ crc(0, piece),   step = 128 (next packet), 4096 W - 896 (its next tile)

with the bytes outside the payload masked to zero and crc(0, piece) two
slice-by-4 steps.  At the end lane l of wave w, whose last tile is tl, stands
d = 4096 (nt - 1 - tl) + 3192 - 1024 (l >> 4) - 8 (l & 15) bytes before the end E'
of the job's last tile and the payload ends pad = E' - end bytes before E'; one
multiplication by xpow[4095 + d - pad] = x^(8 (d - pad)) (inverse powers below
4095) moves it to the payload's end, and the XOR over all lanes of all waves is
Func::crc(0, payload).
"""
import numpy as np
import pytest

from conftest import ocrc

POLY = 0xEDB88320
FI = 36
W = 8  # kReadWaves


def mult(a, b):
    p = 0
    for i in range(31, -1, -1):  # as rd_multmodp: bit 31 of a is x^0
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def x2n(n):
    p, sq = 1 << 31, 1 << 30
    while n:
        if n & 1:
            p = mult(sq, p)
        n >>= 1
        sq = mult(sq, sq)
    return p


def shift(c, nbytes):
    return mult(x2n(8 * nbytes), c)


SLICE = [[0] * 256 for _ in range(4)]
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ POLY if _c & 1 else _c >> 1
    SLICE[0][_i] = _c
for _k in range(1, 4):
    for _b in range(256):
        SLICE[_k][_b] = (SLICE[_k - 1][_b] >> 8) ^ SLICE[0][SLICE[_k - 1][_b] & 255]


def byte_table(nbytes):  # crc_math.h make_shift_table
    k = x2n(8 * nbytes)
    return [[mult(k, b << (8 * j)) for b in range(256)] for j in range(4)]


STEP_PACKET, STEP_TILE = byte_table(128), byte_table(4096 * W - 896)
BIAS, NPOW = 4095, 4095 + 4096 * (W - 1) + 3192 + 1
XPOW = [0] * NPOW
XPOW[BIAS] = 1 << 31
_g, _gi = x2n(8), x2n(0xFFFFFFFF - 8)  # x^8 and its inverse: ord(x) divides 2^32 - 1
for _i in range(BIAS + 1, NPOW):
    XPOW[_i] = mult(_g, XPOW[_i - 1])
for _i in range(BIAS - 1, -1, -1):
    XPOW[_i] = mult(_gi, XPOW[_i + 1])


def lut4(t, x):
    return t[0][x & 255] ^ t[1][(x >> 8) & 255] ^ t[2][(x >> 16) & 255] ^ t[3][x >> 24]


def slice4(x):
    return SLICE[3][x & 255] ^ SLICE[2][(x >> 8) & 255] ^ SLICE[1][(x >> 16) & 255] ^ SLICE[0][x >> 24]


def low_bytes(k):
    return 0 if k <= 0 else (1 << 64) - 1 if k >= 8 else (1 << (8 * k)) - 1


def emulate(mem, offset, size):
    """The payload CRC of the record (offset, size) of `mem` as one workgroup computes it."""
    A, E = offset & ~1023, (offset + size + 1023) & ~1023
    nt = (E - A + 4095) >> 12
    P0, P1 = offset + FI, offset + size
    pad = A + 4096 * nt - P1
    out = 0
    for w in range(W):
        crc = [0] * 64
        for t in range(w, nt, W):
            for lane in range(64):
                pu = A + 4096 * t + 1024 * (lane >> 4)
                base = pu + 8 * (lane & 15)
                c = crc[lane]
                for k in range(8):
                    q = base + 128 * k
                    v = int.from_bytes(mem[q:q + 8], "little") if pu < E else 0
                    sk, ek = P0 - q, P1 - q
                    if sk > 0 or ek < 8:
                        v &= 0 if ek <= sk else low_bytes(ek) & ~low_bytes(sk)
                    piece = slice4(slice4(v & 0xFFFFFFFF) ^ (v >> 32))
                    c = lut4(STEP_TILE if k == 0 else STEP_PACKET, c) ^ piece
                crc[lane] = c
        if w >= nt:
            continue  # a wave without a tile holds zeros
        tl = nt - 1 - ((nt - 1 - w) % W)
        part = 0
        for lane in range(64):
            dl = 4096 * (nt - 1 - tl) + 3192 - 1024 * (lane >> 4) - 8 * (lane & 15)
            part ^= mult(XPOW[BIAS + dl - pad], crc[lane])
        out ^= part
    return out


@pytest.fixture(scope="module")
def mem():
    return np.random.default_rng(11).integers(0, 256, 128 * 1024, dtype=np.uint8).tobytes()


def check(oracle, mem, offset, size):
    assert offset + size <= len(mem) - 4096
    exp = ocrc(oracle, 0, mem[offset + FI:offset + size])
    assert emulate(mem, offset, size) == exp, (offset, size)


def test_tables():
    assert mult(_g, _gi) == 1 << 31
    for c in (1, 0x80000000, 0xDEADBEEF):
        assert lut4(STEP_PACKET, c) == shift(c, 128) and lut4(STEP_TILE, c) == shift(c, 4096 * W - 896)
        # a piece step is the byte loop over 8 bytes from a zero register
        v = c * 0x100000001
        assert slice4(slice4(v & 0xFFFFFFFF) ^ (v >> 32)) == shift(slice4(c), 4) ^ slice4(c)


def test_unshift_inverts_shift():
    for c in (1, 0x80000000, 0x12345678, 0xFFFFFFFF):
        for n in range(4096):
            assert shift(mult(XPOW[BIAS - n], c), n) == c
    for n in (0, 1, 8, 3192, 3192 + 4096 * (W - 1)):
        assert XPOW[BIAS + n] == x2n(8 * n)


def test_every_start_and_end_mod_128(oracle, mem):
    """Payload starts at every offset mod 128 (so mod 16 too), and the ends run
    through every residue mod 128 as well (5 s + 3 is a bijection mod 128)."""
    ends = set()
    for s in range(128):
        start = 2048 + s              # payload start = offset + 36
        er = (5 * s + 3) % 128
        end = start + 1 + ((er - start - 1) % 128) + 128 * (s % 3)
        ends.add(end % 128)
        check(oracle, mem, start - FI, end - start + FI)
    assert len(ends) == 128


def test_every_start_and_end_mod_16(oracle, mem):
    for s in range(16):
        for e in range(16):
            start = 1024 + 112 + s
            end = start + 1 + ((e - start - 1) % 16)
            check(oracle, mem, start - FI, end - start + FI)


def test_inside_one_piece(oracle, mem):
    for start, n in ((3072 + 8 * 5 + 1, 1), (3072 + 8 * 5 + 2, 5), (3072 + 8 * 5, 8), (3072 + 1016 + 3, 4)):
        check(oracle, mem, start - FI, n + FI)


def test_across_units_and_tiles(oracle, mem):
    for offset, size in ((1000, 37), (1000, 100), (4090, 37 + 1), (4090, 4097 + FI), (1, 1023 + FI), (0, 1024),
                         (92, 988 + FI), (1023, 4095 + FI), (2048 + 100, 8192 + FI), (5000, 20001),
                         (3 * 1024 - 36, 1 + FI), (3 * 1024 - 37, 1 + FI), (7, 4096 * 3 - 7), (100, 4096 * 4 + 5),
                         (3000, 4096 * 5 + FI), (1, 4096 * 7), (2047, 4096 * 8 - 2047), (500, 4096 * 13 + 77), (700, 4096 * 20 + 9)):
        check(oracle, mem, offset, size)
