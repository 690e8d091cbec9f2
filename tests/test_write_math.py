"""The algebra behind write frames that yield the file CRC (include/tfs_write.h,
DESIGN.md §3.10), on the CPU against the oracle:

  * crc.combine (tfs_crc32_combine): Func::crc(s, A + B) from Func::crc(s, A),
    Func::crc(0, B) and len(B), for any seed s;
  * the prefix rule of a WriteDataMessage body H || D:
    Func::crc(0, D) = Func::crc(FLAG, H || D) ^ shift(Func::crc(FLAG, H), |D|);
  * the device's general-length shift -- 27 levels of 5-bit-chunk tables of
    shift(c, 2^k bytes) -- restated in Python and checked against
    oracle_crc(c, zeros(n)).
"""
import struct

import numpy as np
import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

FLAG = pk.TFS_PACKET_FLAG_V1
POLY = 0xEDB88320
LEVELS = 27


def multmodp(a, b):
    """a * b mod P in the reflected domain (bit 31 = x^0)."""
    p, m = 0, 1 << 31
    while True:
        if a & m:
            p ^= b
            if a & (m - 1) == 0:
                break
        m >>= 1
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def level_tables():
    """tables[k][j][e] = shift(e << 5j, 2^k bytes): what packet_data_fold_kernel keeps in LDS."""
    out = []
    xp = multmodp(1 << 23, 1 << 31)  # x^8
    for _ in range(LEVELS):
        out.append([[multmodp(xp, (e << (5 * j)) & 0xFFFFFFFF) for e in range(32)] for j in range(7)])
        xp = multmodp(xp, xp)
    return out


TABLES = level_tables()


def shift_levels(c, nbytes):
    assert 0 <= nbytes < 1 << LEVELS
    for k in range(LEVELS):
        if (nbytes >> k) & 1:
            t = TABLES[k]
            r = 0
            for j in range(7):
                r ^= t[j][(c >> (5 * j)) & 31]
            c = r
    return c


def prefix_len(pcode, body):
    """H's length when the body is a well-formed WRITE_DATA body, else 0."""
    if pcode != pk.WRITE_DATA_MESSAGE or len(body) < 36:
        return 0
    length_, = struct.unpack_from("<i", body, 16)
    count, = struct.unpack_from("<i", body, 32)
    if count < 0 or count > 27 or length_ < 0:
        return 0
    hlen = 36 + 8 * count
    return hlen if hlen + length_ == len(body) else 0


@pytest.mark.parametrize("seed", [0, FLAG])
@pytest.mark.parametrize("nb", [0, 1, 15, 16, 1023, 1024, 65536, (1 << 21) + 1])
def test_combine_matches_oracle(oracle, seed, nb):
    import tfs_amd.crc as crc
    for na in (0, 1, 37, 4096):
        a = synth_bytes(3 + na, na).tobytes()
        b = synth_bytes(1000 + nb, nb).tobytes()
        got = crc.combine(ocrc(oracle, seed, a), ocrc(oracle, 0, b), len(b))
        assert got == ocrc(oracle, seed, a + b), (seed, na, nb)


def test_combine_is_a_pure_shift_with_zero_crc_b(oracle):
    import tfs_amd.crc as crc
    for n in (0, 1, 7, 4096, 1 << 26, (1 << 27) - 1):
        assert crc.combine(0x9E3779B9, 0, n) == shift_levels(0x9E3779B9, n), n
    for n in (0, 1, 7, 4096):
        assert crc.combine(0x9E3779B9, 0, n) == ocrc(oracle, 0x9E3779B9, bytes(n)), n
    # the 64-bit length is honoured: 2^32 + 5 bytes in one step or in two
    big = (1 << 32) + 5
    assert crc.combine(0x12345678, 0, big) == crc.combine(crc.combine(0x12345678, 0, 1 << 32), 0, 5)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 31, 32, 1023, 65536, 131073, (1 << 21) - 1])
def test_level_shift_matches_oracle(oracle, n):
    zeros = bytes(n)
    for c in (0, 1, 0x80000000, 0xFFFFFFFF, 0xCADE6EAE, FLAG):
        assert shift_levels(c, n) == ocrc(oracle, c, zeros), (hex(c), n)


def test_level_shift_every_single_bit(oracle):
    # one level at a time: bits 0..22 against the oracle's zero-byte loop, the top
    # levels by squaring (level k+1 applied once == level k applied twice)
    c = 0xDEADBEEF
    for k in range(23):
        assert shift_levels(c, 1 << k) == ocrc(oracle, c, bytes(1 << k)), k
    for k in range(22, LEVELS - 1):
        assert shift_levels(c, 1 << (k + 1)) == shift_levels(shift_levels(c, 1 << k), 1 << k), k


@pytest.mark.parametrize("count", [0, 3, 6, 27])
def test_prefix_rule(oracle, count):
    for nd in (0, 1, 3, 15, 16, 17, 1023, 1024, 1025, 65536, 131073):
        data = synth_bytes(7 * count + nd, nd).tobytes()
        body = pk.write_data_body(0x1234, 0xABCDEF01, 65536, data, ds=list(range(count)))
        hlen = prefix_len(pk.WRITE_DATA_MESSAGE, body)
        assert hlen == 36 + 8 * count and body[hlen:] == data
        p = ocrc(oracle, FLAG, body[:hlen])
        assert ocrc(oracle, 0, data) == ocrc(oracle, FLAG, body) ^ shift_levels(p, nd), (count, nd)


def test_prefix_rule_rejects_malformed():
    data = b"d" * 100
    good = pk.write_data_body(1, 2, 0, data, ds=[1, 2, 3])
    assert prefix_len(pk.WRITE_DATA_MESSAGE, good) == 60
    assert prefix_len(pk.WRITE_DATA_MESSAGE + 1, good) == 0          # another pcode
    assert prefix_len(pk.WRITE_DATA_MESSAGE, good[:35]) == 0         # shorter than WriteDataInfo + count

    def patched(at, v):
        b = bytearray(good)
        struct.pack_into("<i", b, at, v)
        return bytes(b)

    assert prefix_len(pk.WRITE_DATA_MESSAGE, patched(16, -1)) == 0    # length_ < 0
    assert prefix_len(pk.WRITE_DATA_MESSAGE, patched(16, 101)) == 0   # length_ past the body
    assert prefix_len(pk.WRITE_DATA_MESSAGE, patched(16, 99)) == 0    # hlen + length_ != body
    assert prefix_len(pk.WRITE_DATA_MESSAGE, patched(32, -1)) == 0    # count < 0
    body28 = pk.write_data_body(1, 2, 0, data, ds=list(range(28)))
    assert prefix_len(pk.WRITE_DATA_MESSAGE, body28) == 0             # count = 28
    body27 = pk.write_data_body(1, 2, 0, data, ds=list(range(27)))
    assert prefix_len(pk.WRITE_DATA_MESSAGE, body27) == 252


def test_write_part_layout():
    import tfs_amd.crc as crc
    assert crc.WRITE_PART_DTYPE.itemsize == 16
    assert crc.WRITE_PART_DTYPE.fields["data_crc"][1] == 8
    assert np.zeros(1, crc.WRITE_PART_DTYPE)["data_len"].dtype == np.int32
