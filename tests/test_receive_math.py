"""CPU-side checks of the arithmetic a receive session rests on (include/tfs_receive.h,
DESIGN.md §3.20), against zlib and the oracle.  With c(p) = Func::crc(0, p), shift as in
tfs_crc32_combine and G the granule:

  word(g)  = c(granule bytes received so far || zeros up to the granule's end)
           = XOR over the pieces that arrived of shift(c(piece), granule_end - piece_end)
  crc(FLAG, H || D || F) = shift(crc(FLAG, H), |D| + 4) ^ shift(c(D), 4) ^ c(F)
  c(payload [a, b)) = shift(c(head edge), b - he) ^ XOR_g shift(word(g), b - (g + 1) G) ^ c(tail edge)
"""
import struct
import zlib

import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

FLAG = pk.TFS_PACKET_FLAG_V1
M32 = 0xFFFFFFFF


def zcrc(seed, data):
    """Func::crc(seed, data) (no inversions) through zlib's CRC-32."""
    return zlib.crc32(bytes(data), seed ^ M32) ^ M32


def shift(c, n):
    """shift(c, n) = c * x^(8n) mod P: the register after n zero bytes."""
    return zcrc(c, bytes(n))


@pytest.fixture(scope="module")
def G():
    import tfs_amd.crc as crc
    assert crc.receive_granule() == crc.lib().tfs_receive_granule() >= 64
    return crc.receive_granule()


def word(pieces, G):
    """pieces: (start in the granule, bytes); the granule word as the session gathers it."""
    w = 0
    for start, b in pieces:
        w ^= shift(zcrc(0, b), G - (start + len(b)))
    return w


def test_shift_is_appending_zeros(oracle):
    import tfs_amd.crc as crc
    d = synth_bytes(1, 100).tobytes()
    for n in (0, 1, 4, 4095, 4096, 70000):
        assert shift(zcrc(0, d), n) == zcrc(0, d + bytes(n)) == crc.combine(zcrc(0, d), 0, n)
    assert ocrc(oracle, 0, d) == zcrc(0, d)


def test_granule_word_from_pieces(oracle, G):
    g = synth_bytes(2, G).tobytes()
    want = zcrc(0, g)
    assert want == ocrc(oracle, 0, g)
    assert word([(0, g)], G) == want
    for cut in (1, 17, G // 2, G - 1):
        two = [(0, g[:cut]), (cut, g[cut:])]
        assert word(two, G) == want and word(two[::-1], G) == want   # either order of arrival
    three = [(0, g[:5]), (5, g[5:G - 30]), (G - 30, g[G - 30:])]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        assert word([three[i] for i in order], G) == want
    # one piece alone: the rest of the granule counts as zeros
    assert word([(0, g[:100])], G) == zcrc(0, g[:100] + bytes(G - 100))
    assert word([(100, g[100:])], G) == zcrc(0, bytes(100) + g[100:])


def test_incomplete_tail_granule(G):
    tail = synth_bytes(3, 333).tobytes()
    assert word([(0, tail)], G) == zcrc(0, tail + bytes(G - 333))
    assert word([(0, tail[:300]), (300, tail[300:])], G) == zcrc(0, tail + bytes(G - 333))
    assert word([], G) == 0 == zcrc(0, bytes(G))


@pytest.mark.parametrize("nd", [0, 1, 36, 1023, 4096, 4097, 70001])
@pytest.mark.parametrize("flag", [0, 1, 2])
def test_frame_identity(oracle, nd, flag):
    d = synth_bytes(50 + nd, nd).tobytes()
    h = struct.pack("<IQiiiQ", 0xC0FFEE, 0, 12345, nd, 0, 0)
    f = struct.pack("<i", flag)
    want = zcrc(FLAG, h + d + f)
    assert want == ocrc(oracle, FLAG, h + d + f)
    assert shift(zcrc(FLAG, h), nd + 4) ^ shift(zcrc(0, d), 4) ^ zcrc(0, f) == want
    assert zcrc(FLAG, h) == zcrc(0, h) ^ shift(FLAG, 32)             # the seed moves like any register
    # c(D) gathered from pieces cut anywhere, each moved to the end of the data
    cd, at = 0, 0
    for n in (7, 1, 4000, 4096, 10**9):
        p = d[at:at + n]
        at += len(p)
        cd ^= shift(zcrc(0, p), nd - at)
    assert cd == zcrc(0, d)


def fold(img, a, b, G):
    """The record fold over words and edges, as receive_plan.h cuts the payload."""
    nwords = -(-len(img) // G)
    words = [zcrc(0, img[g * G:(g + 1) * G].ljust(G, b"\0")) for g in range(nwords)]
    up, down = -(-a // G) * G, b // G * G
    if up > down:
        return zcrc(0, img[a:b]), 0, b - a
    c = shift(zcrc(0, img[a:up]), b - up) ^ zcrc(0, img[down:b])
    for g in range(up // G, down // G):
        c ^= shift(words[g], b - (g + 1) * G)
    return c, down // G - up // G, (up - a) + (b - down)


def test_record_fold(oracle, G):
    img = synth_bytes(7, 75 * G + 500).tobytes()
    cases = {
        "inside one granule": (G + 40, G + 900, 0),
        "inside one granule, to its end": (G + 40, 2 * G, 0),
        "starts on the grid": (2 * G, 3 * G + 77, 1),
        "ends on the grid": (G + 11, 3 * G, 1),
        "both": (G, 3 * G, 2),
        "one whole granule": (G - 5, 2 * G + 5, 1),
        "two whole granules": (G - 1, 3 * G + 1, 2),
        "seventy whole granules": (3 * G - 100, 73 * G + 123, 70),
        "across a boundary, no whole granule": (G - 10, G + 10, 0),
        "to the last byte of the ragged tail": (74 * G + 1, 75 * G + 500, 0),
    }
    for name, (a, b, whole) in cases.items():
        c, n, reread = fold(img, a, b, G)
        assert c == zcrc(0, img[a:b]), name
        assert n == whole, name
        assert reread <= 2 * (G - 1), name
    a, b = cases["two whole granules"][:2]
    assert fold(img, a, b, G)[0] == ocrc(oracle, 0, img[a:b])
