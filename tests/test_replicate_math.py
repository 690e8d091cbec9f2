"""CPU-side checks of the arithmetic a replicate session rests on (include/tfs_replicate.h,
DESIGN.md §3.18), against zlib and the oracle.

With P a set of pieces that partition the data, c(p) = Func::crc(0, p) and shift as in
tfs_crc32_combine:

  fold x <- shift(x, |p|) ^ c(p) over consecutive pieces  = Func::crc(0, their concatenation)
  crc(FLAG, H || D || F) = crc(seed = shift(crc(FLAG, H), |D|) ^ crc(0, D), F)

and, as the device folds it (every piece moved to the end of the body at once),

  crc(FLAG, H || D || F) = crc(FLAG, H || 0^|D| || F) ^ XOR_p shift(c(p), bytes after p + 4).
"""
import random
import struct
import zlib

import pytest

from conftest import ocrc
from tfs_amd import packet as pk
from tfs_amd.synth import synth_bytes

FLAG = pk.TFS_PACKET_FLAG_V1
M32 = 0xFFFFFFFF
LENGTHS = [0, 1, 35, 36, 37, 1023, 1024, 1025, 65536, 1 << 20]


def zcrc(seed, data):
    """Func::crc(seed, data) (no inversions) through zlib's CRC-32."""
    return zlib.crc32(data, seed ^ M32) ^ M32


def cuts(nd, rng):
    """Piece lengths that sum to nd: runs of 1-byte pieces, pieces of 0..36 bytes, long pieces."""
    out, left = [], nd
    while left:
        kind = rng.random()
        n = 1 if kind < 0.2 else rng.randint(0, 36) if kind < 0.6 else rng.randint(1, max(1, nd // 3))
        n = min(n, left)
        out.append(n)
        left -= n
    return out + [0]


def info_bytes(block_id, offset, length):
    return struct.pack("<IQiiiQ", block_id, 0, offset, length, 0, 0)


@pytest.mark.parametrize("nd", LENGTHS)
def test_piece_fold_is_the_crc_of_the_concatenation(oracle, nd):
    import tfs_amd.crc as crc
    d = synth_bytes(300 + nd, nd).tobytes()
    want = zcrc(0, d)
    if nd <= 65536:
        assert want == ocrc(oracle, 0, d)
    for trial in range(3 if nd > 65536 else 8):
        rng = random.Random(nd * 31 + trial)
        x, at = 0, 0
        for n in cuts(nd, rng):
            x = crc.combine(x, zcrc(0, d[at:at + n]), n)
            at += n
        assert at == nd and x == want, (nd, trial)


@pytest.mark.parametrize("nd", LENGTHS)
@pytest.mark.parametrize("flag", [0, 1, 2])
def test_frame_crc_from_the_pieces(oracle, nd, flag):
    import tfs_amd.crc as crc
    d = synth_bytes(500 + nd, nd).tobytes()
    h = info_bytes(0xC0FFEE, 3 << 20, nd)
    f = struct.pack("<i", flag)
    assert len(h) == 32
    want = zcrc(FLAG, h + d + f)
    if nd <= 65536:
        assert want == ocrc(oracle, FLAG, h + d + f)
    # the issue's form: the pre-shifted seed, XOR crc(0, D), carried over F
    seed = crc.combine(zcrc(FLAG, h), 0, nd) ^ zcrc(0, d)
    assert zcrc(seed, f) == want
    # the device's form: the zero-data body, XOR every piece moved to the end of the body
    zero_body = crc.combine(zcrc(FLAG, h), 0, nd + 4) ^ zcrc(0, f)
    assert zero_body == zcrc(FLAG, h + bytes(nd) + f)
    rng = random.Random(nd * 7 + flag)
    x, at = zero_body, 0
    for n in cuts(nd, rng):
        x ^= crc.combine(zcrc(0, d[at:at + n]), 0, nd - (at + n) + 4)
        at += n
    assert x == want
