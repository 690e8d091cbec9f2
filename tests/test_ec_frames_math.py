"""The frame kernels' CRC arithmetic (tfs_ec_kernels.hip ec_frames_kernel's tile end and
ec_frames_seal_kernel), restated step by step on the CPU against the
oracle's Func::crc(FLAG_V1, H || D || F): the lanes' chains over their eight pieces with
the 128-byte step, the move to the end of the tile's bytes with one power (pad for the
chunk's short last tile), one word per tile; then the seal's lane runs over the words of
the whole tiles, the power by squaring, the last tile's word, and the join with head and
tail by linearity.  No GPU."""
import struct

import pytest

from conftest import ocrc
from test_marshal_math import BIAS, POW_N, X128, X4K, XPOW, crc0, multmodp, x2n
from tfs_amd.synth import synth_bytes

FLAG_V1 = 0x4E534654
NORMAL, PARITY = 1, 2


def tile_word(data, t, length):
    """ec_frames_kernel's end of tile t of a frame's data (`length` bytes): crc(0, the tile's bytes)."""
    lo = 4096 * t
    left = length - lo
    pad = 0 if left >= 4096 else 4096 - left
    acc = 0
    for lane in range(64):
        u, off = lane >> 4, 8 * (lane & 15)
        ok = lo + 1024 * u < length  # a lane whose unit lies past the chunk holds zeros
        c = 0
        for pc in range(8):
            q = lo + 1024 * u + off + 128 * pc
            piece = bytes(data[q:q + 8]) if ok else bytes(8)
            assert len(piece) == 8
            c = crc0(piece) if pc == 0 else multmodp(X128, c) ^ crc0(piece)
        dl = 3192 - (1024 * u + off)
        assert 0 <= BIAS + dl - pad < POW_N
        acc ^= multmodp(XPOW[BIAS + dl - pad], c)
    return acc


def powk(x, k):
    r = 1 << 31
    while k:
        if k & 1:
            r = multmodp(r, x)
        x = multmodp(x, x)
        k >>= 1
    return r


def seal(words, block_id, offset, length, flag, version, frame_len, total):
    """ec_frames_seal_kernel for one frame: the header CRC from the tile words."""
    nc = (length - 1) >> 12
    lastb = length - (nc << 12)
    assert 1024 <= lastb <= 4096 and len(words) == nc + 1
    c = 0
    if nc:
        R = (nc + 63) // 64
        for lane in range(64):
            b = min(lane * R, nc)
            e = min(b + R, nc)
            v = 0
            for t in range(b, e):
                v = multmodp(X4K, v) ^ words[t]
            c ^= multmodp(powk(X4K, nc - e), v)
    c = multmodp(XPOW[BIAS + lastb], c) ^ words[nc]
    hc = FLAG_V1
    for w in (block_id, 0, 0, offset, length, 0, 0, 0):
        hc = crc_word(hc ^ w)
    last_len = total - (total - 1) // frame_len * frame_len
    pw = x2n(8 * (last_len + 4)) if offset + length == total else x2n(8 * (frame_len + 4))
    fcrc = multmodp(pw, hc) ^ crc_word(c) ^ crc_word(flag)
    return (fcrc if version >= 1 else 0), c


def crc_word(x):
    """rd_slice4: the register after four bytes, entered as one word."""
    from test_marshal_math import BYTE
    for _ in range(4):
        x = BYTE[x & 255] ^ (x >> 8)
    return x


def body_of(block_id, offset, data, flag):
    return struct.pack("<IQIIIQ", block_id, 0, offset, len(data), 0, 0) + bytes(data) + struct.pack("<I", flag)


@pytest.mark.parametrize("frame_len", [4096, 8192])
@pytest.mark.parametrize("units", [1, 2, 3, 4])
def test_tile_words_and_seal_give_the_frame_crc(oracle, frame_len, units):
    """Frames 0 (whole, F on), 1 (whole, F off) and the last one of 1 - 4 units, versions 0 and 1."""
    total = 2 * frame_len + 1024 * units
    member = synth_bytes(900 + frame_len + units, total).tobytes()
    for k in range(3):
        off = k * frame_len
        data = member[off:off + frame_len]
        assert len(data) == (frame_len if k < 2 else 1024 * units)
        words = [tile_word(data, t, len(data)) for t in range((len(data) + 4095) // 4096)]
        for t, w in enumerate(words):
            assert w == ocrc(oracle, 0, data[4096 * t:4096 * t + 4096])
        for flag0 in (NORMAL, PARITY):
            flag = flag0 if k == 0 else 0
            want = ocrc(oracle, FLAG_V1, body_of(77 + k, off, data, flag))
            for version in (0, 1):
                got, dcrc = seal(words, 77 + k, off, len(data), flag, version, frame_len, total)
                assert dcrc == ocrc(oracle, 0, data)
                assert got == (want if version else 0), (k, flag, version)


def test_f_word_changes_the_crc_and_nothing_else(oracle):
    """F on and off over the same data: the two CRCs differ by crc(0, F) alone."""
    data = synth_bytes(5, 4096).tobytes()
    words = [tile_word(data, 0, 4096)]
    on, _ = seal(words, 9, 0, 4096, PARITY, 1, 4096, 8192)
    off, _ = seal(words, 9, 0, 4096, 0, 1, 4096, 8192)
    assert on == ocrc(oracle, FLAG_V1, body_of(9, 0, data, PARITY)) and off == ocrc(oracle, FLAG_V1, body_of(9, 0, data, 0))
    assert on ^ off == crc_word(PARITY)


def test_long_frame_lane_runs(oracle):
    """A frame of 70 tiles: the seal's lanes take runs of two words and the last lanes none."""
    length = 69 * 4096 + 2048
    data = synth_bytes(6, length).tobytes()
    words = [ocrc(oracle, 0, data[4096 * t:4096 * t + 4096]) for t in range(70)]
    got, dcrc = seal(words, 3, 0, length, NORMAL, 2, 70 * 4096, length)
    assert dcrc == ocrc(oracle, 0, data) and got == ocrc(oracle, FLAG_V1, body_of(3, 0, data, NORMAL))
