"""The task kernels' CRC arithmetic (tfs_ec_kernels.hip ec_task_kernel's source word and
ec_fetch_check_kernel), restated lane by lane on the CPU against the
oracle's Func::crc(FLAG_V1, le32 n || D || le32 data_file_size): the pieces as the kernel
loads them from the incoming buffer -- not at all at or past n, byte-masked where one
straddles n, whatever lies behind the data (trailer, gap) left out --, the lanes' chains
with the 128-byte step, the move to the data's end inside the tile with one power (a
negative one for the lanes behind it), one word per tile; then the check's lane runs over
the whole tiles' words, the last tile's word 1 .. 4096 bytes on, and the join of head,
data and tail by linearity with the power by squaring.  No GPU."""
import struct

import pytest

from conftest import ocrc
from test_ec_frames_math import crc_word, powk
from test_marshal_math import BIAS, POW_N, X128, X4K, XPOW, crc0, multmodp
from tfs_amd.packet import read_raw_reply_frame
from tfs_amd.synth import synth_bytes

FLAG_V1 = 0x4E534654
HEAD = 28
NS = [1, 7, 8, 9, 1023, 4095, 4096, 4097, 8191]


def low_bytes(k):
    return 0 if k <= 0 else (1 << 64) - 1 if k >= 8 else (1 << (8 * k)) - 1


def source_word(buf, tile_at, nrem):
    """ec_task_kernel's word of one tile of a source: `buf` is the incoming buffer, the tile's first data byte
    lies at tile_at, nrem data bytes of the frame remain from there on.  Returns (word, the bytes the loads read)."""
    pad = 0 if nrem >= 4096 or nrem <= 0 else 4096 - nrem
    acc, read_to = 0, 0
    for lane in range(64):
        lo = 1024 * (lane >> 4) + 8 * (lane & 15)
        c = 0
        for pc in range(8):
            k = nrem - (lo + 128 * pc)
            v = 0
            if k > 0:  # the load
                at = tile_at + lo + 128 * pc
                assert at % 8 == 0
                v = int.from_bytes(buf[at:at + 8], "little")
                read_to = max(read_to, at + 8)
            v &= low_bytes(k)
            p = crc0(v.to_bytes(8, "little"))
            c = p if pc == 0 else multmodp(X128, c) ^ p
        dl = 3192 - lo
        assert 0 <= BIAS + dl - pad < POW_N
        acc ^= multmodp(XPOW[BIAS + dl - pad], c)
    return acc, read_to


def check(words, n, head, dfs):
    """ec_fetch_check_kernel for one frame whose expected length is n: (status, crc)."""
    nc = (n - 1) >> 12
    lastb = n - (nc << 12)
    assert 1 <= lastb <= 4096
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
    crc = multmodp(powk(XPOW[BIAS + 1], n + 4), crc_word(FLAG_V1 ^ n)) ^ crc_word(c) ^ crc_word(dfs)
    flag, blen, pcode, version, _, hcrc, dn = struct.unpack("<IIhhQII", head)
    if flag != FLAG_V1 or blen != 8 + n or pcode != 46 or dn != n:
        return -1, crc, c
    if version >= 1 and hcrc != crc:
        return -1010, crc, c
    return 0, crc, c


def placed(frame, frame_len):
    """The frame at 4 modulo 8 in a buffer of garbage: (buffer, the frame's start)."""
    buf = bytearray(synth_bytes(len(frame), 8 + frame_len + 96).tobytes())
    buf[4:4 + len(frame)] = frame
    return buf, 4


@pytest.mark.parametrize("frame_len,n", [(fl, n) for fl in (4096, 8192) for n in NS + [8192] if n <= fl])
def test_source_words_and_check_give_the_frame_crc(oracle, frame_len, n):
    data = synth_bytes(1000 + n + frame_len, n).tobytes()
    dfs = 0x01020304 + n
    body = struct.pack("<I", n) + data + struct.pack("<I", dfs)
    want = ocrc(oracle, FLAG_V1, body)
    for version in (0, 1, 2):
        frame = read_raw_reply_frame(data, dfs, version, 77 + n, want if version else 0)
        assert frame[24:] == body
        buf, at = placed(frame, frame_len)
        words, read_to = [], 0
        for t in range(frame_len // 4096):
            w, r = source_word(buf, at + HEAD + 4096 * t, n - 4096 * t)
            assert w == ocrc(oracle, 0, data[4096 * t:4096 * t + 4096])
            words.append(w)
            read_to = max(read_to, r)
        # the loads stay inside the aligned 8-byte word that holds the frame's last byte
        assert read_to <= (at + len(frame) + 7) // 8 * 8
        st, crc, dcrc = check(words, n, bytes(buf[at:at + HEAD]), dfs)
        assert (st, crc, dcrc) == (0, want, ocrc(oracle, 0, data))
        # damage, the lower-numbered check first
        crc_err = -1010 if version else 0
        for pos, exp in [(HEAD, crc_err), (HEAD + n - 1, crc_err), (HEAD + n + 2, crc_err), (22, crc_err), (0, -1), (6, -1),
                         (8, -1), (24, -1)]:
            hurt = bytearray(buf)
            hurt[at + pos] ^= 0x04
            ws = [source_word(hurt, at + HEAD + 4096 * t, n - 4096 * t)[0] for t in range(frame_len // 4096)]
            d = int.from_bytes(hurt[at + HEAD + n:at + HEAD + n + 4], "little")
            assert check(ws, n, bytes(hurt[at:at + HEAD]), d)[0] == exp, (pos, version)
        # a byte behind the trailer is not the frame's: nothing changes
        hurt = bytearray(buf)
        hurt[at + HEAD + n + 4] ^= 0xFF
        ws = [source_word(hurt, at + HEAD + 4096 * t, n - 4096 * t)[0] for t in range(frame_len // 4096)]
        assert ws == words


def test_long_frame_lane_runs(oracle):
    """A frame of 70 tiles whose last holds 5 bytes: the check's lanes take runs of two words, the last lanes none."""
    n = 69 * 4096 + 5
    data = synth_bytes(6, n).tobytes()
    words = [ocrc(oracle, 0, data[4096 * t:4096 * t + 4096]) for t in range(70)]
    want = ocrc(oracle, FLAG_V1, struct.pack("<I", n) + data + struct.pack("<I", 9))
    head = read_raw_reply_frame(data, 9, 2, 1, want)[:HEAD]
    assert check(words, n, head, 9) == (0, want, ocrc(oracle, 0, data))
