"""The end of the tile in ec_scrub_kernel (tfs_ec_kernels.hip), restated
lane by lane on the CPU against the byte-wise compare: lane l holds the 8 bytes at offset
8 (l & 15) of packet r of unit l >> 4 in register pair r; it XORs the stored parity's
pieces into the code's, ORs the eight results, and a ballot of the wave turns "any lane
of unit l >> 4 nonzero" into four bits.  A lane whose unit lies past the chunk loads
nothing: both sides are zero.  No GPU.
"""
import numpy as np
import pytest

from tfs_amd.synth import synth_bytes


def lane_pieces(tile, lane, live_units):
    """The lane's eight register pairs over one member's tile (None past the chunk: nothing loaded)."""
    u, off = lane >> 4, 8 * (lane & 15)
    if u >= live_units:
        return [(0, 0)] * 8
    out = []
    for r in range(8):
        q = 1024 * u + off + 128 * r
        w = tile[q:q + 8].view("<u4")
        out.append((int(w[0]), int(w[1])))
    return out


def tile_end(code, stored, live_units):
    """The word the wave writes: bit u set when unit u differs."""
    ballot = 0
    for lane in range(64):
        acc, par = lane_pieces(code, lane, live_units), lane_pieces(stored, lane, live_units)
        d = 0
        for r in range(8):
            d |= (acc[r][0] ^ par[r][0]) | (acc[r][1] ^ par[r][1])
        if d != 0:
            ballot |= 1 << lane
    bits = 0
    for u in range(4):
        if (ballot >> (16 * u)) & 0xFFFF:
            bits |= 1 << u
    return bits


def bytewise(code, stored, live_units):
    bits = 0
    for u in range(live_units):
        if (code[1024 * u:1024 * u + 1024] != stored[1024 * u:1024 * u + 1024]).any():
            bits |= 1 << u
    return bits


def tiles(seed, live_units):
    """A tile of `live_units` units; the bytes past them do not exist for the kernel and differ here on purpose."""
    code = synth_bytes(seed, 4096)
    stored = code.copy()
    stored[1024 * live_units:] ^= 0xFF
    return code, stored


@pytest.mark.parametrize("live", [1, 2, 3, 4])
def test_clean_tile_and_every_unit_alone(live):
    code, stored = tiles(10 + live, live)
    assert tile_end(code, stored, live) == bytewise(code, stored, live) == 0
    for u in range(live):
        s = stored.copy()
        s[1024 * u + 517] ^= 0x10
        assert tile_end(code, s, live) == bytewise(code, s, live) == 1 << u
    s = stored.copy()
    for u in range(live):
        s[1024 * u + 1023 - u] ^= 1
    assert tile_end(code, s, live) == bytewise(code, s, live) == (1 << live) - 1


@pytest.mark.parametrize("live", [1, 2, 3, 4])
def test_single_wrong_bit_in_every_unit_and_packet(live):
    """Byte 0, 7, 8 and 127 of every packet of every live unit: the first and last byte of a lane's piece, the
    next lane's first, the packet's last."""
    code, stored = tiles(20 + live, live)
    for u in range(live):
        for pkt in range(8):
            for b in (0, 7, 8, 127):
                for bit in (0, 7):
                    s = stored.copy()
                    s[1024 * u + 128 * pkt + b] ^= 1 << bit
                    got = tile_end(code, s, live)
                    assert got == bytewise(code, s, live) == 1 << u, (u, pkt, b, bit, got)


def test_lanes_past_the_chunk_contribute_nothing():
    """With 1, 2, 3 live units the lanes of the other units hold zeros on both sides, whatever lies in memory there."""
    for live in (1, 2, 3):
        code, stored = tiles(30 + live, live)
        assert (code[1024 * live:] != stored[1024 * live:]).all()
        assert tile_end(code, stored, live) == 0
        assert tile_end(code, stored, 4) == (0xF << live) & 0xF


def test_lane_layout_covers_the_tile_once():
    """Every byte of the tile belongs to exactly one (lane, packet) piece."""
    seen = np.zeros(4096, np.int32)
    for lane in range(64):
        for r in range(8):
            q = 1024 * (lane >> 4) + 8 * (lane & 15) + 128 * r
            seen[q:q + 8] += 1
    assert (seen == 1).all()
