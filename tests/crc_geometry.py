"""The stripe geometry of the CRC kernels, restated for the tests.

`make_geo` in tfs_amd/csrc/tfs_crc_kernels.hip lays a payload out in stripes of
64 lanes x RUN bytes.  For RUN = 16 (the only run length of the product
library) the stripe grid is anchored at E, the payload's last 16-byte boundary
B16 rounded up to a 128-byte line (plus the record kernels' anchor offset
`aoff`).  A non-zero initial register is XORed into the first four message
bytes, starting in the dword at A = start & ~3; when the payload starts inside
that dword (s = start - A != 0) and A is the last dword of stripe 0, the high
seed bytes belong to lane 0's first dword of stripe 1 and the kernels carry
them there (`inj` in lane_chain and wg_file_crc).  That only happens when

    A + 4 == sb0 + 1024   <=>   start = 124 + s (mod 128)  [aoff = 0]

so it depends on the payload's absolute (device) address, not on its offset in
a buffer.  This module computes the geometry from an absolute address, builds
the payload shapes that reach the edge in closed form, and checks that a list
of placed cases covers every class of them.  Plain Python, no GPU.
"""
from collections import namedtuple

RUN = 16
STRIPE = 64 * RUN          # bytes per stripe
LINE = 128                 # the anchor's granule
MIN_PARALLEL_LEN = 32      # kMinParallelLen: shorter payloads take the byte loop

Geo = namedtuple("Geo", "start end A s B16 E nstripes sb0 nvalid")

# The classes of the edge the GPU tests must reach.
EDGE_S = (1, 2, 3)                 # start - A: 3, 2 or 1 seed bytes stay in stripe 0
EDGE_NS = (2, 3, 17, 18, 33)       # stripe 1 last / a middle one / the latency form's 16 waves wrapping once, twice
EDGE_D = (0, 16, 112)              # E - B16: nvalid 64, 63, 57
EDGE_T = (0, 1, 15)                # tail bytes after B16

Edge = namedtuple("Edge", "s ns d t residue length")


def geo(addr, length, aoff=0):
    """make_geo<16>(addr, length, seed, aoff): the wave-uniform geometry."""
    assert aoff % 16 == 0 and 0 <= aoff < LINE
    start, end = addr, addr + length
    A = start & ~3
    B16 = end & ~15
    E = ((B16 - aoff + LINE - 1) & ~(LINE - 1)) + aoff
    nvalid = 64 - (E - B16) // RUN
    body = E - A if length >= MIN_PARALLEL_LEN else 0
    nstripes = (body + STRIPE - 1) // STRIPE
    sb0 = E - nstripes * STRIPE
    return Geo(start, end, A, start - A, B16, E, nstripes, sb0, nvalid)


def seed_crosses(addr, length, aoff=0):
    """True when the seed's high bytes land in stripe 1 (the kernels' `inj`)."""
    g = geo(addr, length, aoff)
    return length >= MIN_PARALLEL_LEN and g.s != 0 and g.A + 4 == g.sb0 + STRIPE


def edge_length(s, ns, d, t):
    """The payload length that starts at residue 124 + s and crosses with these parameters."""
    assert s in (1, 2, 3) and ns >= 2 and d % 16 == 0 and 0 <= d <= 112 and 0 <= t <= 15
    return STRIPE * (ns - 1) + 4 - s - d + t


def edge_case(s, ns, d, t):
    return Edge(s, ns, d, t, (124 + s) % LINE, edge_length(s, ns, d, t))


def edge_cases(ss=EDGE_S, nss=EDGE_NS, ds=EDGE_D, ts=EDGE_T):
    """The edge list of the GPU tests: 3 x 5 x 3 x 3 = 135 shapes."""
    return [edge_case(s, ns, d, t) for s in ss for ns in nss for d in ds for t in ts]


def neighbours(e):
    """The two placements next to an edge case that do not cross: the same length
    one dword-aligned (residue 124 + 0) and one dword earlier (residue 120 + s)."""
    return [(124, e.length), (120 + e.s, e.length)]


def classify(addr, length, aoff=0):
    """(s, ns, d) of a placed payload that crosses, None when it does not."""
    if not seed_crosses(addr, length, aoff):
        return None
    g = geo(addr, length, aoff)
    return (g.s, g.nstripes, g.E - g.B16)


def place(cursor, residue, align=LINE):
    """The first address >= cursor with addr % align == residue."""
    return cursor + (residue - cursor) % align


def edge_layout(base_addr, cases=None, slack=LINE):
    """Offsets from `base_addr` (the absolute device address of a buffer) at which
    the edge list and its neighbours sit: [(offset, length, is_edge)].  The two
    neighbours of a case overlap it, s and 4 bytes ahead of it; at least `slack`
    bytes follow every payload before the next group begins (the CRC batches read
    any bytes of their buffer, so overlapping payloads are fine there)."""
    out = []
    cursor = base_addr + 8
    for e in cases if cases is not None else edge_cases():
        x = place(cursor, e.residue)
        out.append((x - base_addr, e.length, True))
        out.append((x - e.s - base_addr, e.length, False))       # residue 124 + 0
        out.append((x - 4 - base_addr, e.length, False))         # residue 120 + s
        cursor = x + e.length + slack
    return out


def edge_layout_cap(cases=None, slack=LINE):
    """Bytes that hold edge_layout at any base address, with 256 bytes to spare."""
    return max(o + n for o, n, _ in edge_layout(0, cases, slack)) + LINE + 256


def assert_edge_coverage(cases, aoff=0):
    """`cases`: (absolute device address, length) pairs as a test actually placed
    them.  Fails unless at least one of them crosses in every (s, ns, d) class of
    the edge list -- an empty or lopsided list cannot pass silently."""
    seen = set()
    for addr, length in cases:
        k = classify(int(addr), int(length), aoff)
        if k is not None:
            seen.add(k)
    want = {(s, ns, d) for s in EDGE_S for ns in EDGE_NS for d in EDGE_D}
    missing = sorted(want - seen)
    assert not missing, "stripe-0 seed edge not reached for (s, ns, d) in %r (%d placed cases, %d classes seen)" % (
        missing[:8], len(cases), len(seen))
    return seen
