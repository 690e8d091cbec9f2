"""The marshalling kernels' CRC arithmetic (tfs_ec_kernels.hip record_walk as
ec_marshal_kernel calls it / ec_marshal_fold_kernel), restated step by step on the CPU against
the oracle's byte loop: the lanes' chains over their eight masked pieces with the
128-byte step, the move to the segment's end with one power (inverse powers below
the bias), cont / tail, and the fold's lane runs.  No GPU.
"""
import numpy as np

from conftest import ocrc
from tfs_amd.synth import synth_bytes

POLY = 0xEDB88320
FI = 36
BIAS = 4095            # kMarshalPowBias
POW_N = BIAS + 4096 + 1


def multmodp(a, b):
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x2n(n):
    """x^n mod P."""
    p, sq = 1 << 31, 1 << 30
    while n:
        if n & 1:
            p = multmodp(sq, p)
        sq = multmodp(sq, sq)
        n >>= 1
    return p


BYTE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ POLY if _c & 1 else _c >> 1
    BYTE.append(_c)
G, GI = x2n(8), x2n(0xFFFFFFFF - 8)
XPOW = [0] * POW_N
XPOW[BIAS] = 1 << 31
for _i in range(BIAS + 1, POW_N):
    XPOW[_i] = multmodp(G, XPOW[_i - 1])
for _i in range(BIAS - 1, -1, -1):
    XPOW[_i] = multmodp(GI, XPOW[_i + 1])
X128 = x2n(8 * 128)
X4K = x2n(8 * 4096)


def crc0(bs):
    c = 0
    for b in bs:
        c = BYTE[(c ^ b) & 255] ^ (c >> 8)
    return c


def tile_pass(img, t, recs, first):
    """One wave's CRC side for tile t of one member: {('cont', t) | ('tail', r): value}, and header bytes."""
    lo, hi = 4096 * t, 4096 * t + 4096
    out, hdr = {}, {}
    r = first
    while r < len(recs):
        H, P1 = recs[r]
        if H >= hi:
            break
        P0 = H + FI
        for p in range(max(H, lo), min(P0, hi)):
            assert (r, p - H) not in hdr
            hdr[(r, p - H)] = int(img[p]) if p < len(img) else 0
        if P0 < hi:
            acc = 0
            for lane in range(64):
                u, off = lane >> 4, 8 * (lane & 15)
                c = 0
                for pc in range(8):
                    q = lo + 1024 * u + off + 128 * pc
                    piece = bytes((int(img[q + b]) if P0 <= q + b < P1 and q + b < len(img) else 0) for b in range(8))
                    c = crc0(piece) if pc == 0 else multmodp(X128, c) ^ crc0(piece)
                dl = 3192 - (1024 * u + off)
                pad = 0 if P1 >= hi else hi - P1
                assert 0 <= BIAS + dl - pad < POW_N
                acc ^= multmodp(XPOW[BIAS + dl - pad], c)
            key = ("cont", t) if P1 > hi else ("tail", r)
            assert key not in out  # one writer
            out[key] = acc
        r += 1
    return out, hdr


def fold(P0, P1, cont, tail):
    t0, tl = P0 >> 12, (P1 - 1) >> 12
    nc = tl - t0
    c = 0
    if nc:
        R = (nc + 63) // 64
        for lane in range(64):
            b = min(t0 + lane * R, tl)
            e = min(b + R, tl)
            v = 0
            for t in range(b, e):
                v = multmodp(X4K, v) ^ cont[t]
            c ^= multmodp(x2n(8 * 4096 * (tl - e)), v)
    d = P1 - (tl << 12)
    assert 1 <= d <= 4096
    return multmodp(XPOW[BIAS + d], c) ^ tail


def layout():
    """Payload ranges [P0, P1): starts and ends at every residue mod 8, and on either side of
    128, 1024 and 4096 byte boundaries; a 1-byte payload; one payload across three tiles."""
    pay, pos = [(41, 42)], 42
    for s in range(8):
        for e in range(8):
            p0 = (pos + FI + 7) // 8 * 8 + s
            p1 = p0 + 8 + ((e - s) % 8)
            pay.append((p0, p1))
            pos = p1
    base = (pos + 4095) // 4096 * 4096
    for q in (128, 1024, 4096):
        for ds in (-1, 0, 1):
            pay.append((base + q + ds, base + q + ds + 60))           # starts around the boundary
            pay.append((base + q + 1500 + ds, base + 4096 + q + ds))  # ends around it, from the tile before
            base += 8192
    pay.append((base + 100, base + 3 * 4096 - 5))
    return pay, base + 3 * 4096 + 1024


def test_pass_and_fold_against_byte_loop(oracle):
    pay, size = layout()
    img = synth_bytes(4242, size)
    recs = [(p0 - FI, p1) for p0, p1 in pay]
    assert all(a[1] <= b[0] for a, b in zip(recs, recs[1:]))
    ntiles = (size + 4095) // 4096
    cont, tail, hdr = {}, {}, {}
    for t in range(ntiles):
        first = next((i for i, (_, p1) in enumerate(recs) if p1 > 4096 * t), len(recs))
        out, h = tile_pass(img, t, recs, first)
        for (kind, k), v in out.items():
            (cont if kind == "cont" else tail)[k] = v
        assert not set(h) & set(hdr)
        hdr.update(h)
    starts = {p0 % 8 for p0, _ in pay}
    ends = {p1 % 8 for _, p1 in pay}
    assert starts == ends == set(range(8))
    for r, (H, P1) in enumerate(recs):
        got = fold(H + FI, P1, cont, tail[r])
        assert got == ocrc(oracle, 0, img[H + FI:P1].tobytes()), (r, H, P1)
        assert bytes(hdr[(r, i)] for i in range(FI)) == img[H:H + FI].tobytes()


def test_fold_lane_runs(oracle):
    """The fold alone, over records of 1 .. 200 tiles with cont / tail from the byte loop:
    one tile per lane, several tiles per lane, lanes without a tile."""
    img = synth_bytes(99, 201 * 4096 + 5000)
    for P0, P1 in [(4096 + 17, 2 * 4096), (100, 63 * 4096 + 9), (4000, 65 * 4096 + 4096), (5, 66 * 4096 + 1),
                   (4096 * 3, 4096 * 134 - 1), (77, 200 * 4096 + 4321)]:
        t0, tl = P0 >> 12, (P1 - 1) >> 12
        cont = {t: ocrc(oracle, 0, img[max(P0, 4096 * t):4096 * t + 4096].tobytes()) for t in range(t0, tl)}
        tail = ocrc(oracle, 0, img[max(P0, 4096 * tl):P1].tobytes())
        assert fold(P0, P1, cont, tail) == ocrc(oracle, 0, img[P0:P1].tobytes()), (P0, P1)


def test_tables_match_the_library_header():
    """The restatement's constants are the kernel's (tfs_ec_device.h)."""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "tfs_amd", "csrc", "tfs_ec_device.h")).read()
    assert int(re.search(r"kMarshalPowBias = (\d+);", src).group(1)) == BIAS
    assert re.search(r"kMarshalPowN = kMarshalPowBias \+ 4096 \+ 1;", src)
    assert multmodp(XPOW[0], XPOW[2 * BIAS]) == 1 << 31  # x^-4095 bytes times x^+4095 bytes
