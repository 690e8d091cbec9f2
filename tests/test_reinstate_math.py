"""The reinstate kernel's two walks and its slot bookkeeping (tfs_ec_kernels.hip
ec_reinstate_kernel), restated lane by lane on the CPU: the walk
takes a lane's eight 8-byte pieces -- in[] while a source that is a data member
passes by, acc[o][*] of an output that is a data member after the member loop --
and the data member's slot, which selects its rows of first / cont and its records
whatever position the member has among a launch's sources or outputs.  The oracle's
decode provides the rebuilt bytes; every CRC is checked against the oracle's byte
loop, through tests/test_marshal_math.py's fold.  No GPU.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, ocrc
from test_marshal_math import BIAS, FI, POW_N, X128, XPOW, crc0, fold, multmodp
from tfs_amd.synth import synth_bytes

NONE = 0xFFFFFFFF   # kReinstateNoSlot
OUT_GROUP = 4       # kMaxOutGroup


@pytest.fixture(scope="module")
def ec_oracle():
    so = os.path.join(ROOT, "oracle", "liboracle_ec.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle_ec.so"])
    L = ctypes.CDLL(so)
    L.oracle_ec_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.oracle_ec_decode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_int]
    return L


def lane_pieces(member, T, total):
    """pieces[lane][c]: the lane layout of in[c] for a source, and of acc[o][c] for an output, whose stores go to
    base + 128 c: 8 bytes at 4096 T + 1024 (lane >> 4) + 128 c + 8 (lane & 15); zero past the chunk's last unit."""
    out = []
    for lane in range(64):
        unit = 4096 * T + 1024 * (lane >> 4)
        row = []
        for c in range(8):
            q = unit + 128 * c + 8 * (lane & 15)
            row.append(bytes(member[q:q + 8]) if unit < total else bytes(8))
        out.append(row)
    return out


def walk(pieces, T, slot, plan, res):
    """One wave's segment walk over `pieces` for the data member `slot` (the kernels' record_walk)."""
    recs, first, mend, ntiles = plan
    lo, hi = 4096 * T, 4096 * T + 4096
    r = first[slot * ntiles + T]
    while r < mend[slot]:
        H, P1 = recs[r]
        if H >= hi:
            break
        P0 = H + FI
        assert P1 > lo  # first[] never names a record that ends at or before the tile's start: live is all ones
        if P0 > lo:
            for lane in range(64):
                for c in range(8):
                    q = lo + 1024 * (lane >> 4) + 8 * (lane & 15) + 128 * c
                    for b in range(8):
                        if 0 <= q + b - H < FI:
                            assert (r, q + b - H) not in res["hdr"]
                            res["hdr"][(r, q + b - H)] = pieces[lane][c][b]
        if P0 < hi:
            acc = 0
            for lane in range(64):
                u, off = lane >> 4, 8 * (lane & 15)
                c = 0
                for pc in range(8):
                    q = lo + 1024 * u + off + 128 * pc
                    piece = bytes(pieces[lane][pc][b] if P0 <= q + b < P1 else 0 for b in range(8))
                    c = crc0(piece) if pc == 0 else multmodp(X128, c) ^ crc0(piece)
                dl = 3192 - (1024 * u + off)
                pad = 0 if P1 >= hi else hi - P1
                assert 0 <= BIAS + dl - pad < POW_N
                acc ^= multmodp(XPOW[BIAS + dl - pad], c)
            key = ("cont", slot * ntiles + T) if P1 > hi else ("tail", r)
            assert key not in res  # one writer per word, over every launch of the chunk
            res[key] = acc
        r += 1


def make_plan(payloads, ntiles):
    """ec_marshal_plan.h's arrays: recs member after member, first[slot][T], mend[slot]."""
    recs, first, mend = [], [], []
    for pay in payloads:
        begin = len(recs)
        recs += [(p0 - FI, p1) for p0, p1 in pay]
        for t in range(ntiles):
            first.append(next((begin + i for i, (_, p1) in enumerate(pay) if p1 > 4096 * t), len(recs)))
        mend.append(len(recs))
    return recs, first, mend, ntiles


def session(k, m, erased, fam, payloads, total):
    """Every launch of one whole-member chunk, as reinstate_launch lays them out."""
    ntiles = (total + 4095) // 4096
    plan = make_plan(payloads, ntiles)
    sources = [i for i in range(k + m) if erased[i] == 0][:k]
    outputs = [i for i in range(k) if erased[i] != 0] + [i for i in range(k, k + m) if erased[i] == 1]
    res = {"hdr": {}}
    launches = []
    for o0 in range(0, len(outputs), OUT_GROUP):
        group = outputs[o0:o0 + OUT_GROUP]
        src_slot = [s if o0 == 0 and s < k else NONE for s in sources]  # the source walk: the first launch only
        out_slot = [o if o < k else NONE for o in group]
        launches.append((src_slot, out_slot))
        for T in range(ntiles):
            for s, slot in zip(sources, src_slot):
                if slot != NONE:
                    walk(lane_pieces(fam[s], T, total), T, slot, plan, res)
            for o, slot in zip(group, out_slot):
                if slot != NONE:
                    walk(lane_pieces(fam[o], T, total), T, slot, plan, res)
    return plan, res, launches


def payloads_of(k, sizes):
    """Per member: a record inside tile 0, one from tile 0 into tile 1, one that ends exactly on tile 1's end or
    runs into the short last tile; starts and ends at varying residues mod 8."""
    out = []
    for i in range(k):
        a = (41 + i, 1500 + 17 * i)
        b = (a[1] + FI + (i % 3), 4096 + 300 + 9 * i)
        c = (b[1] + FI, 8192 if i % 2 == 0 else min(8192 + 500 + i, sizes[i]))
        assert c[1] <= sizes[i]
        out.append([a, b, c])
    return out


CASES = [
    (3, 2, [0, 1, 0, 0, -1], "data 0 and 2 and parity 0 as sources, data 1 rebuilt"),
    (3, 2, [1, 0, 1, 0, 0], "one data and two parity sources, two data outputs"),
    (6, 6, [1] * 6 + [0] * 6, "six data outputs: four in the first launch, two in the second"),
]


@pytest.mark.parametrize("k,m,erased,what", CASES, ids=[c[3] for c in CASES])
def test_walks_and_slots_against_byte_loop(oracle, ec_oracle, k, m, erased, what):
    total = 2 * 4096 + 1024
    sizes = [total - 100 * i for i in range(k)]
    fam = []
    for i in range(k):
        a = np.zeros(total, np.uint8)
        a[:sizes[i]] = synth_bytes(600 + 10 * k + i, sizes[i])
        fam.append(a)
    fam += [np.zeros(total, np.uint8) for _ in range(m)]
    p = (ctypes.c_void_p * (k + m))(*[a.ctypes.data for a in fam])
    assert ec_oracle.oracle_ec_encode(k, m, p, None, total) == 0
    orig = [a.copy() for a in fam]
    for i in range(k + m):
        if erased[i] != 0:
            fam[i][:] = 0x5A
    assert ec_oracle.oracle_ec_decode(k, m, (ctypes.c_int * (k + m))(*erased), p, None, total) == 0
    assert all((fam[i] == orig[i]).all() for i in range(k + m) if erased[i] != -1 or i < k)
    payloads = payloads_of(k, sizes)
    (recs, first, mend, ntiles), res, launches = session(k, m, erased, fam, payloads, total)
    assert len(launches) == (2 if k == 6 else 1)
    if k == 6:
        assert launches[0] == ([NONE] * 6, [0, 1, 2, 3]) and launches[1] == ([NONE] * 6, [4, 5])
    else:
        assert any(s != NONE for s in launches[0][0]) and any(s == NONE for s in launches[0][0])
    r = 0
    for slot in range(k):  # every record of every data member, surviving and rebuilt, in the caller's order
        for P0, P1 in payloads[slot]:
            cont = {t: res[("cont", slot * ntiles + t)] for t in range(P0 >> 12, (P1 - 1) >> 12)}
            got = fold(P0, P1, cont, res[("tail", r)])
            assert got == ocrc(oracle, 0, fam[slot][P0:P1].tobytes()), (slot, r, P0, P1)
            assert bytes(res["hdr"][(r, j)] for j in range(FI)) == fam[slot][P0 - FI:P0].tobytes()
            r += 1
    assert r == len(recs) == mend[-1]
    n_cont = sum(((P1 - 1) >> 12) - (P0 >> 12) for pay in payloads for P0, P1 in pay)
    assert len(res) == 1 + len(recs) + n_cont  # hdr, one tail per record, one cont per tile a payload runs through


def test_constants_match_the_library_header():
    import re
    src = open(os.path.join(ROOT, "tfs_amd", "csrc", "tfs_ec_device.h")).read()
    assert int(re.search(r"kReinstateNoSlot = (0x[0-9A-Fa-f]+)u;", src).group(1), 16) == NONE
    assert int(re.search(r"kMaxOutGroup = (\d+);", src).group(1)) == OUT_GROUP
