"""Scrub locate (include/tfs_ec.h tfs_ec_locate(_device)): which data member is
wrong in a unit that every parity member flags, and that member's right bytes.

No test restates the locate algorithm.  A family is synth_bytes data and oracle_ec_encode parity;
the test damages known units of known members, and the expected member is the one it damaged,
the expected repaired unit the original unit, diff_bytes the count of bytes it changed, and the
expected parity mask "stored parity differs from oracle_ec_encode of the data as given"
(tests/test_scrub.py's expected).  The device runs prefill results and repaired units with 0xA5 and
download every member afterwards: no member byte was written.

The check "no encoding matrix -> TFS_EXIT_MATRIX_INVALID" cannot be reached from here: a coder
that tfs_ec_config hands out has one unless the device failed during the upload.
"""
import ctypes

import numpy as np
import pytest

from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode)
from test_scrub import encode
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

PARAM, DATA_INVALID, SIZE_INVALID = -1016, -16001, -16002
CLEAN, PARITY, DATA, NONE = 0, 1, 2, 3
SIZE = 32768  # 32 units per member
FILL = 0xA5


def clean_family(ec_oracle, k, m, seed, size=SIZE):  # noqa: F811
    data = [synth_bytes(seed + 17 * i, size) for i in range(k)]
    return data, encode(ec_oracle, k, m, data, size)


def parity_mask(ec_oracle, k, m, data, parity, size, units):  # noqa: F811
    """Per listed unit: bit p set when stored parity p differs from jerasure's code of the data as given."""
    code = encode(ec_oracle, k, m, data, size)
    return [sum(int((parity[p][1024 * u:1024 * u + 1024] != code[p][1024 * u:1024 * u + 1024]).any()) << p
                for p in range(m)) for u in units]


def run_device(ctx, ec, mem, size, units, n, want_fixed=True, stream=None):
    """(result, fixed [n, 1024] or None) of the device form; asserts rc == 0 and that no member was written."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import LOCATE_RESULT_DTYPE
    d = [crc.DeviceBuffer(ctx, size).upload(a) for a in mem]
    d_res = crc.DeviceBuffer(ctx, 8 * n).upload(np.full(8 * n, FILL, np.uint8))
    d_fix = crc.DeviceBuffer(ctx, 1024 * n).upload(np.full(1024 * n, FILL, np.uint8)) if want_fixed else None
    assert ec.locate_device(d, size, units, n, d_res, d_fix, stream=stream) == 0
    ctx.stream_sync(stream) if stream else ctx.sync()
    res = d_res.download(LOCATE_RESULT_DTYPE, n)
    fixed = d_fix.download(np.uint8, 1024 * n).reshape(n, 1024) if want_fixed else None
    for i, (b, a) in enumerate(zip(d, mem)):
        assert (b.download(np.uint8, size) == a).all(), i
    for b in d + [d_res] + ([d_fix] if want_fixed else []):
        b.free()
    return res, fixed


def host_as_device(host, res, fixed):
    """The host form's (result, fixed, rc) against the device form's: the same results, the same repaired units, and
    the rows of entries that are not DATA left as the binding made them (zero) where the device run kept its prefill."""
    hres, hfixed, rc = host
    data = res["kind"] == DATA
    return rc == 0 and (hres == res).all() and (hfixed[data] == fixed[data]).all() and not hfixed[~data].any() and \
        (fixed[~data] == FILL).all()


def judge(res, fixed, units, want, orig, pmask, pn):
    """want: {unit: (kind, member, diff_bytes)} (absent: CLEAN); orig: the undamaged data members."""
    for k, u in enumerate(units):
        kind, member, diff = want.get(u, (CLEAN, -1, 0))
        r = res[k]
        assert (int(r["kind"]), int(r["member"]), int(r["diff_bytes"])) == (kind, member, diff), (k, u, r)
        assert int(r["parity"]) == pmask[k], (k, u, r)
        assert int(r["flags"]) == int(pn >= 3) and int(r["reserved"]) == 0, (k, u, r)
        if fixed is not None:
            if kind == DATA:
                assert (fixed[k] == orig[member][1024 * u:1024 * u + 1024]).all(), (k, u)
            else:
                assert (fixed[k] == FILL).all(), (k, u)


def damage_every_member(k, data, seed):
    """Units 3j, 3j + 1, 3j + 2 of data member j: one bit in byte 0 of packet 0 (lane 0), one bit in byte 127 of
    packet 7 (lane 15), the whole unit randomised.  Returns (hurt data, want)."""
    hurt, want = [a.copy() for a in data], {}
    for j in range(k):
        u = 3 * j
        hurt[j][1024 * u] ^= 1 << (j % 8)
        want[u] = (DATA, j, 1)
        hurt[j][1024 * (u + 1) + 1023] ^= 0x80 >> (j % 8)
        want[u + 1] = (DATA, j, 1)
        noise = synth_bytes(seed + 1000 + j, 1024)
        old = hurt[j][1024 * (u + 2):1024 * (u + 3)].copy()
        hurt[j][1024 * (u + 2):1024 * (u + 3)] = noise
        want[u + 2] = (DATA, j, int((noise != old).sum()))
        assert want[u + 2][2] > 1000
    return hurt, want


@pytest.mark.parametrize("k,m", [(5, 3), (2, 2), (10, 2), (1, 2), (4, 4), (4, 5)])
def test_geometries(gpu_ctx, ec_oracle, k, m):  # noqa: F811
    """Every data member located in turn, three damages each, clean units between; (4, 5) takes a second group of
    syndromes.  Dense form over the whole family, host form beside the device form."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, k, m, 100 * k + m)
    hurt, want = damage_every_member(k, data, 100 * k + m)
    n = SIZE // 1024
    assert 3 * k <= n
    pmask = parity_mask(ec_oracle, k, m, hurt, parity, SIZE, range(n))
    assert all(pmask[u] == (1 << m) - 1 for u in want) and sum(1 for x in pmask if x) == 3 * k
    ec = ErasureCode(gpu_ctx, k, m)
    assert ec.rc == 0
    res, fixed = run_device(gpu_ctx, ec, hurt + parity, SIZE, None, n)
    judge(res, fixed, range(n), want, data, pmask, m)
    given = [a.copy() for a in hurt + parity]
    assert host_as_device(ec.locate(given, SIZE), res, fixed)
    assert all((a == b).all() for a, b in zip(given, hurt + parity))
    ec.free()


@pytest.fixture(scope="module")
def zoo(ec_oracle):  # noqa: F811
    """(5, 3) with every kind: (orig data, hurt data, hurt parity, want)."""
    data, parity = clean_family(ec_oracle, 5, 3, 5300)
    hd, hp, want = [a.copy() for a in data], [a.copy() for a in parity], {}
    hp[0][1024 * 1 + 77] ^= 2
    want[1] = (PARITY, -1, 0)                      # one parity member wrong
    hd[1][1024 * 2 + 500] ^= 0x40
    want[2] = (DATA, 1, 1)
    hp[1][1024 * 3 + 5] ^= 1
    hp[2][1024 * 3 + 900] ^= 0x10
    want[3] = (PARITY, -1, 0)                      # two of three wrong
    hd[0][1024 * 4 + 10] ^= 8
    hd[3][1024 * 4 + 10] ^= 8
    want[4] = (NONE, -1, 0)                        # two data members, the same byte
    hp[1][1024 * 5 + 1023] ^= 0x80
    want[5] = (PARITY, -1, 0)
    hd[2][1024 * 6 + 10] ^= 1
    hd[4][1024 * 6 + 700] ^= 1
    want[6] = (NONE, -1, 0)                        # two data members, different bytes
    hd[1][1024 * 7 + 300] ^= 4
    hp[2][1024 * 7 + 20] ^= 4
    want[7] = (NONE, -1, 0)                        # a data member and a parity member
    noise = synth_bytes(99, 1024)
    want[8] = (DATA, 4, int((noise != hd[4][1024 * 8:1024 * 9]).sum()))
    hd[4][1024 * 8:1024 * 9] = noise
    hd[0][1024 * 31 + 1023] ^= 0x80
    want[31] = (DATA, 0, 1)                        # the member's last byte
    return data, hd, hp, want


LIST = [7, 2, 5, 9, 2, 31, 0, 8, 3]  # unsorted, unit 2 twice; the first tile holds all four kinds


@pytest.mark.parametrize("n", [1, 4, 5, 9])
def test_list_shapes(gpu_ctx, ec_oracle, zoo, n):  # noqa: F811
    """Indexed and dense lists of 1, 4, 5 and 9 entries (a last tile with one valid entry), device and host form."""
    from tfs_amd.ec import ErasureCode
    data, hd, hp, want = zoo
    assert [want.get(u, (CLEAN,))[0] for u in LIST[:4]] == [NONE, DATA, PARITY, CLEAN]
    ec = ErasureCode(gpu_ctx, 5, 3)
    for units in (LIST[:n], None):
        named = units if units is not None else list(range(n))
        pmask = parity_mask(ec_oracle, 5, 3, hd, hp, SIZE, named)
        res, fixed = run_device(gpu_ctx, ec, hd + hp, SIZE, units, n)
        judge(res, fixed, named, want, data, pmask, 3)
        # the host form's dense list is the whole of what it is given: the first n units of every member
        host = ec.locate(hd + hp, SIZE, units=units) if units is not None else ec.locate([a[:1024 * n] for a in hd + hp], 1024 * n)
        assert host_as_device(host, res, fixed)
    ec.free()


def test_every_kind_and_no_fixed(gpu_ctx, ec_oracle, zoo):  # noqa: F811
    """The whole family in one dense call: every kind where the test put it, CLEAN elsewhere; without an output for
    repaired units the results are the same."""
    from tfs_amd.ec import ErasureCode
    data, hd, hp, want = zoo
    n = SIZE // 1024
    pmask = parity_mask(ec_oracle, 5, 3, hd, hp, SIZE, range(n))
    ec = ErasureCode(gpu_ctx, 5, 3)
    res, fixed = run_device(gpu_ctx, ec, hd + hp, SIZE, None, n)
    judge(res, fixed, range(n), want, data, pmask, 3)
    assert sorted(set(res["kind"].tolist())) == [CLEAN, PARITY, DATA, NONE]
    res2, none = run_device(gpu_ctx, ec, hd + hp, SIZE, None, n, want_fixed=False)
    assert none is None and (res2 == res).all()
    hres, hnone, rc = ec.locate(hd + hp, SIZE, want_fixed=False)
    assert rc == 0 and hnone is None and (hres == res).all()
    ec.free()


def test_two_parity_members_are_unconfirmed(gpu_ctx, ec_oracle):  # noqa: F811
    """(5, 2): a single wrong member is located and repaired exactly, a wrong parity unit told apart, and no result
    carries CONFIRMED (asserted in judge)."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 2, 5200)
    hd, hp = [a.copy() for a in data], [a.copy() for a in parity]
    hd[3][1024 * 4 + 600] ^= 0x20
    hp[1][1024 * 9] ^= 1
    want = {4: (DATA, 3, 1), 9: (PARITY, -1, 0)}
    units = [9, 4, 0]
    ec = ErasureCode(gpu_ctx, 5, 2)
    res, fixed = run_device(gpu_ctx, ec, hd + hp, SIZE, units, 3)
    judge(res, fixed, units, want, data, parity_mask(ec_oracle, 5, 2, hd, hp, SIZE, units), 2)
    ec.free()


def test_caller_streams(gpu_ctx, ec_oracle, zoo):  # noqa: F811
    """Two calls with different lists on two streams of the context, neither waited for in between: each has its own
    list's results."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import LOCATE_RESULT_DTYPE, ErasureCode
    data, hd, hp, want = zoo
    ec = ErasureCode(gpu_ctx, 5, 3)
    d = [crc.DeviceBuffer(gpu_ctx, SIZE).upload(a) for a in hd + hp]
    lists = [[2, 8, 31, 4, 1], [6, 0, 2]]
    outs = [(crc.DeviceBuffer(gpu_ctx, 8 * len(u)), crc.DeviceBuffer(gpu_ctx, 1024 * len(u)).upload(
        np.full(1024 * len(u), FILL, np.uint8))) for u in lists]
    streams = [gpu_ctx.stream_create(), gpu_ctx.stream_create()]
    try:
        for u, (r, f), s in zip(lists, outs, streams):
            assert ec.locate_device(d, SIZE, list(u), len(u), r, f, stream=s) == 0
        for u, (r, f), s in zip(lists, outs, streams):
            gpu_ctx.stream_sync(s)
            res = r.download(LOCATE_RESULT_DTYPE, len(u))
            fixed = f.download(np.uint8, 1024 * len(u)).reshape(len(u), 1024)
            judge(res, fixed, u, want, data, parity_mask(ec_oracle, 5, 3, hd, hp, SIZE, u), 3)
        for b, a in zip(d, hd + hp):
            assert (b.download(np.uint8, SIZE) == a).all()
    finally:
        for s in streams:
            gpu_ctx.stream_destroy(s)
        ec.free()


def test_host_form_in_pieces(gpu_ctx, ec_oracle, zoo):  # noqa: F811
    """Nine entries through staging pieces of four (include/tfs_crc_testing.h): three pieces, the last with one entry,
    the same results as the device form and as one piece."""
    from tfs_amd.ec import ErasureCode
    data, hd, hp, want = zoo
    ec = ErasureCode(gpu_ctx, 5, 3)
    res, fixed = run_device(gpu_ctx, ec, hd + hp, SIZE, LIST, len(LIST))
    whole = ec.locate(hd + hp, SIZE, units=LIST)
    assert ec.L.tfs_ec_locate_set_piece(ec.h, 4) == 0
    pieces = ec.locate(hd + hp, SIZE, units=LIST)
    dense = ec.locate(hd + hp, SIZE)                # eight pieces of four
    assert ec.L.tfs_ec_locate_set_piece(ec.h, 0) == 0
    for got in (whole, pieces):
        assert host_as_device(got, res, fixed)
    n = SIZE // 1024
    dres, dfixed = run_device(gpu_ctx, ec, hd + hp, SIZE, None, n)
    judge(dres, dfixed, range(n), want, data, parity_mask(ec_oracle, 5, 3, hd, hp, SIZE, range(n)), 3)
    assert host_as_device(dense, dres, dfixed)
    ec.free()


def test_refused_calls(gpu_ctx, ec_oracle, zoo):  # noqa: F811
    """Every check in the header's order -- a call that fails two of them gets the earlier status -- with nothing
    written, then a clean call on the same coder."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import LOCATE_RESULT_DTYPE, ErasureCode
    data, hd, hp, want = zoo
    mem = hd + hp
    ec = ErasureCode(gpu_ctx, 5, 3)
    one = ErasureCode(gpu_ctx, 2, 1)
    L = ec.L
    res = np.full(32, FILL, np.uint8)
    u32 = ctypes.c_uint32

    def host(h, members, size, units, n, result=res):
        p = (ctypes.c_void_p * len(members))(*[None if a is None else a.ctypes.data for a in members])
        u = None if units is None else (u32 * len(units))(*units)
        return L.tfs_ec_locate(h, p, size, u, n, None if result is None else result.ctypes.data, None)
    assert host(None, mem, SIZE, [1], 1) == PARAM
    assert host(one.h, mem[:3], 1000, [1], 1) == PARAM                     # pn < 2 comes before the size
    assert host(ec.h, [None] + mem[1:], 0, [1], 1) == SIZE_INVALID         # the size before the members
    assert host(ec.h, mem, 1000, [1], 1) == SIZE_INVALID and host(ec.h, mem, -1024, [1], 1) == SIZE_INVALID
    assert host(ec.h, mem[:7] + [None], SIZE, [99], 1) == DATA_INVALID     # a NULL parity member before the bounds
    assert host(ec.h, [None] + mem[1:], SIZE, [1], 1) == DATA_INVALID
    assert host(ec.h, mem, SIZE, [0, 32], 2, result=None) == PARAM         # unit 32 of 32 before the result
    assert host(ec.h, mem, SIZE, [0xFFFFFFFF], 1) == PARAM and host(ec.h, mem, SIZE, None, 33) == PARAM
    assert host(ec.h, mem, 1024, [1], 1) == PARAM
    assert host(ec.h, mem, SIZE, [1], 1, result=None) == PARAM
    assert host(ec.h, mem, SIZE, None, 0, result=None) == 0 and host(ec.h, mem, SIZE, [], 0) == 0
    assert (res == FILL).all()
    # the device form: the same checks, and hipStreamPerThread
    d = [crc.DeviceBuffer(gpu_ctx, SIZE).upload(a) for a in mem]
    d_res = crc.DeviceBuffer(gpu_ctx, 32).upload(res)
    assert L.tfs_ec_locate_device(None, None, SIZE, None, 1, d_res.ptr, None, None) == PARAM
    assert one.locate_device(d[:3], SIZE, [1], 1, d_res) == PARAM
    assert ec.locate_device(d, 1000, [1], 1, d_res) == SIZE_INVALID
    assert ec.locate_device(d[:2] + [None] + d[3:], SIZE, [1], 1, d_res) == DATA_INVALID
    assert ec.locate_device(d, SIZE, [3, 32], 2, d_res) == PARAM and ec.locate_device(d, SIZE, None, 33, d_res) == PARAM
    assert ec.locate_device(d, SIZE, [1], 1, d_res, stream=2) == PARAM     # hipStreamPerThread
    assert ec.locate_device(d, SIZE, [1], 1, None) == PARAM
    assert ec.locate_device(d, SIZE, None, 0, None) == 0
    gpu_ctx.sync()
    assert (d_res.download(np.uint8, 32) == FILL).all()
    # the coder still works
    assert ec.locate_device(d, SIZE, [2, 1, 4, 0], 4, d_res) == 0
    gpu_ctx.sync()
    got = d_res.download(LOCATE_RESULT_DTYPE, 4)
    judge(got, None, [2, 1, 4, 0], want, data, parity_mask(ec_oracle, 5, 3, hd, hp, SIZE, [2, 1, 4, 0]), 3)
    hres, _, rc = ec.locate(mem, SIZE, units=[2, 1, 4, 0], want_fixed=False)
    assert rc == 0 and (hres == got).all()
    one.free()
    ec.free()
