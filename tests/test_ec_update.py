"""Parity update (include/tfs_ec.h tfs_ec_update(_device)): a data member's in-place
change carried into the stored parity from the delta of that member alone.

No test restates the code.  A family is synth_bytes data and oracle_ec_encode parity; expected
parity bytes are jerasure's encode of the data with the new bytes, or -- where the stored parity is
not the code of anything -- the parity as it was XOR jerasure's encode of a family that is zero
except for the changed member = the delta.  The device runs give parity members that are not bound
a buffer of 0xA5 and download every buffer afterwards: a member that is not bound, a unit that is
not listed and the delta buffers themselves are as they were.

The check "no encoding matrix -> TFS_EXIT_MATRIX_INVALID" cannot be reached from here: a coder
that tfs_ec_config hands out has one unless the device failed during the upload.
"""
import ctypes
import itertools

import numpy as np
import pytest

from test_reinstate import ec_oracle  # noqa: F401  (the fixture: jerasure's encode)
from test_scrub import encode
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

PARAM, DATA_INVALID, SIZE_INVALID = -1016, -16001, -16002
SIZE = 32768  # 32 units per member
NU = SIZE // 1024
FILL = 0xA5


def clean_family(ec_oracle, k, m, seed, size=SIZE):  # noqa: F811
    data = [synth_bytes(seed + 17 * i, size).copy() for i in range(k)]
    return data, encode(ec_oracle, k, m, data, size)


def units_of(arr, units):
    """The listed units of a member, side by side: the layout of the delta buffers."""
    return np.concatenate([arr[1024 * u:1024 * u + 1024] for u in units]) if len(units) else np.zeros(0, np.uint8)


def parity_change(ec_oracle, k, m, j, size, units, delta):  # noqa: F811
    """jerasure's parity of a family that is zero except for member j, which holds delta slot i in unit units[i]."""
    fam = [np.zeros(size, np.uint8) for _ in range(k)]
    for i, u in enumerate(units):
        fam[j][1024 * u:1024 * u + 1024] = delta[1024 * i:1024 * i + 1024]
    return encode(ec_oracle, k, m, fam, size)


def run_device(ctx, ec, parity, size, member, a, b, units, n, bound=None, stream=None, want_rc=0):
    """The parity members after the device form.  parity: pn arrays; bound: the members passed to the call (default
    all); the others get a buffer of FILL that must come back as FILL.  Asserts rc and that a and b were not written."""
    import tfs_amd.crc as crc
    pn = len(parity)
    bound = range(pn) if bound is None else bound
    d_par = [crc.DeviceBuffer(ctx, size).upload(parity[p] if p in bound else np.full(size, FILL, np.uint8)) for p in range(pn)]
    d_a = crc.DeviceBuffer(ctx, max(a.size, 1024)).upload(a) if a is not None else None
    d_b = crc.DeviceBuffer(ctx, max(b.size, 1024)).upload(b) if b is not None else None
    rc = ec.update_device([d if p in bound else None for p, d in enumerate(d_par)], size, member, d_a, d_b, units, n, stream=stream)
    assert rc == want_rc, rc
    ctx.stream_sync(stream) if stream else ctx.sync()
    out = [d.download(np.uint8, size) for d in d_par]
    for p in range(pn):
        if p not in bound:
            assert (out[p] == FILL).all(), p
    for d, h in ((d_a, a), (d_b, b)):
        if d is not None:
            assert (d.download(np.uint8, h.size) == h).all()
            d.free()
    for d in d_par:
        d.free()
    return out


def same(got, want):
    return all((g == w).all() for g, w in zip(got, want))


def unlisted_as_before(got, before, units):
    keep = np.ones(NU, bool)
    keep[list(units)] = False
    return all((g.reshape(-1, 1024)[keep[:g.size // 1024]] == b.reshape(-1, 1024)[keep[:g.size // 1024]]).all()
               for g, b in zip(got, before))


@pytest.mark.parametrize("k,m", [(5, 3), (2, 2), (10, 2), (1, 2), (4, 4), (4, 5)])
def test_geometries(gpu_ctx, ec_oracle, k, m):  # noqa: F811
    """Every data member in turn: new bytes in three units, a = old, b = new.  Every parity member is then jerasure's
    encode of the new data, the unlisted units are as they were, and a and b swapped give the same bytes."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, k, m, 100 * k + m)
    ec = ErasureCode(gpu_ctx, k, m)
    assert ec.rc == 0
    for j in range(k):
        units = [(3 * j + 2) % NU, (3 * j) % NU, NU - 1 - j]  # unsorted
        assert len(set(units)) == 3
        new = [a.copy() for a in data]
        for i, u in enumerate(units):
            new[j][1024 * u:1024 * u + 1024] = synth_bytes(9000 + 10 * j + i, 1024)
        want = encode(ec_oracle, k, m, new, SIZE)
        assert not same(want, parity)
        old_u, new_u = units_of(data[j], units), units_of(new[j], units)
        got = run_device(gpu_ctx, ec, parity, SIZE, j, old_u, new_u, units, 3)
        assert same(got, want), j
        assert unlisted_as_before(got, parity, units), j
        assert same(run_device(gpu_ctx, ec, parity, SIZE, j, new_u, old_u, units, 3), want), j
    ec.free()


def test_delta_only_form(gpu_ctx, ec_oracle):  # noqa: F811
    """b == NULL with a = old ^ new: the bytes of the two-buffer form, and jerasure's."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5310)
    units, j = [30, 4, 17, 5], 2
    new = [a.copy() for a in data]
    for i, u in enumerate(units):
        new[j][1024 * u:1024 * u + 1024] = synth_bytes(77 + i, 1024)
    old_u, new_u = units_of(data[j], units), units_of(new[j], units)
    ec = ErasureCode(gpu_ctx, 5, 3)
    two = run_device(gpu_ctx, ec, parity, SIZE, j, old_u, new_u, units, 4)
    one = run_device(gpu_ctx, ec, parity, SIZE, j, old_u ^ new_u, None, units, 4)
    assert same(one, two) and same(one, encode(ec_oracle, 5, 3, new, SIZE))
    ec.free()


@pytest.mark.parametrize("k,m,j", [(5, 3, 4), (4, 5, 0)])
def test_stale_parity(gpu_ctx, ec_oracle, k, m, j):  # noqa: F811
    """Parity members of random bytes: after ^ before is jerasure's encode of a family that is zero except member j =
    the delta, and zero in the unlisted units."""
    from tfs_amd.ec import ErasureCode
    before = [synth_bytes(4000 + p, SIZE).copy() for p in range(m)]
    units = [9, 0, 31, 16, 2]
    a, b = synth_bytes(4100, 1024 * 5).copy(), synth_bytes(4101, 1024 * 5).copy()
    ec = ErasureCode(gpu_ctx, k, m)
    got = run_device(gpu_ctx, ec, before, SIZE, j, a, b, units, 5)
    change = parity_change(ec_oracle, k, m, j, SIZE, units, a ^ b)
    assert same([g ^ x for g, x in zip(got, before)], change)
    assert unlisted_as_before(got, before, units)
    assert all(c.reshape(-1, 1024)[u].any() for c in change for u in units)
    ec.free()


def test_sparse_deltas(gpu_ctx, ec_oracle):  # noqa: F811
    """One bit in byte 0 of packet 0 (lane 0's first dword), one bit in byte 127 of packet 7 (lane 15's last), a
    36-byte change that straddles a unit boundary, and a listed unit whose delta is zero."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5320)
    j = 3
    new = [a.copy() for a in data]
    new[j][1024 * 6] ^= 0x01                       # unit 6: byte 0 of packet 0
    new[j][1024 * 21 + 1023] ^= 0x80               # unit 21: byte 127 of packet 7
    at = 1024 * 12 - 20                            # units 11 and 12: a FileInfo's 36 bytes over the boundary
    new[j][at:at + 36] = synth_bytes(5, 36)
    units = [21, 11, 6, 12, 27]                    # unit 27: nothing changes there
    old_u, new_u = units_of(data[j], units), units_of(new[j], units)
    assert int(np.count_nonzero(old_u ^ new_u)) <= 2 + 36 and not (old_u ^ new_u)[4096:].any()
    want = encode(ec_oracle, 5, 3, new, SIZE)
    ec = ErasureCode(gpu_ctx, 5, 3)
    got = run_device(gpu_ctx, ec, parity, SIZE, j, old_u, new_u, units, 5)
    assert same(got, want) and unlisted_as_before(got, parity, units)
    assert all((g[1024 * 27:1024 * 28] == p[1024 * 27:1024 * 28]).all() for g, p in zip(got, parity))
    assert all(not (g[1024 * u:1024 * u + 1024] == p[1024 * u:1024 * u + 1024]).all() for g, p in zip(got, parity) for u in units[:4])
    zero = run_device(gpu_ctx, ec, parity, SIZE, j, np.zeros(2048, np.uint8), None, [3, 8], 2)  # an all-zero delta
    assert same(zero, parity)
    ec.free()


def test_bound_subset(gpu_ctx, ec_oracle):  # noqa: F811
    """Only parity 1 bound: the other members' device buffers are untouched (run_device's FILL).  Every subset of a
    pn = 3 family gives the full call's bytes for the members it binds."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5330)
    units, j = [1, 2, 3, 29, 7], 0
    a, b = units_of(data[j], units), synth_bytes(88, 1024 * 5).copy()
    new = [x.copy() for x in data]
    for i, u in enumerate(units):
        new[j][1024 * u:1024 * u + 1024] = b[1024 * i:1024 * i + 1024]
    want = encode(ec_oracle, 5, 3, new, SIZE)
    ec = ErasureCode(gpu_ctx, 5, 3)
    full = run_device(gpu_ctx, ec, parity, SIZE, j, a, b, units, 5)
    assert same(full, want)
    for r in (1, 2, 3):
        for bound in itertools.combinations(range(3), r):
            got = run_device(gpu_ctx, ec, parity, SIZE, j, a, b, units, 5, bound=bound)
            assert all((got[p] == want[p]).all() for p in bound), bound
    ec.free()


ORDER = [13, 0, 31, 7, 22, 1, 30, 16, 9, 4, 27, 18, 2, 25, 11, 6, 20, 29, 3, 15, 24, 8, 17, 28, 5, 14, 21, 10, 26, 19, 12, 23]


def test_lists(gpu_ctx, ec_oracle):  # noqa: F811
    """Lists of 1, 3, 4, 5, 16, 17 and 32 units -- unsorted, with unit 0 and the last unit from n = 3 on; 16 travels
    in the launch arguments and 17 is uploaded, and the two agree on the 16 units they share -- and the dense form."""
    from tfs_amd.ec import ErasureCode
    assert sorted(ORDER) == list(range(NU))
    before = [synth_bytes(4200 + p, SIZE).copy() for p in range(3)]
    delta = synth_bytes(4300, SIZE).copy()          # slot i belongs to unit ORDER[i], whatever the list's length
    ec = ErasureCode(gpu_ctx, 5, 3)
    got = {}
    for n in (1, 3, 4, 5, 16, 17, 32):
        units = ORDER[:n]
        got[n] = run_device(gpu_ctx, ec, before, SIZE, 1, delta[:1024 * n], None, units, n)
        change = parity_change(ec_oracle, 5, 3, 1, SIZE, units, delta[:1024 * n])
        assert same([g ^ x for g, x in zip(got[n], before)], change), n
        assert unlisted_as_before(got[n], before, units), n
    for g16, g17, x in zip(got[16], got[17], before):
        r16, r17, rx = g16.reshape(-1, 1024), g17.reshape(-1, 1024), x.reshape(-1, 1024)
        assert (r16[ORDER[:16]] == r17[ORDER[:16]]).all() and (r16[ORDER[16]] == rx[ORDER[16]]).all()
        assert (r17[ORDER[16]] != rx[ORDER[16]]).any()
    for n in (1, 5, 32):                              # the dense form: entry k is unit k
        dense = run_device(gpu_ctx, ec, before, SIZE, 1, delta[:1024 * n], None, None, n)
        change = parity_change(ec_oracle, 5, 3, 1, SIZE, range(n), delta[:1024 * n])
        assert same([g ^ x for g, x in zip(dense, before)], change), n
    ec.free()


def test_one_unit_members(gpu_ctx, ec_oracle):  # noqa: F811
    """size = 1024: one unit per member, by list and dense."""
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5340, size=1024)
    new = [a.copy() for a in data]
    new[4] = synth_bytes(61, 1024).copy()
    want = encode(ec_oracle, 5, 3, new, 1024)
    ec = ErasureCode(gpu_ctx, 5, 3)
    assert same(run_device(gpu_ctx, ec, parity, 1024, 4, data[4], new[4], [0], 1), want)
    assert same(run_device(gpu_ctx, ec, parity, 1024, 4, data[4], new[4], None, 1), want)
    ec.free()


def test_refused_calls(gpu_ctx, ec_oracle):  # noqa: F811
    """Every check in the header's order -- a call that fails two of them gets the earlier status -- with no parity byte
    written, then a clean call on the same coder."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5350)
    ec = ErasureCode(gpu_ctx, 5, 3)
    L = ec.L
    a = synth_bytes(1, 1024 * 20).copy()
    host = [p.copy() for p in parity]
    u32 = ctypes.c_uint32

    def h(handle, member, par, size, units, n, a=a, b=None):
        p = None if par is None else (ctypes.c_void_p * len(par))(*[None if x is None else x.ctypes.data for x in par])
        u = None if units is None else (u32 * max(len(units), 1))(*units)
        return L.tfs_ec_update(handle, member, p, size, u, n, None if a is None else a.ctypes.data,
                               None if b is None else b.ctypes.data)
    assert h(None, 99, None, 1000, [1], 1) == PARAM                       # 1: ec NULL before everything
    assert h(ec.h, 5, host, 1000, [1], 1) == PARAM                        # 3: the member before the size
    assert h(ec.h, -1, host, SIZE, [1], 1) == PARAM
    assert h(ec.h, 0, None, 1000, [1], 1) == SIZE_INVALID                 # 4: the size before the parity members
    assert h(ec.h, 0, host, 0, [1], 1) == SIZE_INVALID and h(ec.h, 0, host, -1024, [1], 1) == SIZE_INVALID
    assert h(ec.h, 0, None, SIZE, [99], 1) == DATA_INVALID                # 5: no parity before the bounds
    assert h(ec.h, 0, [None, None, None], SIZE, [99], 1) == DATA_INVALID
    assert h(ec.h, 0, host, SIZE, [3, 32, 3], 3, a=None) == PARAM         # 6: unit 32 of 32 (and a duplicate, and no a)
    assert h(ec.h, 0, host, SIZE, [0xFFFFFFFF], 1) == PARAM and h(ec.h, 0, host, SIZE, None, 33) == PARAM
    assert h(ec.h, 0, host, 1024, [1], 1) == PARAM
    assert h(ec.h, 0, host, SIZE, [3, 7, 3], 3, a=None) == PARAM          # 7: a unit named twice, short list
    assert h(ec.h, 0, host, SIZE, list(range(19)) + [5], 20) == PARAM     # ... and a list past the in-arguments limit
    assert h(ec.h, 0, host, SIZE, [], 0, a=None) == 0 and h(ec.h, 0, host, SIZE, None, 0, a=None) == 0   # 8 before 9
    assert h(ec.h, 0, host, SIZE, [1], 1, a=None) == PARAM                # 9: a NULL
    assert same(host, parity)
    # the device form: the same checks and hipStreamPerThread; a duplicate, an out-of-range unit and the refused
    # stream leave every parity byte as it was
    d = [crc.DeviceBuffer(gpu_ctx, SIZE).upload(p) for p in parity]
    d_a = crc.DeviceBuffer(gpu_ctx, a.size).upload(a)
    assert L.tfs_ec_update_device(None, 0, None, SIZE, None, 1, d_a.ptr, None, None) == PARAM
    assert ec.update_device(d, 1000, 5, d_a, None, [1], 1) == PARAM
    assert ec.update_device(d, 1000, 0, d_a, None, [1], 1) == SIZE_INVALID
    assert ec.update_device([None] * 3, SIZE, 0, d_a, None, [99], 1) == DATA_INVALID
    assert ec.update_device(d, SIZE, 0, d_a, None, [3, 32], 2) == PARAM and ec.update_device(d, SIZE, 0, d_a, None, None, 33) == PARAM
    assert ec.update_device(d, SIZE, 0, d_a, None, [4, 9, 4], 3) == PARAM
    assert ec.update_device(d, SIZE, 0, d_a, None, list(range(19)) + [18], 20) == PARAM
    assert ec.update_device(d, SIZE, 0, d_a, None, [1], 1, stream=2) == PARAM     # hipStreamPerThread
    assert ec.update_device(d, SIZE, 0, None, None, None, 0) == 0
    assert ec.update_device(d, SIZE, 0, None, None, [1], 1) == PARAM
    gpu_ctx.sync()
    assert all((b.download(np.uint8, SIZE) == p).all() for b, p in zip(d, parity))
    # the coder still works
    assert ec.update_device(d, SIZE, 0, d_a, None, [2, 1], 2) == 0
    gpu_ctx.sync()
    change = parity_change(ec_oracle, 5, 3, 0, SIZE, [2, 1], a[:2048])
    assert all((b.download(np.uint8, SIZE) == (p ^ c)).all() for b, p, c in zip(d, parity, change))
    for b in d + [d_a]:
        b.free()
    ec.free()


def test_stream_order(gpu_ctx, ec_oracle):  # noqa: F811
    """On a caller's stream, an update from member 0 and then one from member 3 to the same unit, with no
    synchronisation between them: the parity is jerasure's encode with both changes."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5360)
    u = 14
    new = [a.copy() for a in data]
    new[0][1024 * u:1024 * u + 1024] = synth_bytes(31, 1024)
    new[3][1024 * u:1024 * u + 1024] = synth_bytes(32, 1024)
    want = encode(ec_oracle, 5, 3, new, SIZE)
    ec = ErasureCode(gpu_ctx, 5, 3)
    d = [crc.DeviceBuffer(gpu_ctx, SIZE).upload(p) for p in parity]
    bufs = [crc.DeviceBuffer(gpu_ctx, 1024).upload(x[j][1024 * u:1024 * u + 1024]) for j in (0, 3) for x in (data, new)]
    s = gpu_ctx.stream_create()
    try:
        assert ec.update_device(d, SIZE, 0, bufs[0], bufs[1], [u], 1, stream=s) == 0
        assert ec.update_device(d, SIZE, 3, bufs[2], bufs[3], [u], 1, stream=s) == 0
        gpu_ctx.stream_sync(s)
        assert same([b.download(np.uint8, SIZE) for b in d], want)
    finally:
        gpu_ctx.stream_destroy(s)
        for b in d + bufs:
            b.free()
        ec.free()


def test_host_form(gpu_ctx, ec_oracle):  # noqa: F811
    """The host form gives the device form's bytes for pageable and page-locked parity, by list, dense, and with one
    member bound; with pieces of three units a 10-unit list takes four pieces with the same result; host parity bytes
    outside the listed units are untouched."""
    import tfs_amd.crc as crc
    from tfs_amd.ec import ErasureCode
    data, parity = clean_family(ec_oracle, 5, 3, 5370)
    units, j = ORDER[:10], 2
    new = [a.copy() for a in data]
    for i, u in enumerate(units):
        new[j][1024 * u:1024 * u + 1024] = synth_bytes(600 + i, 1024)
    old_u, new_u = units_of(data[j], units), units_of(new[j], units)
    want = encode(ec_oracle, 5, 3, new, SIZE)
    ec = ErasureCode(gpu_ctx, 5, 3)
    dev = run_device(gpu_ctx, ec, parity, SIZE, j, old_u, new_u, units, 10)
    assert same(dev, want)
    pageable = [p.copy() for p in parity]
    assert ec.update(pageable, SIZE, j, old_u, new_u, units=units) == 0
    assert same(pageable, dev) and unlisted_as_before(pageable, parity, units)
    pins = [crc.PinnedBuffer(gpu_ctx, SIZE) for _ in range(3)]
    for b, p in zip(pins, parity):
        b.array[:] = p
    assert ec.update([b.array for b in pins], SIZE, j, old_u ^ new_u, units=units) == 0      # the delta-only form
    assert same([b.array for b in pins], dev)
    for b in pins:
        b.free()
    assert ec.L.tfs_ec_update_set_piece(ec.h, 3) == 0
    pieces = [p.copy() for p in parity]
    assert ec.update(pieces, SIZE, j, old_u, new_u, units=units) == 0                         # 3 + 3 + 3 + 1
    dense_p = [p.copy() for p in parity]
    dense_d = synth_bytes(900, 1024 * 7).copy()
    assert ec.update(dense_p, SIZE, 4, dense_d) == 0                                          # dense: units 0 .. 6
    assert ec.L.tfs_ec_update_set_piece(ec.h, 0) == 0
    assert same(pieces, dev)
    change = parity_change(ec_oracle, 5, 3, 4, SIZE, range(7), dense_d)
    assert same([g ^ x for g, x in zip(dense_p, parity)], change)
    # the parity server's call: its one member bound, a larger array around the member to catch a stray write
    wide = np.full(SIZE + 2048, FILL, np.uint8)
    wide[1024:1024 + SIZE] = parity[1]
    assert ec.update([None, wide[1024:1024 + SIZE], None], SIZE, j, old_u, new_u, units=units) == 0
    assert (wide[1024:1024 + SIZE] == dev[1]).all() and (wide[:1024] == FILL).all() and (wide[1024 + SIZE:] == FILL).all()
    ec.free()
