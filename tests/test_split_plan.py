"""The split plan with the cut anywhere in a block and with more
than 262,144 files.

split_ao_count / _scan / _write (tfs_crc_kernels.hip) build the unit list of a
throughput launch and decide where the plan is written; split_ao_fold_kernel
joins the results.  The cases here put the capacity cut at chosen places of the
scan -- inside wave 0 of a block, across the lane-63 hand-off, in waves 1-3
(which add the earlier waves' sums), on a block's first file, in the launch's
last, partial block, with the total at room and room + 1 exactly -- and run
launches whose block counts are scanned 2, 3 and 9 to a thread, up to the
4 Mi-segment clamp.  tests/split_plan_model.py states what the kernels must
return; the CPU test asserts from that model alone that every case reaches the
place it names, and the GPU tests compare every CRC of every launch with the
oracle and the plan's header with the model.

Every descriptor is one of at most 700 (offset, len, seed) triples over one
region (files overlap, as in test_split_files.py), so the oracle computes each
triple once per regime.  Reference: Func::crc src/common/func.cpp:426-435.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import pytest

import split_plan_model as sp

THREADS = 16

Spec = namedtuple("Spec", "regime n at p over kt drop seed_as expect")


def _spec(regime, n, at=None, p=None, over=None, kt=None, drop=False, seed_as=None, **expect):
    return Spec(regime, n, at, p, over, kt, drop, seed_as, expect)


MEAN1 = (0.5, 0.3, 0.1, 0.05, 0.03, 0.02)  # over LARGE_K: mean 0.94

# at = (block, thread) of the cut file; expect = what where() must say of the cut
# (slot: which of the `per` blocks of its scan thread the cut's block is).
SPECS = {
    # small regime: room 65,536, one block count per scan thread
    "wave0_lane1": _spec("small", 3000, (4, 1), wave=0, lane=1, per=1),
    "wave0_lane37": _spec("small", 3000, (4, 37), wave=0, lane=37, per=1),
    "wave0_lane62": _spec("small", 3000, (4, 62), wave=0, lane=62, per=1),
    "handoff_lane63": _spec("small", 3000, (4, 63), wave=0, lane=63, per=1),
    "handoff_lane0_of_wave1": _spec("small", 3000, (4, 64), wave=1, lane=0, per=1),
    "wave1_lane36": _spec("small", 3000, (5, 100), wave=1, lane=36, per=1),
    "wave2_lane63": _spec("small", 3000, (5, 191), wave=2, lane=63, per=1),
    "wave3_lane63": _spec("small", 3000, (5, 255), wave=3, lane=63, per=1),
    "first_file_of_block": _spec("small", 3000, (6, 0), wave=0, lane=0, per=1),
    # the last block partial (2,900 = 11 * 256 + 84)
    "last_file": _spec("small", 2900, (11, 83), wave=1, lane=19, per=1, nb=12, last_block_files=84),
    "total_is_room_plus_1": _spec("small", 2900, (11, 83), over=1, kt=1, seed_as="total_is_room",
                                  wave=1, lane=19, per=1, nb=12, last_block_files=84),
    "total_is_room": _spec("small", 2900, (11, 83), over=1, kt=1, drop=True),
    # the existing capacity test's shape (a few hundred files of up to 64 MiB), off the wave boundary
    "long_files_block0": _spec("huge", 300, (0, 229), wave=3, lane=37, per=1),
    # large regime: more than 1,024 blocks, several block counts per scan thread
    "n263989_no_cut": _spec("large", 263989, p=MEAN1),
    "n263989_first_of_2": _spec("large", 263989, (700, 165), wave=2, lane=37, per=2, slot=0, nb=1032),
    "n263989_second_of_2": _spec("large", 263989, (701, 165), wave=2, lane=37, per=2, slot=1, nb=1032),
    "n600000_third_of_3": _spec("large", 600000, (1562, 165), wave=2, lane=37, per=3, slot=2, nb=2344),
    "n2100000_no_cut": _spec("large", 2100000, p=MEAN1),
    "n2100000_cut": _spec("large", 2100000, (5460, 165), wave=2, lane=37, per=9, slot=6, nb=8204),
}
NAMES = list(SPECS)

Case = namedtuple("Case", "name regime n room K ids off len seed ext cut z")


@functools.lru_cache(maxsize=None)
def case(name):
    s = SPECS[name]
    rng = np.random.default_rng(zlib.crc32((s.seed_as or name).encode()))
    values = sp.REGIMES[s.regime][0]
    room = sp.cap_for(s.n)
    K = sp.draw_K(rng, s.n, values, s.p)
    z = None
    if s.at:
        t = s.at[0] * sp.AO_BLOCK + s.at[1]
        K, z = sp.place_cut(K, room, t, values, rng, over=s.over, kt=s.kt)
        if s.drop:  # one segment less: the cut file now fits
            K[t] -= 1
    ids, off, ln, seed = sp.build_files(K, rng, sp.pool_for(s.regime))
    ext, cut = sp.model(K, room)
    for a in (K, ids, off, ln, seed):
        a.setflags(write=False)
    return Case(name, s.regime, s.n, room, K, ids, off, ln, seed, ext, cut, z)


# ---- CPU: every case reaches the place it names ---------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_place(name):
    s, c = SPECS[name], case(name)
    n, K, room = c.n, c.K, c.room
    cum = np.cumsum(K)
    w = sp.where(n, c.cut)
    assert room == sp.cap_for(n) == min(max(2 * n, 65536), 4 << 20)
    assert w["per"] == -(-w["nb"] // 1024) and w["nb"] == -(-n // 256)
    assert (sp.segments(c.len) == K).all()  # the descriptors say what K says
    assert (c.off.astype(np.int64) + c.len <= sp.pool_for(c.regime).region - sp.PAD).all()
    pool = sp.pool_for(c.regime)  # every descriptor is a triple of the pool: the distinct ones are counted by id
    assert (c.off == pool.off[c.ids]).all() and (c.len == pool.len[c.ids]).all() and (c.seed == pool.seed[c.ids]).all()
    assert len(np.unique(c.ids)) <= len(pool.off) <= sp.MAX_TRIPLES
    if s.at is None or s.drop:  # no cut: every file's segments fit
        assert c.cut == n and c.ext == int(cum[-1]) <= room and c.ext > 0
        assert not s.drop or c.ext == room  # `run + v > room` at equality
    else:
        t = c.cut
        assert (w["block"], w["thread"]) == s.at and t < n
        for k, v in s.expect.items():
            assert w[k] == v, (k, w)
        assert w["scan_thread"] * w["per"] + w["slot"] == w["block"]
        assert (int(cum[t - 1]) if t else 0) == c.ext <= room < int(cum[t])
        assert c.ext > 0 and K[t] > 0
        if s.over is not None:
            assert int(cum[t]) == room + s.over
        # mixed K on both sides, a whole file in the cut's wave before the cut, split-sized files after it
        assert len(np.unique(K[:t])) >= 3
        if w["lane"]:
            assert t - w["lane"] <= c.z < t and K[c.z] == 0
        if t + 1 < n:
            assert (K[t + 1:] > 0).any() and len(np.unique(K[t + 1:])) >= 3
    if name == "first_file_of_block":  # file (5, 255) fits, file (6, 0) does not
        assert K[c.cut - 1] > 0 and c.cut % 256 == 0
    if name == "total_is_room_plus_1":  # reached by the last file alone; the file before it lands on room exactly
        assert c.ext == room and int(cum[-1]) == room + 1 and c.cut == n - 1
        assert (case("total_is_room").K[:-1] == K[:-1]).all() and case("total_is_room").K[-1] == K[-1] - 1
    if name == "n600000_third_of_3":
        assert w["block"] > 1024
    if n == 2100000:
        assert room == 4194304 < 2 * n  # the clamp
    if name.endswith("no_cut"):
        assert 0.8 < K.mean() < 1.1
    if name == "n2100000_cut":
        assert 2.8 < K.mean() < 3.2


def test_model_and_place_cut():
    assert sp.model([3, 0, 2, 5], 5) == (5, 3) and sp.model([3, 0, 2, 5], 4) == (3, 2)
    assert sp.model([6, 1], 5) == (0, 0) and sp.model([1, 2], 3) == (3, 2) and sp.model([1, 2], 2) == (1, 1)
    assert [sp.cap_for(n) for n in (300, 32768, 32769, 2097152, 2097153)] == [65536, 65536, 65538, 4194304, 4194304]
    rng = np.random.default_rng(5)
    for t in (100, 127, 128, 300, 999):
        K, z = sp.place_cut(sp.draw_K(rng, 1000, sp.LARGE_K), 600, t)
        assert sp.model(K, 600)[1] == t


# ---- GPU ------------------------------------------------------------------------
Env = namedtuple("Env", "img host pool crc crc0")


def _oracle_mt(oracle, host, offs, lens, seeds):
    import tfs_amd.crc as crc
    d = np.zeros(len(offs), crc.DESC_DTYPE)
    d["offset"], d["len"], d["aux"] = offs, lens, seeds
    out = np.zeros(len(offs), np.uint32)
    assert oracle.oracle_crc_batch_mt(d.ctypes.data, len(offs), host.ctypes.data, out.ctypes.data, THREADS) == 0
    return out


@pytest.fixture(scope="module")
def envs(gpu_ctx, oracle):
    """regime -> its region on the device (filled there, downloaded for the oracle) and
    the oracle's CRC of every triple of its pool, with the triple's seed and with seed 0."""
    import tfs_amd.crc as crc
    made = {}

    def get(regime):
        if regime not in made:
            pool = sp.pool_for(regime)
            img = crc.DeviceBuffer(gpu_ctx, pool.region)
            gpu_ctx.synth_fill_device(img, pool.region, 0x5917 + len(made), 0)
            gpu_ctx.sync()
            host = img.download(np.uint8, pool.region)
            zero = np.zeros(len(pool.off), np.uint32)  # verify mode checksums from seed 0; no verify case is "huge"
            made[regime] = Env(img, host, pool, _oracle_mt(oracle, host, pool.off, pool.len, pool.seed),
                               _oracle_mt(oracle, host, pool.off, pool.len, zero) if regime != "huge" else None)
        return made[regime]

    yield get
    for e in made.values():
        e.img.free()


def _desc(c, aux):
    import tfs_amd.crc as crc
    d = np.zeros(c.n, crc.DESC_DTYPE)
    d["offset"], d["len"], d["aux"] = c.off, c.len, aux
    return d


def _assert_crcs(c, got, exp, what=""):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (c.name, what, "cut %d" % c.cut, bad.size,
                           [(int(i), int(c.K[i]), int(c.len[i]), int(c.off[i]) % 16) for i in bad[:10]])


def _assert_stats(c, st):
    assert st["files"] == c.n and st["cap"] == sp.cap_for(c.n), (c.name, st)
    assert st["used"] == c.ext and st["units"] == c.n + c.ext, (c.name, st, c.ext, c.cut)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_split_plan_launch(name, gpu_ctx, envs):
    """One device-resident compute launch of the case on the product context: all n
    CRCs the oracle's; the plan's header what the model says."""
    import tfs_amd.crc as crc
    c, env = case(name), envs(SPECS[name].regime)
    dd = crc.DeviceBuffer(gpu_ctx, 16 * c.n).upload(_desc(c, c.seed))
    out = crc.DeviceBuffer(gpu_ctx, 4 * c.n)
    try:
        gpu_ctx.batch_device(dd, c.n, env.img, out)
        gpu_ctx.sync()
        _assert_stats(c, gpu_ctx.split_stats())
        _assert_crcs(c, out.download(np.uint32, c.n), env.crc[c.ids])
    finally:
        dd.free()
        out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wave2_lane63", "n263989_second_of_2"])
def test_split_plan_verify_finds_wrong_expectations(name, gpu_ctx, envs):
    """Verify mode over a cut: one bit flipped in 200 expectations, 100 before the cut
    (60 of them on split files) and 100 after it (30 of them on files longer than
    128 KiB that stayed whole): n_bad == 200, verdict 0 at exactly those files, every
    CRC the oracle's; twice on one stream (the plan is reused)."""
    import tfs_amd.crc as crc
    c, env = case(name), envs(SPECS[name].regime)
    n, K, i = c.n, c.K, np.arange(c.n)
    assert 0 < c.cut < n
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    wrong = np.zeros(0, np.int64)
    for mask, m in ((i < c.cut) & (K > 0), 60), (i < c.cut, 40), ((i >= c.cut) & (K > 0), 30), (i >= c.cut, 70):
        wrong = np.concatenate([wrong, rng.choice(np.setdiff1d(np.nonzero(mask)[0], wrong), m, replace=False)])
    wrong = np.sort(wrong)
    assert wrong.size == len(set(wrong)) == 200 and int((wrong < c.cut).sum()) == 100
    assert int((K[wrong[wrong < c.cut]] > 0).sum()) >= 40 and int((K[wrong[wrong >= c.cut]] > 0).sum()) >= 10
    exp = env.crc0[c.ids]
    aux = exp.copy()
    aux[wrong] ^= (1 << rng.integers(0, 32, 200)).astype(np.uint32)
    dd = crc.DeviceBuffer(gpu_ctx, 16 * n).upload(_desc(c, aux))
    dc, dok, dnb = crc.DeviceBuffer(gpu_ctx, 4 * n), crc.DeviceBuffer(gpu_ctx, n), crc.DeviceBuffer(gpu_ctx, 4)
    try:
        for rep in range(2):
            for b in (dc, dok, dnb):
                b.zero()
            gpu_ctx.verify_device(dd, n, env.img, dc, dok, dnb)
            gpu_ctx.sync()
            _assert_stats(c, gpu_ctx.split_stats())
            assert int(dnb.download(np.uint32)[0]) == 200, rep
            ok = dok.download(np.uint8, n)
            assert np.array_equal(np.nonzero(ok == 0)[0], wrong) and int((ok == 1).sum()) == n - 200, rep
            _assert_crcs(c, dc.download(np.uint32, n), exp, "rep %d" % rep)
    finally:
        for b in (dd, dc, dok, dnb):
            b.free()


@pytest.mark.gpu
def test_split_plan_reused_across_shapes_on_one_stream(envs):
    """One plan, four shapes queued on one stream of a fresh context with no sync
    between them: a cut, nothing split (1,000 files of at most 128 KiB: the header
    says so), mixed K without a cut, and 263,989 files with a cut, for which the
    plan grows.  Every output in full after one sync; split_stats describes the
    last launch."""
    import tfs_amd.crc as crc
    rng = np.random.default_rng(9200)

    def plain(name, regime, K):
        ids, off, ln, seed = sp.build_files(K, rng, sp.pool_for(regime))
        ext, cut = sp.model(K, sp.cap_for(len(K)))
        return Case(name, regime, len(K), sp.cap_for(len(K)), K, ids, off, ln, seed, ext, cut, None)

    launches = [case("wave1_lane36"),
                plain("whole", "small", np.zeros(1000, np.int64)),
                plain("mixed", "small", sp.draw_K(rng, 400, sp.SMALL_K)),
                case("n263989_first_of_2")]
    assert launches[0].cut < launches[0].n and launches[3].cut < launches[3].n
    assert launches[1].ext == 0 and (launches[1].len <= sp.KSEG).all()
    assert launches[2].cut == 400 and 0 < launches[2].ext < 65536
    hosts = {r: envs(r) for r in ("small", "large")}
    ctx = crc.Context(0)
    bufs, st = [], None
    try:
        st = ctx.stream_create()
        imgs = {}
        for r, e in hosts.items():  # the fresh context's own copy of each region
            imgs[r] = crc.DeviceBuffer(ctx, e.pool.region).upload(e.host)
            bufs.append(imgs[r])
        queued = []
        for c in launches:
            dd = crc.DeviceBuffer(ctx, 16 * c.n).upload(_desc(c, c.seed))
            out = crc.DeviceBuffer(ctx, 4 * c.n)
            bufs += [dd, out]
            queued.append((c, dd, out))
        for c, dd, out in queued:
            ctx.batch_device(dd, c.n, imgs[c.regime], out, stream=st)
        ctx.stream_sync(st)
        _assert_stats(launches[3], ctx.split_stats())
        for c, dd, out in queued:
            _assert_crcs(c, out.download(np.uint32, c.n), hosts[c.regime].crc[c.ids])
    finally:
        for b in bufs:
            b.free()
        if st:
            ctx.stream_destroy(st)
        ctx.close()
