"""Model of the address-ordered split plan and the inputs that
steer it, for tests/test_split_plan.py.  No GPU, no product code.

A throughput launch of n files gives the plan room for cap_for(n) segments.
File i has K[i] = (len - 1) // 128 KiB whole segments when len > 128 KiB, else
0.  The files before `cut` are split, where cut is the first file whose segments
no longer fit, cum[cut] > room; `ext` = cum[cut - 1] segments are made, and the
files from the cut on stay whole (split_ao_count / _scan / _write in
tfs_crc_kernels.hip).  where() names the place the cut takes in the scan: its
block of 256 files, its thread, wave and lane there, and which of the `per`
blocks of one scan thread the block is.

build_files() turns a K vector into descriptors over one small region, every
descriptor one of a pool of a few hundred (offset, len, seed) triples, so an
oracle computes each triple once and every file of a launch of millions is
compared by lookup.
"""
import numpy as np

KSEG = 128 * 1024
AO_BLOCK = 256       # files per block of the count / write kernels
WAVE = 64
SCAN_THREADS = 1024  # the scan kernel is one workgroup of this many threads
MAX_SEGMENTS = 4 << 20
MAX_TRIPLES = 700

SMALL_K = (0, 1, 2, 3, 5, 7, 40, 72)
LARGE_K = (0, 1, 2, 3, 5, 7)
HUGE_K = (100, 255, 511)  # files of up to 64 MiB (and 0: the whole file the cut wave needs)

HEADS = (1, 17, 4097, KSEG - 1, KSEG)                # len = K * 128 KiB + head
WHOLE_LENS = (0, 100, 65536, KSEG) + HEADS[:-1]      # K == 0
OFFSETS = tuple(j + 16 * 797 * j for j in range(16))  # every residue mod 16, up to ~187 KiB
PAD = 4096


def cap_for(n):
    """split_prepare (tfs_crc_abi.cpp): room for max(2n, 65,536) segments, 4 Mi at most."""
    return min(max(2 * n, 65536), MAX_SEGMENTS)


def segments(lens):
    lens = np.asarray(lens, np.int64)
    return np.where(lens > KSEG, (lens - 1) // KSEG, 0)


def model(K, room):
    """(ext, cut) as the kernels define them."""
    K = np.asarray(K, np.int64)
    cum = np.cumsum(K)
    over = np.nonzero(cum > room)[0]
    cut = int(over[0]) if over.size else len(K)
    return (int(cum[cut - 1]) if cut else 0), cut


def where(n, cut):
    """The place of file `cut` in the scan of a launch of n files."""
    nb = (n + AO_BLOCK - 1) // AO_BLOCK
    per = (nb + SCAN_THREADS - 1) // SCAN_THREADS
    block, thread = divmod(cut, AO_BLOCK)
    return {"nb": nb, "per": per, "block": block, "thread": thread, "wave": thread // WAVE, "lane": thread % WAVE,
            "scan_thread": block // per, "slot": block % per, "last_block_files": n - (nb - 1) * AO_BLOCK}


def draw_K(rng, n, values, p=None):
    return rng.choice(np.asarray(values, np.int64), n, p=p)


def place_cut(K, room, t, values=None, rng=None, over=None, kt=None):
    """A copy of K edited so that model(K, room)[1] == t: cum[t - 1] <= room < cum[t].
    values: what K is drawn from (default: the values in K); rng: default seeded by t.

    kt: K[t] (default: K[t] if positive, else the largest value).  over: cum[t] -
    room exactly (1..kt); None leaves it anywhere in that range.  One file with
    K == 0 sits in the cut's wave before t (at t - 2 when t is lane 0 and has no
    such lane), and a file with K > 0 follows t unless t is the last file.  Only as
    many files before t change as it takes to move their sum, each to another value
    of `values`, so K stays mixed on both sides.  Returns (K, z), z the K == 0 file."""
    K = np.array(K, np.int64)
    n = len(K)
    vals = np.unique(K) if values is None else np.array(sorted(values), np.int64)
    rng = np.random.default_rng(t) if rng is None else rng
    assert 0 < t < n
    if kt is None:
        kt = int(K[t]) if K[t] > 0 else int(vals[-1])
    K[t] = kt
    assert kt > 0 and (over is None or 1 <= over <= kt)
    hi = room if over is None else room + over - kt
    lo = room - kt + 1 if over is None else hi
    lane = t % WAVE
    z = t - 1 - int(rng.integers(0, lane)) if lane else (t - 2 if t >= 2 else None)
    free = np.arange(t)
    if z is not None:
        K[z] = 0
        free = free[free != z]
    if t + 1 < n and not (K[t + 1:] > 0).any():
        K[t + 1 + int(rng.integers(0, n - t - 1))] = vals[vals > 0][0]
    assert 0 <= lo and hi <= int(vals[-1]) * free.size, "no K over these values puts the cut at t"
    # coarse: move random files towards `hi` without passing it
    for _ in range(200):
        diff = hi - int(K[:t].sum())
        if diff == 0:
            break
        idx = rng.permutation(free)
        new = rng.choice(vals, idx.size)
        d = new - K[idx]
        ok = d > 0 if diff > 0 else d < 0
        idx, new, d = idx[ok], new[ok], d[ok]
        m = int(np.searchsorted(np.cumsum(np.abs(d)), abs(diff), side="right"))
        if m == 0:
            break
        K[idx[:m]] = new[:m]
    # fine: single moves, each strictly closer to [lo, hi]
    def dist(s):
        return max(lo - s, 0, s - hi)
    s = int(K[:t].sum())
    while dist(s):
        sub = rng.permutation(free)[:4096]
        D = vals[None, :] - K[sub][:, None]
        after = np.maximum(np.maximum(lo - (s + D), (s + D) - hi), 0)
        after[D == 0] = dist(s)
        i, j = np.unravel_index(int(np.argmin(after)), after.shape)
        assert after[i, j] < dist(s), "stuck %d away from the target sum" % dist(s)
        K[sub[i]] = vals[j]
        s = int(K[:t].sum())
    ext, cut = model(K, room)
    assert cut == t and ext == s and lo <= s <= hi
    assert z is None or K[z] == 0
    assert t + 1 == n or (K[t + 1:] > 0).any()
    return K, z


class Pool:
    """per (offset, len, seed) triples for each value of K, over one region."""

    def __init__(self, values, per, rng):
        self.values = tuple(sorted(set(values) | {0}))
        self.per = per
        seeds = [0, 0xFFFFFFFF]
        while len(seeds) < 4:  # two random words with no zero byte
            w = int(rng.integers(0, 2**32))
            if all((w >> s) & 0xFF for s in (0, 8, 16, 24)):
                seeds.append(w)
        self.seeds = tuple(seeds)
        off, ln, seed = [], [], []
        for k in self.values:
            lens = WHOLE_LENS if k == 0 else tuple(k * KSEG + h for h in HEADS)
            shift = int(rng.integers(0, 16))
            for c in range(per):
                ln.append(lens[c % len(lens)])
                off.append(OFFSETS[(c + c // 16 + shift) % 16])
                seed.append(seeds[int(rng.integers(0, 4))])
        self.off = np.array(off, np.uint64)
        self.len = np.array(ln, np.uint32)
        self.seed = np.array(seed, np.uint32)
        self.base = np.full(max(self.values) + 1, -1, np.int64)  # K -> its first triple
        self.base[list(self.values)] = np.arange(len(self.values)) * per
        self.region = (int((self.off + self.len).max()) + PAD + 7) // 8 * 8
        assert len(self.off) <= MAX_TRIPLES
        assert (segments(self.len) == np.repeat(self.values, per)).all()

    def pick(self, K, rng):
        """One triple of the pool for each file: ids with segments(len[ids]) == K."""
        K = np.asarray(K, np.int64)
        b = self.base[K]
        assert (b >= 0).all()
        return b + rng.integers(0, self.per, len(K))


REGIMES = {"large": (LARGE_K, 64, 9101), "small": (SMALL_K, 64, 9102), "huge": (HUGE_K, 20, 9103)}
_pools = {}


def pool_for(regime):
    """The regime's pool: the same triples in every process (the oracle's results are shared)."""
    if regime not in _pools:
        values, per, seed = REGIMES[regime]
        _pools[regime] = Pool(values, per, np.random.default_rng(seed))
    return _pools[regime]


def build_files(K, rng, pool=None):
    """(ids, offset, len, seed): rows for K from the pool (default: the smallest
    regime that holds max(K)); files overlap freely."""
    if pool is None:
        top = int(np.max(K))
        pool = pool_for("large" if top <= max(LARGE_K) else "small" if top <= max(SMALL_K) else "huge")
    ids = pool.pick(K, rng)
    return ids, pool.off[ids], pool.len[ids], pool.seed[ids]
