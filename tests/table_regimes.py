"""Hand-built inputs that put the seed table build (table.hip) and the neighbourhood table (probe.hip) on their edges (DESIGN.md 4.2'').
Shared by tests/test_table_regimes.py (CPU: every input is in the regime it names, the model equals the oracle on it) and
tests/test_gpu_table_regimes.py (GPU: the device tables against tests/table_model.py on those inputs).

NON-OVERLAPPING WINDOWS.  With step = span + 1 the position rule (hazard H6) gives offset = 0 and start_offset = step: the indexed
windows [step i, step i + span), i >= 1, do not overlap and one free base lies between them, so the key of every window is chosen
freely (-1: the window holds an N and is not indexed).  All capacity edges are built this way.  The members of a bucket are dealt
round-robin over the target (member m of every bucket before member m + 1 of any), so that they come from different partition tiles
wherever the table has several: their arrival order is then a race between workgroups, not lane order.

The values below restate constants of table.hip; the `unsorted` count a regime expects ties it to them."""
import functools

import numpy as np

import table_model as M

TB_KEYS_TILE = 65536        # TB_KEYS_THREADS x TB_KEYS_PER: positions per tile of table_keys_kernel
TB_PART_TILE = 8192         # elements per tile of the partition passes
TB_COARSE_BITS = 12         # coarse partitions = top 12 key bits
TB_FINE_BITS = 18           # fine partitions of the three-level build = top 18 key bits
TB_FIN_CAP = 22528          # positions table_finish_kernel holds in LDS for a coarse partition
TB_FIN_CAP_FINE = 8192      # ... for a fine partition
LDS_SORT_MAX = 32           # buckets the finish kernel sorts in LDS; table_sort_buckets_kernel takes those of 33 and more
SORT_MAX = 512              # buckets above it keep their arrival order
SHELL_MIN = 9               # the global sort is a shell sort from 9 entries on, an insertion sort below
REL_GROUPS = 64             # table_partition_rel_kernel gives up on a tile that reaches this many twelve-bit groups past its first

TWO_LEVEL, THREE_LEVEL, ATOMIC, GAVE_UP = 1, 2, 3, 4   # SA_TABLE_BUILD_*

SHAPE_12OF19 = "TTT0T00TT00T0T0TTTT"
SHAPE_W9 = "TT0TT0TT0TT0T"
SHAPE_W11_HOLES = "TTTTT11TTTT"            # a transition mask with holes
SHAPE_W13 = "TTT0T00TT00T0T0TTTTT"         # 26-bit keys: the three-level build at a quarter of 14of22's index
SHAPE_14OF22 = "TTT0T0TT00TT00T0T0TTTT"

EDGE_SIZES = [1, 2, SHELL_MIN - 1, SHELL_MIN, LDS_SORT_MAX - 1, LDS_SORT_MAX, LDS_SORT_MAX + 1, LDS_SORT_MAX + 2, SORT_MAX - 1, SORT_MAX]


class Regime:
    def __init__(self, name, shape, step, target, build, unsorted=0, claims=None):
        self.name, self.shape, self.step = name, M.Shape(shape), int(step)
        self.target = np.ascontiguousarray(target, dtype=np.uint8)
        self.build, self.unsorted = build, unsorted      # what the partition build is expected to report
        self.claims = dict(claims or {})                 # facts of facts() this input was built for

    def __repr__(self):
        return "<regime %s>" % self.name

    @functools.cached_property
    def codes(self):
        return M.encode(self.target)

    @functools.cached_property
    def entries(self):
        """(keys, positions) of the table, ordered by (key, position)"""
        return M.seed_entries(self.codes, self.shape, self.step)

    def facts(self):
        """the histogram facts the regimes are named after, from the model alone"""
        keys, pos = self.entries
        S = self.shape
        bits = 2 * S.weight
        three = bits > 2 * TB_COARSE_BITS
        part = keys >> (bits - (TB_FINE_BITS if three else TB_COARSE_BITS))
        psize = np.unique(part, return_counts=True)[1] if keys.size else np.zeros(0, dtype=np.int64)
        cap = TB_FIN_CAP_FINE if three else TB_FIN_CAP
        bsize = np.unique(keys, return_counts=True)[1] if keys.size else np.zeros(0, dtype=np.int64)
        f = {"num_steps": M.position_rule(self.target.size, S.span, self.step)[1], "num_index": int(keys.size),
             "parts": int(psize.size), "part_max": int(psize.max()) if psize.size else 0, "parts_over": int((psize > cap).sum()),
             "bucket_sizes": set(bsize.tolist())}
        if three and keys.size:
            # the third level sees the pairs grouped by their twelve-bit group; a tile of 8192 of them reaches from the group of its
            # first to the group of its last
            g = keys >> (bits - TB_COARSE_BITS)
            t0 = np.arange(0, keys.size, TB_PART_TILE)
            t1 = np.minimum(t0 + TB_PART_TILE, keys.size) - 1
            f["rel_groups_max"] = int((g[t1] - g[t0]).max())
            f["tiles"] = int(t0.size)
        return f

    def expect(self, atomic):
        """-> (build, unsorted partitions) sa_get_table_build_info reports"""
        return (ATOMIC, 0) if atomic else (self.build, self.unsorted if self.build in (TWO_LEVEL, THREE_LEVEL) else 0)


# ---- builders ----------------------------------------------------------------------------------------------------------------------------
def windows(shape, keys, seed=1):
    """the target of non-overlapping windows with these keys (-1: not indexed); everything but the care positions is random ACGT"""
    S = M.Shape(shape)
    step = S.span + 1
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.size
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=step * n + S.span)].copy()
    base = step * (1 + np.arange(n, dtype=np.int64))
    valid = keys >= 0
    for j in range(S.weight):
        t[base[valid] + S.pos[j]] = np.frombuffer(b"ACGT", dtype=np.uint8)[(keys[valid] >> (2 * (S.weight - 1 - j))) & 3]
    t[base[~valid] + S.pos[0]] = ord("N")
    return t, step


def spread(buckets):
    """(key, size) pairs -> one key per window, the members of every bucket dealt round-robin (larger buckets first in every round)"""
    keys = np.array([k for k, _ in buckets], dtype=np.int64)
    sizes = np.array([s for _, s in buckets], dtype=np.int64)
    assert np.unique(keys).size == keys.size
    o = np.argsort(-sizes, kind="stable")
    keys, sizes = keys[o], sizes[o]
    b = np.repeat(np.arange(keys.size), sizes)
    m = np.arange(b.size) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    return keys[b[np.lexsort((b, m))]]


def sizes_to(total, edges, fill):
    """bucket sizes that sum to `total`: the edge sizes, then fill sizes in turn"""
    sizes = list(edges)
    rem = total - sum(sizes)
    assert rem >= 0
    i = 0
    while rem > 0:
        s = min(fill[i % len(fill)], rem)
        sizes.append(s)
        rem -= s
        i += 1
    return sizes


def partition_buckets(part, low_bits, sizes, seed):
    """buckets of these sizes inside one partition (key >> low_bits == part): distinct low keys, the first and the last among them"""
    rng = np.random.default_rng(seed)
    assert len(sizes) <= (1 << low_bits)
    low = rng.permutation(1 << low_bits)[:len(sizes)]
    if 0 not in low:
        low[0] = 0
    if (1 << low_bits) - 1 not in low:
        low[-1] = (1 << low_bits) - 1
    assert np.unique(low).size == low.size
    return [((part << low_bits) | int(l), int(s)) for l, s in zip(low, sizes)]


# ---- two-level build ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coarse_cap(n, shape=SHAPE_12OF19, fill=(4, 5, 6, 7, 8, 9, 10, 11)):
    """one coarse partition of exactly n positions with every edge bucket size in it, next to a neighbour partition that fits and 9000
    single positions in other partitions (so that the two members of a pair lie a partition tile apart)"""
    S = M.Shape(shape)
    low = 2 * S.weight - TB_COARSE_BITS
    P = 1234
    b = partition_buckets(P, low, sizes_to(n, EDGE_SIZES + [SORT_MAX + 1, 2, LDS_SORT_MAX, LDS_SORT_MAX + 1, SORT_MAX], fill), 11)
    b += partition_buckets(P + 1, low, sizes_to(3000, EDGE_SIZES, fill), 12)
    rng = np.random.default_rng(13)
    others = rng.choice(np.setdiff1d(np.arange(4096), [P, P + 1]), size=9000)
    single = np.unique((others.astype(np.int64) << low) | rng.integers(0, 1 << low, size=9000))
    b += [(int(k), 1) for k in single]
    t, step = windows(shape, spread(b), seed=n)
    return Regime("coarse partition of %d, %s" % (n, shape), shape, step, t, TWO_LEVEL, unsorted=int(n > TB_FIN_CAP),
                  claims={"part_max": n, "parts_over": int(n > TB_FIN_CAP)})


@functools.lru_cache(maxsize=None)
def sizes_fit_w9():
    """every edge bucket size and a bucket of 513 in partitions that fit (weight 9: 64 buckets per coarse partition)"""
    low = 18 - TB_COARSE_BITS
    b = []
    for i, part in enumerate((7, 8, 2000, 4095) + tuple(range(100, 116))):
        b += partition_buckets(part, low, EDGE_SIZES + [SORT_MAX + 1, 3, 5, 17, 100], 20 + i)
    t, step = windows(SHAPE_W9, spread(b), seed=5)
    return Regime("edge bucket sizes in partitions that fit, weight 9", SHAPE_W9, step, t, TWO_LEVEL, claims={"parts_over": 0, "parts": 20})


@functools.lru_cache(maxsize=None)
def steps(n):
    """exactly n indexed windows (num_steps = n), keys from a pool of 3000 so that buckets hold several members from far apart"""
    rng = np.random.default_rng(n)
    pool = rng.choice(1 << 18, size=3000, replace=False)
    t, step = windows(SHAPE_W9, pool[rng.integers(0, pool.size, size=n)], seed=n)
    return Regime("num_steps %d" % n, SHAPE_W9, step, t, TWO_LEVEL, claims={"num_steps": n, "num_index": n})


@functools.lru_cache(maxsize=None)
def valid_among(n_valid, n=20000):
    """n windows of which exactly n_valid are indexed (num_index = n_valid), scattered"""
    rng = np.random.default_rng(100 + n_valid)
    n = max(n, n_valid + 1000)
    keys = np.full(n, -1, dtype=np.int64)
    pool = rng.choice(1 << 24, size=2500, replace=False)
    keys[rng.choice(n, size=n_valid, replace=False)] = pool[rng.integers(0, pool.size, size=n_valid)]
    t, step = windows(SHAPE_12OF19, keys, seed=n_valid)
    return Regime("num_index %d of %d windows" % (n_valid, n), SHAPE_12OF19, step, t, TWO_LEVEL, claims={"num_steps": n, "num_index": n_valid})


@functools.lru_cache(maxsize=None)
def invalid_tiles():
    """whole tiles of windows that are not indexed between valid ones: two partition tiles, then two keys tiles"""
    rng = np.random.default_rng(77)
    pool = rng.choice(1 << 18, size=500, replace=False)
    v = lambda n: pool[rng.integers(0, pool.size, size=n)]
    keys = np.concatenate([v(3000), np.full(2 * TB_PART_TILE, -1), v(3000), np.full(2 * TB_KEYS_TILE, -1), v(3000)])
    t, step = windows(SHAPE_W9, keys, seed=7)
    return Regime("tiles of invalid windows", SHAPE_W9, step, t, TWO_LEVEL, claims={"num_index": 9000, "num_steps": keys.size})


@functools.lru_cache(maxsize=None)
def one_partition(part, n=6000):
    """every valid key in one coarse partition (12of19)"""
    b = partition_buckets(part, 12, sizes_to(n, EDGE_SIZES, (2, 3, 4, 5, 6, 7)), 30 + part)
    t, step = windows(SHAPE_12OF19, spread(b), seed=part)
    return Regime("all keys in coarse partition %d" % part, SHAPE_12OF19, step, t, TWO_LEVEL, claims={"parts": 1, "part_max": n})


@functools.lru_cache(maxsize=None)
def last_bucket(n):
    """every valid key is 4^k - 1 (12of19)"""
    t, step = windows(SHAPE_12OF19, np.full(n, (1 << 24) - 1), seed=n)
    return Regime("all %d keys in the last bucket" % n, SHAPE_12OF19, step, t, TWO_LEVEL, claims={"parts": 1, "bucket_sizes": {n}})


@functools.lru_cache(maxsize=None)
def every_partition():
    """one position in each of the 4096 coarse partitions (12of19)"""
    rng = np.random.default_rng(41)
    keys = (rng.permutation(4096).astype(np.int64) << 12) | rng.integers(0, 4096, size=4096)
    t, step = windows(SHAPE_12OF19, keys, seed=41)
    return Regime("one position per coarse partition", SHAPE_12OF19, step, t, TWO_LEVEL, claims={"parts": 4096, "part_max": 1})


def ordinary_text(n, seed):
    """ordinary sequence with N runs, soft-masked stretches, record separators and IUPAC letters; clean ACGT at both ends (seed starts
    1 .. 60 have their left context run off the block start, the last anchors their right context off its end)"""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    lo, hi = 150, n - 150
    for _ in range(max(n // 400, 3)):
        a = int(rng.integers(lo, hi))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            t[a:a + int(rng.integers(1, 12))] = ord("N")
        elif kind == 1:
            w = int(rng.integers(1, 40))
            t[a:a + w] = np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, size=w)]
        elif kind == 2:
            t[a] = ord("&")
        else:
            t[a] = rng.choice(np.frombuffer(b"RYKMSWn", dtype=np.uint8))
    # low-complexity stretches: buckets and runs of more than a few entries
    a = int(rng.integers(lo, hi - 200))
    t[a:a + 90] = ord("A")
    a = int(rng.integers(lo, hi - 200))
    t[a:a + 120] = np.frombuffer(b"AC" * 60, dtype=np.uint8)
    return t


@functools.lru_cache(maxsize=None)
def ordinary(step, n=60000, shape=SHAPE_12OF19):
    """overlapping windows on ordinary sequence: steps 1, 2 and span + 1"""
    return Regime("ordinary sequence, %s step %d" % (shape, step), shape, step, ordinary_text(n, 900 + step), TWO_LEVEL,
                  claims={"num_steps": M.position_rule(n, len(shape), step)[1]})


# ---- three-level build -------------------------------------------------------------------------------------------------------------------
def group_key(shape, group, rest):
    return (int(group) << (2 * M.Shape(shape).weight - TB_COARSE_BITS)) | int(rest)


@functools.lru_cache(maxsize=None)
def groups_span(n_groups, first=0, lead=0, shape=SHAPE_W13):
    """one position in each of n_groups consecutive twelve-bit groups from `first` on: 64 of them are what a tile of the third level
    still takes, 65 make it give up.  lead: that many positions of group 100 in front, so that the span starts a tile further on"""
    S = M.Shape(shape)
    rest_bits = 2 * S.weight - TB_COARSE_BITS
    rng = np.random.default_rng(1000 + first)   # (the 65-group table is the 64-group table and one position more)
    b = [(group_key(shape, first + g, rng.integers(0, 1 << rest_bits)), 1) for g in range(n_groups)]
    claims = {"rel_groups_max": n_groups - 1, "num_index": n_groups + lead}
    if lead:
        assert lead % TB_PART_TILE == 0 and first > 100 + REL_GROUPS
        pool = rng.choice(1 << rest_bits, size=lead // 8, replace=False)
        b += [(group_key(shape, 100, r), 8) for r in pool]
        claims["tiles"] = lead // TB_PART_TILE + 1
    t, step = windows(shape, spread(b), seed=n_groups)
    return Regime("%d groups from %d on, %d in front, %s" % (n_groups, first, lead, shape), shape, step, t,
                  THREE_LEVEL if n_groups <= REL_GROUPS else GAVE_UP, claims=claims)


@functools.lru_cache(maxsize=None)
def many_tiles(shape=SHAPE_W13, n_groups=40, per_group=2600, first=2000):
    """>= 100 000 positions in >= 3 tiles, every tile inside fewer than 64 groups; ~9 members per bucket"""
    S = M.Shape(shape)
    rest_bits = 2 * S.weight - TB_COARSE_BITS
    rng = np.random.default_rng(61)
    keys = []
    for g in range(n_groups):
        pool = rng.choice(1 << rest_bits, size=300, replace=False)
        keys.append((np.int64(first + g) << rest_bits) | pool[rng.integers(0, 300, size=per_group)])
    keys = rng.permutation(np.concatenate(keys))
    t, step = windows(shape, keys, seed=62)
    return Regime("%d positions in %d groups, %s" % (keys.size, n_groups, shape), shape, step, t, THREE_LEVEL,
                  claims={"num_index": n_groups * per_group, "parts_over": 0})


@functools.lru_cache(maxsize=None)
def fine_cap(n, shape=SHAPE_W13):
    """one fine partition of exactly n positions with buckets of 2, 32, 33 and 512 (and a second one that fits, with 32 | 33), a few
    groups on"""
    S = M.Shape(shape)
    low = 2 * S.weight - TB_FINE_BITS
    nb = 1 << low
    F = (3000 << 6) | 17                      # fine partition 17 of group 3000
    rest = n - (2 + 2 + 32 + 33 + 512 + 511 + 513 + 9 + 8 + 1 + 31 + 34)
    per = rest // (nb - 12)
    sizes = [2, 2, 32, 33, 512, 511, 513, 9, 8, 1, 31, 34] + [per] * (nb - 13) + [rest - per * (nb - 13)]
    assert sum(sizes) == n and len(sizes) == nb and min(sizes) > 0
    b = partition_buckets(F, low, sizes, 71)
    b += partition_buckets(F + 1, low, [32, 33, 2, 1, 31, 34, 9, 8] + [5] * 100, 72)
    b += partition_buckets((3004 << 6) | 63, low, [3, 33, 32, 7] + [4] * 60, 73)     # groups 3001 .. 3003 stay empty
    # 9000 single positions in the groups behind (so that the two members of a pair lie a partition tile apart)
    rng = np.random.default_rng(74)
    rest_bits = 2 * S.weight - TB_COARSE_BITS
    single = np.unique((rng.integers(3005, 3010, size=9000).astype(np.int64) << rest_bits) | rng.integers(0, 1 << rest_bits, size=9000))
    b += [(int(k), 1) for k in single]
    t, step = windows(shape, spread(b), seed=n)
    return Regime("fine partition of %d, %s" % (n, shape), shape, step, t, THREE_LEVEL, unsorted=int(n > TB_FIN_CAP_FINE),
                  claims={"part_max": n, "parts_over": int(n > TB_FIN_CAP_FINE)})


@functools.lru_cache(maxsize=None)
def group_gaps():
    """full twelve-bit groups with empty ones between them, all within one tile's reach"""
    rng = np.random.default_rng(81)
    b = []
    for g in (500, 505, 540, 563):
        pool = rng.choice(1 << 14, size=150, replace=False)
        b += [(group_key(SHAPE_W13, g, r), int(s)) for r, s in zip(pool, rng.integers(1, 20, size=150))]
    t, step = windows(SHAPE_W13, spread(b), seed=81)
    return Regime("empty groups between full ones", SHAPE_W13, step, t, THREE_LEVEL, claims={"rel_groups_max": 63, "tiles": 1})


@functools.lru_cache(maxsize=None)
def last_fine():
    """the last fine partition alone (every key's top 18 bits set)"""
    b = partition_buckets((1 << TB_FINE_BITS) - 1, 8, sizes_to(3000, EDGE_SIZES, (8, 10, 12, 14, 16)), 91)
    t, step = windows(SHAPE_W13, spread(b), seed=91)
    return Regime("the last fine partition alone", SHAPE_W13, step, t, THREE_LEVEL, claims={"parts": 1, "part_max": 3000})


TWO_LEVEL_REGIMES = {
    "cap 22528": lambda: coarse_cap(TB_FIN_CAP),
    "cap 22529": lambda: coarse_cap(TB_FIN_CAP + 1),
    "cap 22529 w11 holes": lambda: coarse_cap(TB_FIN_CAP + 1, SHAPE_W11_HOLES, (14, 16, 18, 20, 22, 24, 26, 28)),
    "sizes fit w9": sizes_fit_w9,
    **{"steps %d" % n: (lambda n=n: steps(n)) for n in (1, TB_PART_TILE - 1, TB_PART_TILE, TB_PART_TILE + 1, TB_KEYS_TILE - 1, TB_KEYS_TILE,
                                                        TB_KEYS_TILE + 1)},
    **{"index %d" % n: (lambda n=n: valid_among(n)) for n in (0, 1, TB_PART_TILE, TB_PART_TILE + 1)},
    "invalid tiles": invalid_tiles,
    "partition 0": lambda: one_partition(0),
    "partition 4095": lambda: one_partition(4095),
    "last bucket 512": lambda: last_bucket(SORT_MAX),
    "last bucket 3000": lambda: last_bucket(3000),
    "every partition": every_partition,
    "ordinary step 1": lambda: ordinary(1),
    "ordinary step 2": lambda: ordinary(2),
    "ordinary step 20": lambda: ordinary(20),
}
THREE_LEVEL_REGIMES = {
    "64 groups": lambda: groups_span(REL_GROUPS),
    "65 groups": lambda: groups_span(REL_GROUPS + 1),
    "64 groups, second tile": lambda: groups_span(REL_GROUPS, first=1000, lead=TB_PART_TILE),
    "65 groups, second tile": lambda: groups_span(REL_GROUPS + 1, first=1000, lead=TB_PART_TILE),
    "many tiles": many_tiles,
    "fine 8192": lambda: fine_cap(TB_FIN_CAP_FINE),
    "fine 8193": lambda: fine_cap(TB_FIN_CAP_FINE + 1),
    "group gaps": group_gaps,
    "last fine": last_fine,
}
# (each of these moves 1 GiB of index: no more than three)
WEIGHT14_REGIMES = {
    "14of22 many tiles": lambda: many_tiles(SHAPE_14OF22),
    "14of22 fine 8193": lambda: fine_cap(TB_FIN_CAP_FINE + 1, SHAPE_14OF22),
    "14of22 65 groups": lambda: groups_span(REL_GROUPS + 1, shape=SHAPE_14OF22),
}


# ---- neighbourhood table -----------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 63, 64, 65, 128, 129, 600)   # (0: every other key)


@functools.lru_cache(maxsize=None)
def nbr_runs(shape=SHAPE_W9, fill_to=0):
    """Runs of chosen lengths and piece patterns.  Base keys have every field in {A, C}: a transition word of one has a field in
    {G, T}, so the runs of different base keys share no bucket and the pieces of each are chosen freely.  fill_to: that many further
    positions whose keys have three fields or more in {G, T} -- they touch none of those runs and make the table dense (one position
    per key or more: the wave-per-key copy)."""
    S = M.Shape(shape)
    masks = S.masks(True)[1:]
    npieces = 1 + len(masks)
    base = iter(int("".join("01"[(i >> b) & 1] for b in range(S.weight)), 4) for i in range(1, 1 << S.weight))
    b, want = [], {}

    def run(pieces):                          # pieces[j]: entries of piece j (0 the key itself)
        k = next(base)
        assert len(pieces) == npieces
        for j, n in enumerate(pieces):
            if n:
                b.append((k ^ ([0] + masks)[j], n))
        want[k] = sum(pieces)
        return k

    z = [0] * npieces
    for L in RUN_LENGTHS:
        run([L] + z[1:])                                                     # the key's own bucket alone
        run([0] + [L // len(masks) + (1 if j < L % len(masks) else 0) for j in range(len(masks))])   # own bucket empty, transitions only
        run([L - L // 2] + z[1:-1] + [L // 2])                               # first and last piece, the middle empty
    run(list(range(1, npieces + 1)))                                         # every piece non-empty
    run([0, 0] + list(range(1, npieces - 1)))                                # empty pieces first
    run(list(range(1, npieces - 1)) + [0, 0])                                # ... last
    run([3, 4] + [0] * (npieces - 4) + [5, 6])                               # ... in the middle
    run([2, 70] + z[2:])                                                     # one piece of more than 64 entries
    run(z[:-1] + [100])
    run([1] * npieces)
    keys = spread(b)
    if fill_to:
        rng = np.random.default_rng(8)
        pool = rng.integers(0, S.nkeys, size=60000)
        high = sum(((pool >> (2 * f)) & 2) >> 1 for f in range(S.weight))
        pool = np.unique(pool[high >= 3])
        keys = rng.permutation(np.concatenate([keys, pool[rng.integers(0, pool.size, size=fill_to)]]))
    t, step = windows(shape, keys, seed=3)
    r = Regime("neighbourhood runs, %s%s" % (shape, ", dense" if fill_to else ""), shape, step, t, TWO_LEVEL)
    r.want_runs = want
    return r


@functools.lru_cache(maxsize=None)
def nbr_density(num_index):
    """weight 9, 262 144 keys: num_index = nkeys - 1 takes the lane-per-key copy, num_index = nkeys the wave-per-key copy"""
    nkeys = 1 << 18
    rng = np.random.default_rng(5)
    pool = rng.choice(nkeys, size=30000, replace=False)
    keys = pool[rng.integers(0, pool.size, size=nkeys)]
    keys[:64] = pool[0]                       # (one bucket and its runs above a wave's 64 lanes)
    if num_index < nkeys:
        keys[rng.choice(nkeys, size=nkeys - num_index, replace=False)] = -1
    t, step = windows(SHAPE_W9, keys, seed=6)
    return Regime("num_index %d of %d keys" % (num_index, nkeys), SHAPE_W9, step, t, TWO_LEVEL, claims={"num_index": num_index})


@functools.lru_cache(maxsize=None)
def nbr_ordinary(shape=SHAPE_12OF19, n=4200):
    """an ordinary step-1 target of ~4 kb: every (anchor mod 384, anchor mod 4) and (lend mod 384, lend mod 4) occurs, seed starts 1 .. 60,
    anchors within 54 bases of the block end, N / masked / '&' / IUPAC inside both contexts"""
    return Regime("ordinary 4 kb, %s step 1" % shape, shape, 1, ordinary_text(n, 17), TWO_LEVEL)


NBR_REGIMES = {
    "runs w9": lambda: nbr_runs(SHAPE_W9),
    "runs w11 holes": lambda: nbr_runs(SHAPE_W11_HOLES),
    "runs w9 dense": lambda: nbr_runs(SHAPE_W9, fill_to=1 << 18),
    "ordinary 12of19": lambda: nbr_ordinary(SHAPE_12OF19),
    "ordinary w11 holes": lambda: nbr_ordinary(SHAPE_W11_HOLES),
}
# fill -> (engine options, transition, lookup mode, left_skip as a multiple of seed_size); the copy kernel of the default fill depends on
# num_index against the number of keys
FILLS = {
    "default": ({}, True, 2, 1),
    "one stage": ({"nbr_one_stage": 1}, True, 2, 1),
    "positions": ({"no_ctx": 1}, True, 1, 0),
    "anchor context": ({"ctx_skip_seed": 0}, True, 2, 0),
    "notransition": ({}, False, 2, 1),
    "notransition positions": ({"no_ctx": 1}, False, 1, 0),
}
