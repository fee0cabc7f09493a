"""Hand-built HSP sets that put the repeat masker's coverage stage (segalign_amd/csrc/coverage.hip: the difference array, its touched
range, the three prefix scans per tile, the run slots; coverage_finish in api_rm.hip) at its block-end, range, depth, M and capacity edges.
Shared by tests/test_coverage_regimes.py (CPU: every input is shown, on tests/coverage_model.py, to be in the regime it names, and the
oracle is held to the model) and tests/test_gpu_coverage_regimes.py (GPU: sa_rm_coverage_intervals against the model).

A Regime is (name, hsps, block_len, the Ms it is run at) and `holds`, a predicate over the regime that reads the model: the claim of its
construction.  Positions are block positions; an HSP (query_start, len) counts query_start .. query_start + len - 1.

The touched range of the device is [lo, hi] = [smallest counted start, largest clipped end]; hi is the position of the last -1 of the
difference array, one behind the last counted position, so a hull of `span` counted positions is scanned as span + 1 words that start at
cov_diff + lo: `lo mod 4` decides between the scan's 16-byte and scalar loads, span + 1 against 2048 and 2048 * 256 its tiles."""
import functools

import numpy as np

import coverage_model as CM

SEG = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])  # engine.SEG_DTYPE, oracle.SEG_DTYPE
SCAN_TILE = 2048


def recs(pairs):
    """[(query_start, len)] -> records (ref_start and score play no part in the stage)"""
    h = np.zeros(len(pairs), dtype=SEG)
    if len(pairs):
        a = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
        h["query_start"], h["len"] = a[:, 0], a[:, 1]
    h["ref_start"] = 7
    h["score"] = 3000
    return h


class Regime:
    def __init__(self, name, hsps, block_len, Ms, holds):
        self.name, self.hsps, self.block_len, self.Ms, self.holds = name, np.ascontiguousarray(hsps, dtype=SEG), int(block_len), tuple(Ms), holds
        self._want = {}

    @functools.cached_property
    def depth(self):
        return CM.true_depth(self.hsps, self.block_len)

    def want(self, M):
        if M not in self._want:
            self._want[M] = CM.runs_of(self.depth, M)
        return self._want[M]

    @functools.cached_property
    def ends(self):
        """query_start + len of every HSP that counts something before clipping, exact"""
        h = self.hsps[self.hsps["len"] > 0]
        return h["query_start"].astype(np.int64) + h["len"].astype(np.int64)

    def want_if_dropped(self, M):
        """the answer of a stage that DROPS an HSP which leaves the block instead of clipping it"""
        h = self.hsps
        inside = h["query_start"].astype(np.int64) + h["len"].astype(np.int64) <= self.block_len
        return CM.numpy_model(h[inside], self.block_len, M)

    def __repr__(self):
        return "Regime(%s, n=%d, block_len=%d)" % (self.name, self.hsps.size, self.block_len)


# ---- past the end of the block ----------------------------------------------------------------------------------------------------------
def past_end_merge(L=100):
    """(L-20, 10) and (L-15, 30): clipped, ONE run L-20 .. L-1, open at the block end -> nothing; dropped instead, (L-20, 10) would be left"""
    return Regime("past-end-merge", recs([(L - 20, 10), (L - 15, 30)]), L, (1,),
                  lambda r: r.want(1) == [] and r.want_if_dropped(1) == [(L - 20, 10)] and r.ends.max() > L and r.depth[L - 1] == 1)


def past_end_depth2(L=100):
    """the same pair at M = 2: the two overlap on L-15 .. L-11 -> [(L-15, 5)]; dropped instead, nothing reaches depth 2"""
    return Regime("past-end-depth2", recs([(L - 20, 10), (L - 15, 30)]), L, (2,),
                  lambda r: r.want(2) == [(L - 15, 5)] and r.want_if_dropped(2) == [] and r.depth.max() == 2)


def ends_at_block_len(L=100):
    """an HSP ending exactly at block_len: its run covers the last position and is dropped as open; an earlier run is kept"""
    return Regime("ends-at-block-len", recs([(10, 5), (L - 10, 10)]), L, (1,),
                  lambda r: r.ends.max() == L and r.depth[L - 1] == 1 and r.want(1) == [(10, 5)])


def ends_before_block_len(L=100):
    """an HSP ending at block_len - 1: the last position is uncovered and closes the run"""
    return Regime("ends-at-block-len-1", recs([(L - 10, 9)]), L, (1,),
                  lambda r: r.ends.max() == L - 1 and r.depth[L - 1] == 0 and r.want(1) == [(L - 10, 9)])


def starts_at_last(L=100):
    return Regime("starts-at-last-position", recs([(20, 3), (L - 1, 1)]), L, (1,),
                  lambda r: r.depth[L - 1] == 1 and r.depth[L - 2] == 0 and r.want(1) == [(20, 3)])


def starts_at_block_len(L=100):
    """starts at (and past) block_len: counts nothing, whatever its length"""
    return Regime("starts-at-block-len", recs([(20, 3), (L, 5), (L, 0xFFFFFFFF), (L + 1, 1), (0xFFFFFFFF, 0xFFFFFFFF)]), L, (1, 2),
                  lambda r: r.depth.sum() == 3 and r.want(1) == [(20, 3)] and r.want(2) == [])


def end_past_2_32(L=100):
    """query_start + len does not fit 32 bits: the end is clipped in 64-bit arithmetic, not wrapped to a small position"""
    return Regime("end-past-2^32", recs([(10, 5), (12, 0xFFFFFFFF), (L // 2, 0xFFFFFFFF - 3)]), L, (1, 2),
                  lambda r: r.ends.max() >= 1 << 32 and ((r.ends[1:] & 0xFFFFFFFF) < L).all() and r.want(1) == [] and r.want(2) == [(12, 3)]
                  and r.depth[L - 1] == 2)


PAST_END = (past_end_merge, past_end_depth2, ends_at_block_len, ends_before_block_len, starts_at_last, starts_at_block_len, end_past_2_32)


# ---- the touched range ------------------------------------------------------------------------------------------------------------------
FIRST_MOD4 = (0, 1, 2, 3)
SPANS = (1, 2, 255, 256, 257, 2046, 2047, 2048, 2049, 524287, 524288, 524289)  # counted hull; the scans get span + 1 words


def boundary_positions(first, span):
    """the positions whose scan index (position - first) is a multiple of 2048, inside the span + 1 scanned words"""
    return [first + k * SCAN_TILE for k in range(1, span // SCAN_TILE + 1)]


@functools.lru_cache(maxsize=None)
def touched(first_mod4, span, base=1000, block_len=None):
    """counted hull [first, first + span - 1] with first = base + first_mod4 (base a multiple of 4): a run that begins on the first
    position, a run that ends on the last, and at EVERY 2048 boundary B of the scan inside the hull a run boundary on both sides of it,
    by turns
      kind 0  (B-3, 2) and (B, 2): an END marker on B-1, the last word of a tile, a START marker on B, the first word of the next
      kind 1  (B-1, 1): a START marker on B-1, an END marker on B
    (a boundary on the hull's last position takes kind 0, its start marker being the last position's own HSP; the boundary on the word
    behind the hull, where span is a multiple of 2048, holds the hull's final end marker and nothing else can), and between them pairs
    of overlapping HSPs (depth 2 on two positions) every 611 positions."""
    assert base % 4 == 0
    first = base + first_mod4
    last = first + span - 1
    L = last + 11 if block_len is None else block_len
    pairs = [(first, 1), (last, 1)] if span > 1 else [(first, 1)]
    for k, B in enumerate(boundary_positions(first, span)):
        for p, n in ((B - 3, 2), (B, 2)) if (k % 2 == 0 or B >= last) else ((B - 1, 1),):
            if first <= p and p + n - 1 <= last:
                pairs.append((p, n))
    for p in range(first + 5, last - 8, 611):
        off = (p - first) % SCAN_TILE
        if not ((off <= 8 and p - first >= SCAN_TILE) or off >= SCAN_TILE - 12):  # (clear of the HSPs at the boundaries)
            pairs += [(p, 3), (p + 1, 3)]

    def holds(r):
        covered = np.flatnonzero(r.depth)
        runs = r.want(1)
        starts, ends = {a for a, n in runs}, {a + n for a, n in runs}  # where the device's start and end flags sit
        bounds = boundary_positions(first, span)
        inner = [B for B in bounds if B <= last]
        kinds = [(B - 1 in ends and B in starts, B - 1 in starts and B in ends) for B in inner]
        return (covered[0] == first and covered[-1] == last and first % 4 == first_mod4 and runs[0][0] == first and sum(runs[-1]) == last + 1
                and all(k0 != k1 for k0, k1 in kinds) and (len(inner) < 2 or (any(k0 for k0, _ in kinds) and any(k1 for _, k1 in kinds)))
                and all(B in ends for B in bounds if B > last)
                and len(bounds) == span // SCAN_TILE and (span < 30 or len(r.want(2)) > 0))

    return Regime("touched-%d-%d" % (first_mod4, span), recs(pairs), L, (1, 2), holds)


# ---- depth --------------------------------------------------------------------------------------------------------------------------------
DEPTHS = (255, 256, 257, 511, 512)


@functools.lru_cache(maxsize=None)
def stacked(D, L=5000, at=1000):
    """D copies of (at, 50), a depth-1 HSP (at + 50, 10) directly behind the stack and one (at + 100, 20) apart from it"""
    h = recs([(at, 50)] * D + [(at + 50, 10), (at + 100, 20)])
    h = h[np.random.default_rng(D).permutation(h.size)]
    return Regime("depth-%d" % D, h, L, (1, 2, 255),
                  lambda r: r.depth.max() == D and (r.depth[at:at + 50] == D).all() and r.depth[at + 50] == 1 and r.depth[at + 100] == 1
                  and r.want(255) != r.want(1) and r.want(255) == ([(at, 50)] if D % 256 == 255 else []))


# ---- M ------------------------------------------------------------------------------------------------------------------------------------
def m_gives_nothing(L=3000):
    """M = 0: the whole block is one run that nothing closes; M = 256: no uint8 counter reaches it"""
    rng = np.random.default_rng(11)
    h = recs([(int(a), int(n)) for a, n in zip(rng.integers(0, L - 100, 60), rng.integers(0, 30, 60))])
    h = np.concatenate([h, recs([(500, 60)] * 300)])
    return Regime("M-0-and-256", h, L, (0, 256),
                  lambda r: r.want(0) == [] and r.want(256) == [] and len(r.want(1)) > 10 and r.depth.max() >= 300)


# ---- the cap on run slots -----------------------------------------------------------------------------------------------------------------
def capped(L):
    """1000 HSPs in a block of L <= 10: the device's run slots are min(2 * 1000 + 2, L + 1) = L + 1.  Every other position of the block
    is counted 200 times (L = 1: position 0, 1000 times, which a uint8 counter reads as 232)"""
    per = 1000 // len(range(0, L, 2))
    pairs = [(p, 1) for p in range(0, L, 2) for _ in range(per)]
    Ms = (1, per & 0xFF, (per & 0xFF) + 1)

    def holds(r):
        open_last = (L - 1) % 2 == 0  # the last position is counted: its run stays open
        every_other = [(p, 1) for p in range(0, L, 2)][:-1 if open_last else None]
        return (r.hsps.size == 1000 and min(2 * r.hsps.size + 2, L + 1) == L + 1 and r.depth.max() == per
                and r.want(1) == every_other and r.want(Ms[1]) == every_other and r.want(Ms[2]) == [])

    return Regime("cap-block-%d" % L, recs(pairs), L, Ms, holds)


# ---- degenerate ---------------------------------------------------------------------------------------------------------------------------
def only_len_zero(L=1000):
    return Regime("only-len-0", recs([(5, 0), (700, 0), (L - 1, 0), (L, 0), (L + 5, 0)]), L, (0, 1, 2),
                  lambda r: r.depth.sum() == 0 and all(r.want(M) == [] for M in (0, 1, 2)))


def no_hsps(L=1000):
    return Regime("no-hsps", recs([]), L, (0, 1), lambda r: r.hsps.size == 0 and r.want(0) == [] and r.want(1) == [])


def tiny_blocks():
    return [
        Regime("block-1", recs([(0, 1)]), 1, (1,), lambda r: r.depth.tolist() == [1] and r.want(1) == []),
        Regime("block-1-long", recs([(0, 9)]), 1, (1,), lambda r: r.depth.tolist() == [1] and r.want(1) == []),
        Regime("block-2-first", recs([(0, 1)]), 2, (1,), lambda r: r.depth.tolist() == [1, 0] and r.want(1) == [(0, 1)]),
        Regime("block-2-last", recs([(1, 1)]), 2, (1,), lambda r: r.depth.tolist() == [0, 1] and r.want(1) == []),
        Regime("block-2-both", recs([(0, 2)]), 2, (1,), lambda r: r.depth.tolist() == [1, 1] and r.want(1) == []),
        Regime("block-2-stacked", recs([(0, 1), (0, 2)]), 2, (1, 2), lambda r: r.depth.tolist() == [2, 1] and r.want(1) == [] and r.want(2) == [(0, 1)]),
    ]


def small_regimes():
    """every regime but the touched ranges (those are listed by touched(first_mod4, span))"""
    return ([f() for f in PAST_END] + [stacked(D) for D in DEPTHS] + [m_gives_nothing(), capped(10), capped(1), only_len_zero(), no_hsps()]
            + tiny_blocks())


# ---- the second upload batch ---------------------------------------------------------------------------------------------------------------
BATCH = 1 << 24  # HSPs per upload of sa_rm_coverage_intervals


@functools.lru_cache(maxsize=None)
def second_batch(L=4096):
    """2^24 + 5 HSPs of len <= 3: the first 2^24 (one full upload) are random and end before L - 196, the last five (the second
    upload) lie on positions the first batch leaves untouched and decide the tail of the answer:
      (L-150, 3) twice    a closed run of depth 2
      (L-100, 2)          a closed run of depth 1
      (L-3, 1), (L-2, 3)  the second runs past the end: clipped, it joins the first into a run that stays open -- nothing is returned for
                          either; dropped instead, (L-3, 1) would be returned
    so a second batch that is lost, or read from the front of the list again, gives another answer at M = 1 and at M = 2"""
    rng = np.random.default_rng(24)
    h = np.zeros(BATCH + 5, dtype=SEG)
    h["query_start"][:BATCH] = rng.integers(0, L - 200, BATCH, dtype=np.uint32)
    h["len"][:BATCH] = rng.integers(0, 4, BATCH, dtype=np.uint32)
    h[BATCH:] = recs([(L - 150, 3), (L - 150, 3), (L - 100, 2), (L - 3, 1), (L - 2, 3)])

    def holds(r):
        head = CM.true_depth(r.hsps[:BATCH], L)
        again = head + CM.true_depth(r.hsps[:5], L)         # the second upload read from offset 0
        undropped = CM.true_depth(r.hsps[:-1], L)           # the record that leaves the block dropped whole
        tail1, tail2 = [(L - 150, 3), (L - 100, 2)], [(L - 150, 3)]
        return (r.hsps.size == BATCH + 5 and (head[L - 196:] == 0).all() and head[:L - 200].min() > 512
                and r.want(1)[-2:] == tail1 and r.want(2)[-1:] == tail2 and r.want(1)[:-2] == CM.runs_of(head, 1)
                and all(CM.runs_of(d, M) != r.want(M) for d in (head, again) for M in (1, 2))
                and CM.runs_of(undropped, 1)[-3:] == tail1 + [(L - 3, 1)] and len(r.want(200)) > 100)

    return Regime("second-batch", h, L, (1, 2, 200), holds)


# ---- eight callers at once: each its own block length (1 000 .. 600 000) and its own regime -----------------------------------------------
def thread_regimes():
    return [past_end_merge(1000), past_end_depth2(310007), touched(1, 2049, base=52000, block_len=77777), stacked(256, L=123457, at=99000),
            touched(3, 524289, base=4000, block_len=600000), end_past_2_32(40001), ends_at_block_len(250000), stacked(511, L=1999, at=1800)]
