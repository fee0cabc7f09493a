"""The rules the call core (segalign_amd/csrc/core.hip saf_core) is held to, in plain Python, and the inputs of
tests/test_gpu_core_paths.py.

Written from the rules, not from the code:
  * the reference iterations ("segments") of a call are those of its chunks in order, each chunk planned by src/seed_filter.cu:718-745
    over the inclusive prefix of hits per seed word (plan_general: tests/probe_model.py's plan without the table-direct limit of eight);
  * consecutive segments form extension batches: at most MAX_SEGS_ABS = 8 on the general path and MAX_SEGS_TD = 512 in a table-direct
    call; on the general path a batch also ends in front of the segment that would take it past hit_batch hits, unless that segment is
    the batch's first; a batch without hits does not run and is not counted;
  * a batch with more candidates than the chain buffers hold runs its chain stages in ceil(n_long / chain_cap) slices;
  * the way the survivors reach the host (route) follows from the kind of call, the number of batches and segments, three options and
    whether the per-segment chain refused a segment;
  * segment g belongs to the chunk whose iterations hold it.
The segment hit ends come from tests/probe_model.py's plans (held to the oracle by tests/test_probe_regimes.py), never from the engine.
tests/test_core_paths_model.py shows on the CPU, with the oracle, that every input is in the regime it names."""
import functools

import numpy as np

import probe_model as PM
import probe_regimes as R
from segalign_amd import synth

SHAPE = "TTT0T00TT00T0T0TTTT"
MAX_SEGS_ABS = 8             # kernels.h: segments of a batch of the general path
MAX_SEGS_TD = 512            # kernels.h MAX_SEGS: segments of a table-direct call (one batch)
HIT_BATCH = 1 << 27          # core.hip: hits of a batch of the general path (option hit_batch = 0)
DEDUP_SEGS = 512             # dedup.hip: segment ids the per-segment LDS chain handles
DEDUP_SEG_MAX = 2048         # ... records of one segment it takes (option dedup_seg_max = 0)
DEDUP_TOTAL = 131072         # ... and survivors of a call
L2_NSUB = 256                # kernels.h: sub-lists of the second-level list

ROUTE_NONE, ROUTE_SPEC_CHAIN, ROUTE_CHAIN_AFTER_SYNC, ROUTE_LIBRARY_SORTS, ROUTE_RAW, ROUTE_RM_SORT, ROUTE_RM_COVERAGE = range(7)
OVER_SURVIVORS, OVER_CANDIDATES, OVER_ENTROPY, OVER_SECOND_LEVEL = 1, 2, 4, 8


# ---- the rules -------------------------------------------------------------------------------------------------------------------------
def plan_general(prefix, max_hits):
    """src/seed_filter.cu:718-745 on the inclusive prefix of hits per seed word, any number of iterations -> the hit offsets at which
    the iterations end ([]: no hits)."""
    num_seeds = int(prefix.size)
    num_hits = int(prefix[-1]) if num_seeds else 0                                      # :716
    if num_hits == 0:
        return []
    maxh = int(max_hits) & 0xFFFFFFFF
    if num_hits < maxh:                                                                 # :721-724
        num_iter, limit = 2, num_hits
    else:                                                                               # :725-728
        num_iter, limit = num_hits // maxh + 2, maxh
    limit_pos = []
    for _ in range(num_iter - 1):                                                       # :732-739
        pos = int(np.searchsorted(prefix, limit, side="left")) - 1
        limit_pos.append(pos)
        limit = min((int(prefix[pos]) if pos >= 0 else 0) + maxh, num_hits)
    limit_pos.append(num_seeds - 1)                                                     # :741
    if limit_pos[-1] == limit_pos[-2]:                                                  # :743
        limit_pos.pop()
    return [int(prefix[p]) if p >= 0 else 0 for p in limit_pos]


def batches(seg_ends, td, hit_batch=0):
    """seg_ends: the hit offset at which every segment of the call ends, in call order -> [(first segment, segments, hits)] of the
    batches that run"""
    cap = MAX_SEGS_TD if td else MAX_SEGS_ABS
    limit = hit_batch or HIT_BATCH
    out, it, lo = [], 0, 0
    while it < len(seg_ends):
        first, n, hi = it, 0, lo
        while it < len(seg_ends) and n < cap:
            if not td and n > 0 and seg_ends[it] - lo > limit:
                break
            hi = seg_ends[it]
            n += 1
            it += 1
        if hi > lo:
            out.append((first, n, hi - lo))
        lo = hi
    return out


def slices(n_long, chain_cap):
    return -(-n_long // chain_cap) if n_long > chain_cap else 0


def route(survivors, td=True, batches=1, segments=2, rm=False, raw=False, coverage=False, spec_dedup=1, no_small_dedup=0, refused=False,
          sliced=False):
    """refused: a segment holds more survivors than the per-segment chain takes (or the call more than DEDUP_TOTAL)"""
    if survivors == 0:
        return ROUTE_NONE
    small = segments <= DEDUP_SEGS and not no_small_dedup
    spec = td and not rm and not raw and batches == 1 and small and bool(spec_dedup)
    if spec and not refused and not sliced and survivors <= DEDUP_TOTAL:
        return ROUTE_SPEC_CHAIN
    if raw:
        return ROUTE_RAW
    if rm:
        return ROUTE_RM_COVERAGE if coverage else ROUTE_RM_SORT
    if small and not spec and not refused and survivors <= DEDUP_TOTAL:       # (a chain that was tried speculatively is not tried again)
        return ROUTE_CHAIN_AFTER_SYNC
    return ROUTE_LIBRARY_SORTS


def spec_tried(td=True, batches=1, segments=2, rm=False, raw=False, spec_dedup=1, no_small_dedup=0):
    return bool(td and not rm and not raw and batches == 1 and segments <= DEDUP_SEGS and not no_small_dedup and spec_dedup)


def owner(g, iters):
    """chunk of segment g of a call whose chunks hold iters[c] segments"""
    first = np.concatenate([[0], np.cumsum(iters)])
    assert 0 <= g < first[-1]
    return int(np.searchsorted(first, g, side="right")) - 1


# ---- an input and what the model says of its calls ---------------------------------------------------------------------------------------
class Input:
    """a target and a query under a chunk size and a threshold; helpers.Case runs it on both sides"""

    def __init__(self, name, target, query, chunk, hspthresh=3000):
        self.name, self.target, self.query, self.chunk, self.hspthresh = name, target, query, int(chunk), int(hspthresh)

    def __repr__(self):
        return "<input %s>" % self.name

    @functools.cached_property
    def world(self):
        return R.World.from_text(self.name, SHAPE, self.target, 1)

    @functools.cached_property
    def text_query(self):
        return R.TextQuery(self.world.S, self.query)

    def chunks(self):
        end = self.query.size - len(SHAPE)
        return [(i, min(i + self.chunk, end)) for i in range(0, end, self.chunk)]

    def call(self, first, last, rev=False):
        """chunks first .. last of a strand as one call -> (start, end)"""
        ch = self.chunks()
        return ch[first][0], ch[last][1]

    @functools.lru_cache(maxsize=None)
    def chunk_prefix(self, c, rev=False):
        """inclusive prefix of hits per seed word of chunk c"""
        s, e = self.chunks()[c]
        k = self.text_query.keys(rev)[s:e]
        return PM.word_prefix(self.world.table, k[k >= 0])

    def plan(self, first, last, rev=False, max_hits=1 << 30):
        """-> (segments of every chunk, hit offsets of the segment ends over the call, hits of every chunk)"""
        iters, ends, hits, base = [], [], [], 0
        for c in range(first, last + 1):
            p = self.chunk_prefix(c, rev)
            e = plan_general(p, max_hits)
            iters.append(len(e))
            ends += [base + x for x in e]
            hits.append(int(p[-1]) if p.size else 0)
            base += hits[-1]
        return iters, ends, hits

    def max_hits_for(self, c, want, rev=False):
        """the largest MAX_HITS under which chunk c is planned in `want` iterations"""
        p = self.chunk_prefix(c, rev)
        h = int(p[-1])
        for mh in range(h // max(want - 2, 1) + 1, 0, -1):
            if len(plan_general(p, mh)) == want:
                return mh
        raise AssertionError("no MAX_HITS plans %d iterations" % want)


def sparse(target, query, chunk, keep, seed, empty=()):
    """the query with everything but the first `keep` bases of every chunk replaced by unrelated sequence; chunks in `empty` keep nothing"""
    q = synth.random_dna(query.size, seed)
    for c, s in enumerate(range(0, query.size, chunk)):
        if c not in empty:
            q[s:s + keep] = query[s:s + keep]
    return q


@functools.lru_cache(maxsize=None)
def single():
    """one 12 kb chunk a call: ~4000 hits, most of them candidates, 70-100 records"""
    t, q = synth.make_pair(60000, 71, 72, sub_rate=0.08, mask_frac=0.1, records=2, indel_every=120)
    return Input("single", t, q, 12000)


@functools.lru_cache(maxsize=None)
def sixteen():
    """sixteen 6 kb chunks whose first 700 bases are related to the target: a few records per chunk"""
    t, q = synth.make_pair(100000, 73, 74, sub_rate=0.08, mask_frac=0.1, records=2, indel_every=120, invert_frac=0)
    return Input("sixteen", t, sparse(t, q[:16 * 6000 + 18], 6000, 700, 75), 6000)


SPLIT_CHUNK = 5000
SPLIT_EMPTY = (0, 1, 6, 7, 14, 15)      # runs of N: first, in the middle, last
SPLIT_BARREN = (3, 4, 8, 10, 11, 12)    # unrelated sequence: seeds and hits, no record
SPLIT_LAST = 13                         # the last seeded chunk holds every record


@functools.lru_cache(maxsize=None)
def split():
    """sixteen 5 kb chunks: chunks without seeds first, in the middle and last; chunks with hits and no record between chunks with
    records"""
    t, q = synth.make_pair(100000, 76, 77, sub_rate=0.08, mask_frac=0.1, records=2, indel_every=120, invert_frac=0)
    q = q[:16 * SPLIT_CHUNK + 18].copy()
    noise = synth.random_dna(q.size, 78)
    for c in SPLIT_BARREN:                  # (and the first bases behind it: no record of the next chunk begins at the chunk's last seeds)
        q[c * SPLIT_CHUNK:(c + 1) * SPLIT_CHUNK + 60] = noise[c * SPLIT_CHUNK:(c + 1) * SPLIT_CHUNK + 60]
    for c in SPLIT_EMPTY:
        q[c * SPLIT_CHUNK:(c + 1) * SPLIT_CHUNK] = ord("N")
    q[16 * SPLIT_CHUNK:] = ord("N")
    return Input("split", t, q, SPLIT_CHUNK)


@functools.lru_cache(maxsize=None)
def split_last():
    """the same grid with every record in the last seeded chunk: all other seeded chunks are unrelated sequence"""
    a = split()
    q = a.query.copy()
    noise = synth.random_dna(q.size, 79)
    for c in range(16):
        if c not in SPLIT_EMPTY and c != SPLIT_LAST:
            q[c * SPLIT_CHUNK:(c + 1) * SPLIT_CHUNK] = noise[c * SPLIT_CHUNK:(c + 1) * SPLIT_CHUNK]
    return Input("split_last", a.target, q, SPLIT_CHUNK)


def uneven_max_hits(inp, first, last, rev=False):
    """a MAX_HITS just above half the hits of the call's largest chunk: three iterations for the chunks at or above it, two below"""
    return max(inp.plan(first, last, rev)[2]) // 2 + 1


def four_chunk_max_hits(inp):
    """a MAX_HITS under which each of the first four chunks is planned in three iterations"""
    hits = inp.plan(0, 3)[2]
    for mh in range(min(hits), max(hits) // 2, -1):
        if inp.plan(0, 3, max_hits=mh)[0] == [3, 3, 3, 3]:
            return mh
    raise AssertionError("no MAX_HITS gives the four chunks three iterations each")


LATE_NOISE = 14000


@functools.lru_cache(maxsize=None)
def late():
    """one 25 kb chunk whose first 14 kb are unrelated sequence: under a MAX_HITS that gives it 17 iterations, the first batch holds the
    unrelated part's hits and few candidates, the later ones the related part's"""
    t, q = synth.make_pair(60000, 81, 82, sub_rate=0.08, mask_frac=0.1, records=2, indel_every=120, invert_frac=0)
    q = q.copy()
    q[:LATE_NOISE] = synth.random_dna(LATE_NOISE, 83)
    return Input("late", t, q, 25000)
