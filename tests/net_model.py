"""The model of sa_net_chains (include/segalign_amd.h): the sequential rule, stated literally in plain Python, a separately
written recursive rule, and the per-base ownership check that holds at thresholds 1.

Input: chains in CSR form (first[n + 1] into block_start[] / block_end[], half-open blocks on one axis, ascending and disjoint within a
chain), score[n] int64, group[n] uint32 or None.  Output: FILL_DTYPE records ordered by (group, start), parent an index into them."""
import bisect

import numpy as np

FILL_DTYPE = np.dtype([("group", "<u4"), ("chain", "<u4"), ("parent", "<i4"), ("depth", "<u4"), ("start", "<u4"), ("end", "<u4"),
                       ("ali", "<u4"), ("first_block", "<u4"), ("n_blocks", "<u4"), ("pad", "<u4"), ("score", "<i8")])
FIELDS = ["group", "chain", "parent", "depth", "start", "end", "ali", "first_block", "n_blocks", "score"]
TOP = 1 << 31  # the root space is [0, TOP)


def _input(first, block_start, block_end, score, group):
    first = [int(x) for x in first]
    bs, be = [int(x) for x in block_start], [int(x) for x in block_end]
    score = [int(x) for x in score]
    n = len(first) - 1
    group = [0] * n if group is None else [int(x) for x in group]
    assert len(score) == n and len(group) == n and first[0] == 0 and first[-1] == len(bs) == len(be)
    return first, bs, be, score, group, n


def priority_order(score, group):
    """Per group (ascending) the chains in priority order: score descending, then input index."""
    out = {}
    for c in sorted(range(len(score)), key=lambda c: (group[c], -score[c], c)):
        out.setdefault(group[c], []).append(c)
    return out


def clip(first, bs, be, c, a, b):
    """Chain c's blocks clipped to [a, b): -> (index of the first clipped block, their number, the clipped intervals)."""
    got = [(k, max(bs[k], a), min(be[k], b)) for k in range(first[c], first[c + 1]) if be[k] > a and bs[k] < b]
    return (got[0][0] if got else 0), len(got), [(s, e) for _, s, e in got]


def _finish(fills):
    """Temporary fills [group, chain, parent, depth, start, end, ali, first_block, n_blocks, score] into output order."""
    order = sorted(range(len(fills)), key=lambda k: (fills[k][0], fills[k][4]))
    new = {old: k for k, old in enumerate(order)}
    out = np.zeros(len(fills), dtype=FILL_DTYPE)
    for k, old in enumerate(order):
        g, c, parent, depth, start, end, ali, fb, nb, sc = fills[old]
        out[k] = (g, c, -1 if parent < 0 else new[parent], depth, start, end, ali, fb, nb, 0, sc)
    return out


def net(first, block_start, block_end, score, group=None, min_space=1, min_fill=1):
    """The sequential rule.  -> (fills, stats dict with chains, blocks, groups, fills, max_depth, filled).
    Two things keep it usable on a few thousand chains without changing what it states.  A space shorter than min_space is never
    searched, so it is dropped when it would be created.  The open spaces of a group are disjoint and kept in ascending order, and a
    space that does not meet a chain's hull clips to nothing, so the spaces a chain is offered are one run, found by bisection."""
    first, bs, be, score, group, n = _input(first, block_start, block_end, score, group)
    min_space, min_fill = max(1, int(min_space)), max(1, int(min_fill))
    fills = []
    for g, chains in priority_order(score, group).items():
        spaces = [(0, TOP, -1, 0)]  # (a, b, parent, depth), ascending and disjoint
        ends = [TOP]                # their b, for the bisection
        for c in chains:
            if first[c] == first[c + 1]:
                continue
            k = bisect.bisect_right(ends, bs[first[c]])  # the first space with b > the hull's start
            k1 = k
            while k1 < len(spaces) and spaces[k1][0] < be[first[c + 1] - 1]:
                k1 += 1
            nxt = []
            for a, b, parent, depth in spaces[k:k1]:
                fb, nb, cl = clip(first, bs, be, c, a, b)
                ali = sum(e - s for s, e in cl)
                if ali < min_fill:
                    nxt.append((a, b, parent, depth))
                    continue
                me = len(fills)
                start, end = cl[0][0], cl[-1][1]
                fills.append([g, c, parent, depth, start, end, ali, fb, nb, score[c]])
                new = [(a, start, parent, depth)] + [(e0, s1, me, depth + 1) for (_, e0), (s1, _) in zip(cl, cl[1:])] + [(end, b, parent, depth)]
                nxt += [sp for sp in new if sp[1] - sp[0] >= min_space]
            spaces[k:k1] = nxt
            ends[k:k1] = [sp[1] for sp in nxt]
    out = _finish(fills)
    st = dict(chains=n, blocks=len(bs), groups=len(set(group)), fills=int(out.size), max_depth=int(out["depth"].max()) if out.size else 0,
              filled=int(np.unique(out["chain"]).size))
    return out, st


def net_recursive(first, block_start, block_end, score, group=None, min_space=1, min_fill=1):
    """The recursive rule: the chain that fills a space is the best-priority chain that qualifies in it; then the remainders and the gaps.
    Every space scans its whole group from the top: no scan-position shortcut."""
    first, bs, be, score, group, n = _input(first, block_start, block_end, score, group)
    min_space, min_fill = max(1, int(min_space)), max(1, int(min_fill))
    fills = []
    for g, chains in priority_order(score, group).items():
        stack = [(0, TOP, -1, 0)]
        while stack:
            a, b, parent, depth = stack.pop()
            if b - a < min_space:
                continue
            for c in chains:
                lo = [k for k in range(first[c], first[c + 1]) if be[k] > a]
                ks = [k for k in lo if bs[k] < b]
                ali = sum(min(be[k], b) - max(bs[k], a) for k in ks)
                if ks and ali >= min_fill:
                    break
            else:
                continue
            start, end = max(bs[ks[0]], a), min(be[ks[-1]], b)
            me = len(fills)
            fills.append([g, c, parent, depth, start, end, ali, ks[0], len(ks), score[c]])
            stack.append((a, start, parent, depth))
            stack.append((end, b, parent, depth))
            for k in ks[:-1]:
                stack.append((be[k], bs[k + 1], me, depth + 1))
    return _finish(fills)


def clipped_blocks(fill, block_start, block_end):
    """The clipped blocks of one fill: its chain's blocks first_block .. first_block + n_blocks - 1 intersected with [start, end)."""
    k0, k1 = int(fill["first_block"]), int(fill["first_block"]) + int(fill["n_blocks"])
    return [(max(int(block_start[k]), int(fill["start"])), min(int(block_end[k]), int(fill["end"]))) for k in range(k0, k1)]


def owners(first, block_start, block_end, score, group=None):
    """Base by base: {(group, base): the best-priority chain with a block over it}.  For small coordinates only."""
    first, bs, be, score, group, n = _input(first, block_start, block_end, score, group)
    own = {}
    for g, chains in priority_order(score, group).items():
        for c in chains:
            for k in range(first[c], first[c + 1]):
                for x in range(bs[k], be[k]):
                    own.setdefault((g, x), c)
    return own


def same(got, want):
    """Every field of every fill."""
    assert got.size == want.size, (got.size, want.size)
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8])
    assert (got["pad"] == 0).all()


def csr(chains):
    """[[(start, end), ...], ...] -> (first, block_start, block_end)."""
    first = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
    flat = [b for c in chains for b in c]
    return first, np.array([b[0] for b in flat], dtype=np.uint32), np.array([b[1] for b in flat], dtype=np.uint32)


def random_set(rng, n_max=60, blocks=(1, 12), span=400, groups=1, score_hi=6):
    """n <= n_max chains of blocks[0] .. blocks[1] blocks on [0, span + ...), small scores so that ties occur, `groups` sparse group ids."""
    n = int(rng.integers(1, n_max + 1))
    chains = []
    for _ in range(n):
        nb = int(rng.integers(blocks[0], blocks[1] + 1))
        x = int(rng.integers(0, span))
        c = []
        for _ in range(nb):
            ln = int(rng.integers(1, 30))
            c.append((x, x + ln))
            x += ln + int(rng.integers(0, 40))  # 0: abutting blocks
        chains.append(c)
    first, bs, be = csr(chains)
    score = rng.integers(-2, score_hi, n).astype(np.int64)
    ids = np.array([7, 0, 4_000_000_000, 19], dtype=np.uint32)[:groups]
    group = ids[rng.integers(0, groups, n)]
    return first, bs, be, score, group
