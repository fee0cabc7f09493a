"""Inputs for the tests of sa_net_classify (tests/test_net_class_model.py on the CPU, tests/test_gpu_net_class.py on the device): random
sets with both strands in one net, and hand-built nets stated directly as (start, other start, bases) blocks."""
import numpy as np

import hsp_chain_gap_model as GM
import hsp_chain_model as M
import net_class_model as NC
import net_model as N

THRESHOLDS = [(s, f) for s in (1, 5, 25) for f in (1, 3, 12)]
OGROUPS = np.array([11, 0, 4_000_000_000, 3], dtype=np.uint32)  # sparse ids
QLEN = 3000  # the length of every other-axis sequence: what a strand-1 chain is flipped in


def random_input(seed, n_lo=10, n_hi=16):
    """HSPs on both strands, two target groups, 2 - 4 ogroups; chained per strand with hsp_chain_gap_model.chain_all.  -> dict with hsps,
    members, first, score, group (the net's), ogroup, ostrand, size per chain."""
    rng = np.random.default_rng(2200 + seed)
    n_og = 2 + seed % 3
    rows = [[], []]  # per strand: (ref_start, query_start, bases, score), and the chaining group of each
    keys = [[], []]
    for _ in range(int(rng.integers(n_lo, n_hi))):  # runs of HSPs along one diagonal each, close enough to chain
        strand = int(rng.random() < 0.35)
        tg, og = int(rng.integers(0, 2)), int(rng.integers(0, n_og))
        rs = 400 + int(rng.integers(0, 500))
        d = int(rng.integers(0, 4)) * 90 + (1500 if rng.random() < 0.2 else 0)  # some far away on the other axis
        twin = rng.random() < 0.25  # the same bases of the other axis claimed in the other target group too
        for _ in range(int(rng.integers(1, 7))):
            b = int(rng.integers(4, 40))
            row = (rs, rs - 380 + d + int(rng.integers(0, 3)), b, int(rng.integers(20, 200)))
            rows[strand].append(row)
            keys[strand].append(tg * 8 + og)
            if twin:
                rows[strand].append(row)
                keys[strand].append((1 - tg) * 8 + og)
            rs += b + int(rng.integers(3, 50))
    hs, members, first, score, group, ogroup, ostrand = [], [], [0], [], [], [], []
    base = 0
    for strand in (0, 1):
        h = M.make(rows[strand])
        if not h.size:
            continue
        _, _, chains, mem, _ = GM.chain_all(h, np.array(keys[strand], dtype=np.uint32), max_gap=60, min_score=0,
                                            diag_pen=int(rng.integers(0, 3)), anti_pen=int(rng.integers(0, 2)))
        hs.append(h)
        members += [int(i) + base for i in mem["hsp_index"]]
        first += [first[-1] + int(x) for x in np.cumsum(chains["n_members"])]
        score += [int(x) for x in chains["score"]]
        group += [int(g) // 8 for g in chains["group"]]
        ogroup += [int(OGROUPS[int(g) % 8]) for g in chains["group"]]
        ostrand += [strand] * chains.size
        base += h.size
    n = len(score)
    return dict(hsps=np.concatenate(hs), members=np.array(members, dtype=np.uint32), first=np.array(first, dtype=np.uint32),
                score=np.array(score, dtype=np.int64), group=np.array(group, dtype=np.uint32), ogroup=np.array(ogroup, dtype=np.uint32),
                ostrand=np.array(ostrand, dtype=np.uint8), size=np.full(n, QLEN, dtype=np.uint32))


def blocks_of(inp):
    """-> (block_start, block_end, oblock_start, oblock_end) of a random input, the net on the target axis."""
    h = inp["hsps"][inp["members"].astype(np.int64)]
    bs = h["ref_start"].astype(np.uint32)
    be = (bs + h["len"] + 1).astype(np.uint32)
    obs, obe = NC.other_blocks(inp["hsps"], inp["members"], inp["first"], "target", inp["ostrand"], inp["size"])
    return bs, be, obs, obe


def filters_of(fills, rng):
    """A filter whose thresholds lie inside what the fills hold, so that it keeps some and drops some."""
    if not fills.size:
        return dict(min_score=0)
    sc, size, ali = fills["score"], fills["end"].astype(np.int64) - fills["start"], fills["ali"]
    pick = lambda a, q: int(np.quantile(a, q))
    return dict(min_score=pick(sc, 0.15 * rng.random()), min_top_score=pick(sc, 0.5 * rng.random()), min_size=pick(size, 0.3 * rng.random()),
                min_ali=pick(ali, 0.3 * rng.random()), max_far=int(rng.choice([0, 5, 60, 400, 3000])))


class Net:
    """A hand-built input: chains of (start, other start, bases) blocks, netted by the model.  fills may be replaced before classify."""

    def __init__(self, chains, scores, group=None, ogroup=None, ostrand=None, net_kw={}):
        self.first, self.bs, self.be = N.csr([[(s, s + n) for s, _, n in c] for c in chains])
        self.obs = np.array([o for c in chains for _, o, _ in c], dtype=np.uint32)
        self.obe = np.array([o + n for c in chains for _, o, n in c], dtype=np.uint32)
        self.score = np.asarray(scores, dtype=np.int64)
        self.group = None if group is None else np.asarray(group, dtype=np.uint32)
        self.ogroup = None if ogroup is None else np.asarray(ogroup, dtype=np.uint32)
        self.ostrand = None if ostrand is None else np.asarray(ostrand, dtype=np.uint8)
        self.fills, _ = N.net(self.first, self.bs, self.be, self.score, self.group, **net_kw)

    def args(self):
        return self.first, self.bs, self.be, self.obs, self.obe, self.fills

    def classify(self, fn=NC.classify, filter=None):
        return fn(*self.args(), ogroup=self.ogroup, ostrand=self.ostrand, filter=filter)


def comb(n_blocks, start=100, ostart=10_000, bases=10, pitch=40):
    """A chain of n_blocks blocks of `bases` bases every `pitch`, the other axis moving alike: n_blocks - 1 gaps of pitch - bases."""
    return [(start + k * pitch, ostart + k * pitch, bases) for k in range(n_blocks)]


def comb_minus(n_blocks, start=100, oend=90_000, bases=10, pitch=40):
    """The same on strand 1: the other blocks descend from oend."""
    return [(start + k * pitch, oend - k * pitch - bases, bases) for k in range(n_blocks)]


def nested(depth, ostep=0):
    """`depth` chains, chain k lying in the one gap of chain k - 1 (two blocks each, the gap shrinking): a net `depth` deep, one fill per
    level.  Other starts: 50 000 + k * ostep + the axis offset."""
    chains = []
    for k in range(depth):
        a, b = 1000 + 10 * k, 1000 + 10 * (2 * depth - k) + 5
        chains.append([(a, 50_000 + k * ostep + a, 5), (b, 50_000 + k * ostep + b, 5)])
    return chains
