"""Inputs for the tests of sa_lift_intervals (tests/test_lift_model.py on the CPU, tests/test_gpu_lift.py on the device): hand-built chains
stated directly as (start, other start, bases) blocks, and random nets built the way tests/net_class_cases.py builds them, with random
intervals over them."""
import numpy as np

import lift_model as L
import net_class_cases as K
import net_model as N

FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (multiple, blocks)


class Chains:
    """Chains of (start, other start, bases) blocks; the other starts of a strand-1 chain descend."""

    def __init__(self, chains, group=None, ogroup=None, ostrand=None):
        self.first, self.bs, self.be = N.csr([[(s, s + n) for s, _, n in c] for c in chains])
        self.obs = np.array([o for c in chains for _, o, _ in c], dtype=np.uint32)
        self.obe = np.array([o + n for c in chains for _, o, n in c], dtype=np.uint32)
        self.group = None if group is None else np.asarray(group, dtype=np.uint32)
        self.ogroup = None if ogroup is None else np.asarray(ogroup, dtype=np.uint32)
        self.ostrand = None if ostrand is None else np.asarray(ostrand, dtype=np.uint8)

    def args(self):
        return self.first, self.bs, self.be, self.obs, self.obe

    def kw(self):
        return dict(group=self.group, ogroup=self.ogroup, ostrand=self.ostrand)

    def lift(self, intervals, fn=L.lift, iv_group=None, **kw):
        """intervals: [(start, end)]."""
        s = np.array([a for a, _ in intervals], dtype=np.uint32)
        e = np.array([b for _, b in intervals], dtype=np.uint32)
        return fn(*self.args(), s, e, iv_group=None if iv_group is None else np.asarray(iv_group, dtype=np.uint32), **self.kw(), **kw)


def intervals_over(rng, first, bs, be, group, n, none_group=7):
    """n intervals over chains: points, pieces of one block, spans over several blocks of one chain with ragged ends, long random ones,
    and some in a group that has no chain.  -> (iv_start, iv_end, iv_group)."""
    nb = int(first[-1])
    chain_of = np.repeat(np.arange(first.size - 1), np.diff(first.astype(np.int64)))
    lo, hi = max(0, int(bs.min()) - 30), int(be.max()) + 30
    groups = np.unique(group)
    ivs, ive, ivg = [], [], []
    for _ in range(n):
        kind = int(rng.integers(0, 5))
        k = int(rng.integers(0, nb))
        c = int(chain_of[k])
        g = int(group[c])
        if kind == 0:  # a point
            s = int(rng.integers(lo, hi))
            e, g = s + 1, int(rng.choice(groups))
        elif kind == 1:  # inside one block
            s = int(rng.integers(int(bs[k]), int(be[k])))
            e = int(rng.integers(s + 1, int(be[k]) + 1))
        elif kind == 2:  # over several blocks of one chain, the ends ragged by a few bases
            j = int(rng.integers(k, min(int(first[c + 1]), k + 4)))
            s = max(0, int(bs[k]) + int(rng.integers(-2, 3)))
            e = max(s + 1, int(be[j]) + int(rng.integers(-2, 3)))
        elif kind == 3:  # long
            s = int(rng.integers(lo, hi))
            e, g = s + int(rng.integers(20, 400)), int(rng.choice(groups))
        else:  # a group without a chain
            s = int(rng.integers(lo, hi))
            e, g = s + int(rng.integers(1, 50)), none_group
        ivs.append(s)
        ive.append(e)
        ivg.append(g)
    return np.array(ivs, dtype=np.uint32), np.array(ive, dtype=np.uint32), np.array(ivg, dtype=np.uint32)


def random_case(seed, n_intervals=300):
    """A random net of net_class_cases (both strands with the minus chains flipped, two groups, sparse ogroups) and intervals over it.
    -> dict with args, kw, iv_start, iv_end, iv_group."""
    inp = K.random_input(seed)
    bs, be, obs, obe = K.blocks_of(inp)
    s, e, g = intervals_over(np.random.default_rng(2300 + seed), inp["first"], bs, be, inp["group"], n_intervals)
    return dict(args=(inp["first"], bs, be, obs, obe), kw=dict(group=inp["group"], ogroup=inp["ogroup"], ostrand=inp["ostrand"]),
                iv_start=s, iv_end=e, iv_group=g)


def run(case, fn=L.lift, ratio=(95, 100), multiple=False, blocks=False):
    a = case["args"]
    return fn(a[0], a[1], a[2], a[3], a[4], case["iv_start"], case["iv_end"], iv_group=case["iv_group"], min_match=ratio, multiple=multiple,
              blocks=blocks, **case["kw"])
