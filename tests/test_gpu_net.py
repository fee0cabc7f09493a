"""GPU: sa_net_chains (include/segalign_amd.h) against the model of tests/net_model.py.  Every test first asserts with the
model that its input is in the regime it names, then compares every field of every fill, and the counts fills, filled and max_depth.
rounds, spaces and the times are not compared.  The entry needs no sequence: the tests build chains directly, on an interface without
a processor."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_model as M
import net_model as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 1 << 31


@pytest.fixture(scope="module")
def E(engine):
    engine.InitializeInterface(1)
    return engine


class Case:
    """An input and the model's answer to it."""

    def __init__(self, chains, score, group=None, csr=None, **kw):
        self.first, self.bs, self.be = csr if csr is not None else N.csr(chains)
        self.score = np.asarray(score, dtype=np.int64)
        self.group = None if group is None else np.asarray(group, dtype=np.uint32)
        self.kw = kw
        self.fills, self.st = N.net(self.first, self.bs, self.be, self.score, self.group, **kw)

    def of(self, chain):
        return self.fills[self.fills["chain"] == chain]


def held(E, case):
    """One engine call held against the model.  -> the engine's stats."""
    got, st = E.NetChains(case.first, case.bs, case.be, case.score, case.group, **case.kw)
    N.same(got, case.fills)
    for k in ("chains", "blocks", "groups", "fills", "max_depth", "filled"):
        assert st[k] == case.st[k], (k, st[k], case.st[k])
    assert st["rounds"] >= 1 and st["spaces"] >= st["groups"]
    return st


# ---- sizes and nesting ----
def test_no_chain(E):
    got, st = E.NetChains([0], [], [], [])
    assert got.size == 0 and got.dtype == E.NET_FILL_DTYPE and (st["chains"], st["fills"], st["rounds"]) == (0, 0, 0)


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_chains(E, n):
    case = Case([[(100, 200), (300, 400)], [(150, 350)]][:n], [5, 4][:n])
    assert case.fills.size == (1, 2)[n - 1]
    held(E, case)


@pytest.mark.parametrize("blocks", [1, 2, 1025])
def test_one_chain_of_so_many_blocks(E, blocks):
    case = Case([[(7 + 30 * k, 20 + 30 * k) for k in range(blocks)]], [3])
    assert case.fills.size == 1 and case.fills["n_blocks"][0] == blocks and case.fills["ali"][0] == 13 * blocks
    held(E, case)


def test_only_empty_chains(E):
    case = Case([[], [], []], [3, 1, 2], group=[5, 5, 9])
    assert case.fills.size == 0 and case.st["groups"] == 2
    held(E, case)


def test_two_nested_chains(E):
    case = Case([[(300, 350)], [(100, 200), (400, 500)]], [1, 2])
    assert case.fills[["chain", "parent", "depth"]].tolist() == [(1, -1, 0), (0, 0, 1)]
    held(E, case)


def test_nesting_40_deep(E):
    chains = [[(10 * k, 10 * k + 5), (1000 - 10 * k - 5, 1000 - 10 * k)] for k in range(40)]
    perm = np.random.default_rng(40).permutation(40)
    case = Case([chains[k] for k in perm], [100 - int(k) for k in perm])
    assert case.st["max_depth"] == 39 and case.fills.size == 40 and case.fills["depth"].tolist() == list(range(40))
    st = held(E, case)
    assert st["rounds"] >= 40


# ---- scan tiles ----
def covered_then_winner(ahead):
    """Chain 0 fills the root and opens the gap [1000, 2000); `ahead` - 1 chains that lie under its first block follow in priority; the
    winner, at position `ahead` of the group, is the first that meets the gap."""
    chains = [[(0, 1000), (2000, 3000)]] + [[(3 * k + 1, 3 * k + 3)] for k in range(ahead - 1)] + [[(1200, 1500)], [(1100, 1900)]]
    return chains, [10 ** 6 - k for k in range(len(chains))]


@pytest.mark.parametrize("position", [63, 64, 65, 129])
def test_a_winner_at_this_position_of_its_group(E, position):
    chains, score = covered_then_winner(position)
    case = Case(chains, score)
    order = N.priority_order([int(x) for x in case.score], [0] * len(chains))[0]
    assert order[position] == position and case.of(position)[["depth", "start", "end"]].tolist() == [(1, 1200, 1500)]
    assert case.st["filled"] == 3 and case.of(position + 1)["start"].tolist() == [1100, 1500]  # the last chain takes what is left of the gap
    held(E, case)


def test_200_chains_ahead_of_the_winner_rejected_by_the_hull_and_then_by_min_fill(E):
    chains = [[(0, 1000), (2000, 3000)]] + [[(3 * k + 1, 3 * k + 3)] for k in range(100)]  # under the first block: the hull rejects them
    chains += [[(990 - k, 1002)] for k in range(50)] + [[(1998, 2010 + k)] for k in range(50)]  # two bases in the gap: min_fill rejects them
    chains += [[(1200, 1500)]]
    case = Case(chains, [10 ** 6 - k for k in range(len(chains))], min_fill=3)
    assert case.fills[["chain", "depth", "ali"]].tolist() == [(0, 0, 2000), (201, 1, 300)]
    held(E, case)
    case = Case(chains, [10 ** 6 - k for k in range(len(chains))], min_fill=2)  # one lower and the first of them wins
    assert case.fills["chain"].tolist()[:2] == [0, 101] and case.fills.size > 2
    held(E, case)


# ---- rounds and fan-out ----
def test_a_staircase_of_300_disjoint_chains_with_falling_scores(E):
    case = Case([[(10 * k, 10 * k + 5)] for k in range(300)], [1000 - k for k in range(300)])
    assert case.fills["chain"].tolist() == list(range(300)) and case.st["max_depth"] == 0
    st = held(E, case)
    assert st["rounds"] == 301  # one round per fill along a line, and the one that finds nothing


def comb(teeth=1025):
    return [(20 * k, 20 * k + 10) for k in range(teeth)]


def test_a_comb_whose_1024_gaps_are_each_filled_by_another_chain(E):
    rng = np.random.default_rng(7)
    chains = [comb()] + [[(20 * k + 12, 20 * k + 18)] for k in range(1024)]
    case = Case(chains, [10 ** 6] + rng.integers(0, 50, 1024).tolist())
    assert case.fills.size == 1025 and (case.fills["depth"] == 1).sum() == 1024 and (case.fills["parent"][1:] == 0).all()
    st = held(E, case)
    assert st["rounds"] == 3 and st["spaces"] >= 1 + 1025


def test_one_long_chain_under_a_comb_gives_1024_fills_of_one_chain(E):
    case = Case([[(5, 20 * 1024 + 5)], comb()], [1, 2])
    assert case.of(0).size == 1024 and (case.of(0)["first_block"] == 0).all() and (case.of(0)["ali"] == 10).all()
    assert case.st["filled"] == 2 and case.st["fills"] == 1025
    held(E, case)


# ---- ties, thresholds and extremes ----
def test_equal_scores_are_decided_by_the_input_index(E):
    chains = [[(100 + 30 * k, 200 + 30 * k)] for k in range(70)]
    case = Case(chains, [7] * 70)
    assert case.fills["chain"].tolist() == list(range(70)) and case.fills["ali"].tolist() == [100] + [30] * 69
    held(E, case)
    case = Case(chains[::-1], [7] * 70)
    assert case.fills["chain"].tolist() == list(range(69, -1, -1)) and case.fills["ali"].tolist() == [30] * 69 + [100]
    held(E, case)


@pytest.mark.parametrize("min_fill,fills", [(30, 2), (31, 1)])
def test_min_fill_at_the_clipped_count_and_one_above(E, min_fill, fills):
    case = Case([[(100, 200)], [(180, 230)]], [9, 1], min_fill=min_fill)
    assert case.fills.size == fills
    held(E, case)


@pytest.mark.parametrize("min_space,fills", [(40, 4), (41, 3), (100, 3), (101, 2)])
def test_min_space_at_a_gap_and_a_remainder_and_one_above(E, min_space, fills):
    # chain 0's gap is 40 long and holds chain 1; its left remainder [0, 100) holds chain 2; the right one is long and holds chain 3
    case = Case([[(100, 200), (240, 300)], [(210, 230)], [(10, 20)], [(350, 360)]], [9, 1, 1, 1], min_space=min_space)
    assert case.fills.size == fills
    held(E, case)


def test_abutting_blocks_open_no_gap(E):
    case = Case([[(0, 10), (10, 20), (20, 30), (40, 50)], [(5, 45)], [(9, 11), (19, 21)]], [9, 5, 7])
    assert case.fills[["chain", "depth", "start", "end", "first_block", "n_blocks"]].tolist() == [(0, 0, 0, 50, 0, 4), (1, 1, 30, 40, 4, 1)]
    held(E, case)


def test_coordinates_at_2_to_the_31_minus_1(E):
    case = Case([[(TOP - 11, TOP - 1)], [(0, 1), (TOP - 30, TOP - 5)], [(TOP - 3, TOP - 1)], [(TOP - 40, TOP - 1)]], [5, 4, 9, 1])
    assert case.fills[["chain", "depth", "start", "end", "ali"]].tolist() == [(1, 0, 0, TOP - 11, 20), (3, 1, TOP - 40, TOP - 30, 10),
                                                                             (0, 0, TOP - 11, TOP - 3, 8), (2, 0, TOP - 3, TOP - 1, 2)]
    held(E, case)


def test_scores_at_plus_and_minus_2_to_the_62_and_0(E):
    score = [0, 2 ** 62, -2 ** 62, -1, 1, -2 ** 62, 2 ** 62]
    case = Case([[(100 + 10 * k, 200 + 10 * k)] for k in range(7)], score)
    assert case.fills["chain"].tolist() == [0, 1, 6] and case.fills["score"].tolist() == [0, 2 ** 62, 2 ** 62]
    held(E, case)
    case = Case([[(100 + 200 * k, 200 + 200 * k)] for k in range(7)], score)  # disjoint: the order only decides the rounds
    assert case.fills["score"].tolist() == score
    held(E, case)


# ---- groups ----
def test_unsorted_sparse_group_ids_and_one_chain_groups(E):
    rng = np.random.default_rng(31)
    first, bs, be, score, _ = N.random_set(rng, n_max=200, span=900)
    n = score.size
    group = np.where(np.arange(n) % 3 == 0, (rng.permutation(n) * 7 + 11).astype(np.uint32), np.uint32(4_000_000_000))
    group[n // 2:][np.arange(n - n // 2) % 3 == 1] = 5
    case = Case(None, score, group, csr=(first, bs, be))
    sizes = np.unique(group, return_counts=True)[1]
    assert n > 60 and not np.array_equal(group, np.sort(group)) and (sizes == 1).sum() > 20 and (sizes > 10).sum() == 2 and case.st["max_depth"] >= 1
    held(E, case)


# ---- random sets, threads ----
PARAMS = [dict(min_space=1, min_fill=1), dict(min_space=5, min_fill=12), dict(min_space=25, min_fill=3)]
_sets = {}


def random_case(seed, k):
    if (seed, k) not in _sets:
        rng = np.random.default_rng(3000 + seed)
        n = int(rng.integers(200, 2001))
        chains = []
        for _ in range(n):
            x, c = int(rng.integers(0, 12 * n)), []
            for _ in range(int(rng.integers(1, 13))):
                ln = int(rng.integers(1, 60))
                c.append((x, x + ln))
                x += ln + int(rng.integers(0, 200))
            chains.append(c)
        sizes = rng.integers(1, 40, 4)
        group = rng.choice(np.array([9, 0, 4_000_000_000, 70], dtype=np.uint32), size=n, p=sizes / sizes.sum())
        _sets[(seed, k)] = Case(chains, rng.integers(-5, 40, n), group, **PARAMS[k])
    return _sets[(seed, k)]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(6))
def test_random_sets(E, seed, k):
    case = random_case(seed, k)
    counts = np.unique(case.fills["chain"], return_counts=True)[1]
    assert case.st["max_depth"] >= 2 and case.st["filled"] < case.st["chains"] and counts.max() > 1 and case.st["groups"] == 4
    assert np.unique(case.score).size < case.score.size
    held(E, case)


def test_eight_threads_get_the_serial_results(E):
    cases = [random_case(s, (s + 1) % 3) for s in range(6)] + [random_case(0, 0), random_case(1, 1)]
    out, errors = [None] * 8, []

    def work(i):
        try:
            c = cases[i]
            out[i] = E.NetChains(c.first, c.bs, c.be, c.score, c.group, **c.kw)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(8):
        N.same(out[i][0], cases[i].fills)


# ---- engine-fed input ----
def scatter(rng, n, diagonals=4, step=40, jitter=6):
    """n HSPs along a few diagonals, in shuffled input order (as tests/test_gpu_hsp_chain_all.py builds them)."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * 700 + int(rng.integers(-jitter, jitter + 1))
        q = 1000 + k * step // diagonals + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(5, 50)), int(rng.integers(-40, 300))))
    return M.make(rows)[rng.permutation(n)]


@pytest.mark.parametrize("axis", ["target", "query"])
def test_chains_from_the_chain_all_entry(E, axis):
    rng = np.random.default_rng(77)
    h = scatter(rng, 900)
    g = rng.choice(np.array([3, 1, 900_000], dtype=np.uint32), size=h.size)
    chains, members, chain_of, _ = E.ChainHspsAll(h, g, diag_pen=1, max_gap=400, min_score=0)
    idx, first = E.chain_csr(members)
    bs, be = E.net_blocks(h, idx, first, axis=axis)
    key = "ref_start" if axis == "target" else "query_start"
    assert first.size == chains.size + 1 and np.array_equal(bs, h[key][idx]) and np.array_equal(be - bs, h["len"][idx] + 1)
    case = Case(None, chains["score"], chains["group"], csr=(first, bs, be))
    assert chains.size > 50 and case.st["max_depth"] >= 1 and case.st["filled"] < chains.size and case.st["fills"] > case.st["filled"]
    held(E, case)


# ---- failures ----
CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
E.NetChains(%s)
print("returned")
"""


@pytest.mark.parametrize("args,words", [("[0, 2], [10, 15], [16, 30], [1]", [b"overlap", b"chain 0"]),
                                        ("[0, 1], [10], [20], [1], min_space=(1 << 31) + 1", [b"min_space", b"out of range"])])
def test_bad_input_fails_with_a_message(args, words):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"NetChains" in r.stderr and all(w in r.stderr for w in words)
