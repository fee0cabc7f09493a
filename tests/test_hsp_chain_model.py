"""CPU: the chaining model (tests/hsp_chain_model.py; contract in include/segalign_amd.h) against an exhaustive search
over every valid chain, and one hand case per clause of the contract."""
import itertools

import numpy as np
import pytest

import hsp_chain_model as M


def exhaustive(h, g, dp, ap, mg):
    """best[i] = the largest score of any valid chain that ends at i, and the chains (input-index tuples) that reach it."""
    n = h.size
    best = [None] * n
    argbest = [[] for _ in range(n)]
    order = list(M.rank_order(h, g))
    for k in range(1, n + 1):
        for sub in itertools.combinations(order, k):  # rank order: the only order in which a subset can chain
            if not all(M.precedes(h, g, sub[x], sub[x + 1], mg) for x in range(k - 1)):
                continue
            s = sum(int(h["score"][x]) for x in sub) - sum(M.penalty(h, sub[x], sub[x + 1], dp, ap) for x in range(k - 1))
            e = sub[-1]
            if best[e] is None or s > best[e]:
                best[e], argbest[e] = s, [sub]
            elif s == best[e]:
                argbest[e].append(sub)
    return best, argbest


def random_set(rng, n, groups):
    rows = []
    for _ in range(n):
        r, d = int(rng.integers(0, 120)), int(rng.integers(-12, 13))
        rows.append((r, max(0, r + d), int(rng.integers(1, 25)), int(rng.integers(-30, 200))))
    h = M.make(rows)
    g = rng.integers(0, groups, n).astype(np.uint32) if groups > 1 else None
    return h, g


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("params", [(0, 0, 0), (3, 1, 0), (0, 2, 40), (5, 0, 25)])
def test_model_equals_exhaustive_search(seed, params):
    dp, ap, mg = params
    rng = np.random.default_rng(100 + seed)
    unique_checked = 0
    for groups in (1, 3):
        for n in (1, 4, 7, 9):
            h, g = random_set(rng, n, groups)
            f, pred, members = M.chain(h, g, dp, ap, mg, min_score=-10 ** 9)
            best, arg = exhaustive(h, g, dp, ap, mg)
            # a chain may always restart at a node: the recurrence's max(0, .) is the search's freedom to drop a prefix
            assert [int(x) for x in f] == best, (groups, n)
            gi = np.zeros(n, dtype=np.uint32) if g is None else g
            for grp in np.unique(gi):
                idx = [i for i in range(n) if gi[i] == grp]
                top = max(best[i] for i in idx)
                winners = [c for i in idx if best[i] == top for c in arg[i]]
                if len(winners) == 1:
                    got = tuple(int(x) for x in members["hsp_index"][members["group"] == grp])
                    assert got == winners[0]
                    unique_checked += 1
    assert unique_checked > 0


def nodes(rows, groups=None, **kw):
    h = M.make(rows)
    f, pred, members = M.chain(h, groups, **kw)
    return [int(x) for x in f], [int(x) for x in pred], [int(x) for x in members["hsp_index"]]


def test_abutting_chains_and_one_base_of_overlap_does_not():
    a = (100, 50, 10, 7)  # target 100..109, query 50..59
    assert nodes([a, (110, 60, 5, 3)])[1] == [-1, 0]                       # abuts in both
    assert nodes([a, (109, 60, 5, 3)])[1] == [-1, -1]                      # one target base shared
    assert nodes([a, (110, 59, 5, 3)])[1] == [-1, -1]                      # one query base shared
    assert nodes([a, (110, 70, 5, 3)])[1] == [-1, 0] and nodes([a, (120, 60, 5, 3)])[1] == [-1, 0]


def test_max_gap_at_the_limit_and_one_past_it():
    a = (100, 50, 10, 7)
    assert nodes([a, (115, 65, 5, 3)], max_gap=5)[1] == [-1, 0]            # both gaps exactly 5
    assert nodes([a, (116, 65, 5, 3)], max_gap=5)[1] == [-1, -1]           # target gap 6
    assert nodes([a, (115, 66, 5, 3)], max_gap=5)[1] == [-1, -1]           # query gap 6
    assert nodes([a, (116, 66, 5, 3)], max_gap=0)[1] == [-1, 0]            # 0: unlimited


def test_a_candidate_value_of_exactly_zero_gives_no_predecessor():
    # f(0) = 6; pen = anti_pen * 6 bases of gap = 6: value 0
    f, pred, _ = nodes([(100, 50, 10, 6), (113, 63, 5, 3)], anti_pen=1)
    assert (f, pred) == ([6, 3], [-1, -1])
    f, pred, _ = nodes([(100, 50, 10, 7), (113, 63, 5, 3)], anti_pen=1)
    assert (f, pred) == ([7, 4], [-1, 0])
    f, pred, _ = nodes([(100, 50, 10, 0), (110, 60, 5, 3)])                # f(0) = 0 without any penalty
    assert (f, pred) == ([0, 3], [-1, -1])


def test_a_predecessor_tie_goes_to_the_lower_rank():
    # ranks: input 1 (ref 90) before input 0 (ref 100); both offer 7 to input 2
    f, pred, _ = nodes([(100, 5, 10, 7), (90, 30, 10, 7), (200, 100, 5, 1)])
    assert f[2] == 8 and pred[2] == 1
    # the same with the later one better by one: it wins
    assert nodes([(100, 5, 10, 8), (90, 30, 10, 7), (200, 100, 5, 1)])[1][2] == 0


def test_an_end_tie_goes_to_the_lower_rank():
    _, _, members = nodes([(300, 300, 10, 9), (100, 900, 10, 9)])
    assert members == [1]  # rank order: input 1, input 0; both score 9 and do not chain
    _, _, members = nodes([(300, 300, 10, 9), (100, 900, 10, 8)])
    assert members == [0]


def test_identical_duplicates_never_chain_to_each_other():
    f, pred, members = nodes([(100, 50, 10, 7)] * 3)
    assert f == [7, 7, 7] and pred == [-1, -1, -1] and members == [0]


def test_groups_separate_and_min_score_cuts():
    rows = [(100, 50, 10, 7), (110, 60, 5, 3), (100, 50, 10, 2)]
    g = np.array([5, 5, 2], dtype=np.uint32)
    h = M.make(rows)
    f, pred, members = M.chain(h, g, min_score=3)
    assert [int(x) for x in f] == [7, 10, 2] and [int(x) for x in pred] == [-1, 0, -1]
    assert [(int(m["hsp_index"]), int(m["group"]), int(m["f"])) for m in members] == [(0, 5, 7), (1, 5, 10)]
    _, _, members = M.chain(h, g, min_score=2)
    assert [int(x) for x in members["group"]] == [2, 5, 5]
