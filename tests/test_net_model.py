"""CPU: the model of sa_net_chains (tests/net_model.py).  On random sets the sequential rule equals a separately written
recursive rule, ownership is decided base by base at thresholds 1, and the output has the shape the contract promises; then one
hand-worked case per clause of the rule."""
import numpy as np
import pytest

import net_model as N

THRESHOLDS = [(s, f) for s in (1, 5, 25) for f in (1, 3, 12)]


def fields(fills, *names):
    return [tuple(int(f[k]) for k in names) for f in fills]


def gaps_of(fill, bs, be):
    cl = N.clipped_blocks(fill, bs, be)
    return [(e0, s1) for (_, e0), (s1, _) in zip(cl, cl[1:])]


@pytest.mark.parametrize("seed", range(72))
def test_random_sets(seed):
    rng = np.random.default_rng(seed)
    first, bs, be, score, group = N.random_set(rng, groups=1 + seed % 4)
    min_space, min_fill = THRESHOLDS[seed % 9]
    fills, st = N.net(first, bs, be, score, group, min_space, min_fill)
    N.same(N.net_recursive(first, bs, be, score, group, min_space, min_fill), fills)
    assert st["fills"] == fills.size and st["groups"] == np.unique(group).size

    # the order, and unique starts per group
    key = (fills["group"].astype(np.uint64) << np.uint64(32)) | fills["start"].astype(np.uint64)
    assert (key[1:] > key[:-1]).all()
    for k, f in enumerate(fills):
        cl = N.clipped_blocks(f, bs, be)
        c = int(f["chain"])
        assert first[c] <= f["first_block"] and f["first_block"] + f["n_blocks"] <= first[c + 1] and f["n_blocks"] >= 1
        assert all(s < e for s, e in cl) and cl[0][0] == f["start"] and cl[-1][1] == f["end"]
        assert f["ali"] == sum(e - s for s, e in cl) >= min_fill
        assert f["score"] == score[c] and f["group"] == group[c]
        if f["parent"] < 0:
            assert f["depth"] == 0
        else:  # a child lies inside a gap of its parent's clipped blocks, one level down, and after it in the order
            p = fills[f["parent"]]
            assert f["parent"] < k and p["group"] == f["group"] and f["depth"] == p["depth"] + 1
            assert any(a <= f["start"] and f["end"] <= b for a, b in gaps_of(p, bs, be))
            assert (score[p["chain"]], -int(p["chain"])) > (score[c], -c)  # the parent has the better priority
    # siblings (the fills of one parent, or the top fills of one group) are disjoint
    for parent, g in set(fields(fills, "parent", "group")):
        sib = sorted(fields(fills[(fills["parent"] == parent) & (fills["group"] == g)], "start", "end"))
        assert all(e0 <= s1 for (_, e0), (s1, _) in zip(sib, sib[1:]))

    # thresholds 1: base by base
    if (min_space, min_fill) == (1, 1):
        own = N.owners(first, bs, be, score, group)
        got = {}
        for f in fills:
            for s, e in N.clipped_blocks(f, bs, be):
                for x in range(s, e):
                    assert (int(f["group"]), x) not in got
                    got[(int(f["group"]), x)] = int(f["chain"])
        assert got == own


def test_the_random_sets_reach_every_regime():
    seen = dict(tie=0, deep=0, multi=0, unfilled=0, groups=0)
    for seed in range(72):
        first, bs, be, score, group = N.random_set(np.random.default_rng(seed), groups=1 + seed % 4)
        fills, st = N.net(first, bs, be, score, group, *THRESHOLDS[seed % 9])
        seen["tie"] += np.unique(score).size < score.size
        seen["deep"] += st["max_depth"] >= 2
        seen["multi"] += np.unique(fills["chain"]).size < fills.size
        seen["unfilled"] += st["filled"] < st["chains"]
        seen["groups"] += st["groups"] > 1
    assert all(v >= 10 for v in seen.values()), seen


def run(chains, score, group=None, **kw):
    first, bs, be = N.csr(chains)
    fills, st = N.net(first, bs, be, score, group, **kw)
    N.same(N.net_recursive(first, bs, be, score, group, **kw), fills)
    return fills, st


ROW = ("chain", "parent", "depth", "start", "end", "ali", "first_block", "n_blocks")


def test_a_chain_clipped_into_a_left_remainder_and_a_gap_at_once():
    # chain 0: [100, 200) [300, 400); chain 1: [50, 120) [180, 320) [390, 450): left of the fill, inside its gap, right of it
    fills, st = run([[(100, 200), (300, 400)], [(50, 120), (180, 320), (390, 450)]], [10, 5])
    assert fields(fills, *ROW) == [(1, -1, 0, 50, 100, 50, 2, 1), (0, -1, 0, 100, 400, 200, 0, 2), (1, 1, 1, 200, 300, 100, 3, 1),
                                   (1, -1, 0, 400, 450, 50, 4, 1)]
    assert (st["fills"], st["filled"], st["max_depth"]) == (4, 2, 1)


def test_a_chain_wholly_covered_does_not_fill():
    fills, st = run([[(100, 300)], [(150, 200), (220, 250)]], [10, 9])
    assert fields(fills, "chain", "start", "end") == [(0, 100, 300)] and st["filled"] == 1


def test_a_block_that_straddles_a_space_edge_is_clipped():
    # chain 1's block [150, 260) straddles the start of chain 0's gap [200, 300) and its second block the gap's end
    fills, _ = run([[(100, 200), (300, 400)], [(150, 260), (280, 330)]], [10, 5])
    assert fields(fills, *ROW) == [(0, -1, 0, 100, 400, 200, 0, 2), (1, 0, 1, 200, 300, 80, 2, 2)]
    first, bs, be = N.csr([[(100, 200), (300, 400)], [(150, 260), (280, 330)]])
    assert N.clipped_blocks(fills[1], bs, be) == [(200, 260), (280, 300)]


def test_equal_scores_are_decided_by_the_input_index():
    fills, _ = run([[(100, 200)], [(150, 250)]], [7, 7])
    assert fields(fills, "chain", "start", "end") == [(0, 100, 200), (1, 200, 250)]
    fills, _ = run([[(100, 200)], [(150, 250)]], [7, 8])
    assert fields(fills, "chain", "start", "end") == [(0, 100, 150), (1, 150, 250)]


def test_min_fill_at_the_clipped_count_and_one_above():
    chains = [[(100, 200)], [(180, 230)]]  # chain 1 keeps 30 bases right of chain 0
    assert fields(run(chains, [9, 1], min_fill=30)[0], "chain", "start", "ali") == [(0, 100, 100), (1, 200, 30)]
    assert fields(run(chains, [9, 1], min_fill=31)[0], "chain", "start", "ali") == [(0, 100, 100)]


def test_min_space_at_a_gaps_size_and_one_above():
    chains = [[(100, 200), (240, 300)], [(210, 230)]]  # chain 0's gap is 40 long
    assert fields(run(chains, [9, 1], min_space=40)[0], "chain", "depth", "start") == [(0, 0, 100), (1, 1, 210)]
    assert fields(run(chains, [9, 1], min_space=41)[0], "chain", "depth", "start") == [(0, 0, 100)]
    # a remainder is held to min_space too: the left remainder [0, 100) is not searched at 101
    chains = [[(100, 200)], [(10, 20)]]
    assert len(run(chains, [9, 1], min_space=100)[0]) == 2 and len(run(chains, [9, 1], min_space=101)[0]) == 1


def test_an_empty_chain_never_fills():
    fills, st = run([[], [(5, 9)], []], [100, 1, 50])
    assert fields(fills, "chain", "first_block", "n_blocks") == [(1, 0, 1)] and (st["chains"], st["filled"]) == (3, 1)
    fills, st = run([[], []], [3, 4])
    assert fills.size == 0 and st["groups"] == 1


def test_groups_never_interact():
    fills, st = run([[(100, 200)], [(100, 200)], [(150, 250)]], [5, 9, 1], group=[7, 3, 7])
    assert fields(fills, "group", "chain", "start", "end") == [(3, 1, 100, 200), (7, 0, 100, 200), (7, 2, 200, 250)] and st["groups"] == 2
