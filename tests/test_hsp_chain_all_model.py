"""CPU: the model of sa_chain_hsps_all (tests/hsp_chain_all_model.py; contract in include/segalign_amd.h) against the
properties the contract states, on random sets and on one hand case per clause."""
import numpy as np
import pytest

import hsp_chain_all_model as A
import hsp_chain_model as M


def random_set(seed):
    """n <= 60 HSPs with small scores (ties in f), in one to four groups, max_gap on every second seed."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 10 if seed % 3 == 0 else 61))
    rows = [(int(rng.integers(0, 40)) * 10, int(rng.integers(0, 40)) * 10, int(rng.integers(1, 12)), int(rng.integers(-2, 4))) for _ in range(n)]
    g = rng.integers(0, int(rng.integers(1, 5)), n).astype(np.uint32) * 7
    kw = dict(diag_pen=int(rng.integers(0, 2)), anti_pen=0, max_gap=120 if seed & 1 else 0, min_score=int(rng.integers(-2, 4)))
    return M.make(rows), g, kw


def ranks(h, g):
    r = np.zeros(h.size, dtype=np.int64)
    r[M.rank_order(h, g)] = np.arange(h.size)
    return r


@pytest.mark.parametrize("seed", range(60))
def test_random_sets_keep_the_contract(seed):
    h, g, kw = random_set(seed)
    n = h.size
    f, pred, chains, members, chain_of = A.chain_all(h, g, **kw)
    f0, pred0, all_chains, all_members, all_of = A.chain_all(h, g, **dict(kw, min_score=-2 ** 62))
    rank = ranks(h, g)
    assert np.array_equal(f, f0) and np.array_equal(pred, pred0)
    assert len(np.unique(f)) < n or n < 4 or seed % 3 == 0, "no tie in f"

    # the chains partition the HSPs, whatever min_score is
    assert sorted(all_members["hsp_index"].tolist()) == list(range(n)) and (all_of != A.NONE).all()
    assert int(all_chains["n_members"].sum()) == n
    kept_in_all = [k for k in range(all_chains.size) if all_chains["score"][k] >= kw["min_score"]]
    assert np.array_equal(chains[["group", "head", "n_members", "score", "joined"]], all_chains[kept_in_all][["group", "head", "n_members", "score", "joined"]])
    assert ((chain_of == A.NONE) == ~np.isin(all_of, kept_in_all)).all()

    # head: the node of highest priority in the subtree, by a sweep in descending rank (a node's children come before it)
    prio = np.zeros(n, dtype=np.int64)
    prio[sorted(range(n), key=lambda u: (-int(f[u]), int(rank[u])))] = np.arange(n)
    best = prio.copy()
    for v in sorted(range(n), key=lambda u: -int(rank[u])):
        if pred[v] >= 0:
            best[pred[v]] = min(best[pred[v]], best[v])
    by_prio = np.argsort(prio)
    for k in range(all_chains.size):
        c = all_chains[k]
        m = all_members[c["first_member"]:c["first_member"] + c["n_members"]]
        idx = m["hsp_index"].astype(np.int64)
        assert (m["chain"] == k).all() and (all_of[idx] == k).all() and np.array_equal(m["f"], f[idx]) and (m["group"] == c["group"]).all()
        assert (by_prio[best[idx]] == c["head"]).all() and idx[-1] == c["head"]
        # a contiguous piece of a pred walk, in rank order
        assert all(pred[idx[i + 1]] == idx[i] for i in range(idx.size - 1)) and (np.diff(rank[idx]) > 0).all()
        assert pred[idx[0]] == c["joined"] and (c["joined"] < 0 or all_of[c["joined"]] != k)
        # the score: the members' scores minus the links' penalties, the cut link's included
        total = int(h["score"][idx].sum()) - sum(M.penalty(h, int(pred[v]), int(v), kw["diag_pen"], kw["anti_pen"]) for v in idx if pred[v] >= 0)
        assert c["score"] == total == int(f[c["head"]]) - (int(f[c["joined"]]) if c["joined"] >= 0 else 0)

    # the output order, and the first chain of a group is sa_chain_hsps's
    keys = [(int(c["group"]), -int(c["score"]), int(rank[c["head"]])) for c in all_chains]
    assert keys == sorted(keys) and np.array_equal(all_chains["first_member"], np.cumsum(all_chains["n_members"]) - all_chains["n_members"])
    _, _, best_members = M.chain(h, g, **dict(kw, min_score=-2 ** 62))
    for grp in np.unique(g):
        k = int(np.flatnonzero(all_chains["group"] == grp)[0])
        c, want = all_chains[k], best_members[best_members["group"] == grp]
        got = all_members[c["first_member"]:c["first_member"] + c["n_members"]]
        assert np.array_equal(got["hsp_index"], want["hsp_index"]) and np.array_equal(got["f"], want["f"])
        assert c["score"] == want["f"][-1] and c["joined"] == -1


# ---- one hand case per clause ----
STEM = [(100, 100, 10, 10), (200, 200, 10, 10)]  # 0 -> 1; the branches below follow 1 and do not chain with each other


def test_the_better_branch_of_a_fork_takes_the_stem():
    h = M.make(STEM + [(400, 300, 10, 50), (300, 400, 10, 30)])
    f, pred, chains, members, chain_of = A.chain_all(h)
    assert f.tolist() == [10, 20, 70, 50] and pred.tolist() == [-1, 0, 1, 1]
    assert chains[["head", "n_members", "score", "joined"]].tolist() == [(2, 3, 70, -1), (3, 1, 30, 1)]
    assert members["hsp_index"].tolist() == [0, 1, 2, 3] and chain_of.tolist() == [0, 0, 0, 1]


def test_of_two_branches_of_equal_f_the_lower_rank_takes_the_stem():
    h = M.make(STEM + [(400, 300, 10, 50), (300, 400, 10, 50)])  # HSP 3 has the lower ref_start: the lower rank
    f, pred, chains, members, chain_of = A.chain_all(h)
    assert f[2] == f[3] == 70 and pred[2] == pred[3] == 1
    assert chains[["head", "n_members", "score", "joined"]].tolist() == [(3, 3, 70, -1), (2, 1, 50, 1)]
    assert chain_of.tolist() == [0, 0, 1, 0]


def test_joined_names_the_stem_node_the_walk_stopped_at():
    h = M.make(STEM + [(300, 300, 10, 10), (150, 5000, 10, 5)])  # HSP 3 follows 0 alone: 1 ends behind its start
    f, pred, chains, _, _ = A.chain_all(h)
    assert pred.tolist() == [-1, 0, 1, 0] and f[3] == 15
    assert chains[["head", "n_members", "score", "joined"]].tolist() == [(2, 3, 30, -1), (3, 1, 5, 0)]


# 0 -> 1 -> 2 is the best chain (700).  3 (score -150) follows 1; 4 and 5 follow 3 alone under max_gap and do not chain with each
# other: 4 takes 3 into a chain cut at 1 that scores 150 - 200 = -50, 5 is cut at 3 and scores 140 - 50 = 90.
NEGATIVE = [(100, 100, 10, 100), (200, 200, 10, 100), (300, 1000, 10, 500), (1000, 300, 10, -150), (2000, 400, 10, 100), (1500, 500, 10, 90)]


def test_a_joined_score_may_be_negative():
    f, pred, chains, members, chain_of = A.chain_all(M.make(NEGATIVE), max_gap=1000, min_score=-100)
    assert f.tolist() == [100, 200, 700, 50, 150, 140] and pred.tolist() == [-1, 0, 1, 1, 3, 3]
    assert chains[["head", "n_members", "score", "joined"]].tolist() == [(2, 3, 700, -1), (5, 1, 90, 3), (4, 2, -50, 1)]
    assert chain_of.tolist() == [0, 0, 0, 2, 2, 1]


def test_a_chain_dropped_by_min_score_still_stops_the_chain_that_joins_it():
    f, pred, chains, members, chain_of = A.chain_all(M.make(NEGATIVE), max_gap=1000, min_score=0)
    assert chains[["head", "n_members", "score", "joined"]].tolist() == [(2, 3, 700, -1), (5, 1, 90, 3)]
    assert chain_of.tolist() == [0, 0, 0, A.NONE, A.NONE, 1] and members["hsp_index"].tolist() == [0, 1, 2, 5]


def test_chains_of_equal_score_come_in_the_rank_order_of_their_heads():
    h = M.make([(500, 100, 10, 40), (100, 500, 10, 40), (900, 50, 10, 41)])  # none chains with another; input order is not rank order
    g = np.array([3, 3, 3], dtype=np.uint32)
    f, pred, chains, members, chain_of = A.chain_all(h, g)
    assert (pred == -1).all()
    assert chains[["group", "head", "score"]].tolist() == [(3, 2, 41), (3, 1, 40), (3, 0, 40)] and chain_of.tolist() == [2, 1, 0]
