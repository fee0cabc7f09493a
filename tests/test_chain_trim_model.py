"""CPU: the trim model (tests/chain_trim_model.py; contract in include/segalign_amd.h): the crossover against a brute
force over all x, trimmed chains inside sa_chain_hsps's relation, the exact scores against an independent re-scoring of the trimmed
chain, and every clause of the validation."""
import numpy as np
import pytest

import chain_trim_model as T
import hsp_chain_gap_model as G
import hsp_chain_model as M
import hsp_chain_overlap_model as O
from gapped_model import SUB


def test_the_crossover_equals_a_brute_force_over_all_x():
    rng = np.random.default_rng(3)
    for o in [0, 1, 2, 3, 7, 64, 65, 200]:
        for vals in ([-100, 91], [0, 1], [-3, -2, 5]):  # few values: many ties
            a, b = [int(v) for v in rng.choice(vals, o)], [int(v) for v in rng.choice(vals, o)]
            s = [sum(a[:x]) + sum(b[x:]) for x in range(o + 1)]
            assert T.crossover(a, b) == s.index(max(s))
    assert T.crossover([5, 5, 5], [5, 5, 5]) == 0 and T.crossover([1, 1], [0, 0]) == 2 and T.crossover([0, 0], [1, 1]) == 0
    assert T.crossover([1, -1, 1], [0, 0, 0]) == 1  # S = 0, 1, 0, 1: the first of the two maxima


def world(seed, n=30, chains=4):
    """A random target, a query that copies it member by member with mismatches, and chains of overlapping members."""
    rng = np.random.default_rng(seed)
    t, q = rng.integers(0, 4, 20000).astype(np.uint8), rng.integers(0, 4, 20000).astype(np.uint8)
    rows, lists = [], []
    for c in range(chains):
        r, s, cur = 100 + 4000 * c, 300 + 4000 * c, []
        bases = [int(x) for x in rng.integers(5, 60, n)]
        for k, b in enumerate(bases):
            rows.append((r, s, b, int(rng.integers(-50, 5000))))
            cur.append(len(rows) - 1)
            q[s:s + b] = np.where(rng.random(b) < 0.2, (t[r:r + b] + 1) % 4, t[r:r + b])
            if k + 1 == n:
                break
            half = (min(b, bases[k + 1]) - 1) // 2  # the largest overlap the two take: 2 o < min(bases)
            o = int(rng.integers(0, half + 1)) * int(rng.integers(0, 2))
            kind, gap = int(rng.integers(0, 3)), int(rng.integers(0, 9))  # on both axes alike, on the target only, on the query only
            r, s = (r + b - o, s + b - o) if kind == 0 else (r + b - o, s + b + gap) if kind == 1 else (r + b + gap, s + b - o)
        lists.append(cur)
    return t, q, M.make(rows), lists


def csr(lists):
    return np.array([i for c in lists for i in c], dtype=np.uint32), np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.uint32)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("kw", [dict(), dict(diag_pen=3, anti_pen=2), dict(gap_costs="loose", anti_pen=1)])
def test_trimmed_chains_are_collinear_and_their_scores_are_exact(seed, kw):
    t, q, h, lists = world(seed)
    members, first = csr(lists)
    out, chains, links = T.trim(t, q, SUB, h, members, first, **kw)
    assert out.size == members.size and (links["o"] > 0).sum() > 10 and (links["x"] > 0).any() and (links["x"] < links["o"]).any()
    tab = G.validate(kw["gap_costs"]) if "gap_costs" in kw else None
    at = 0
    for c in range(len(lists)):
        lo, hi = int(first[c]), int(first[c + 1])
        score = 0
        for k in range(lo, hi):
            r, s, b, sc = O.node(out, k)
            src = O.node(h, int(members[k]))
            if (r, s, b) == src[:3]:
                assert sc == src[3]  # untouched: bit for bit, its input score included
            else:
                assert b >= 1 and sc == sum(T.columns(t, q, SUB, r, s, b))
            score += sc
            if k + 1 < hi:
                assert M.precedes(out, None, k, k + 1)  # sa_chain_hsps's relation: no shared base on either axis
                l = links[at]
                at += 1
                assert G.link_penalty(out, k, k + 1, kw.get("diag_pen", 0), kw.get("anti_pen", 0), tab) == \
                    O.link_penalty(h, int(members[k]), int(members[k + 1]), kw.get("diag_pen", 0), kw.get("anti_pen", 0), tab)
                score -= G.link_penalty(out, k, k + 1, kw.get("diag_pen", 0), kw.get("anti_pen", 0), tab)
                nr, ns = O.node(out, k + 1)[:2]
                assert (nr - (r + b), ns - (s + b)) == (int(l["gap_r"]), int(l["gap_q"]))
        assert int(chains["score"][c]) == score
    assert at == links.size and int(chains["bases_cut"].sum()) == int(links["o"].sum())
    lost = sum(O.node(h, int(m))[2] for m in members) - sum(O.node(out, k)[2] for k in range(out.size))
    assert lost == int(links["o"].sum())


def test_a_member_cut_at_both_ends_down_to_one_base():
    t, q = np.zeros(100, dtype=np.uint8), np.zeros(100, dtype=np.uint8)
    # the middle member [20, 27) shares three target bases with each neighbour; it mismatches in its first and its last three columns,
    # the neighbours match in theirs: it loses both ends and keeps its middle base
    q[20:23] = 1
    q[24:27] = 1
    h = M.make([(10, 1, 13, 7), (20, 20, 7, 7), (24, 40, 10, 7)])
    out, chains, links = T.trim(t, q, SUB, h, np.array([0, 1, 2], dtype=np.uint32), np.array([0, 3], dtype=np.uint32))
    assert [tuple(int(v) for v in l) for l in links] == [(3, 3, 0, 9), (3, 0, 0, 16)]
    assert [O.node(out, k)[:3] for k in range(3)] == [(10, 1, 13), (23, 23, 1), (24, 40, 10)]
    assert int(out["score"][0]) == 7 and int(out["score"][2]) == 7 and int(out["score"][1]) == int(SUB[0])  # one matching column
    assert tuple(int(v) for v in chains[0]) == (14 + int(SUB[0]), 2, 6)


@pytest.mark.parametrize("what,clause", [("outside", "inside the block"), ("half", "overlaps"), ("far", "overlaps"), ("index", "not in the input"),
                                         ("first", "first")])
def test_every_validation_clause(what, clause):
    t, q = np.zeros(20000, dtype=np.uint8), np.zeros(20000, dtype=np.uint8)
    h = M.make([(100, 100, 50, 1), (140, 140, 50, 1), (19990, 100, 20, 1), (120, 120, 50, 1), (1000, 1000, 9000, 1), (5903, 5903, 9000, 1)])
    members, first = {"outside": ([0, 2], [0, 2]), "half": ([0, 3], [0, 2]), "far": ([4, 5], [0, 2]), "index": ([0, 6], [0, 2]),
                      "first": ([0, 1], [1, 2])}[what]
    with pytest.raises(ValueError, match=clause):
        T.trim(t, q, SUB, h, members, first)
    T.trim(t, q, SUB, h, [0, 1], [0, 2])
    h[5]["ref_start"] = h[5]["query_start"] = 5904  # o = 4096
    T.trim(t, q, SUB, h, [4, 5], [0, 2])
