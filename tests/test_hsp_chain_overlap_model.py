"""CPU: the overlap chaining model (tests/hsp_chain_overlap_model.py; contract in include/segalign_amd.h) against an
exhaustive search over every valid chain under the new relation and charge, against hsp_chain_model / hsp_chain_gap_model where no
overlap is allowed or none occurs, and one hand case per clause of the relation."""
import itertools

import numpy as np
import pytest

import hsp_chain_gap_model as G
import hsp_chain_model as M
import hsp_chain_overlap_model as O

HAND = {"pos": [2, 10, 100, 1000], "q_gap": [5, 50, 60, 60], "t_gap": [7, 7, 700, 800], "both_gap": [20, 30, 300, 3000]}


def exhaustive(h, g, dp, ap, mg, t, mo):
    """best[i] = the largest score of any valid chain that ends at i: member scores less every link's pen' and charge."""
    n = h.size
    best = [None] * n
    order = [int(x) for x in M.rank_order(h, g)]
    for k in range(1, n + 1):
        for sub in itertools.combinations(order, k):  # rank order: the only order in which a subset can chain
            if not all(O.precedes(h, g, sub[x], sub[x + 1], mo, mg) for x in range(k - 1)):
                continue
            s = sum(int(h["score"][x]) for x in sub)
            s -= sum(O.link_penalty(h, sub[x], sub[x + 1], dp, ap, t) + O.charge(h, sub[x], sub[x + 1]) for x in range(k - 1))
            e = sub[-1]
            if best[e] is None or s > best[e]:
                best[e] = s
    return best


def random_set(rng, n, groups, spread):
    """HSPs near the main diagonal, long enough to overlap their neighbours by a few bases."""
    rows = []
    for _ in range(n):
        r, d = int(rng.integers(0, spread)), int(rng.integers(-6, 7)) * int(rng.integers(0, 2))
        rows.append((r + 10, r + 10 + d, int(rng.integers(1, 40)), int(rng.integers(-30, 3000))))
    h = M.make(rows)
    g = rng.integers(0, groups, n).astype(np.uint32) if groups > 1 else None
    return h, g


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("table", [None, "loose", "hand"])
@pytest.mark.parametrize("params", [(0, 0, 0, 8), (3, 1, 0, 64), (0, 2, 30, 5)])
def test_model_equals_exhaustive_search(seed, table, params):
    dp, ap, mg, mo = params
    t = None if table is None else G.validate(HAND if table == "hand" else table)
    rng = np.random.default_rng(300 + seed)
    linked = overlapping = 0
    for groups in (1, 3):
        for n, spread in ((1, 100), (4, 60), (7, 120), (9, 150), (8, 90)):
            h, g = random_set(rng, n, groups, spread)
            f, pred, _ = O.chain(h, g, dp, ap, mg, min_score=-10 ** 9, gap_costs=t, max_overlap=mo)
            assert [int(x) for x in f] == exhaustive(h, g, dp, ap, mg, t, mo), (groups, n)
            linked += int((pred >= 0).sum())
            overlapping += sum(1 for i, p in enumerate(pred) if p >= 0 and O.overlap(h, int(p), i) > 0)
    assert linked > 0 and overlapping > 0, "no set had an overlapping link"


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("table", [None, "medium"])
def test_no_allowance_is_the_old_model(seed, table):
    rng = np.random.default_rng(400 + seed)
    h, g = random_set(rng, 120, 3, 900)
    kw = dict(diag_pen=2, anti_pen=1, max_gap=200, min_score=500)
    want = G.chain(h, g, gap_costs=table, **kw)
    got = O.chain(h, g, gap_costs=table, max_overlap=0, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    assert not np.array_equal(O.chain(h, g, gap_costs=table, max_overlap=16, **kw)[1], want[1]), "the set has no overlap to allow"


@pytest.mark.parametrize("table", [None, "loose"])
def test_an_input_without_overlaps_is_the_old_model_under_any_allowance(table):
    rng = np.random.default_rng(9)
    rows = [(100 + 50 * k + int(rng.integers(0, 5)), 100 + 50 * k + int(rng.integers(0, 5)), int(rng.integers(5, 40)), int(rng.integers(2000, 5000)))
            for k in range(80)]  # starts 45 .. 55 apart, at most 40 bases: no two share a base on either axis
    h = M.make(rows)[rng.permutation(80)]
    assert all(O.overlap(h, j, i) == 0 or O.overlap(h, i, j) == 0 for j in range(80) for i in range(80) if i != j)
    order = list(M.rank_order(h))
    assert all(O.overlap(h, order[a], order[b]) == 0 for a in range(80) for b in range(a + 1, 80))
    want = G.chain(h, None, diag_pen=1, anti_pen=1, gap_costs=table)
    got = O.chain(h, None, diag_pen=1, anti_pen=1, gap_costs=table, max_overlap=4096)
    assert all(np.array_equal(a, b) for a, b in zip(want, got)) and (want[1] >= 0).sum() > 40


# ---- one hand case per clause ----
def two(j, i):
    return M.make([j, i])


def test_the_allowance_is_inclusive():
    h = two((100, 100, 50, 500), (140, 140, 50, 700))  # re_j = 150: o = 10 on both axes
    assert O.overlap(h, 0, 1) == 10
    assert O.precedes(h, None, 0, 1, 10) and not O.precedes(h, None, 0, 1, 9)
    assert O.chain(h, max_overlap=10)[1][1] == 0 and O.chain(h, max_overlap=9)[1][1] == -1
    big = two((1000, 1000, 9000, 500), (1000 + 9000 - 4096, 1000 + 9000 - 4096, 9000, 700))
    assert O.overlap(big, 0, 1) == 4096 and O.precedes(big, None, 0, 1, 4096)
    big[1]["ref_start"] -= 1
    big[1]["query_start"] -= 1
    assert O.overlap(big, 0, 1) == 4097 and not O.precedes(big, None, 0, 1, 4096)
    with pytest.raises(ValueError):
        O.validate(4097)
    with pytest.raises(ValueError):
        O.validate(5, reserved=1)


@pytest.mark.parametrize("short", ["j", "i"])
def test_an_overlap_must_stay_below_half_of_the_shorter_hsp(short):
    o = 7
    for bases, ok in ((2 * o + 1, True), (2 * o, False)):
        bj, bi = (bases, 60) if short == "j" else (60, bases)
        h = two((100, 100, bj, 500), (100 + bj - o, 100 + bj - o, bi, 700))
        assert O.overlap(h, 0, 1) == o and O.precedes(h, None, 0, 1, 64) == ok
        assert (O.chain(h, max_overlap=64)[1][1] == 0) == ok


def test_overlap_on_the_target_only_the_query_only_and_both():
    # j = [100, 150) x [100, 150)
    for (ri, qi), o, gaps in (((145, 160), 5, (0, 15)), ((170, 142), 8, (28, 0)), ((147, 141), 9, (6, 0)), ((138, 144), 12, (0, 6))):
        h = two((100, 100, 50, 1000), (ri, qi, 50, 1000))
        assert O.overlap(h, 0, 1) == o and O.trimmed_gaps(h, 0, 1) == gaps and O.precedes(h, None, 0, 1, 64)
        w = (65536 * 1000) // 50
        assert O.weight(h, 0) == w and O.charge(h, 0, 1) == (o * w) >> 16 == 20 * o
        f, pred, _ = O.chain(h, anti_pen=1, max_overlap=64)
        assert pred[1] == 0 and f[1] == 2000 - sum(gaps) - 20 * o


def test_the_charge_takes_the_lower_weight_and_a_negative_score_charges_nothing():
    h = M.make([(100, 100, 50, 1000), (140, 140, 40, 1000), (140, 140, 40, -5)])
    assert O.weight(h, 0) < O.weight(h, 1) and O.charge(h, 0, 1) == (10 * O.weight(h, 0)) >> 16 == 200
    assert O.weight(h, 2) == 0 and O.charge(h, 0, 2) == 0
    f, pred, _ = O.chain(h, max_overlap=10)
    assert (int(f[1]), int(pred[1])) == (1800, 0) and (int(f[2]), int(pred[2])) == (995, 0)
    assert ((3 * 43690) >> 16) == 1  # w = floor(65536 * 2 / 3) = 43690: the shift floors 1.99 to 1
    assert O.weight(M.make([(0, 0, 3, 2)]), 0) == 43690


def test_max_gap_is_taken_on_the_trimmed_gap():
    h = two((100, 100, 50, 1000), (145, 175, 50, 1000))  # o = 5: the query gap is 25 untrimmed and 30 trimmed
    assert O.trimmed_gaps(h, 0, 1) == (0, 30)
    assert O.precedes(h, None, 0, 1, 64, max_gap=30) and not O.precedes(h, None, 0, 1, 64, max_gap=29)
    assert O.chain(h, max_gap=30, max_overlap=64)[1][1] == 0 and O.chain(h, max_gap=29, max_overlap=64)[1][1] == -1


def test_the_table_sees_the_trimmed_gaps_and_their_zero():
    t = G.validate(HAND)
    h = two((100, 100, 50, 1000), (145, 155, 50, 1000))  # untrimmed (-5, 5); trimmed (0, 10): a gap in the query only
    assert O.trimmed_gaps(h, 0, 1) == (0, 10) and O.link_penalty(h, 0, 1, 0, 0, t) == G.gapcost(t, 0, 10) == 50
    assert O.chain(h, gap_costs=t, max_overlap=64)[0][1] == 2000 - 50 - 100
    h = two((100, 100, 50, 1000), (145, 145, 50, 1000))  # trimmed (0, 0): no gap cost at all, the charge alone
    assert O.link_penalty(h, 0, 1, 3, 3, t) == 0 and O.chain(h, gap_costs=t, max_overlap=64)[0][1] == 2000 - 100
    h = two((100, 100, 50, 1000), (160, 145, 50, 1000))  # trimmed (15, 0): the target-only case
    assert O.link_penalty(h, 0, 1, 0, 0, t) == G.gapcost(t, 15, 0) and O.link_penalty(h, 0, 1, 2, 0, t) == G.gapcost(t, 15, 0) + 2 * 15


def test_the_diagonal_term_is_untrimmed_and_groups_separate():
    h = two((100, 100, 50, 1000), (145, 155, 50, 1000))
    assert O.link_penalty(h, 0, 1, 7, 0, None) == 70
    g = np.array([0, 1], dtype=np.uint32)
    assert not O.precedes(h, g, 0, 1, 64) and O.chain(h, g, max_overlap=64)[1][1] == -1


def test_rank_order_is_an_evaluation_order():
    rng = np.random.default_rng(17)
    h, g = random_set(rng, 150, 2, 700)
    rank = np.zeros(150, dtype=np.int64)
    rank[M.rank_order(h, g)] = np.arange(150)
    links = [(j, i) for j in range(150) for i in range(150) if i != j and O.precedes(h, g, j, i, 4096)]
    assert len(links) > 1000 and any(O.overlap(h, j, i) > 0 for j, i in links)
    assert all(rank[j] < rank[i] and h["ref_start"][j] < h["ref_start"][i] and h["query_start"][j] < h["query_start"][i] for j, i in links)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("kw", [dict(max_overlap=64), dict(max_overlap=0, gap_costs="loose"), dict(max_overlap=7, diag_pen=2, anti_pen=1, max_gap=25),
                                dict(max_overlap=4096, gap_costs=HAND, anti_pen=1, min_score=4000)])
def test_the_row_form_of_the_model_equals_the_integer_form(seed, kw):
    rng = np.random.default_rng(500 + seed)
    h, g = random_set(rng, 160, 3, 1200)
    h["len"][:8] = rng.integers(200, 9000, 8)  # a few long HSPs, so that large overlaps occur under the largest allowance
    want, got = O.chain(h, g, **kw), O.chain_rows(h, g, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(want, got)) and (want[1] >= 0).sum() > 40
    none = np.zeros(0, dtype=M.SEG)
    assert all(np.array_equal(a, b) for a, b in zip(O.chain(none, None, **kw), O.chain_rows(none, None, **kw)))
