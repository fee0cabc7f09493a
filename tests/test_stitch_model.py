"""CPU: the link checker tests/cpp/stitch_check.c (a row-major full-matrix global Gotoh with the walk rules of sa_stitch_chains) against
an enumeration of every alignment of small rectangles and hand-worked cases, and the chain assembly of tests/stitch_model.py."""
import itertools

import numpy as np
import pytest

import stitch_model as S

A, C, G, T, SEP = 0, 1, 2, 3, 7


def matrix(match, mismatch):
    m = np.full(64, -mismatch, dtype=np.int32)
    for a in range(4):
        m[a * 8 + a] = match
    return m


UNIT = matrix(1, 1)
BIG = matrix(10, 10)


def ops_of(text):
    """'2I4M' -> uint32 ops."""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 2 | "MID".index(ch))
            n = ""
    return np.array(out, dtype=np.uint32)


def best_by_enumeration(x, y, sub, O, E):
    """The maximum, over every sequence of M / I / D that consumes x and y, of the score counted by runs."""
    best = None

    def go(i, j, seq):
        nonlocal best
        if i == len(x) and j == len(y):
            s, prev = 0, None
            a = b = 0
            for op in seq:
                if op == "M":
                    s += int(sub[x[a] * 8 + y[b]])
                    a += 1
                    b += 1
                else:
                    s -= (O if op != prev else 0) + E
                    if op == "I":
                        b += 1
                    else:
                        a += 1
                prev = op
            best = s if best is None else max(best, s)
            return
        if i < len(x) and j < len(y):
            go(i + 1, j + 1, seq + ["M"])
        if j < len(y):
            go(i, j + 1, seq + ["I"])
        if i < len(x):
            go(i + 1, j, seq + ["D"])
    go(0, 0, [])
    return best


def check_link(x, y, sub, O, E):
    res, ops = S.link(x, y, sub, O, E)
    assert not res["dead"]
    assert res["score"] == best_by_enumeration(list(x), list(y), sub, O, E), (x, y, O, E)
    assert S.consumed(ops) == (len(x), len(y))
    t, q = np.array(x, dtype=np.uint8), np.array(y, dtype=np.uint8)
    assert S.rescore(t, q, sub, 0, 0, ops, O, E) == res["score"]
    ln, op = ops >> 2, ops & 3
    assert np.all(ln > 0) and np.all(op[1:] != op[:-1])
    gaps = ops[op != S.OP_M]
    assert (res["gap_opens"], res["gap_bases"]) == (gaps.size, int((gaps >> 2).sum()))
    assert res["matches"] + res["mismatches"] == int(ln[op == S.OP_M].sum())
    return res, ops


@pytest.mark.parametrize("O,E", [(0, 1), (1, 1), (3, 1), (2, 0)])
def test_every_rectangle_up_to_3_by_3(O, E):
    for dt, dq in itertools.product(range(4), repeat=2):
        for x in itertools.product((A, C), repeat=dt):
            for y in itertools.product((A, C), repeat=dq):
                check_link(x, y, UNIT, O, E)


def test_random_rectangles_up_to_6_by_6():
    rng = np.random.default_rng(7)
    for k in range(120):
        dt, dq = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        x, y = rng.integers(0, 2, dt).tolist(), rng.integers(0, 2, dq).tolist()
        O, E = int(rng.integers(0, 5)), int(rng.integers(0, 3))
        sub = matrix(int(rng.integers(1, 4)), int(rng.integers(0, 4)))
        check_link(x, y, sub, O, E)


def test_the_empty_link_and_the_one_sided_links():
    res, ops = S.link([], [], UNIT, 400, 30)
    assert (res["score"], res["dead"], ops.size) == (0, 0, 0)
    res, ops = S.link([A, C, G], [], UNIT, 400, 30)
    assert res["score"] == -(400 + 3 * 30) and np.array_equal(ops, ops_of("3D"))
    res, ops = S.link([], [A, C], UNIT, 400, 30)
    assert res["score"] == -(400 + 2 * 30) and np.array_equal(ops, ops_of("2I"))


def test_tie_h_equals_m_equals_e_takes_m():
    # O = 0, E = 1, x = A, y = AA: H(1,1) = 1, so E(1,2) = 0; M(1,2) = H(0,1) + 1 = 0 too.  M is taken, then (0,1) is an I
    res, ops = check_link([A], [A, A], UNIT, 0, 1)
    assert res["score"] == 0 and np.array_equal(ops, ops_of("1I1M"))


def test_an_e_tie_opens():
    # O = 0, E = 1, x = A, y = AAC: H(1,3) = E(1,3) = -1 (M(1,3) = -3).  In state E at (1,3): E(1,2) = 0 = H(1,2) - O, a tie, which
    # opens: state H at (1,2), where H == M (the case above).  Extending instead would give 1M2I, which scores the same
    res, ops = check_link([A], [A, A, C], UNIT, 0, 1)
    assert res["score"] == -1 and np.array_equal(ops, ops_of("1I1M1I"))


def test_free_opens():
    # O = 0: a D run of three is three back-to-back opens that cost nothing, reported as one run
    res, ops = check_link([A, A, A], [], UNIT, 0, 2)
    assert res["score"] == -6 and np.array_equal(ops, ops_of("3D")) and (res["gap_opens"], res["gap_bases"]) == (1, 3)
    # a mismatch column costs 3, a D and an I cost 1 each
    res, ops = check_link([A], [C], matrix(1, 3), 0, 1)
    assert res["score"] == -2 and S.consumed(ops) == (1, 1) and res["gap_opens"] == 2


@pytest.mark.parametrize("x,y,want", [([A, C, G, T], [G, G, A, C, G, T], "2I4M"), ([A, C, G, T], [A, C, G, T, G, G], "4M2I"),
                                      ([G, G, A, C, G, T], [A, C, G, T], "2D4M"), ([A, C, G, T, G, G], [A, C, G, T], "4M2D")],
                         ids=["I_at_the_start", "I_at_the_end", "D_at_the_start", "D_at_the_end"])
def test_a_gap_run_at_each_corner(x, y, want):
    res, ops = check_link(x, y, BIG, 2, 1)
    assert res["score"] == 40 - (2 + 2) and np.array_equal(ops, ops_of(want))


def test_a_separator_in_either_range_is_dead():
    for x, y in (([A, C, SEP, G], [A, C, G]), ([A, C, G], [A, SEP, C, G]), ([SEP], []), ([], [SEP]), ([A, SEP], [A, SEP])):
        res, ops = S.link(x, y, BIG, 2, 1)
        assert res["dead"] == 1 and ops.size == 0
    res, _ = S.link([A, C, G], [A, C, G], BIG, 2, 1)
    assert res["dead"] == 0 and res["score"] == 30


# ---- the assembly ----
def seqs(n=200, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n).astype(np.uint8)
    return t, t.copy()


def test_abutting_members_merge_into_one_m_run():
    t, q = seqs()
    h = S.make([(10, 10, 4, 0), (15, 15, 9, 0)])
    recs, ops, links, cnt = S.stitch(t, q, BIG, h, *S.csr([[0, 1]]), gap_open=2, gap_extend=1)
    assert recs.size == 1 and np.array_equal(ops, ops_of("15M")) and int(recs[0]["score"]) == 150
    assert (links[0]["dt"], links[0]["dq"], links[0]["score"], links[0]["flags"], links[0]["cells"]) == (0, 0, 0, 0, 1)
    assert (recs[0]["ref_start"], recs[0]["ref_end"], recs[0]["n_members"], recs[0]["matches"]) == (10, 25, 2, 15)


def test_a_link_of_matches_merges_with_both_neighbours():
    t, q = seqs()
    h = S.make([(10, 10, 3, 0), (20, 20, 3, 0)])
    recs, ops, links, _ = S.stitch(t, q, BIG, h, *S.csr([[0, 1]]), gap_open=2, gap_extend=1)
    assert np.array_equal(ops, ops_of("14M")) and int(recs[0]["score"]) == 140 and int(links[0]["score"]) == 60
    assert (recs[0]["gap_opens"], recs[0]["gap_bases"], recs[0]["n_ops"]) == (0, 0, 1)
    S.check_invariants(t, q, BIG, recs, ops, 2, 1)


def test_a_link_with_a_gap_sits_between_its_members():
    t, _ = seqs()
    q = np.concatenate([t[:30], t[33:]])  # three target bases the query lacks
    h = S.make([(10, 10, 9, 0), (40, 37, 9, 0)])
    recs, ops, links, _ = S.stitch(t, q, BIG, h, *S.csr([[0, 1]]), gap_open=2, gap_extend=1)
    assert int(links[0]["score"]) == 170 - 5 and int(recs[0]["score"]) == 370 - 5
    ln, op = ops >> 2, ops & 3
    assert op.tolist() == [0, 2, 0] and int(ln[1]) == 3 and S.consumed(ops) == (40, 37)
    S.check_invariants(t, q, BIG, recs, ops, 2, 1)


def test_a_chain_of_one_member():
    t, q = seqs()
    h = S.make([(5, 7, 11, 999)])
    recs, ops, links, cnt = S.stitch(t, q, UNIT, h, *S.csr([[0]]))
    assert recs.size == 1 and links.size == 0 and np.array_equal(ops, ops_of("12M"))
    r = recs[0]
    assert (r["chain"], r["first_member"], r["n_members"], r["flags"], r["ref_start"], r["ref_end"], r["query_start"], r["query_end"]) == \
        (0, 0, 1, 0, 5, 17, 7, 19)
    want = int(UNIT.astype(np.int64)[t[5:17].astype(np.int64) * 8 + q[7:19]].sum())
    assert int(r["score"]) == want  # from the codes, not from the HSP's score field
    S.check_invariants(t, q, UNIT, recs, ops)


def test_every_link_broken():
    t, q = seqs()
    h = S.make([(10 * k, 10 * k, 3, 0) for k in range(5)])
    recs, ops, links, cnt = S.stitch(t, q, BIG, h, *S.csr([[0, 1, 2, 3, 4]]), gap_open=2, gap_extend=1, max_link=5)
    assert recs.size == 5 and recs["flags"].tolist() == [S.LONG] * 4 + [0] and recs["first_member"].tolist() == [0, 1, 2, 3, 4]
    assert np.all(recs["n_members"] == 1) and np.all(links["flags"] == S.LONG) and np.all(links["cells"] == 0) and np.all(links["score"] == 0)
    assert cnt == dict(links=4, swept=0, long_links=4, dead_links=0, low_links=0, cells=0, records=5)
    assert np.array_equal(ops, np.tile(ops_of("4M"), 5))


def test_a_break_in_the_middle():
    t, q = seqs()
    t[27] = SEP
    h = S.make([(0, 0, 3, 0), (10, 10, 3, 0), (30, 30, 3, 0), (40, 40, 3, 0)])
    recs, ops, links, cnt = S.stitch(t, q, BIG, h, *S.csr([[0, 1, 2, 3]]), gap_open=2, gap_extend=1)
    assert recs["first_member"].tolist() == [0, 2] and recs["n_members"].tolist() == [2, 2] and recs["flags"].tolist() == [S.DEAD, 0]
    assert links["flags"].tolist() == [0, S.DEAD, 0] and int(links[1]["score"]) == S.NEVER and int(links[1]["cells"]) == 17 * 17
    assert (recs[0]["ref_end"], recs[1]["ref_start"]) == (14, 30)
    S.check_invariants(t, q, BIG, recs, ops, 2, 1)
    # min_link_score at a link's score keeps it, one above breaks it
    s0 = int(links[0]["score"])
    assert S.stitch(t, q, BIG, h, *S.csr([[0, 1]]), gap_open=2, gap_extend=1, min_link_score=s0)[0].size == 1
    low = S.stitch(t, q, BIG, h, *S.csr([[0, 1]]), gap_open=2, gap_extend=1, min_link_score=s0 + 1)
    assert low[0]["flags"].tolist() == [S.LOW, 0] and int(low[2][0]["score"]) == s0


def test_several_chains_share_an_hsp():
    t, q = seqs()
    h = S.make([(0, 0, 3, 0), (10, 10, 3, 0), (20, 20, 3, 0)])
    recs, ops, links, _ = S.stitch(t, q, BIG, h, *S.csr([[0, 1], [], [1, 2], [0, 2]]), gap_open=2, gap_extend=1)
    assert recs["chain"].tolist() == [0, 2, 3] and links["chain"].tolist() == [0, 2, 3]
    assert [S.record_ops(recs, ops, k).tolist() for k in range(3)] == [ops_of("14M").tolist(), ops_of("14M").tolist(), ops_of("24M").tolist()]
