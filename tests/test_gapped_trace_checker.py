"""CPU: the path checker (tests/cpp/gapped_trace_check.c) against an unpruned full-matrix Gotoh traceback under the same tie rules,
against the extension checker (tests/cpp/gapped_check.c), and on hand-worked cases of the contract in include/segalign_amd.h
(sa_gapped_align)."""
import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T

SUB = G.SUB
HUGE = 1 << 28
A, C, G_, Tb, L, N, SEP = 0, 1, 2, 3, 4, 5, 7


def full_traceback(X, Y, sub, O, E):
    """Unpruned DP over the whole (len X + 1) x (len Y + 1) matrix with the dead-cell rule, its best cell (antidiagonal order, then
    smallest i) and the walk back from it under the contract's tie rules.  -> (best, bi, bj, ops in walk order, tie events)."""
    n, m = len(X), len(Y)
    ninf = float("-inf")
    H = [[ninf] * (m + 1) for _ in range(n + 1)]
    Ea = [[ninf] * (m + 1) for _ in range(n + 1)]
    Fa = [[ninf] * (m + 1) for _ in range(n + 1)]
    Ma = [[ninf] * (m + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                continue
            if (i >= 1 and X[i - 1] == SEP) or (j >= 1 and Y[j - 1] == SEP):
                continue
            e = max(Ea[i][j - 1], H[i][j - 1] - O) - E if j >= 1 else ninf
            f = max(Fa[i - 1][j], H[i - 1][j] - O) - E if i >= 1 else ninf
            mm = H[i - 1][j - 1] + int(sub[X[i - 1] * 8 + Y[j - 1]]) if i >= 1 and j >= 1 else ninf
            Ea[i][j], Fa[i][j], Ma[i][j], H[i][j] = e, f, mm, max(mm, e, f)
    best, bi, bj = 0, 0, 0
    for d in range(1, n + m + 1):
        for i in range(max(0, d - m), min(d, n) + 1):
            if H[i][d - i] > best:
                best, bi, bj = H[i][d - i], i, d - i
    walk, ties = [], []
    i, j, st = bi, bj, "H"
    while i + j > 0:
        if st == "H":
            if i >= 1 and j >= 1 and H[i][j] == Ma[i][j]:
                if H[i][j] == Ea[i][j] or H[i][j] == Fa[i][j]:
                    ties.append("M=gap")
                walk.append(T.OP_M)
                i, j = i - 1, j - 1
            elif H[i][j] == Ea[i][j]:
                st = "E"
            else:
                st = "F"
        elif st == "E":
            walk.append(T.OP_I)
            if Ea[i][j - 1] == H[i][j - 1] - O:
                ties.append("E open")
            st = "E" if Ea[i][j - 1] > H[i][j - 1] - O else "H"
            j -= 1
        else:
            walk.append(T.OP_D)
            if Fa[i - 1][j] == H[i - 1][j] - O:
                ties.append("F open")
            st = "F" if Fa[i - 1][j] > H[i - 1][j] - O else "H"
            i -= 1
    return int(best), bi, bj, runs(walk), ties


def runs(ops):
    out = []
    for op in ops:
        if out and (out[-1] & 3) == op:
            out[-1] += 4
        else:
            out.append(4 | op)
    return np.array(out, dtype=np.uint32)


def codes(s):
    return np.array(["ACGTLNXE".index(ch) for ch in s], dtype=np.uint8)


def mutate(rng, s, sub_rate, indel_rate):
    out = []
    for ch in s:
        r = rng.random()
        if r < indel_rate / 2:
            continue
        if r < indel_rate:
            out.extend(rng.integers(0, 4, size=int(rng.integers(1, 4))).tolist())
        out.append(int(rng.integers(0, 4)) if rng.random() < sub_rate else int(ch))
    return np.array(out, dtype=np.uint8)


SMALL_SUB = np.where(np.eye(8, dtype=bool), 10, -10).astype(np.int32).reshape(64)


def case(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 45))
    X = rng.integers(0, 4, size=n).astype(np.uint8)
    Y = mutate(rng, X, 0.15, 0.12) if seed % 2 else rng.integers(0, 4, size=int(rng.integers(1, 45))).astype(np.uint8)
    if len(Y) == 0:
        Y = np.array([A], dtype=np.uint8)
    if seed % 5 == 0:
        X[rng.integers(0, len(X), size=2)] = rng.choice([L, N])
        Y[int(rng.integers(0, len(Y)))] = SEP
    O, E = [(400, 30), (0, 30), (50, 5), (0, 10), (10, 10)][seed % 5]
    sub = SMALL_SUB if seed % 5 >= 3 else (SUB if seed % 4 else np.where(np.eye(8, dtype=bool), 100, -60).astype(np.int32).reshape(64))
    return X, Y, sub, O, E


def right(X, Y, sub, O, E, **kw):
    kw.setdefault("ydrop", HUGE)
    return T.side(X, Y, sub, 0, 0, +1, gap_open=O, gap_extend=E, **kw)


@pytest.mark.parametrize("seed", range(60))
def test_paths_equal_the_unpruned_traceback(seed):
    X, Y, sub, O, E = case(seed)
    best, bi, bj, want, _ = full_traceback(X.tolist(), Y.tolist(), sub, O, E)
    # right side: X[i] = T[i]; left side: X[i] = T[a - 1 - i], so the reversed sequences anchored at their ends
    for res, ops, walk in (right(X, Y, sub, O, E),
                           T.side(X[::-1].copy(), Y[::-1].copy(), sub, len(X), len(Y), -1, gap_open=O, gap_extend=E, ydrop=HUGE)):
        assert res[:3] == (best, bi, bj)
        assert np.array_equal(ops, want), (T.OP_M, ops.tolist(), want.tolist())
        assert walk["score"] == best
        assert T.consumed(ops) == (bi, bj)


def test_the_random_cases_meet_every_tie_rule():
    seen = set()
    for seed in range(400):
        X, Y, sub, O, E = case(seed)
        *_, ties = full_traceback(X.tolist(), Y.tolist(), sub, O, E)
        seen.update(ties)
    assert {"M=gap", "E open", "F open"} <= seen


def test_identical_sequences_give_one_match_run():
    rng = np.random.default_rng(5)
    X = rng.integers(0, 4, size=60).astype(np.uint8)
    res, ops, walk = right(X, X, SUB, 400, 30)
    assert res[1:3] == (60, 60)
    assert ops.tolist() == [60 << 2 | T.OP_M]
    assert walk["matches"] == 60 and walk["mismatches"] == 0 and walk["gap_opens"] == 0


@pytest.mark.parametrize("k", [1, 3, 7])
def test_one_insertion(k):
    rng = np.random.default_rng(k)
    X = rng.integers(0, 4, size=80).astype(np.uint8)
    a = 40
    ins = np.full(k, (int(X[a]) + 1) % 4, dtype=np.uint8)
    if ins[-1] == X[a - 1]:
        ins[:] = (int(X[a]) + 2) % 4
    Y = np.concatenate([X[:a], ins, X[a:]])
    res, ops, walk = right(X, Y, SUB, 400, 30)
    assert ops.tolist() == [a << 2 | T.OP_M, k << 2 | T.OP_I, (80 - a) << 2 | T.OP_M]
    assert walk["gap_opens"] == 1 and walk["gap_bases"] == k and walk["score"] == res[0]
    # the same in the other direction: a deletion
    res, ops, _ = right(Y, X, SUB, 400, 30)
    assert ops.tolist() == [a << 2 | T.OP_M, k << 2 | T.OP_D, (80 - a) << 2 | T.OP_M]


def test_m_equal_e_takes_m():
    # X = ACG, Y = AACG, match 10, mismatch -10, O = 0, E = 10.  Cell (1, 2): M = H(0,1) + s(A, A) = -10 + 10 = 0 and
    # E = max(E(1,1), H(1,1) - 0) - 10 = 10 - 10 = 0, so H = 0 = M = E.  The best cell is (3, 4) (20: A A, C C, G G after the query's
    # first base); the walk reaches (1, 2) in state H and must take M there (X[0] with Y[1]), then I for Y[0] from (0, 1).
    X, Y = codes("ACG"), codes("AACG")
    best, bi, bj, want, ties = full_traceback(X.tolist(), Y.tolist(), SMALL_SUB, 0, 10)
    res, ops, _ = right(X, Y, SMALL_SUB, 0, 10)
    assert "M=gap" in ties
    assert res[:3] == (best, bi, bj) == (20, 3, 4)
    assert ops.tolist() == want.tolist() == [3 << 2 | T.OP_M, 1 << 2 | T.OP_I]  # walk order: best cell -> anchor


def test_e_tie_opens():
    # O = 0: a query gap of two bases can be read as one run or as two back-to-back opens; a tie opens, and the run-length form
    # still holds one I run of two (the opens cost nothing)
    X, Y = codes("ACGTACGTAC"), codes("ACGTAGGCGTAC")
    best, bi, bj, want, ties = full_traceback(X.tolist(), Y.tolist(), SMALL_SUB, 0, 10)
    res, ops, walk = right(X, Y, SMALL_SUB, 0, 10)
    assert "E open" in ties
    assert np.array_equal(ops, want) and walk["score"] == res[0]
    assert T.consumed(ops) == (bi, bj)


def test_no_op_consumes_a_separator():
    rng = np.random.default_rng(9)
    X = rng.integers(0, 4, size=50).astype(np.uint8)
    Tt = np.concatenate([X[:30], [SEP], X[30:]]).astype(np.uint8)
    res, ops, _ = right(Tt, X, SUB, 400, 30)
    assert T.consumed(ops)[0] <= 30 and res[1] <= 30
    Q = np.concatenate([X[:20], [SEP], X[20:]]).astype(np.uint8)
    res, ops, _ = right(X, Q, SUB, 400, 30)
    assert T.consumed(ops)[1] <= 20 and res[2] <= 20
    # the left side never crosses the separator in front of the anchor either
    res, ops, _ = T.side(Tt, Tt, SUB, 40, 40, -1, gap_open=400, gap_extend=30)
    assert T.consumed(ops) == (res[1], res[2]) and res[1] <= 9


def test_gap_at_the_anchor_on_both_sides_stays_split():
    rng = np.random.default_rng(11)
    Ls = rng.integers(0, 4, size=40).astype(np.uint8)
    Rs = rng.integers(0, 4, size=40).astype(np.uint8)
    ins1 = np.full(2, (int(Ls[-1]) + 1) % 4, dtype=np.uint8)
    ins2 = np.full(3, (int(Rs[0]) + 1) % 4, dtype=np.uint8)
    t = np.concatenate([Ls, Rs])
    q = np.concatenate([Ls, ins1, ins2, Rs])
    hsp = np.array([(40, 42, 0, 0)], dtype=G.SEG_DTYPE)  # anchor (40, 42): between ins1 and ins2
    recs, paths = T.align(t, q, SUB, hsp)
    lo, ro, cnt = paths[0]
    assert lo.tolist() == [40 << 2 | T.OP_M, 2 << 2 | T.OP_I]
    assert ro.tolist() == [3 << 2 | T.OP_I, 40 << 2 | T.OP_M]
    assert cnt["gap_opens"] == 2 and cnt["gap_bases"] == 5
    pa, ops = T.pack(paths)
    assert pa[0]["n_left"] == 2 and pa[0]["n_right"] == 2 and ops.size == 4
    assert recs[0]["score"] == T.rescore(t, q, SUB, 0, 0, lo, 400, 30)[0] + T.rescore(t, q, SUB, 40, 42, ro, 400, 30)[0]


@pytest.mark.parametrize("seed", range(4))
def test_records_equal_the_extension_checker(seed):
    rng = np.random.default_rng(70 + seed)
    t = rng.integers(0, 4, size=6000).astype(np.uint8)
    q = mutate(rng, t, 0.1, 0.02)
    t[rng.integers(0, t.size, size=60)] = L
    t[[1500, 4000]] = SEP
    q[[2000]] = SEP
    n = 14
    pos = rng.integers(0, min(t.size, q.size) - 50, size=n)
    hsps = np.array([(int(p), int(p) + int(rng.integers(-3, 4)), int(rng.integers(0, 40)), 0) for p in pos], dtype=G.SEG_DTYPE)
    hsps[0] = (1495, 1495, 8, 0)  # next to a separator
    kw = dict(max_extent=600, max_band=[0, 12, 2048, 100][seed], gap_open=[400, 0, 400, 50][seed], ydrop=[9430, 9430, 300, 2000][seed])
    recs, paths = T.align(t, q, SUB, hsps, **kw)
    want = G.extend(t, q, SUB, hsps, **kw)
    assert np.array_equal(recs, want)
    for k, (lo, ro, cnt) in enumerate(paths):
        r = recs[k]
        ar, aq = int(hsps[k]["ref_start"] + hsps[k]["len"] // 2), int(hsps[k]["query_start"] + hsps[k]["len"] // 2)
        assert T.canonical(lo) and T.canonical(ro)
        assert T.consumed(lo) == (ar - r["ref_start"], aq - r["query_start"])
        assert T.consumed(ro) == (r["ref_end"] - ar, r["query_end"] - aq)
        sl, ml, xl = T.rescore(t, q, SUB, int(r["ref_start"]), int(r["query_start"]), lo, kw["gap_open"], 30)
        sr, mr, xr = T.rescore(t, q, SUB, ar, aq, ro, kw["gap_open"], 30)
        assert sl + sr == r["score"] and (ml + mr, xl + xr) == (cnt["matches"], cnt["mismatches"])


def test_cigar_helper():
    from segalign_amd import engine as E
    assert E.cigar(np.array([5 << 2 | 0, 2 << 2 | 1, 3 << 2 | 2], dtype=np.uint32)) == "5M2I3D"
    assert E.cigar(np.zeros(0, dtype=np.uint32)) == ""
    assert E.PATH_DTYPE == T.PATH_DTYPE and E.PATH_DTYPE.itemsize == 32
