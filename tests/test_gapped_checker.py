"""CPU: the gapped-extension checker (tests/cpp/gapped_check.c) against an unpruned Gotoh DP, and hand-worked cases of the
contract in include/segalign_amd.h (sa_gapped_extend)."""
import numpy as np
import pytest

import gapped_model as G

SUB = G.SUB
HUGE = 1 << 28
A, C, G_, T, L, N, SEP = 0, 1, 2, 3, 4, 5, 7


def codes(s):
    return np.array(["ACGTLNXE".index(ch) for ch in s], dtype=np.uint8)


def full_gotoh(X, Y, sub, O, E):
    """Unpruned DP over the whole (len X + 1) x (len Y + 1) matrix with the dead-cell rule: best score and the first cell reaching it
    (antidiagonal order, then smallest i)."""
    n, m = len(X), len(Y)
    ninf = float("-inf")
    H = [[ninf] * (m + 1) for _ in range(n + 1)]
    Ea = [[ninf] * (m + 1) for _ in range(n + 1)]
    Fa = [[ninf] * (m + 1) for _ in range(n + 1)]
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
            Ea[i][j], Fa[i][j], H[i][j] = e, f, max(mm, e, f)
    best, bi, bj = 0, 0, 0
    for d in range(1, n + m + 1):
        for i in range(max(0, d - m), min(d, n) + 1):
            if H[i][d - i] > best:
                best, bi, bj = H[i][d - i], i, d - i
    return int(best), bi, bj


def right(X, Y, **kw):
    return G.side(X, Y, kw.pop("sub", SUB), 0, 0, +1, **kw)


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


@pytest.mark.parametrize("seed", range(40))
def test_checker_equals_unpruned_dp(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 45))
    X = rng.integers(0, 4, size=n).astype(np.uint8)
    if seed % 2:
        Y = mutate(rng, X, 0.15, 0.1)  # homologous
    else:
        Y = rng.integers(0, 4, size=int(rng.integers(1, 45))).astype(np.uint8)  # random
    if len(Y) == 0:
        Y = np.array([A], dtype=np.uint8)
    if seed % 5 == 0:  # soft-masked and N codes, a separator
        X[rng.integers(0, len(X), size=2)] = rng.choice([L, N])
        Y[int(rng.integers(0, len(Y)))] = SEP
    O, E = [(400, 30), (0, 30), (50, 5)][seed % 3]
    sub = SUB if seed % 4 else (np.where(np.eye(8, dtype=bool), 100, -60).astype(np.int32).reshape(64))
    want = full_gotoh(X.tolist(), Y.tolist(), sub, O, E)
    for direction in (+1, -1):
        if direction > 0:
            got = G.side(X, Y, sub, 0, 0, +1, gap_open=O, gap_extend=E, ydrop=HUGE)
        else:  # the left side reads X[i] = T[a_r - 1 - i]
            got = G.side(X[::-1].copy(), Y[::-1].copy(), sub, len(X), len(Y), -1, gap_open=O, gap_extend=E, ydrop=HUGE)
        assert got[:3] == want, (direction, got, want)
        assert got[4] == 0


def test_identical_sequences_score_the_diagonal():
    X = codes("ACGTTGCAAGCTTACG" * 4)
    best, i, j, cells, flags = right(X, X)
    assert (best, i, j, flags) == (int(sum(SUB[c * 8 + c] for c in X)), len(X), len(X), 0)


def test_one_insertion_costs_open_plus_k_extensions():
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 4, size=60).astype(np.uint8), rng.integers(0, 4, size=60).astype(np.uint8)
    for k in (1, 3, 7):
        ins = rng.integers(0, 4, size=k).astype(np.uint8)
        X, Y = np.concatenate([a, b]), np.concatenate([a, ins, b])
        best, i, j, _, _ = right(X, Y)
        matches = int(sum(SUB[c * 8 + c] for c in X))
        assert best == matches - 400 - k * 30
        assert (i, j) == (120, 120 + k)


def test_no_gap_jumps_a_separator():
    rng = np.random.default_rng(3)
    s1, s2 = rng.integers(0, 4, size=40).astype(np.uint8), rng.integers(0, 4, size=80).astype(np.uint8)
    Y = np.concatenate([s1, s2])
    with_sep = np.concatenate([s1, [SEP], s2]).astype(np.uint8)
    best, i, j, _, _ = right(with_sep, Y)
    assert (best, i, j) == (int(sum(SUB[c * 8 + c] for c in s1)), 40, 40)
    # the same base as an ordinary mismatching code: the gap over it pays, so the rule above is what stopped the extension
    best_x, i_x, _, _, _ = right(np.concatenate([s1, [6], s2]).astype(np.uint8), Y)
    assert best_x > best and i_x == 121


def test_soft_masked_tail_is_not_aligned():
    s = codes("ACGTAGGCTTAC" * 3)
    X = np.concatenate([s, np.full(30, L, np.uint8)])
    Y = np.concatenate([s, np.full(30, L, np.uint8)])
    best, i, j, _, _ = right(X, Y)
    assert (best, i, j) == (int(sum(SUB[c * 8 + c] for c in s)), len(s), len(s))


def test_n_run_is_crossed_within_ydrop_only():
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, 4, size=50).astype(np.uint8), rng.integers(0, 4, size=150).astype(np.uint8)
    X = np.concatenate([a, np.full(12, N, np.uint8), b])
    score = lambda s: int(sum(SUB[c * 8 + c] for c in s))
    # around the run by two 12-base gaps (-1520) rather than through it (-12000)
    best, i, j, _, _ = right(X, X)
    assert (best, i, j) == full_gotoh(X.tolist(), X.tolist(), SUB, 400, 30)
    assert (best, i, j) == (score(a) + score(b) - 2 * (400 + 12 * 30), len(X), len(X))
    best, i, j, _, _ = right(X, X, ydrop=1000)
    assert (best, i, j) == (score(a), 50, 50)


def test_tie_goes_to_the_first_antidiagonal_then_smallest_i():
    sub = np.where(np.eye(8, dtype=bool), 10, -10).astype(np.int32).reshape(64)
    # H(2,1) = H(1,2) = 10 both on antidiagonal 3: the smaller i wins
    assert right(codes("GA"), codes("AG"), sub=sub, gap_open=0, gap_extend=0)[:3] == (10, 1, 2)
    # 20 is reached at (2,2) and again at (4,4): the first one stays
    assert right(codes("AACA"), codes("AAGA"), sub=sub)[:3] == (20, 2, 2)
    assert full_gotoh(codes("GA").tolist(), codes("AG").tolist(), sub, 0, 0) == (10, 1, 2)


def test_one_empty_antidiagonal_is_crossed_through_m():
    X = codes("ACGTTGCAAGCTTACGGATC")
    # ydrop below any gap: every odd antidiagonal is empty, the diagonal continues through M
    best, i, j, cells, flags = right(X, X, ydrop=100)
    assert (best, i, j) == (int(sum(SUB[c * 8 + c] for c in X)), 20, 20)
    assert cells == 21 and flags == 0


def test_band_and_extent_caps_set_their_flags():
    X = codes("ACGT" * 50)
    best, i, j, cells, flags = right(X, X, max_extent=50)
    assert flags == G.EXTENT_CAP and (i, j) == (50, 50)
    # free gaps: the band opens up until the cap ends the side
    sub = np.where(np.eye(8, dtype=bool), 10, -10).astype(np.int32).reshape(64)
    best, i, j, cells, flags = right(X, X, sub=sub, gap_open=0, gap_extend=0, max_band=8)
    assert flags & G.BAND_CAP
    assert i < 200
    best2, _, _, cells2, flags2 = right(X, X, sub=sub, gap_open=0, gap_extend=0, max_band=1024)
    assert flags2 == 0 and best2 == 2000 and cells2 > cells


def test_extend_combines_both_sides_and_selection_rules():
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=300).astype(np.uint8)
    q = t.copy()
    t[150] = SEP  # two records in the target
    hsps = np.array([(20, 20, 40, 0), (200, 200, 30, 0), (22, 22, 36, 0), (0, 0, 0, 0)], dtype=G.SEG_DTYPE)
    raw = G.extend(t, q, SUB, hsps)
    assert raw["hsp_index"].tolist() == [0, 1, 2, 3]
    r0 = raw[0]
    assert (r0["ref_start"], r0["ref_end"]) == (0, 150) and (r0["query_start"], r0["query_end"]) == (0, 150)
    assert r0["score"] == int(sum(SUB[c * 8 + c] for c in t[:150]))
    assert (raw[1]["ref_start"], raw[1]["ref_end"]) == (151, 300)
    assert raw[2].tolist()[:5] == r0.tolist()[:5]  # the same extent from another anchor
    sel = G.select(raw, 3000)
    assert sel["hsp_index"].tolist() == [0, 1]  # duplicate extent removed (lowest index kept), order by query_start
