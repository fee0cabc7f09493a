"""GPU: sa_chain_hsps_ovl and sa_chain_hsps_all_ovl (include/segalign_amd.h) against the model of
tests/hsp_chain_overlap_model.py.  Every test compares f and pred of every HSP and the members, and first asserts with the model that
its input is in the regime it names.  The entries need no sequence: the tests build HSP records directly, on an interface without a
processor."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_gap_model as G
import hsp_chain_model as M
import hsp_chain_overlap_model as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = {"pos": [2, 10, 100, 1000], "q_gap": [5, 50, 60, 60], "t_gap": [7, 7, 700, 800], "both_gap": [20, 30, 300, 3000]}


@pytest.fixture(scope="module")
def E(engine):
    engine.InitializeInterface(1)
    engine.reset_option("chain_tile")
    yield engine
    engine.reset_option("chain_tile")


@contextlib.contextmanager
def tile(E, t):
    if t is None:
        E.reset_option("chain_tile")
    else:
        E.set_option("chain_tile", t)
    try:
        yield
    finally:
        E.reset_option("chain_tile")


def tile_in_use(E):
    """The tile the engine cuts by, from the tile steps of 1 025 HSPs in one group: k (k + 1) / 2 for k = ceil(1025 / T) tiles."""
    st = E.ChainHsps(M.make([(1 + 10 * k, 1 + 10 * k, 2, 5) for k in range(1025)]), max_overlap=1)[1]
    return {3: 1024, 6: 512, 15: 256, 45: 128, 153: 64}[st["tile_steps"]]


def run(E, h, g=None, model=None, **kw):
    """One engine call held against the model, node for node and member for member.  -> the model's (f, pred, members)."""
    f, pred, members = model if model is not None else O.chain(h, g, **kw)
    got_m, got_n, st = E.ChainHsps(h, g, nodes=True, **kw)
    assert got_n.size == h.size
    assert np.array_equal(got_n["f"], f), np.flatnonzero(got_n["f"] != f)[:8]
    assert np.array_equal(got_n["pred"], pred), np.flatnonzero(got_n["pred"] != pred)[:8]
    assert got_m.size == members.size and np.array_equal(got_m, members)
    ng = 0 if h.size == 0 else (1 if g is None else np.unique(g).size)
    assert (st["hsps"], st["groups"], st["members"], st["chains"]) == (h.size, ng, members.size, np.unique(members["group"]).size)
    return f, pred, members


def scatter(rng, n, diagonals=2, step=30, score=(300, 4000)):
    """n HSPs along a few diagonals a few bases apart, in shuffled input order: pieces of 20 .. 60 bases whose starts lie about `step`
    apart, so that neighbours on a line share up to some tens of bases, as HSPs on the two sides of an indel do."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * 7 + int(rng.integers(0, 3))
        q = 1000 + k * step + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(20, 61)), int(rng.integers(score[0], score[1]))))
    h = M.make(rows)
    return h[rng.permutation(n)]


def overlapping_links(h, pred):
    return sum(1 for i, p in enumerate(pred) if p >= 0 and O.overlap(h, int(p), i) > 0)


# ---- sizes around the tile ----
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_sizes_around_a_tile_of_64(E, n):
    h = scatter(np.random.default_rng(n), n)
    with tile(E, 64):
        f, pred, members = run(E, h, max_overlap=32)
        assert tile_in_use(E) == 64
    if n >= 63:
        assert overlapping_links(h, pred) > 5
    if n > 64:
        t = M.tile_of(h, None, 64)
        assert any(p >= 0 and t[p] != t[i] for i, p in enumerate(pred)), "no predecessor in an earlier tile"
    if n >= 129:  # n = 65 has one node in its second tile, whose link need not overlap
        assert any(p >= 0 and t[p] != t[i] and O.overlap(h, int(p), i) > 0 for i, p in enumerate(pred)), "no overlapping link across tiles"
    assert (n == 0) == (members.size == 0)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_sizes_at_the_default_tile(E, n):
    h = scatter(np.random.default_rng(50 + n), n)
    _, pred, _ = run(E, h, max_overlap=64, gap_costs="loose", diag_pen=1)
    assert n < 63 or overlapping_links(h, pred) > 5


# ---- one overlapping link in every place the kernels meet a candidate ----
KINDS = [(5, 5), (5, -10), (-20, 8), (3, 9), (12, 6), (1, 1), (64, 64), (0, 0)]  # (re_j - rs_i, qe_j - qs_i)


def ladder(kinds, S):
    """One group of S HSPs per kind: j first in rank, i last, and S - 2 fillers between them that link with nothing under any
    allowance (three bases each, inside j's target span, running against the diagonal among themselves and far above i in the
    query).  -> (hsps, groups, [(j, i)])."""
    assert 2 <= S <= 130
    rows, grp, pairs = [], [], []
    for k, (a, b) in enumerate(kinds):
        R, Q = 1000 + 200000 * k, 500000
        pairs.append((len(rows), len(rows) + S - 1))
        rows.append((R, Q, 200, 1000000 + k))                                   # j: [R, R + 200) on both axes
        rows += [(R + 1 + m, Q + 400000 - 100 * m, 3, 1) for m in range(S - 2)]  # fillers
        rows.append((R + 200 - a, Q + 200 - b, 150, 9000))                        # i
        grp += [k] * S
    return M.make(rows), np.array(grp, dtype=np.uint32), pairs


@pytest.mark.parametrize("name,T,S", [("the predecessor in an earlier tile", 64, 80), ("inside one sub-tile", 256, 4),
                                      ("between two sub-tiles of a tile", 256, 128)])
@pytest.mark.parametrize("table", [None, "hand"])
def test_an_overlapping_link_in_every_place(E, name, T, S, table):
    t = None if table is None else G.validate(HAND)
    h, g, pairs = ladder(KINDS, S)
    model = O.chain(h, g, gap_costs=t, anti_pen=1, max_overlap=64)
    f, pred, _ = model
    tl, sub = M.tile_of(h, g, T), M.tile_of(h, g, 64)
    for (a, b), (j, i) in zip(KINDS, pairs):
        o = max(0, a, b)
        assert O.overlap(h, j, i) == o and pred[i] == j
        assert f[i] == 9000 + f[j] - O.link_penalty(h, j, i, 0, 1, t) - O.charge(h, j, i) and (o == 0 or O.charge(h, j, i) > 0)
        assert {"the predecessor in an earlier tile": tl[j] < tl[i], "inside one sub-tile": sub[j] == sub[i],
                "between two sub-tiles of a tile": tl[j] == tl[i] and sub[j] < sub[i]}[name]
    assert (pred >= 0).sum() == len(KINDS), "a filler linked"
    with tile(E, T):
        run(E, h, g, model=model, gap_costs=t, anti_pen=1, max_overlap=64)
        assert tile_in_use(E) == T
    assert (M.chain(h, g, anti_pen=1)[1] >= 0).sum() == 1, "only the abutting kind links without the allowance"


# ---- the edges of the relation ----
def test_the_allowance_and_the_half_length_edges(E):
    rows, want = [], []

    def pair(j, i, linked):
        rows.extend([j, i])
        want.append(linked)
    pair((100, 100, 50, 500), (140, 140, 50, 700), True)     # o = 10 = max_overlap
    pair((100, 100, 50, 500), (139, 139, 50, 700), False)    # o = 11
    pair((100, 100, 50, 500), (139, 150, 50, 700), False)    # o = 11 on the target alone
    pair((100, 100, 15, 500), (108, 108, 60, 700), True)     # o = 7, bases_j = 2 o + 1
    pair((100, 100, 14, 500), (107, 107, 60, 700), False)    # o = 7, bases_j = 2 o
    pair((100, 100, 60, 500), (153, 153, 15, 700), True)     # o = 7, bases_i = 2 o + 1
    pair((100, 100, 60, 500), (153, 153, 14, 700), False)    # o = 7, bases_i = 2 o
    pair((100, 100, 60, 500), (150, 190, 60, 700), True)     # o = 10, trimmed query gap 40 = max_gap
    pair((100, 100, 60, 500), (150, 191, 60, 700), False)    # trimmed query gap 41 (31 untrimmed)
    h = M.make(rows)
    g = np.repeat(np.arange(len(want), dtype=np.uint32), 2)
    for k, linked in enumerate(want):
        assert O.precedes(h, g, 2 * k, 2 * k + 1, 10, max_gap=40) == linked
    with tile(E, 64):
        _, pred, _ = run(E, h, g, max_overlap=10, max_gap=40)
    assert [int(p) for p in pred[1::2]] == [2 * k if linked else -1 for k, linked in enumerate(want)]
    # the largest allowance, and one base past it
    big = M.make([(1000, 1000, 9000, 500), (1000 + 9000 - 4096, 1000 + 9000 - 4096, 9000, 700),
                  (50000, 50000, 9000, 500), (50000 + 9000 - 4097, 50000 + 9000 - 4097, 9000, 700)])
    assert O.overlap(big, 0, 1) == 4096 and O.overlap(big, 2, 3) == 4097
    with tile(E, 64):
        _, pred, _ = run(E, big, np.array([0, 0, 1, 1], dtype=np.uint32), max_overlap=4096)
    assert list(pred) == [-1, 0, -1, -1]


# ---- who wins ----
def rivals(score_i, s_over, s_abut, over_first, extra=70):
    """Node i = [R, R + 100) on both axes and two candidates on its diagonal: one that overlaps i by 10 bases and one that abuts it.
    over_first: the overlapping one starts earlier, so it has the lower rank.  Neither links with the other (they share their
    start or more than half of the shorter).  Fillers take the set past one sub-tile.  Input order: overlapping, abutting, i."""
    R = 300000
    over = (R - 45, R - 45, 55, s_over) if over_first else (R - 40, R - 40, 50, s_over)
    abut = (R - 40, R - 40, 40, s_abut) if over_first else (R - 45, R - 45, 45, s_abut)
    rows = [over, abut, (R, R, 100, score_i)] + [(R + 1000 + 10 * m, R - 100 * m - 1000, 3, 1) for m in range(extra)]
    return M.make(rows)


@pytest.mark.parametrize("over_first", [True, False])
def test_the_charge_flips_the_winner_and_makes_ties_for_the_lower_rank(E, over_first):
    # w_i = 65536 * 1000 / 100 = 10 a base, the candidates weigh more: the charge of the 10 shared bases is 100
    h = rivals(1000, 5000, 4950, over_first)
    assert O.charge(h, 0, 2) == 100 and O.charge(h, 1, 2) == 0 and not O.precedes(h, None, 0, 1, 64) and not O.precedes(h, None, 1, 0, 64)
    order = list(M.rank_order(h))
    assert (order.index(0) < order.index(1)) == over_first
    with tile(E, 64):
        f, pred, _ = run(E, h, max_overlap=64)
        assert pred[2] == 1 and f[2] == 1000 + 4950            # 5000 - 100 < 4950
        f, pred, _ = run(E, rivals(-5, 5000, 4950, over_first), max_overlap=64)
        assert pred[2] == 0 and f[2] == -5 + 5000              # i weighs nothing: no charge, the overlapping one wins
        for perm in ([0, 1, 2], [1, 0, 2]):                    # a tie made by the charge, in either input order
            t = rivals(1000, 5000, 4900, over_first)
            head = t[:3][perm]
            t = np.concatenate([head, t[3:]])
            lower = perm.index(0 if over_first else 1)
            f, pred, _ = run(E, t, max_overlap=64)
            assert pred[2] == lower and f[2] == 1000 + 4900
        f, pred, _ = run(E, rivals(1000, 5001, 4900, over_first), max_overlap=64)
        assert pred[2] == 0                                    # one more unit and the overlapping one wins whatever its rank
        f, pred, _ = run(E, rivals(1000, 4999, 4900, over_first), max_overlap=64)
        assert pred[2] == 1


def test_linear_terms_table_and_max_gap_together(E):
    rng = np.random.default_rng(61)
    h = scatter(rng, 230, diagonals=3)
    g = rng.integers(0, 3, 230).astype(np.uint32)
    with tile(E, 64):
        f0, p0, _ = run(E, h, g, max_overlap=48)
        f1, p1, _ = run(E, h, g, max_overlap=48, gap_costs="loose", diag_pen=40, anti_pen=3)
        f2, p2, _ = run(E, h, g, max_overlap=48, gap_costs=HAND, diag_pen=4, anti_pen=3, max_gap=25)
    assert not np.array_equal(p0, p1) and not np.array_equal(p1, p2)
    assert min(overlapping_links(h, p) for p in (p0, p1, p2)) > 10
    assert any(p >= 0 and O.overlap(h, int(p), i) > 0 and sum(O.trimmed_gaps(h, int(p), i)) > 0 for i, p in enumerate(p2))


# ---- magnitudes ----
def test_coordinates_next_to_2_to_the_32_and_the_largest_scores(E):
    top = 2 ** 32 - 1
    rng = np.random.default_rng(31)
    rows = [(top - 3000 + 30 * k + int(rng.integers(0, 3)), top - 2990 + 30 * k, 40, 2 ** 31 - 1) for k in range(90)]
    rows[-1] = (top - 20, top - 10, 40, 2 ** 31 - 1)  # its end lies past 2^32
    h = M.make(rows)[rng.permutation(90)]
    assert O.weight(h, 0) == ((2 ** 31 - 1) << 16) // 40 > 2 ** 41
    with tile(E, 64):
        f, pred, members = run(E, h, max_overlap=4096, gap_costs="medium", diag_pen=3, anti_pen=2)
    assert members.size > 60 and overlapping_links(h, pred) > 50 and int(f.max()) > 2 ** 36
    wide = M.make([(5000, 5000, 2 ** 31, 2 ** 31 - 1), (5000 + 2 ** 31 - 4096, 5000 + 2 ** 31 - 4096, 2 ** 31, 2 ** 31 - 1)])
    with tile(E, 64):
        f, pred, _ = run(E, wide, max_overlap=4096)
    assert pred[1] == 0 and f[1] == 2 * (2 ** 31 - 1) - 4095  # w = floor(65536 (2^31 - 1) / 2^31) = 65535: (4096 * 65535) >> 16


# ---- the old entries ----
def test_no_allowance_is_the_old_entry(E):
    rng = np.random.default_rng(67)
    h = scatter(rng, 700)
    g = rng.integers(0, 4, 700).astype(np.uint32)
    for costs in (None, "loose"):
        old_m, old_n, old_st = E.ChainHsps(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs=costs)
        new_m, new_n, _ = E.ChainHsps(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs=costs, max_overlap=0)
        assert np.array_equal(old_m, new_m) and np.array_equal(old_n, new_n)
        p = E.ChainParams(2, 1, 0, 0, 0)
        t = C.byref(E.chain_gap_costs(costs)) if costs else None
        for ov in (None, C.byref(E.ChainOverlap(0, 0))):  # the new symbol with ov == NULL and with max_overlap == 0
            mem, nod, st = C.c_void_p(), C.c_void_p(), E.ChainStats()
            m = E.lib().sa_chain_hsps_ovl(h.ctypes.data, h.size, g.ctypes.data, C.byref(p), t, ov, C.byref(mem), C.byref(nod), C.byref(st))
            got_m = np.frombuffer((C.c_char * (m * 16)).from_address(mem.value), dtype=E.CHAIN_MEMBER_DTYPE).copy()
            got_n = np.frombuffer((C.c_char * (h.size * 16)).from_address(nod.value), dtype=E.CHAIN_NODE_DTYPE).copy()
            E.lib().sa_free_chain(mem, nod)
            assert np.array_equal(got_m, old_m) and np.array_equal(got_n, old_n) and st.pair_evals == old_st["pair_evals"]
        f, pred, members = G.chain(h, g, diag_pen=2, anti_pen=1, gap_costs=costs)
        assert np.array_equal(old_n["f"], f) and np.array_equal(old_m, members)
        assert not np.array_equal(E.ChainHsps(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs=costs, max_overlap=32)[1]["f"], f)
        old_all = E.ChainHspsAll(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs=costs, min_score=3000)
        new_all = E.ChainHspsAll(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs=costs, min_score=3000, max_overlap=0)
        assert all(np.array_equal(a, b) for a, b in zip(old_all[:4], new_all[:4]))


# ---- random sets, all chains, tile independence, threads ----
PARAMS = [dict(max_overlap=64), dict(max_overlap=24, gap_costs="medium", diag_pen=2, anti_pen=1),
          dict(max_overlap=4096, gap_costs=HAND, diag_pen=1, max_gap=40)]
_sets = {}


def random_case(seed, k):
    if (seed, k) not in _sets:
        rng = np.random.default_rng(3000 + seed)
        n = int(rng.integers(300, 601))
        h = scatter(rng, n, diagonals=int(rng.integers(2, 5)), step=int(rng.integers(20, 45)))
        sizes = rng.integers(1, 40, 5)
        g = rng.choice(np.array([0, 5, 6, 70, 4_000_000_000], dtype=np.uint32), size=n, p=sizes / sizes.sum())
        g[np.flatnonzero(g == 5)[:3]] = 12  # a group too small to reach min_score
        kw = dict(PARAMS[k])
        f, _, _ = O.chain(h, g, **kw)
        tops = sorted(int(f[g == x].max()) for x in np.unique(g))
        kw["min_score"] = (tops[0] + tops[1]) // 2 + 1
        _sets[(seed, k)] = (h, g, kw, O.chain(h, g, **kw))
    return _sets[(seed, k)]


def without_overlap(kw):
    return {x: v for x, v in kw.items() if x != "max_overlap"}


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(3))
def test_random_sets(E, seed, k):
    h, g, kw, model = random_case(seed, k)
    _, pred, members = run(E, h, g, model=model, **kw)
    assert 1 <= np.unique(members["group"]).size < np.unique(g).size, "min_score must cut a group and keep one"
    assert overlapping_links(h, pred) > h.size // 20
    plain = G.chain(h, g, **without_overlap(kw))
    assert members.size > plain[2][np.isin(plain[2]["group"], members["group"])].size, "the allowance must lengthen the chains"


@pytest.mark.parametrize("seed,k", [(0, 1), (1, 0), (2, 2)])
def test_all_chains_under_the_allowance(E, seed, k):
    h, g, kw, model = random_case(seed, k)
    kw = dict(kw, min_score=2000)  # keeps secondary chains, drops the small ones
    f, pred, chains, members, chain_of = O.chain_all(h, g, **kw)
    assert np.array_equal(f, model[0]) and chains.size > np.unique(g).size and (chains["joined"] >= 0).any()
    assert (chain_of == 0xFFFFFFFF).any() and (chain_of != 0xFFFFFFFF).any()
    got_c, got_m, got_n, got_o, st = E.ChainHspsAll(h, g, nodes=True, **kw)
    assert np.array_equal(got_n["f"], f) and np.array_equal(got_n["pred"], pred)
    assert got_c.size == chains.size and np.array_equal(got_c, chains)
    assert got_m.size == members.size and np.array_equal(got_m, members)
    assert np.array_equal(got_o, chain_of)
    assert st["joined"] == int((chains["joined"] >= 0).sum()) and st["chains"] == chains.size
    plain = E.ChainHspsAll(h, g, **without_overlap(kw))
    assert not (plain[0].size == chains.size and np.array_equal(plain[0], chains))


@pytest.mark.parametrize("seed", range(3))
def test_results_do_not_depend_on_the_tile(E, seed):
    h, g, kw, model = random_case(seed, (seed + 1) % 3)
    got = []
    for t in (64, 256, None):
        with tile(E, t):
            got.append(E.ChainHsps(h, g, nodes=True, **kw))
    steps = [st["tile_steps"] for _, _, st in got]
    assert steps[0] > steps[1]  # the tile did change
    for m, nd, _ in got:
        assert np.array_equal(m, model[2]) and np.array_equal(nd["f"], model[0]) and np.array_equal(nd["pred"], model[1])


def test_the_largest_tile(E):
    h, g, kw, model = random_case(0, 2)  # 48 KB of tile image and the cost image in LDS
    with tile(E, 1024):
        run(E, h, g, model=model, **kw)
        assert tile_in_use(E) == 1024


def test_eight_threads_get_the_serial_results(E):
    cases = [random_case(s, k) for s in range(3) for k in range(3)][:8]
    out, errors = [None] * 8, []

    def work(i):
        try:
            h, g, kw, _ = cases[i]
            out[i] = E.ChainHsps(h, g, nodes=True, **kw)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(8):
        model = cases[i][3]
        assert np.array_equal(out[i][0], model[2]) and np.array_equal(out[i][1]["f"], model[0]) and np.array_equal(out[i][1]["pred"], model[1])


# ---- validation ----
CHILD = """
import ctypes as C, sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
h = np.zeros(%d, dtype=E.SEG_DTYPE)
ov, p = E.ChainOverlap(%d, %d), E.ChainParams(0, 0, 0, 0, 0)
mem, nod, st, ch, nc, cof = C.c_void_p(), C.c_void_p(), E.ChainStats(), C.c_void_p(), C.c_size_t(0), C.c_void_p()
if %d:
    E.lib().sa_chain_hsps_all_ovl(h.ctypes.data, h.size, None, C.byref(p), None, C.byref(ov), C.byref(ch), C.byref(nc), C.byref(mem), None,
                                  C.byref(cof), C.byref(E.ChainAllStats()))
else:
    E.lib().sa_chain_hsps_ovl(h.ctypes.data, h.size, None, C.byref(p), None, C.byref(ov), C.byref(mem), None, C.byref(st))
print("returned")
"""


@pytest.mark.parametrize("what,max_overlap,reserved,hsps,all_chains", [("max_overlap", 4097, 0, 4, 0), ("max_overlap", 2 ** 32 - 1, 0, 0, 1),
                                                                       ("reserved", 64, 1, 4, 0), ("reserved", 0, 7, 4, 1)])
def test_bad_values_fail_with_a_message(what, max_overlap, reserved, hsps, all_chains):
    with pytest.raises(ValueError, match=what):
        O.validate(max_overlap, reserved)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, hsps, max_overlap, reserved, all_chains)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"ChainHsps" in r.stderr and what.encode() in r.stderr
