"""GPU: sa_chain_hsps_costs and sa_chain_hsps_all_costs (include/segalign_amd.h) against the model of
tests/hsp_chain_gap_model.py.  Every test compares f and pred of every HSP and the members, and first asserts with the model that its
input is in the regime it names.  The entries need no sequence: the tests build HSP records directly, on an interface without a
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 16 break points: every outcome of the four-step search, with a flat segment (q_gap 3 .. 4), equal neighbours and steep starts
FULL = {"pos": [2, 3, 4, 6, 9, 14, 20, 33, 50, 90, 150, 400, 1000, 5000, 20000, 50000],
        "q_gap": [5, 9, 9, 14, 20, 31, 40, 55, 70, 95, 130, 260, 500, 1500, 4000, 7000],
        "t_gap": [7, 8, 12, 13, 25, 30, 44, 50, 77, 90, 140, 250, 530, 1400, 4100, 7100],
        "both_gap": [11, 15, 18, 24, 30, 41, 52, 66, 81, 99, 160, 300, 600, 1700, 4400, 7700]}
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
    st = E.ChainHsps(M.make([(1 + 10 * k, 1 + 10 * k, 2, 5) for k in range(1025)]), gap_costs="loose")[1]
    return {3: 1024, 6: 512, 15: 256, 45: 128, 153: 64}[st["tile_steps"]]


def run(E, h, g=None, model=None, **kw):
    """One engine call held against the model, node for node and member for member.  -> the model's (f, pred, members)."""
    f, pred, members = model if model is not None else G.chain(h, g, **kw)
    got_m, got_n, st = E.ChainHsps(h, g, nodes=True, **kw)
    assert got_n.size == h.size
    assert np.array_equal(got_n["f"], f), np.flatnonzero(got_n["f"] != f)[:8]
    assert np.array_equal(got_n["pred"], pred), np.flatnonzero(got_n["pred"] != pred)[:8]
    assert got_m.size == members.size and np.array_equal(got_m, members)
    ng = 0 if h.size == 0 else (1 if g is None else np.unique(g).size)
    assert (st["hsps"], st["groups"], st["members"], st["chains"]) == (h.size, ng, members.size, np.unique(members["group"]).size)
    return f, pred, members


def scatter(rng, n, diagonals=3, step=60, jitter=4, score=(300, 4000)):
    """n HSPs along a few diagonals, in shuffled input order; the scores are of the size of the presets' costs, so that some links
    pay and some do not."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * 5000 + int(rng.integers(-jitter, jitter + 1)) * int(rng.integers(0, 2))
        q = 1000 + k * step // diagonals + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(5, 50)), int(rng.integers(score[0], score[1]))))
    h = M.make(rows)
    return h[rng.permutation(n)]


def gaps(h, j, i):
    sp = int(h["len"][j]) + 1
    return (int(h["ref_start"][i]) - int(h["ref_start"][j]) - sp, int(h["query_start"][i]) - int(h["query_start"][j]) - sp)


# ---- sizes around the tile ----
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_sizes_around_a_tile_of_64(E, n):
    h = scatter(np.random.default_rng(n), n)
    with tile(E, 64):
        f, pred, members = run(E, h, gap_costs="medium")
        assert tile_in_use(E) == 64
    if n >= 63:
        assert (pred >= 0).any() and any(p >= 0 and gaps(h, p, i) != (0, 0) for i, p in enumerate(pred))
    if n > 64:
        t = M.tile_of(h, None, 64)
        assert any(p >= 0 and t[p] != t[i] for i, p in enumerate(pred)), "no predecessor in an earlier tile"
    assert (n == 0) == (members.size == 0)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_sizes_at_the_default_tile(E, n):
    h = scatter(np.random.default_rng(50 + n), n)
    run(E, h, gap_costs="loose", diag_pen=1)


def test_a_size_past_the_default_tile(E):
    with tile(E, None):
        T = tile_in_use(E)
    assert T in (64, 128, 256, 512, 1024)
    h = scatter(np.random.default_rng(5), T + 76)
    f, pred, _ = run(E, h, gap_costs="loose")
    t = M.tile_of(h, None, T)
    assert any(p >= 0 and t[p] != t[i] for i, p in enumerate(pred)) and any(p >= 0 and t[p] == t[i] for i, p in enumerate(pred))


# ---- a link in every case and every segment, in every place the kernels meet a candidate ----
def segment_of(t, x):
    """-1 below pos[0], k inside [pos[k], pos[k + 1]), n - 1 on the extrapolated tail."""
    return max([k for k, p in enumerate(t["pos"]) if p <= x], default=-1)


def link_kinds(t):
    """(dt, dq) of one link per case and segment: below pos[0], at every break point, inside every segment (one below the next break
    point where there is room), on the tail, and the link without a gap."""
    pos, xs = t["pos"], []
    if pos[0] > 1:
        xs.append(pos[0] - 1)
    for k, p in enumerate(pos):
        xs.append(p)
        nxt = pos[k + 1] if k + 1 < len(pos) else p + 12345
        if nxt - 1 > p:
            xs.append(nxt - 1)
    kinds = [(0, 0)]
    for x in xs:
        kinds += [(0, x), (x, 0)]
        if x >= 2:
            kinds.append((x // 2, x - x // 2))
    return kinds


def ladder(kinds, S):
    """One group of S HSPs per kind: j first in rank, i last, and S - 2 fillers between them that chain with nothing (they lie inside
    j's target span, run against the diagonal among themselves and above i in the query).  -> (hsps, groups, [(j, i)])."""
    assert 2 <= S <= 130
    rows, grp, pairs = [], [], []
    for k, (dt, dq) in enumerate(kinds):
        R, Q = 1000 + 200000 * k, 500000
        pairs.append((len(rows), len(rows) + S - 1))
        rows.append((R, Q, 200, 1000000 + k))                                 # j: target R .. R + 199
        rows += [(R + 1 + m, Q + 400000 - 100 * m, 3, 1) for m in range(S - 2)]  # fillers
        rows.append((R + 200 + dt, Q + 200 + dq, 10, 7))                        # i
        grp += [k] * S
    return M.make(rows), np.array(grp, dtype=np.uint32), pairs


@pytest.mark.parametrize("name,T,S", [("the predecessor in an earlier tile", 64, 80), ("inside one sub-tile", 256, 4),
                                      ("between two sub-tiles of a tile", 256, 128)])
@pytest.mark.parametrize("table", ["full", "medium"])
def test_a_link_in_every_case_and_segment(E, name, T, S, table):
    t = G.validate(FULL if table == "full" else "medium")
    kinds = link_kinds(t)
    h, g, pairs = ladder(kinds, S)
    model = G.chain(h, g, gap_costs=t)
    f, pred, _ = model
    tl, sub = M.tile_of(h, g, T), M.tile_of(h, g, 64)
    seen = set()
    for (dt, dq), (j, i) in zip(kinds, pairs):
        assert gaps(h, j, i) == (dt, dq) and pred[i] == j and f[i] == 7 + f[j] - G.gapcost(t, dt, dq)
        assert {"the predecessor in an earlier tile": tl[j] < tl[i], "inside one sub-tile": sub[j] == sub[i],
                "between two sub-tiles of a tile": tl[j] == tl[i] and sub[j] < sub[i]}[name]
        seen.add((0 if dt == 0 and dq == 0 else 1 if dt == 0 else 2 if dq == 0 else 3, segment_of(t, dt + dq)))
    n = len(t["pos"])
    lowest = -1 if t["pos"][0] > 1 else 0
    both = {k for k in range(n) if k + 1 == n or t["pos"][k + 1] > 2}  # a gap in both has x >= 2
    assert seen >= {(c, k) for c in (1, 2) for k in range(lowest, n)} | {(3, k) for k in both} | {(0, -1)}
    assert (pred >= 0).sum() == len(kinds), "a filler chained"
    with tile(E, T):
        run(E, h, g, model=model, gap_costs=t)
        assert tile_in_use(E) == T


# ---- who wins ----
def candidates(R, Q, cands, score_i=7, extra=60):
    """Node i at (R, Q) and candidates [(dq, score)] that all end at target R (dt = 0, so no two of them chain), padded with fillers to
    more than one sub-tile.  Input order: the candidates, i, the fillers.  A later candidate has the lower rank (it starts earlier)."""
    rows = [(R - 20 - 5 * k, Q - dq - 20 - 5 * k, 20 + 5 * k, s) for k, (dq, s) in enumerate(cands)]
    rows.append((R, Q, 10, score_i))
    rows += [(R + 1000 + 10 * m, Q - 100 * m - 100, 3, 1) for m in range(extra)]
    return M.make(rows)


def test_the_predecessor_differs_under_linear_loose_and_medium(E):
    # costs of a query gap of 32111 / 12111 / 1: loose 7600 / 3600 / 325, medium 57900 / 22900 / 350
    h = candidates(200000, 200000, [(32111, 100000), (12111, 97000), (1, 80000)])
    with tile(E, 64):
        assert run(E, h)[1][3] == 0
        assert run(E, h, gap_costs="loose")[1][3] == 1
        f, pred, _ = run(E, h, gap_costs="medium")
    assert pred[3] == 2 and f[3] == 7 + 80000 - 350
    assert [gaps(h, j, 3) for j in range(3)] == [(0, 32111), (0, 12111), (0, 1)]


def test_two_candidates_made_equal_by_the_gap_cost_go_to_the_lower_rank(E):
    t = G.validate("medium")
    a, b = 1000 + G.gapcost(t, 0, 5000), 1000 + G.gapcost(t, 0, 40)
    assert a != b
    for cands in ([(5000, a), (40, b)], [(40, b), (5000, a)]):
        h = candidates(300000, 300000, cands)
        order = list(M.rank_order(h))
        with tile(E, 64):
            f, pred, _ = run(E, h, gap_costs=t)
        assert f[2] == 1007 and pred[2] == 1 and order.index(1) < order.index(0)
        assert f[0] - G.gapcost(t, *gaps(h, 0, 2)) == f[1] - G.gapcost(t, *gaps(h, 1, 2)) == 1000
    # one more unit on the higher rank and it wins
    h = candidates(300000, 300000, [(5000, a + 1), (40, b)])
    with tile(E, 64):
        assert run(E, h, gap_costs=t)[1][2] == 0


def test_a_candidate_of_exactly_zero_gives_no_predecessor(E):
    t = G.validate("loose")
    c = G.gapcost(t, 0, 111)
    assert c == 600
    with tile(E, 64):
        f, pred, _ = run(E, candidates(300000, 300000, [(111, c)]), gap_costs=t)
        assert (int(f[1]), int(pred[1])) == (7, -1)
        f, pred, _ = run(E, candidates(300000, 300000, [(111, c + 1)]), gap_costs=t)
        assert (int(f[1]), int(pred[1])) == (8, 0)
        f, pred, _ = run(E, candidates(300000, 300000, [(111, c + 3)]), gap_costs=t, anti_pen=2)  # 3 - 2 * 111 < 0
        assert (int(f[1]), int(pred[1])) == (7, -1)


def test_linear_terms_and_table_together(E):
    rng = np.random.default_rng(61)
    h = scatter(rng, 230, jitter=8)
    g = rng.integers(0, 3, 230).astype(np.uint32)
    with tile(E, 64):
        f0, p0, _ = run(E, h, g, gap_costs="loose")
        f1, p1, _ = run(E, h, g, gap_costs="loose", diag_pen=40, anti_pen=3)
        f2, p2, _ = run(E, h, g, diag_pen=40, anti_pen=3)
        run(E, h, g, gap_costs="loose", diag_pen=40, anti_pen=3, max_gap=150)
    assert not np.array_equal(p0, p1) and not np.array_equal(p1, p2) and (p1 >= 0).any()


# ---- magnitudes ----
def test_gaps_next_to_2_to_the_32_leave_int64_headroom(E):
    top = 2 ** 32
    rows = [(10 * k, 10 * k, 10, 2 ** 31 - 1) for k in range(200)]  # an abutting ladder: f reaches 200 (2^31 - 1) > 2^38
    rows.append((top - 200, top - 150, 10, 5))                      # i: both gaps next to 2^32, x = dt + dq > 2^32
    h = M.make(rows)
    dt, dq = gaps(h, 199, 200)
    assert dt > top - 3000 and dq > top - 3000 and dt + dq - 2 ** 31 >= top
    # costs of 2^35 at 2^31: about 2^37 at x; the product (x - pos) * slope passes 2^52 and needs the high word of x - pos
    t = G.validate({"pos": [1, 2 ** 31], "q_gap": [0, 2 ** 35], "t_gap": [0, 2 ** 35], "both_gap": [0, 2 ** 35]})
    s = G.slopes(t["pos"], t["both_gap"])[1]
    assert (dt + dq - 2 ** 31) * s > 2 ** 52 and 2 ** 36 < G.gapcost(t, dt, dq) < 2 ** 38
    with tile(E, 64):
        f, pred, _ = run(E, h, gap_costs=t)
        assert pred[200] == 199 and f[200] == 5 + f[199] - G.gapcost(t, dt, dq)
        # the steepest slope, 2^27 - 2^16, from a cost at its limit of 2^40: a cost next to 2^44 that no chain can pay
        t = G.validate({"pos": [1, 2], "q_gap": [2 ** 40 - 2047, 2 ** 40], "t_gap": [2 ** 40 - 2047, 2 ** 40], "both_gap": [2 ** 40 - 2047, 2 ** 40]})
        assert G.slopes(t["pos"], t["q_gap"])[1] == 2 ** 27 - 2 ** 16 and G.gapcost(t, dt, dq) > 2 ** 43
        f, pred, _ = run(E, h, gap_costs=t, diag_pen=1 << 20, anti_pen=1 << 20)
        assert pred[200] == -1 and f[200] == 5 and pred[199] == 198  # abutting links cost nothing
        rows[-1] = (top - 200, 2000, 10, 5)                         # a target gap alone, next to 2^32: the t_gap case at its far end
        h = M.make(rows)
        f, pred, _ = run(E, h, gap_costs=t)
        assert gaps(h, 199, 200) == (top - 2200, 0) and pred[200] == -1


def test_coordinates_next_to_2_to_the_32(E):
    top = 2 ** 32 - 1
    rng = np.random.default_rng(31)
    rows = [(top - 1000 + 12 * k + int(rng.integers(0, 3)), top - 990 + 12 * k, 10, 900) for k in range(80)]
    rows[-1] = (top - 20, top - 10, 40, 900)  # its end lies past 2^32
    h = M.make(rows)[rng.permutation(80)]
    with tile(E, 64):
        _, _, members = run(E, h, gap_costs="medium", diag_pen=3, anti_pen=2)
    assert members.size > 20


# ---- the old entries ----
def test_no_table_is_the_old_entry(E):
    rng = np.random.default_rng(67)
    h = scatter(rng, 700)
    g = rng.integers(0, 4, 700).astype(np.uint32)
    old_m, old_n, old_st = E.ChainHsps(h, g, nodes=True, diag_pen=2, anti_pen=1)
    new_m, new_n, _ = E.ChainHsps(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs=None)
    assert np.array_equal(old_m, new_m) and np.array_equal(old_n, new_n)
    # the new symbol with g == NULL
    p = E.ChainParams(2, 1, 0, 0, 0)
    mem, nod, st = C.c_void_p(), C.c_void_p(), E.ChainStats()
    m = E.lib().sa_chain_hsps_costs(h.ctypes.data, h.size, g.ctypes.data, C.byref(p), None, C.byref(mem), C.byref(nod), C.byref(st))
    got_m = np.frombuffer((C.c_char * (m * 16)).from_address(mem.value), dtype=E.CHAIN_MEMBER_DTYPE).copy()
    got_n = np.frombuffer((C.c_char * (h.size * 16)).from_address(nod.value), dtype=E.CHAIN_NODE_DTYPE).copy()
    E.lib().sa_free_chain(mem, nod)
    assert np.array_equal(got_m, old_m) and np.array_equal(got_n, old_n) and st.pair_evals == old_st["pair_evals"]
    f, pred, members = M.chain(h, g, diag_pen=2, anti_pen=1)
    assert np.array_equal(old_n["f"], f) and np.array_equal(old_m, members)
    assert not np.array_equal(E.ChainHsps(h, g, nodes=True, diag_pen=2, anti_pen=1, gap_costs="loose")[1]["f"], f)


def test_the_presets_of_the_library_are_the_models(E):
    for name in ("loose", "medium"):
        t, want = E.chain_gap_costs(name), G.table(name)
        assert t.n == 11
        for key in ("pos", "q_gap", "t_gap", "both_gap"):
            assert list(getattr(t, key))[:11] == want[key] and not any(list(getattr(t, key))[11:])
    with pytest.raises(ValueError):
        E.chain_gap_costs("tight")
    assert E.lib().sa_chain_gap_preset(b"tight", C.byref(E.ChainGapCosts())) == -1


# ---- random sets, all chains, tile independence, threads ----
PARAMS = [dict(gap_costs="loose"), dict(gap_costs="medium", diag_pen=2, anti_pen=1), dict(gap_costs=HAND, diag_pen=1, max_gap=400)]
_sets = {}


def random_case(seed, k):
    if (seed, k) not in _sets:
        rng = np.random.default_rng(2000 + seed)
        n = int(rng.integers(300, 2001))
        h = scatter(rng, n, diagonals=int(rng.integers(2, 6)), step=40, jitter=6)
        sizes = rng.integers(1, 40, 5)
        g = rng.choice(np.array([0, 5, 6, 70, 4_000_000_000], dtype=np.uint32), size=n, p=sizes / sizes.sum())
        g[np.flatnonzero(g == 5)[:3]] = 12  # a group too small to reach min_score
        kw = dict(PARAMS[k])
        f, _, _ = G.chain(h, g, **kw)
        tops = sorted(int(f[g == x].max()) for x in np.unique(g))
        kw["min_score"] = (tops[0] + tops[1]) // 2 + 1
        _sets[(seed, k)] = (h, g, kw, G.chain(h, g, **kw))
    return _sets[(seed, k)]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(3))
def test_random_sets(E, seed, k):
    h, g, kw, model = random_case(seed, k)
    _, pred, members = run(E, h, g, model=model, **kw)
    assert 1 <= np.unique(members["group"]).size < np.unique(g).size, "min_score must cut a group and keep one"
    assert (pred >= 0).sum() > h.size // 10
    assert not np.array_equal(pred, M.chain(h, g, **{x: v for x, v in kw.items() if x != "gap_costs"})[1]), "the table changes nothing"


@pytest.mark.parametrize("seed,k", [(0, 1), (1, 2), (2, 0)])
def test_all_chains_under_costs(E, seed, k):
    h, g, kw, model = random_case(seed, k)
    kw = dict(kw, min_score=2000)  # keeps secondary chains, drops the small ones
    f, pred, chains, members, chain_of = G.chain_all(h, g, **kw)
    assert np.array_equal(f, model[0]) and chains.size > np.unique(g).size and (chains["joined"] >= 0).any()
    assert (chain_of == 0xFFFFFFFF).any() and (chain_of != 0xFFFFFFFF).any()
    got_c, got_m, got_n, got_o, st = E.ChainHspsAll(h, g, nodes=True, **kw)
    assert np.array_equal(got_n["f"], f) and np.array_equal(got_n["pred"], pred)
    assert got_c.size == chains.size and np.array_equal(got_c, chains)
    assert got_m.size == members.size and np.array_equal(got_m, members)
    assert np.array_equal(got_o, chain_of)
    assert st["joined"] == int((chains["joined"] >= 0).sum()) and st["chains"] == chains.size
    lin = E.ChainHspsAll(h, g, **{x: v for x, v in kw.items() if x != "gap_costs"})
    assert not (lin[0].size == chains.size and np.array_equal(lin[0], chains))


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


# ---- table validation ----
CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
h = np.zeros(%d, dtype=E.SEG_DTYPE)
t = E.chain_gap_costs(%r)
t.n = %d
(E.ChainHspsAll if %d else E.ChainHsps)(h, None, gap_costs=t)
print("returned")
"""


def changed(**kw):
    t = {k: list(v) for k, v in HAND.items()}
    t.update(kw)
    return t


@pytest.mark.parametrize("what,t,n,hsps,all_chains", [
    ("n", HAND, 0, 4, 0), ("n", HAND, 17, 4, 1), ("pos[0]", changed(pos=[0, 10, 100, 1000]), 4, 4, 0),
    ("pos[2]", changed(pos=[2, 10, 10, 1000]), 4, 0, 0), ("pos[2]", changed(pos=[2, 100, 10, 1000]), 4, 4, 1),
    ("q_gap[0]", changed(q_gap=[-1, 50, 60, 60]), 4, 4, 0), ("t_gap[3]", changed(t_gap=[7, 7, 700, 2 ** 40 + 1]), 4, 4, 0),
    ("both_gap[2]", changed(both_gap=[20, 30, 29, 3000]), 4, 4, 1),
    ("slope of q_gap[0]", changed(q_gap=[5, 5 + 8 * 2048, 5 + 8 * 2048, 5 + 8 * 2048]), 4, 4, 0),
])
def test_bad_tables_fail_with_a_message(what, t, n, hsps, all_chains):
    with pytest.raises(ValueError):
        G.validate({k: v[:n] for k, v in t.items()} if n <= 4 else {k: list(range(1, n + 1)) for k in t})
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, hsps, t, n, all_chains)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"ChainHsps" in r.stderr and b"gap costs" in r.stderr and what.encode() in r.stderr


def test_tables_at_the_limits_are_accepted(E):
    h = scatter(np.random.default_rng(41), 100)
    with tile(E, 1024):
        run(E, h, gap_costs={"pos": [1], "q_gap": [0], "t_gap": [2 ** 40], "both_gap": [2 ** 40]})
    with tile(E, 128):
        run(E, h, gap_costs=changed(q_gap=[5, 5 + 8 * 2048 - 1, 5 + 8 * 2048 - 1, 5 + 8 * 2048 - 1]))
        run(E, h, gap_costs={k: list(range(1, 17)) for k in ("pos", "q_gap", "t_gap", "both_gap")})
        run(E, h, gap_costs={"pos": [2 ** 32 - 2, 2 ** 32 - 1], "q_gap": [3, 4], "t_gap": [3, 3], "both_gap": [0, 2 ** 10]})
