"""GPU: sa_chain_hsps (include/segalign_amd.h) against the model of tests/hsp_chain_model.py.  Every test compares f and
pred of every HSP and the members, and first asserts with the model that its input is in the regime it names.  The entry needs no
sequence: the tests build HSP records directly, on an interface without a processor."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    st = E.ChainHsps(M.make([(1 + 10 * k, 1 + 10 * k, 2, 5) for k in range(1025)]))[1]
    return {3: 1024, 6: 512, 15: 256, 45: 128, 153: 64}[st["tile_steps"]]


def default_tile(E):
    with tile(E, None):
        return tile_in_use(E)


def run(E, h, g=None, model=None, **kw):
    """One engine call held against the model, node for node and member for member.  -> the model's (f, pred, members)."""
    f, pred, members = model if model is not None else M.chain(h, g, **kw)
    got_m, got_n, st = E.ChainHsps(h, g, nodes=True, **kw)
    assert got_n.size == h.size
    assert np.array_equal(got_n["f"], f), np.flatnonzero(got_n["f"] != f)[:8]
    assert np.array_equal(got_n["pred"], pred), np.flatnonzero(got_n["pred"] != pred)[:8]
    assert got_m.size == members.size and np.array_equal(got_m, members)
    ng = 0 if h.size == 0 else (1 if g is None else np.unique(g).size)
    assert (st["hsps"], st["groups"], st["members"], st["chains"]) == (h.size, ng, members.size, np.unique(members["group"]).size)
    only_m, _ = E.ChainHsps(h, g, **kw)  # without the nodes argument
    assert np.array_equal(only_m, members)
    return f, pred, members


def scatter(rng, n, diagonals=3, step=60, jitter=4, score=(20, 300)):
    """n HSPs along a few diagonals, in shuffled input order: most have predecessors."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * 5000 + int(rng.integers(-jitter, jitter + 1))
        q = 1000 + k * step // diagonals + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(5, 50)), int(rng.integers(score[0], score[1]))))
    h = M.make(rows)
    return h[rng.permutation(n)]


# ---- sizes around the tile ----
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_sizes_around_a_tile_of_64(E, n):
    h = scatter(np.random.default_rng(n), n)
    with tile(E, 64):
        f, pred, members = run(E, h, diag_pen=1)
        assert tile_in_use(E) == 64
    if n >= 2:
        assert (pred >= 0).any()
    if n > 64:
        t = M.tile_of(h, None, 64)
        assert any(p >= 0 and t[p] != t[i] for i, p in enumerate(pred)), "no predecessor in an earlier tile"
    assert (n == 0) == (members.size == 0)


def test_a_size_past_the_default_tile(E):
    T = default_tile(E)
    assert T in (64, 128, 256, 512, 1024)
    h = scatter(np.random.default_rng(5), T + 76)
    f, pred, _ = run(E, h, anti_pen=1)
    t = M.tile_of(h, None, T)
    assert any(p >= 0 and t[p] != t[i] for i, p in enumerate(pred)) and any(p >= 0 and t[p] == t[i] for i, p in enumerate(pred))


# ---- a noisy collinear ladder ----
def test_a_noisy_ladder_chains_through_three_tiles(E):
    rng = np.random.default_rng(17)
    rows = [(5000 + 100 * k + int(rng.integers(-3, 4)), 100 * k, 40, 100) for k in range(120)]           # the ladder
    rows += [(int(rng.integers(0, 17000)), int(rng.integers(0, 12000)), 30, int(rng.integers(1, 60))) for _ in range(100)]  # noise
    h = M.make(rows)[rng.permutation(220)]
    with tile(E, 64):
        _, _, members = run(E, h, diag_pen=2, anti_pen=0)
    assert np.unique(M.tile_of(h, None, 64)[members["hsp_index"]]).size >= 3
    assert members.size >= 100


# ---- two interleaved diagonals ----
def test_the_winning_diagonal_flips_with_diag_pen(E):
    # A_k and B_k overlap in the query, so a chain holds at most one of them per k: without penalty B (130 each) wins; B's diagonal
    # jitters by 3, A's does not, and at diag_pen = 20 B pays 9 * 60 while A (100 each) pays nothing
    A = [(1000 * k, 1000 * k + 480, 50, 100) for k in range(10)]
    B = [(1000 * k + 500, 1000 * k + 500 + (3 if k & 1 else 0), 50, 130) for k in range(10)]
    h = M.make(A + B)
    with tile(E, 64):
        _, _, m0 = run(E, h, diag_pen=0)
        _, _, m1 = run(E, h, diag_pen=20)
    assert sorted(m0["hsp_index"]) == list(range(10, 20)) and int(m0["f"][-1]) == 1300
    assert sorted(m1["hsp_index"]) == list(range(0, 10)) and int(m1["f"][-1]) == 1000


# ---- ties ----
def placed(n, specials):
    """n HSPs whose rank is their index.  Fillers (score 1) run against the diagonal, so no filler precedes another; a special
    {rank: (query_start, score)} lies above every filler in the query: fillers may precede it, it precedes no filler."""
    rows = []
    for k in range(n):
        if k in specials:
            q, s = specials[k]
            rows.append((1000 + 100 * k, 2_000_000 + q, 10, s))
        else:
            rows.append((1000 + 100 * k, 1_000_000 - 100 * k, 10, 1))
    return M.make(rows)


@pytest.mark.parametrize("name,T,r1,r2,r3", [
    ("two earlier tiles", 64, 10, 70, 150),
    ("an earlier tile and the node's own tile", 64, 10, 130, 150),
    ("one 64-node sub-tile", 256, 260, 270, 300),
    ("two sub-tiles of one tile", 256, 260, 330, 400),
])
def test_a_predecessor_tie_goes_to_the_lower_rank(E, name, T, r1, r2, r3):
    n = r3 + 20
    h = placed(n, {r1: (300, 50), r2: (200, 50), r3: (1000, 5)})  # r1 and r2 do not chain with each other (query descending)
    perm = np.random.default_rng(r3).permutation(n)
    h = h[perm]
    at = {int(r): int(k) for k, r in enumerate(perm)}  # rank -> input index
    with tile(E, T):
        f, pred, _ = run(E, h)
    j1, j2, i = at[r1], at[r2], at[r3]
    t, sub = M.tile_of(h, None, T), M.tile_of(h, None, 64)
    assert M.precedes(h, None, j1, i) and M.precedes(h, None, j2, i) and not M.precedes(h, None, j1, j2)
    assert f[j1] == f[j2] and f[i] == f[j1] + 5, "the two candidates are not equal"
    assert pred[i] == j1
    want = {"two earlier tiles": t[j1] < t[j2] < t[i], "an earlier tile and the node's own tile": t[j1] < t[j2] == t[i],
            "one 64-node sub-tile": sub[j1] == sub[j2] == sub[i], "two sub-tiles of one tile": t[j1] == t[j2] == t[i] and sub[j1] < sub[j2] < sub[i]}
    assert want[name]


def test_an_end_tie_between_tiles_goes_to_the_lower_rank(E):
    h = placed(200, {10: (300, 500), 150: (200, 500)})
    with tile(E, 64):
        f, pred, members = run(E, h)
    assert f[10] == f[150] == f.max() and M.tile_of(h, None, 64)[10] != M.tile_of(h, None, 64)[150]
    assert members["hsp_index"][-1] == 10


# ---- groups ----
def test_groups_unsorted_and_across_tile_boundaries(E):
    rng = np.random.default_rng(23)
    h = scatter(rng, 220)
    # 40 + 150 + 30 HSPs: group 7 starts mid-tile and spans tiles 0, 1 and 2 of 64; the ids are neither sorted nor dense
    g = np.array([3] * 40 + [7] * 150 + [900_000] * 30, dtype=np.uint32)[rng.permutation(220)]
    with tile(E, 64):
        f, pred, members = run(E, h, g, diag_pen=1)
    order = M.rank_order(h, g)
    gr = g[order]
    assert not np.array_equal(g, np.sort(g))
    assert gr[63] != gr[0] and np.unique(np.flatnonzero(gr == 7) // 64).tolist() == [0, 1, 2] and np.flatnonzero(gr == 7)[0] % 64 != 0
    assert members["group"].tolist() == sorted(members["group"].tolist()) and np.unique(members["group"]).size == 3
    assert all(g[p] == g[i] for i, p in enumerate(pred) if p >= 0)


def test_many_one_hsp_groups(E):
    rng = np.random.default_rng(29)
    h = scatter(rng, 150)
    g = (rng.permutation(150) * 7 + 1).astype(np.uint32)
    with tile(E, 64):
        f, pred, members = run(E, h, g)
    assert (pred == -1).all() and members.size == 150 and np.array_equal(members["group"], np.sort(g))
    assert np.array_equal(f, h["score"])


def test_the_best_candidate_by_value_lies_in_another_group(E):
    h = M.make([(100, 100, 10, 1000), (200, 200, 10, 10), (400, 400, 10, 5)] + [(1000 + 50 * k, 5000 - 50 * k, 10, 1) for k in range(80)])
    g = np.array([1, 2, 2] + [2] * 80, dtype=np.uint32)
    _, pred_ignored, _ = M.chain(h, None)
    assert pred_ignored[2] == 1 and pred_ignored[1] == 0  # without groups the 1000 flows in
    with tile(E, 64):
        f, pred, _ = run(E, h, g)
    assert pred[2] == 1 and pred[1] == -1 and f[2] == 15


# ---- magnitudes ----
def test_coordinates_next_to_2_to_the_32(E):
    top = 2 ** 32 - 1
    rng = np.random.default_rng(31)
    rows = [(top - 1000 + 12 * k + int(rng.integers(0, 3)), top - 990 + 12 * k, 10, 50) for k in range(80)]
    rows[-1] = (top - 20, top - 10, 40, 50)  # its end lies past 2^32
    h = M.make(rows)[rng.permutation(80)]
    assert (h["ref_start"].astype(np.int64) >= top - 1000).all() and (h["ref_start"].astype(np.int64) + h["len"] + 1).max() > 2 ** 32
    with tile(E, 64):
        f, pred, members = run(E, h, diag_pen=3, anti_pen=2)
    assert members.size > 20


def test_scores_of_int32_max_sum_past_2_to_the_33(E):
    h = M.make([(100 * k, 100 * k, 50, 2 ** 31 - 1) for k in range(70)])
    with tile(E, 64):
        f, pred, members = run(E, h, anti_pen=1)
    assert int(members["f"][-1]) > 2 ** 33 and members.size == 70


def test_largest_penalties_on_diagonals_2_to_the_31_apart(E):
    rows = [(10, 3_000_000_000, 20, 2 ** 31 - 1), (3_200_000_000, 3_100_000_000, 20, 100)]
    rows += [(100 + 50 * k, 2_000_000_000 - 50 * k, 10, 7) for k in range(70)]
    h = M.make(rows)
    assert M.precedes(h, None, 0, 1) and M.penalty(h, 0, 1, 1 << 20, 1 << 20) > 2 ** 51
    assert abs((int(h["ref_start"][1]) - int(h["query_start"][1])) - (int(h["ref_start"][0]) - int(h["query_start"][0]))) > 2 ** 31
    assert M.chain(h, None)[1][1] == 0
    with tile(E, 64):
        f, pred, _ = run(E, h, diag_pen=1 << 20, anti_pen=1 << 20)
    assert pred[1] == -1 and f[1] == 100


def test_negative_and_zero_scores(E):
    rng = np.random.default_rng(37)
    h = scatter(rng, 180, score=(-200, 120))
    h["score"][::7] = 0
    h["score"][3] = -2 ** 31
    with tile(E, 64):
        f, pred, members = run(E, h, min_score=-2 ** 40)
    assert (h["score"] < 0).sum() > 40 and (f < 0).any() and (pred >= 0).any()
    assert members.size >= 1


# ---- random sets, tile independence ----
PARAMS = [dict(diag_pen=0, anti_pen=0, max_gap=0), dict(diag_pen=2, anti_pen=1, max_gap=0), dict(diag_pen=1, anti_pen=0, max_gap=400)]
_sets = {}


def random_case(seed, k):
    if (seed, k) not in _sets:
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(300, 2001))
        h = scatter(rng, n, diagonals=int(rng.integers(2, 6)), step=40, jitter=6)
        sizes = rng.integers(1, 40, 6)
        g = rng.choice(np.array([0, 5, 6, 70, 4_000_000_000, 12], dtype=np.uint32), size=n, p=sizes / sizes.sum())
        small = np.flatnonzero(g == 12)[:3]  # a group too small to reach min_score
        g[g == 12] = 5
        g[small] = 12
        kw = dict(PARAMS[k])
        f, _, _ = M.chain(h, g, **kw)
        tops = sorted(int(f[g == x].max()) for x in np.unique(g))
        kw["min_score"] = (tops[0] + tops[1]) // 2 + 1 if len(tops) > 1 else 0
        _sets[(seed, k)] = (h, g, kw, M.chain(h, g, **kw))
    return _sets[(seed, k)]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(6))
def test_random_sets(E, seed, k):
    h, g, kw, model = random_case(seed, k)
    _, _, members = run(E, h, g, model=model, **kw)
    kept = np.unique(members["group"]).size
    assert 1 <= kept < np.unique(g).size, "min_score must cut a group and keep one"


@pytest.mark.parametrize("seed", range(6))
def test_results_do_not_depend_on_the_tile(E, seed):
    h, g, kw, model = random_case(seed, seed % 3)
    got = []
    for t in (64, 256, None):
        with tile(E, t):
            got.append(E.ChainHsps(h, g, nodes=True, **kw))
    steps = [st["tile_steps"] for _, _, st in got]
    assert steps[0] > steps[1]  # the tile did change
    for m, nd, _ in got:
        assert np.array_equal(m, model[2]) and np.array_equal(nd["f"], model[0]) and np.array_equal(nd["pred"], model[1])


# ---- threads ----
def test_eight_threads_get_the_serial_results(E):
    cases = [random_case(s, (s + 1) % 3) for s in range(6)] + [random_case(0, 0), random_case(1, 0)]
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


# ---- parameter validation ----
CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
h = np.zeros(%d, dtype=E.SEG_DTYPE)
if %d: E.set_option("chain_tile", %d)
E.ChainHsps(h, None, diag_pen=%d, anti_pen=%d)
print("returned")
"""


@pytest.mark.parametrize("what,n,t,dp,ap", [
    ("diag_pen", 4, 0, (1 << 20) + 1, 0), ("diag_pen", 4, 0, -1, 0), ("anti_pen", 4, 0, 0, (1 << 20) + 1),
    ("chain_tile", 4, 96, 0, 0), ("chain_tile", 4, 2048, 0, 0), ("chain_tile", 0, 32, 0, 0), ("number of HSPs", (1 << 22) + 1, 0, 0, 0),
])
def test_out_of_range_values_fail_with_a_message(what, n, t, dp, ap):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, n, 1 if t else 0, t, dp, ap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"ChainHsps" in r.stderr and what.encode() in r.stderr


def test_values_at_the_limits_are_accepted(E):
    h = scatter(np.random.default_rng(41), 100)
    with tile(E, 1024):
        run(E, h, diag_pen=1 << 20, anti_pen=1 << 20, max_gap=2 ** 32 - 1)
    with tile(E, 128):
        run(E, h, min_score=2 ** 62)
