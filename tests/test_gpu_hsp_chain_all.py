"""GPU: sa_chain_hsps_all (include/segalign_amd.h) against the model of tests/hsp_chain_all_model.py.  Every test compares
the chains, the members, chain_of and f and pred of every HSP, and first asserts with the model that its input is in the regime it
names.  The entry needs no sequence: the tests build HSP records directly, on an interface without a processor."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_all_model as A
import hsp_chain_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["group", "head", "first_member", "n_members", "score", "joined"]


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


def same(got, model):
    """An engine result (chains, members, nodes, chain_of, stats) against the model's (f, pred, chains, members, chain_of)."""
    chains, members, nodes, chain_of, st = got
    f, pred, m_chains, m_members, m_of = model
    assert np.array_equal(nodes["f"], f), np.flatnonzero(nodes["f"] != f)[:8]
    assert np.array_equal(nodes["pred"], pred), np.flatnonzero(nodes["pred"] != pred)[:8]
    assert chains.size == m_chains.size and members.size == m_members.size
    for k in FIELDS:
        assert np.array_equal(chains[k], m_chains[k]), (k, np.flatnonzero(chains[k] != m_chains[k])[:8])
    for k in ("hsp_index", "group", "chain", "f"):
        assert np.array_equal(members[k], m_members[k]), (k, np.flatnonzero(members[k] != m_members[k])[:8])
    assert np.array_equal(chain_of, m_of), np.flatnonzero(chain_of != m_of)[:8]
    assert (chains["pad"] == 0).all() and (members["pad"] == 0).all()


def run(E, h, g=None, model=None, **kw):
    """One engine call held against the model.  -> the model's (f, pred, chains, members, chain_of)."""
    model = model if model is not None else A.chain_all(h, g, **kw)
    got = E.ChainHspsAll(h, g, nodes=True, **kw)
    same(got, model)
    st = got[4]
    n = h.size
    all_chains = A.chain_all(h, g, **dict(kw, min_score=-2 ** 62))[2].size
    rounds = 0 if n == 0 else max(1, int(n - 1).bit_length())
    ng = 0 if n == 0 else (1 if g is None else np.unique(g).size)
    assert (st["hsps"], st["groups"], st["chains"], st["members"]) == (n, ng, model[2].size, model[3].size)
    assert (st["chains_all"], st["joined"], st["peel_rounds"]) == (all_chains, int((model[2]["joined"] >= 0).sum()), rounds)
    chains, members, chain_of, _ = E.ChainHspsAll(h, g, **kw)  # without the nodes argument
    assert np.array_equal(chains, got[0]) and np.array_equal(members, got[1]) and np.array_equal(chain_of, got[3])
    return model


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
@pytest.mark.parametrize("t", [64, None])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_sizes_around_a_tile(E, n, t):
    h = scatter(np.random.default_rng(n), n)
    with tile(E, t):
        f, pred, chains, members, chain_of = run(E, h, diag_pen=1)
    assert members.size == n and (n < 63 or ((chains["joined"] >= 0).any() and (chains["n_members"] > 1).any()))


# ---- single paths: the depth the doubling rounds must cover ----
@pytest.mark.parametrize("n", [65, 129, 1025])
def test_a_clean_ladder_is_one_chain(E, n):
    h = M.make([(100 + 20 * k, 50 + 20 * k, 10, 3) for k in range(n)])[np.random.default_rng(n).permutation(n)]
    f, pred, chains, members, chain_of = run(E, h)
    assert chains.size == 1 and chains["n_members"][0] == n and chains["score"][0] == 3 * n and (pred >= 0).sum() == n - 1


# ---- comb: one joined chain per stem node ----
def test_a_comb_of_130_joined_chains(E):
    rows = [(1000 * k, 1000 * k, 10, 100) for k in range(130)]                      # the stem
    rows += [(1000 * k + 500, 10 ** 6 - 1000 * k, 10, -5) for k in range(130)]      # side k follows stem node k and nothing follows it
    h = M.make(rows)
    perm = np.random.default_rng(3).permutation(260)
    h = h[perm]
    with tile(E, 64):
        f, pred, chains, members, chain_of = run(E, h, min_score=-5)
    at = np.argsort(perm)  # row -> input index
    assert chains.size == 131 and chains["n_members"][0] == 130 and (chains["n_members"][1:] == 1).all() and (chains["score"][1:] == -5).all()
    assert sorted(chains["joined"][1:].tolist()) == sorted(at[:130].tolist())
    assert all(pred[at[130 + k]] == at[k] for k in range(130))


# ---- star: every atomic of a round lands on one address ----
def test_a_star_of_300_equal_leaves(E):
    rows = [(100, 100, 10, 50)] + [(1000 + 100 * k, 10 ** 6 - 100 * k, 10, 7) for k in range(300)]
    h = M.make(rows)
    perm = np.random.default_rng(4).permutation(301)
    h = h[perm]
    at = np.argsort(perm)
    f, pred, chains, members, chain_of = run(E, h)
    assert (np.delete(f, at[0]) == 57).all() and (np.delete(pred, at[0]) == at[0]).all()
    assert chains.size == 300 and chains["head"][0] == at[1] and chains["n_members"][0] == 2 and chains["score"][0] == 57
    assert (chains["joined"][1:] == at[0]).all() and (chains["score"][1:] == 7).all()
    assert chains["head"][1:].tolist() == at[2:].tolist()  # equal scores: in the rank order of the heads


# ---- a fork across tiles ----
@pytest.mark.parametrize("b_score,winner", [(50, "a"), (60, "b")])
def test_a_fork_whose_branches_lie_in_different_tiles(E, b_score, winner):
    rows = [(10, 10, 10, 10), (30, 30, 10, 10), (500, 2 * 10 ** 6, 10, 50)]          # the stem and branch a
    rows += [(1000 + 100 * k, 10 ** 6 - 100 * k, 10, -5) for k in range(150)]         # fillers: each follows the stem, none another
    rows += [(17000, 1_500_000, 10, b_score)]                                         # branch b: follows the stem and the fillers
    h = M.make(rows)
    with tile(E, 64):
        f, pred, chains, members, chain_of = run(E, h, min_score=-10)
    a, b = 2, 153
    t = M.tile_of(h, None, 64)
    assert t[a] != t[b] and pred[a] == pred[b] == 1 and f[a] == 70 and f[b] == 20 + b_score
    top, cut = (a, b) if winner == "a" else (b, a)
    assert chain_of[0] == chain_of[1] == chain_of[top] == 0 and chains["head"][0] == top
    k = chain_of[cut]
    assert k != 0 and chains["joined"][k] == 1 and chains["n_members"][k] == 1 and chains["score"][k] == f[cut] - 20
    assert chains.size == 152 and (chains["score"][2:] == -5).all()


# ---- groups ----
def test_groups_unsorted_and_across_tile_boundaries(E):
    rng = np.random.default_rng(23)
    h = scatter(rng, 220)
    g = np.array([3] * 40 + [7] * 150 + [900_000] * 30, dtype=np.uint32)[rng.permutation(220)]
    with tile(E, 64):
        f, pred, chains, members, chain_of = run(E, h, g, diag_pen=1)
    gr = g[M.rank_order(h, g)]
    assert not np.array_equal(g, np.sort(g)) and gr[63] != gr[0] and np.flatnonzero(gr == 7)[0] % 64 != 0
    assert np.unique(chains["group"]).tolist() == [3, 7, 900_000] and all((chains["group"] == x).sum() > 1 for x in (3, 7, 900_000))
    assert all(g[j] == c for j, c in zip(chains["joined"], chains["group"]) if j >= 0)


def test_many_one_hsp_groups(E):
    rng = np.random.default_rng(29)
    h = scatter(rng, 150)
    g = (rng.permutation(150) * 7 + 1).astype(np.uint32)
    with tile(E, 64):
        f, pred, chains, members, chain_of = run(E, h, g)
    assert chains.size == 150 and (chains["n_members"] == 1).all() and (chains["joined"] == -1).all()
    assert np.array_equal(chains["group"], np.sort(g)) and np.array_equal(chains["score"], h["score"][chains["head"]])


# ---- min_score ----
def test_a_dropped_chain_still_stops_the_chain_that_joins_it(E):
    # tests/test_hsp_chain_all_model.py: 0 -> 1 -> 2 scores 700; 4 -> 3 is cut at 1 and scores -50; 5 is cut at 3 and scores 90
    rows = [(100, 100, 10, 100), (200, 200, 10, 100), (300, 1000, 10, 500), (1000, 300, 10, -150), (2000, 400, 10, 100), (1500, 500, 10, 90)]
    h = M.make(rows)
    f, pred, chains, members, chain_of = run(E, h, max_gap=1000, min_score=0)
    assert chains[["head", "n_members", "score", "joined"]].tolist() == [(2, 3, 700, -1), (5, 1, 90, 3)]
    assert chain_of.tolist() == [0, 0, 0, A.NONE, A.NONE, 1]
    f, pred, chains, members, chain_of = run(E, h, max_gap=1000, min_score=-100)
    assert chains["score"].tolist() == [700, 90, -50] and chain_of.tolist() == [0, 0, 0, 2, 2, 1]
    run(E, h, max_gap=1000, min_score=701)  # nothing is kept


# ---- magnitudes: the priority key's sign handling ----
def test_f_below_zero_zero_and_past_2_to_the_33_next_to_2_to_the_32(E):
    top = 2 ** 32 - 1
    rows = [(top - 2000 + 100 * k, top - 2000 + 100 * k, 50, 2 ** 31 - 1) for k in range(10)]  # the last one ends past 2^32
    rows[-1] = (top - 20, top - 1100, 40, 2 ** 31 - 1)
    lone = [-2 ** 31, -5, 0, 0, 3, -1, 2 ** 31 - 1]  # nothing precedes or follows these
    rows += [(100 + 50 * k, top - 900 + 100 * k, 10, s) for k, s in enumerate(lone)][::-1]
    h = M.make(rows)
    f, pred, chains, members, chain_of = run(E, h, anti_pen=1, min_score=-2 ** 40)
    assert f.max() > 2 ** 33 and (f < 0).sum() == 3 and (f == 0).sum() == 2 and int(h["ref_start"].max()) + 41 > 2 ** 32
    assert chains.size == 8 and chains["n_members"][0] == 10
    assert chains["score"][1:].tolist() == sorted(lone, reverse=True)  # one group: by score descending across the sign


# ---- random sets, tile independence, threads, sa_chain_hsps ----
PARAMS = [dict(diag_pen=0, anti_pen=0, max_gap=0), dict(diag_pen=2, anti_pen=1, max_gap=0), dict(diag_pen=1, anti_pen=0, max_gap=400)]
_sets = {}


def random_case(seed, k):
    if (seed, k) not in _sets:
        rng = np.random.default_rng(2000 + seed)
        n = int(rng.integers(300, 2001))
        h = scatter(rng, n, diagonals=int(rng.integers(2, 6)), step=40, jitter=6, score=(-40, 300))
        sizes = rng.integers(1, 40, 5)
        g = rng.choice(np.array([0, 5, 6, 70, 4_000_000_000], dtype=np.uint32), size=n, p=sizes / sizes.sum())
        kw = dict(PARAMS[k])
        scores = A.chain_all(h, g, **kw, min_score=-2 ** 62)[2]["score"]
        kw["min_score"] = int(np.median(scores)) + 1  # about half of the chains are dropped
        _sets[(seed, k)] = (h, g, kw, A.chain_all(h, g, **kw))
    return _sets[(seed, k)]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(6))
def test_random_sets(E, seed, k):
    h, g, kw, model = random_case(seed, k)
    f, pred, chains, members, chain_of = run(E, h, g, model=model, **kw)
    assert (chains["joined"] >= 0).any() and (chain_of == A.NONE).any() and np.unique(chains["group"]).size > 1


@pytest.mark.parametrize("seed", range(6))
def test_results_do_not_depend_on_the_tile(E, seed):
    h, g, kw, model = random_case(seed, seed % 3)
    steps = []
    for t in (64, 256, None):
        with tile(E, t):
            got = E.ChainHspsAll(h, g, nodes=True, **kw)
        same(got, model)
        steps.append(got[4]["tile_steps"])
    assert steps[0] > steps[1]  # the tile did change


def test_eight_threads_get_the_serial_results(E):
    cases = [random_case(s, (s + 1) % 3) for s in range(6)] + [random_case(0, 0), random_case(1, 0)]
    out, errors = [None] * 8, []

    def work(i):
        try:
            h, g, kw, _ = cases[i]
            out[i] = E.ChainHspsAll(h, g, nodes=True, **kw)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(8):
        same(out[i], cases[i][3])


@pytest.mark.parametrize("seed", range(3))
def test_the_first_chain_of_a_group_is_the_best_chain(E, seed):
    h, g, kw, _ = random_case(seed, seed)
    kw = dict(kw, min_score=-2 ** 62)
    best, _ = E.ChainHsps(h, g, **kw)
    chains, members, chain_of, _ = E.ChainHspsAll(h, g, **kw)
    assert members.size == h.size
    for grp in np.unique(g):
        c = chains[np.flatnonzero(chains["group"] == grp)[0]]
        got, want = members[c["first_member"]:c["first_member"] + c["n_members"]], best[best["group"] == grp]
        assert np.array_equal(got["hsp_index"], want["hsp_index"]) and np.array_equal(got["f"], want["f"])
        assert c["score"] == want["f"][-1] and c["joined"] == -1


# ---- parameter validation ----
CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
E.ChainHspsAll(np.zeros(4, dtype=E.SEG_DTYPE), None, diag_pen=(1 << 20) + 1)
print("returned")
"""


def test_an_out_of_range_value_fails_with_a_message():
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"ChainHsps" in r.stderr and b"diag_pen" in r.stderr
