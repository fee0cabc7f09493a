"""CPU: the gap-cost chaining model (tests/hsp_chain_gap_model.py; contract in include/segalign_amd.h) against an
exhaustive search over every valid chain, hand cases of the piecewise-linear cost, the case selection, the presets, every clause of
the validation, and the parser of the linearGap file (segalign_amd.engine.parse_linear_gap)."""
import itertools

import numpy as np
import pytest

import hsp_chain_gap_model as G
import hsp_chain_model as M

HAND = {"pos": [2, 10, 100, 1000], "q_gap": [5, 50, 60, 60], "t_gap": [7, 7, 700, 800], "both_gap": [20, 30, 300, 3000]}
TABLES = {"loose": "loose", "medium": "medium", "hand": HAND}


def exhaustive(h, g, dp, ap, mg, t):
    """best[i] = the largest score of any valid chain that ends at i under pen'."""
    n = h.size
    best = [None] * n
    order = list(M.rank_order(h, g))
    for k in range(1, n + 1):
        for sub in itertools.combinations(order, k):  # rank order: the only order in which a subset can chain
            if not all(M.precedes(h, g, sub[x], sub[x + 1], mg) for x in range(k - 1)):
                continue
            s = sum(int(h["score"][x]) for x in sub) - sum(G.link_penalty(h, sub[x], sub[x + 1], dp, ap, t) for x in range(k - 1))
            e = sub[-1]
            if best[e] is None or s > best[e]:
                best[e] = s
    return best


def random_set(rng, n, groups, spread):
    rows = []
    for _ in range(n):
        r, d = int(rng.integers(0, spread)), int(rng.integers(-12, 13)) * int(rng.integers(0, 2))  # half of them on the main diagonal
        rows.append((r, max(0, r + d), int(rng.integers(1, 25)), int(rng.integers(-30, 3000))))
    h = M.make(rows)
    g = rng.integers(0, groups, n).astype(np.uint32) if groups > 1 else None
    return h, g


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("params", [(0, 0, 0), (3, 1, 0), (0, 2, 60)])
def test_model_equals_exhaustive_search(seed, name, params):
    dp, ap, mg = params
    t = G.validate(TABLES[name])
    rng = np.random.default_rng(200 + seed)
    linked = 0
    for groups in (1, 3):
        for n, spread in ((1, 100), (4, 120), (7, 150), (9, 200), (8, 4000)):
            h, g = random_set(rng, n, groups, spread)
            f, pred, _ = G.chain(h, g, dp, ap, mg, min_score=-10 ** 9, gap_costs=t)
            assert [int(x) for x in f] == exhaustive(h, g, dp, ap, mg, t), (groups, n)
            linked += int((pred >= 0).sum())
    assert linked > 0, "no set had a link"


def test_the_row_form_of_the_gap_cost_equals_the_integer_form():
    rng = np.random.default_rng(7)
    for name in sorted(TABLES):
        t = G.validate(TABLES[name])
        dt = rng.integers(0, 400000, 2000) * rng.integers(0, 2, 2000)
        dq = rng.integers(0, 3000, 2000) * rng.integers(0, 2, 2000)
        dt[:3], dq[:3] = [2 ** 32, 2 ** 32, 0], [2 ** 32 - 2, 0, 2 ** 32]
        want = [G.gapcost(t, int(a), int(b)) for a, b in zip(dt, dq)]
        assert [int(x) for x in G.gapcost_rows(t, dt, dq)] == want


# ---- hand cases of g ----
def test_g_below_the_first_break_point_is_the_first_cost():
    assert G.g([5, 10], [100, 200], 1) == 100 and G.g([5, 10], [100, 200], 4) == 100 and G.g([5, 10], [100, 200], 5) == 100


def test_g_at_every_break_point_is_the_table_value():
    for name in ("q_gap", "t_gap", "both_gap"):
        assert [G.g(HAND["pos"], HAND[name], x) for x in HAND["pos"]] == HAND[name]


def test_g_one_below_a_break_point_shows_the_floor():
    # slope of the segment 2 .. 10 of q_gap: floor(65536 * 45 / 8) = 368640 = 5.625 * 65536 exactly: 5 + floor(7 * 5.625) = 44
    assert G.slopes(HAND["pos"], HAND["q_gap"])[0] == 368640 and G.g(HAND["pos"], HAND["q_gap"], 9) == 44
    # 10 / 3 is no dyadic fraction: slope floor(655360 / 3) = 218453; at x = 3 the exact line gives 6.67, the shift floors it to 6
    assert G.slopes([1, 4], [0, 10]) == [218453, 218453]
    assert G.g([1, 4], [0, 10], 3) == (2 * 218453) >> 16 == 6 and G.g([1, 4], [0, 10], 4) == 10
    # medium, one below 111: 600 + floor(99 * 3) = 897
    t = G.table("medium")
    assert G.g(t["pos"], t["q_gap"], 110) == 897


def test_g_beyond_the_last_point_extrapolates_the_last_segment():
    t = G.table("loose")
    assert G.slopes(t["pos"], t["q_gap"])[-2:] == [16384, 16384]  # 25000 / 100000
    assert G.g(t["pos"], t["q_gap"], 252111 + 4000) == 56600 + 1000
    x = 2 ** 33 - 2
    assert G.g(t["pos"], t["q_gap"], x) == 56600 + ((x - 252111) >> 2)
    # the largest slope at the largest gap stays inside the bound of the contract
    pos, c = [1, 2], [0, 2047]
    assert G.slopes(pos, c) == [2047 << 16, 2047 << 16] and (2047 << 16) < 2 ** 27
    assert G.g(pos, c, x) == 2047 * (x - 1) < 2 ** 45


def test_g_with_one_point_is_constant():
    assert G.slopes([7], [300]) == [0]
    assert [G.g([7], [300], x) for x in (1, 6, 7, 8, 2 ** 33 - 2)] == [300] * 5


def test_g_on_a_flat_segment_stays_flat_and_the_flat_tail_too():
    assert G.slopes(HAND["pos"], HAND["q_gap"])[2:] == [0, 0]
    assert [G.g(HAND["pos"], HAND["q_gap"], x) for x in (100, 500, 999, 1000, 10 ** 9)] == [60] * 5
    assert [G.g(HAND["pos"], HAND["t_gap"], x) for x in (2, 5, 9, 10)] == [7, 7, 7, 7]


# ---- case selection ----
def test_the_case_follows_which_gap_is_zero():
    t = G.validate(HAND)
    assert G.gapcost(t, 0, 0) == 0
    assert G.gapcost(t, 0, 10) == 50 and G.gapcost(t, 10, 0) == 7 and G.gapcost(t, 4, 6) == 30 and G.gapcost(t, 1, 1) == 20
    assert G.gapcost(t, 0, 1) == 5 and G.gapcost(t, 1, 0) == 7  # below pos[0]


# ---- presets ----
@pytest.mark.parametrize("name", ["loose", "medium"])
def test_a_preset_is_valid_and_returns_its_table_at_every_break_point(name):
    t = G.validate(name)
    assert len(t["pos"]) == 11 and t["q_gap"] == t["t_gap"]
    for k, x in enumerate(t["pos"]):
        assert G.gapcost(t, 0, x) == t["q_gap"][k] and G.gapcost(t, x, 0) == t["t_gap"][k]
        if x >= 2:
            assert G.gapcost(t, 1, x - 1) == t["both_gap"][k]
    assert G.gapcost(t, 0, 1) == {"loose": 325, "medium": 350}[name] and G.gapcost(t, 1, 1) == {"loose": 660, "medium": 825}[name]


# ---- validation ----
def changed(**kw):
    t = {k: list(v) for k, v in HAND.items()}
    t.update(kw)
    return t


@pytest.mark.parametrize("t,clause", [
    ({"pos": [], "q_gap": [], "t_gap": [], "both_gap": []}, "n"),
    ({k: list(range(1, 18)) for k in ("pos", "q_gap", "t_gap", "both_gap")}, "n"),
    (changed(pos=[0, 10, 100, 1000]), "pos"),
    (changed(pos=[2, 10, 10, 1000]), "pos"),
    (changed(pos=[2, 100, 10, 1000]), "pos"),
    (changed(q_gap=[-1, 50, 60, 60]), "q_gap range"),
    (changed(t_gap=[7, 7, 700, 2 ** 40 + 1]), "t_gap range"),
    (changed(both_gap=[20, 30, 29, 3000]), "both_gap order"),
    (changed(q_gap=[5, 5 + 8 * 2048, 5 + 8 * 2048, 5 + 8 * 2048]), "q_gap slope"),
])
def test_every_validation_clause(t, clause):
    with pytest.raises(ValueError, match=clause):
        G.validate(t)


def test_values_at_the_limits_are_valid():
    G.validate({"pos": [1], "q_gap": [0], "t_gap": [2 ** 40], "both_gap": [2 ** 40]})
    G.validate(changed(q_gap=[5, 5 + 8 * 2048 - 1, 5 + 8 * 2048 - 1, 5 + 8 * 2048 - 1]))  # slope 2^27 - 8192
    G.validate({"pos": [1, 2 ** 30], "q_gap": [0, 2 ** 40], "t_gap": [2 ** 40, 2 ** 40], "both_gap": [0, 0]})
    G.validate({k: list(range(1, 17)) for k in ("pos", "q_gap", "t_gap", "both_gap")})


# ---- the linearGap file ----
FILE = """# a table
tableSize 4
smallSize 111
position 2 10 100 1000
qGap 5 50 60 60
tGap 7 7 700 800

bothGap 20 30 300 3000
"""


def test_the_linear_gap_parser_reads_the_layout_and_refuses_the_rest():
    from segalign_amd.engine import parse_linear_gap
    assert parse_linear_gap(FILE) == HAND
    assert parse_linear_gap(FILE.replace("smallSize 111\n", "")) == HAND  # smallSize is optional and ignored
    for bad in (FILE.replace("tableSize 4", "tableSize 5"), FILE.replace("qGap 5 50 60 60", "qGap 5 50 60"),
                FILE.replace("tGap", "uGap"), FILE.replace("60 60", "60 x"), FILE.replace("tableSize 4", "tableSize 17"),
                FILE.replace("bothGap 20 30 300 3000\n", ""), FILE + "qGap 5 50 60 60\n", FILE.replace("tableSize 4\n", "")):
        with pytest.raises(ValueError):
            parse_linear_gap(bad)
