"""CPU: the inputs of tests/gapped_regimes.py are in the regimes they claim, shown on the serial checkers alone, so that
tests/test_gpu_gapped_regimes.py cannot pass quietly on an input that misses its target."""
import numpy as np
import pytest

import gapped_model as G
import gapped_pieces_model as PM
import gapped_regimes as R
import gapped_trace_model as T


# ---- A ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", sorted(R.A_BANDS))
def test_a_sides_run_past_the_window_in_every_instance(K):
    b, h = R.block_a()
    kw = R.a_params(K)
    assert R.cells_per_lane(kw["max_band"]) == K
    ss = R.sides(b, h, **kw)
    far = 64 * K + 192  # the window base moved at least 192 times: the X stream (64 codes, 64 ahead) was refilled at least twice
    assert sum(s[1] >= far for s in ss) * 2 >= len(ss), [s[1] for s in ss]
    assert not any(s[4] & G.BAND_CAP for s in ss)
    # i << j and i >> j at a moved window
    assert any(s[1] >= far and s[2] - s[1] >= 64 for s in ss) and any(s[1] >= far and s[1] - s[2] >= 64 for s in ss)


@pytest.mark.parametrize("K", sorted(R.A_BANDS))
def test_a_continuation_pieces_run_past_the_window(K):
    b, h = R.block_a()
    _, _, sides = PM.align(b.tc, b.qc, b.sub, h, 3, **R.a_params(K))
    later = [p["res"][1] for pair in sides for _, chain, _ in pair for p in chain[1:]]
    assert sum(i >= 64 * K + 192 for i in later) * 2 >= len(later) > 0, later
    assert max(len(chain) for pair in sides for _, chain, _ in pair) == 3


# ---- B ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,width", sorted(R.B_TUNED))
def test_b_smallest_uncapped_band_is_the_tight_width(name, width):
    """"Caps at width - 1, not at width" is the bisection's result: max_band enters the sweep in the two cap tests only, so a larger
    max_band weakens both tests and changes nothing else -- a side that does not cap at some max_band caps at no larger one."""
    b, anc = R.block_b()
    kw = R.b_params(name, width)
    assert width + 1 in (128, 256, 512, 1088)
    assert R.capped(b, anc[name], max_band=width - 1, **kw)
    ss = R.sides(b, anc[name], max_band=width, **kw)
    assert not any(s[4] & G.BAND_CAP for s in ss)
    assert all(s[1] >= 64 * R.cells_per_lane(width) + 192 for s in ss), ss
    assert R.sides(b, anc[name], max_band=width + 1, **kw) == ss


def test_b_bisection_finds_the_width():
    b, anc = R.block_b()
    assert R.min_uncapped_band(b, anc["rep"], **R.b_params("rep", 127)) == 127
    assert R.min_uncapped_band(b, anc["homo"], **R.b_params("homo", 255)) == 255


@pytest.mark.parametrize("name,width", sorted(R.B_PIECES))
def test_b_continuation_pieces_grow_a_wide_band_again(name, width):
    b, _ = R.block_b()
    kw = R.b_pieces_params(name, width)
    h = R.b_pieces_anchors(name)
    K = R.cells_per_lane(width)
    assert name == "homo" or K == 8
    _, _, sides = PM.align(b.tc, b.qc, b.sub, h[:1], 3, **kw)
    chains = [chain for pair in sides for _, chain, _ in pair]
    assert all(len(c) == 3 and not c[-1]["res"][4] & G.BAND_CAP for c in chains)
    for c in chains:  # piece 1 alone: wider than the next smaller instance's window, on the homopolymer exactly `width`
        o_r, o_q = c[1]["origin"]
        one = R.anchors([(o_r, o_q)])
        low = width - 1 if name == "homo" else 64 * 4  # (the repeat runs at K = 8: 64 * 4 is the window of K = 4)
        assert R.capped(b, one, **dict(kw, max_band=low)) and not R.capped(b, one, **kw)
        assert c[1]["res"][1] >= 64 * K + 192
    # the second anchor lies on the first one's path
    _, _, want = PM.greedy(b.tc, b.qc, b.sub, h, 3000, 3, **kw)
    assert (want["returned"], want["covered"]) == (1, 1)


@pytest.mark.parametrize("name", sorted(R.B_WIDE))
def test_b_widest_instance_holds_a_band_of_1500(name):
    b, anc = R.block_b()
    kw = R.b_params(name, 2048)
    assert R.capped(b, anc[name], max_band=1499, **kw)
    ss = R.sides(b, anc[name], max_band=2048, **kw)
    assert not any(s[4] & G.BAND_CAP for s in ss) and all(s[1] >= 64 * 33 + 192 for s in ss)


# ---- C ----------------------------------------------------------------------------------------------------------------------------

def c_sides(k, **kw):
    b, h, planted = R.block_c()
    r, q, _, _ = h[k].tolist()
    kw = dict(kw, max_band=kw.get("max_band", G.DEFAULT_BAND))
    return [(pl, *T.side(b.tc, b.qc, b.sub, r, q, d, **kw)[:2]) for d, pl in zip((-1, +1), planted[k])]


def test_c_every_path_holds_its_planted_run():
    _, h, planted = R.block_c()
    seen = set()
    for k in range(h.size):
        for pl, res, ops in c_sides(k, **R.C_PARAMS):
            runs = [(kind, ln) for kind, ln, _ in R.gap_runs(ops, res[1] + res[2])]
            assert runs.count(pl) == 1 and not res[4], (k, pl, runs)
            seen.add(pl)
    assert seen == {(kind, ln) for kind in "ID" for ln in R.C_LENGTHS}
    for k in R.C_K2_RECORDS:
        for pl, res, ops in c_sides(k, **R.C_PARAMS_K2):
            assert pl[1] == 70 and pl in [(kind, ln) for kind, ln, _ in R.gap_runs(ops, res[1] + res[2])] and not res[4]


def test_c_one_run_begins_at_a_stage_boundary():
    """A stage of the walk kernel begins at the walk's current i + j and ends once 64 or more antidiagonals are consumed (an M step
    from the last one overshoots to 65).  Before its gap run the last record's right side walks M steps only, two antidiagonals each
    from dstar on, so its stages begin at dstar - 64 k exactly, and the run is entered at one of them."""
    _, h, _ = R.block_c()
    pl, res, ops = c_sides(h.size - 1, **R.C_PARAMS)[1]
    dstar = res[1] + res[2]
    assert ops[0] & 3 == T.OP_M and (int(ops[1]) & 3, int(ops[1]) >> 2) == (T.OP_I, 70)  # nothing but one M run precedes the planted run
    assert [(dstar - d) % 64 for kind, ln, d in R.gap_runs(ops, dstar) if (kind, ln) == pl] == [0]
    assert R.stage_far() == R.C_STAGE_FAR


# ---- D ----------------------------------------------------------------------------------------------------------------------------

def test_d_tie_rules_decide_a_quarter_of_the_sides():
    """Against the two deliberately wrong builds of the path checker: preferring F, E, M as the source of H changes the path, and
    taking the last instead of the first cell of an antidiagonal that reaches a new maximum changes the best cell, of at least a
    quarter of all sides of D.  (Best-cell ties do not arise in the mixed inputs at all: the tiles are there for them.)"""
    b, sets = R.block_d()
    assert np.array_equal(b.sub.reshape(8, 8)[:4, :4], 2 * np.eye(4, dtype=np.int32) - 1)
    cell, path, n = {1: 0, 2: 0}, {1: 0, 2: 0}, 0
    for name, hs, kw in sets:
        for v in (1, 2):
            c, p, m = R.variant_changes(b, hs, v, **kw)
            cell[v] += c
            path[v] += p
        n += m
    assert path[1] * 4 >= n and cell[1] == 0, (path, cell, n)
    assert cell[2] * 4 >= n, (cell, n)


def test_d_tied_cells_sit_in_many_lanes_and_past_the_window():
    b, sets = R.block_d()
    name, hs, kw = sets[-1]
    assert name == "tiles" and kw["max_band"] == 100
    ss = R.sides(b, hs, **dict(kw, max_band=100))
    # each side's best cell is (|P| + 1, |P| + 2), the smaller i of the two tied cells: both slots of a lane at K = 2, the window's
    # first and last lanes, and cells one and two windows (128 cells) further on
    assert sorted(s[1] for s in ss) == sorted(2 * [p + 1 for p in R.D_PREFIXES])
    assert all(s[2] == s[1] + 1 and not s[4] for s in ss)
    assert {0, 1, 63, 64, 127, 128, 129, 256} <= set(R.D_PREFIXES)


def test_default_build_of_the_path_checker_is_the_contract():
    """The variant switch is off unless asked for: the default build still equals gapped_check.c on a tie-heavy input."""
    b, sets = R.block_d()
    _, hs, kw = sets[0]
    kw = dict(kw, max_band=G.DEFAULT_BAND)
    for r, q, _, _ in hs[:4].tolist():
        for d in (-1, +1):
            assert T.side(b.tc, b.qc, b.sub, r, q, d, **kw)[0] == G.side(b.tc, b.qc, b.sub, r, q, d, **kw)
