"""CPU: the contract of sa_fill_chains (include/segalign_amd.h) as tests/chain_fill_model.py restates it.  The scan
checker (tests/cpp/fill_check.c) against a direct Python restatement and the consequences the header lists, one hand case per
clause, a numpy emulation of the kernel's lane layout against the checker, the assembly of the filled chains, and the regimes of the
GPU test's cases with the model in the engine's place."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import chain_fill_cases as K
import chain_fill_model as F
import hsp_chain_model as M
import stitch_model as S
from gapped_model import SUB

HERE = os.path.dirname(os.path.abspath(__file__))
# two letters and the separator: match 2, mismatch -3
SUB2 = np.full((8, 8), -3, dtype=np.int32)
SUB2[0, 0] = SUB2[1, 1] = 2
SUB2[7, :] = SUB2[:, 7] = -50
# the hand cases' matrix: the target is all A, the query's letter is the weight: A 10, C -10, G -1, T -4
HAND = np.full((8, 8), -50, dtype=np.int32)
HAND[0, :4] = [10, -10, -1, -4]


def consequences(x, y, sub, thresh, xdrop, got):
    """What the header promises of every found HSP, whoever found it."""
    m = np.asarray(sub, dtype=np.int64).reshape(64)
    last = {}
    for i, j, ln, score in got:
        n = ln + 1
        assert 0 <= i and i + n <= len(x) and 0 <= j and j + n <= len(y)  # nothing leaves the rectangle
        a, c = np.asarray(x[i:i + n], dtype=np.int64) & 7, np.asarray(y[j:j + n], dtype=np.int64) & 7
        assert not (a == 7).any() and not (c == 7).any()
        w = m[a * 8 + c]
        pre = np.cumsum(w)
        assert int(pre[-1]) == score and score >= thresh  # the exact matrix sum
        assert (pre > 0).all() and (pre[-1] - np.concatenate([[0], pre[:-1]]) > 0).all()  # every prefix and every suffix
        assert (np.maximum.accumulate(pre) - pre <= xdrop).all()  # no prefix more than xdrop below an earlier one
        d = i - j
        if d in last:
            assert i > last[d]  # disjoint and ascending on a diagonal
        last[d] = i + ln
    order = [(i - j, i) for i, j, _, _ in got]
    assert order == sorted(order)


def both(x, y, sub, thresh, xdrop):
    got = [tuple(int(v) for v in r) for r in F.scan(x, y, sub, thresh, xdrop)]
    assert got == F.scan_py(x, y, sub, thresh, xdrop)
    consequences(x, y, sub, thresh, xdrop, got)
    return got


def test_every_rectangle_up_to_4_by_4_over_two_letters():
    n = 0
    for dt, dq in itertools.product(range(1, 5), repeat=2):
        for x in itertools.product((0, 1), repeat=dt):
            for y in itertools.product((0, 1), repeat=dq):
                for thresh, xdrop in ((1, 0), (2, 3), (4, 1), (5, 100)):
                    n += len(both(x, y, SUB2, thresh, xdrop))
    assert n > 5000


def test_a_hundred_random_rectangles_up_to_12_by_12():
    rng = np.random.default_rng(5)
    n = seps = 0
    for _ in range(100):
        dt, dq = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        x, y = rng.integers(0, 2, dt), rng.integers(0, 2, dq)
        x[rng.random(dt) < 0.06] = 7
        y[rng.random(dq) < 0.06] = 7
        seps += int((x == 7).any() or (y == 7).any())
        n += len(both(x, y, SUB2, int(rng.integers(1, 9)), int(rng.integers(0, 7))))
    assert n > 300 and seps > 20


def main_diagonal(y, thresh, xdrop, x=None):
    """The hand cases: target all A (or x), the query's letters are the weights; -> the main diagonal's (i, len, score)."""
    y = np.array(["ACGT&".index(c) if c != "&" else 7 for c in y])
    x = np.zeros(y.size, dtype=np.int64) if x is None else np.array([7 if c == "&" else 0 for c in x])
    return [(i, ln, sc) for i, j, ln, sc in both(x, y, HAND, thresh, xdrop) if i == j]


def test_the_xdrop_boundary():
    assert main_diagonal("ATGA", 10, 5) == [(0, 3, 15)]  # b - s = 5 = xdrop: goes on
    assert main_diagonal("ATGGA", 10, 5) == [(0, 0, 10), (4, 0, 10)]  # 6 = xdrop + 1: ends; the next segment starts behind the cell


def test_s_is_zero_exactly():
    assert main_diagonal("ACAA", 10, 100) == [(0, 0, 10), (2, 1, 20)]
    assert main_diagonal("CAA", 10, 100) == [(1, 1, 20)]  # s < 0 at once: nothing flushed, the next cell starts afresh


def test_the_threshold_boundary():
    assert main_diagonal("AAC", 20, 100) == [(0, 1, 20)] and main_diagonal("AAC", 21, 100) == []


def test_a_segment_that_ends_at_the_last_cell_and_two_on_one_diagonal():
    assert main_diagonal("CAA", 20, 100) == [(1, 1, 20)]
    assert main_diagonal("AACCCAAA", 20, 15) == [(0, 1, 20), (5, 2, 30)]
    assert main_diagonal("AAGAA", 20, 15) == [(0, 4, 39)]  # a dip inside xdrop keeps it one segment


def test_a_separator_in_either_sequence_inside_and_at_the_edge():
    assert main_diagonal("AA&AA", 20, 100) == [(0, 1, 20), (3, 1, 20)]
    assert main_diagonal("AAAAA", 20, 100, x="AA&AA") == [(0, 1, 20), (3, 1, 20)]
    assert main_diagonal("&AA", 20, 100) == [(1, 1, 20)] and main_diagonal("AA&", 20, 100) == [(0, 1, 20)]
    assert main_diagonal("AAA", 20, 100, x="&AA") == [(1, 1, 20)] and main_diagonal("AAA", 20, 100, x="AA&") == [(0, 1, 20)]
    assert main_diagonal("A&A", 20, 100) == []  # the separator resets: 10 + 10 across it is no segment


def test_one_row_one_column_and_one_cell():
    assert both([0], [0, 1, 0, 0], HAND, 10, 0) == [(0, 3, 0, 10), (0, 2, 0, 10), (0, 0, 0, 10)]  # d ascending: j descending
    assert both([0, 0, 0], [0], HAND, 10, 0) == [(0, 0, 0, 10), (1, 0, 0, 10), (2, 0, 0, 10)]
    assert both([0], [0], HAND, 10, 0) == [(0, 0, 0, 10)] and both([0], [1], HAND, 10, 0) == []


def lanes(x, y, sub, thresh, xdrop):
    """fill.hip's layout in numpy: tasks of 64 adjacent diagonals, lane l on d0 + l, the task stepping along the target rows from
    max(d0, 0) to min(dt - 1, dq - 1 + d0 + 63); a lane is live where 0 <= j < dq and d < dt.  A count pass, an exclusive prefix sum
    and an emit pass that writes from each lane's offset on."""
    x, y, m = np.asarray(x, dtype=np.int64) & 7, np.asarray(y, dtype=np.int64) & 7, np.asarray(sub, dtype=np.int64).reshape(64)
    dt, dq = x.size, y.size
    tasks = [-(dq - 1) + 64 * v for v in range((dt + dq - 1 + 63) // 64)]

    def sweep(off):
        cnt = np.zeros(64 * len(tasks), dtype=np.int64)
        out = {}
        for w, d0 in enumerate(tasks):
            d = d0 + np.arange(64)
            s, b, start, bend, n = (np.zeros(64, dtype=np.int64) for _ in range(5))
            i0 = np.maximum(d, 0)

            def flush(who):
                hit = who & (b >= thresh)
                for l in np.flatnonzero(hit):
                    if off is not None:
                        out[int(off[64 * w + l] + n[l])] = (int(i0[l] + start[l]), int(i0[l] - d[l] + start[l]), int(bend[l] - start[l]), int(b[l]))
                n[hit] += 1
                s[who] = 0
                b[who] = 0

            for i in range(max(d0, 0), min(dt - 1, dq - 1 + d0 + 63) + 1):
                j = i - d
                live = (d < dt) & (j >= 0) & (j < dq)
                yy = y[np.clip(j, 0, dq - 1)]
                sep = live & ((x[i] == 7) | (yy == 7))
                flush(sep)
                go = live & ~sep
                k = i - i0
                fresh = go & (s == 0) & (b == 0)
                start[fresh] = k[fresh]
                s[go] += m[x[i] * 8 + yy][go]
                up = go & (s > b)
                b[up] = s[up]
                bend[up] = k[up]
                flush(go & ((s <= 0) | (b - s > xdrop)))
            flush(np.ones(64, dtype=bool))
            cnt[64 * w:64 * w + 64] = n
        return cnt, out

    cnt, _ = sweep(None)
    off = np.concatenate([[0], np.cumsum(cnt)])
    _, out = sweep(off)
    assert sorted(out) == list(range(int(off[-1])))
    return [out[k] for k in range(len(out))]


@pytest.mark.parametrize("dt,dq", [(1, 1), (1, 63), (32, 32), (33, 32), (64, 64), (1, 129), (129, 1), (70, 200), (200, 70), (65, 65)])
def test_the_kernels_lane_layout_in_numpy_equals_the_checker(dt, dq):
    rng = np.random.default_rng(dt * 1000 + dq)
    x, y = rng.integers(0, 4, dt), rng.integers(0, 4, dq)
    if dt > 40:
        x[dt // 2] = 7
    if dq > 40:
        y[dq // 3] = 7
    for thresh, xdrop in ((90, 100), (300, 200)):
        want = [tuple(int(v) for v in r) for r in F.scan(x, y, SUB, thresh, xdrop)]
        assert lanes(x, y, SUB, thresh, xdrop) == want
        assert len(want) > 0 or dt * dq < 100 or thresh > 90


# ---- the assembly ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world():
    t, q, hsps, W = K.build_world()
    return K.codes(t), K.codes(q), hsps, W


def fill(world, chains, **kw):
    t, q, hsps, _ = world
    members, first = S.csr(chains)
    return F.fill(t, q, SUB, hsps, members, first, **kw)


def invariants(world, chains, res, **kw):
    """What the contract promises of the output as a whole."""
    t, q, hsps, _ = world
    out, first_out, origin, ch, links, found = res
    members, first = S.csr(chains)
    assert first_out[0] == 0 and first_out[-1] == out.size == origin.size
    assert np.array_equal(origin[origin != F.NONE], members) and np.array_equal(out[origin != F.NONE], hsps[members])
    assert int((origin == F.NONE).sum()) == int(links["n_fill"].sum()) == int(ch["fills"].sum())
    for c in range(len(chains)):
        for k in range(int(first_out[c]), int(first_out[c + 1]) - 1):
            assert M.precedes(out, None, k, k + 1)
    assert found.size == int(links["n_hsps"][(links["flags"] & F.CROWDED) == 0].sum())
    for l in np.flatnonzero(links["n_hsps"]):
        assert links["cells"][l] == int(links["dt"][l]) * int(links["dq"][l])


def test_a_chain_with_nothing_to_fill_comes_back_unchanged(world):
    _, _, hsps, W = world
    chains = W["random"][0][:5]
    res = fill(world, chains, thresh=1 << 30)
    members, first = S.csr(chains)
    assert np.array_equal(res[0], hsps[members]) and np.array_equal(res[1], first) and np.array_equal(res[2], members)
    assert np.all(res[3]["fills"] == 0) and np.all(res[4]["n_hsps"] == 0) and res[5].size == 0
    plain = [int(hsps["score"][c].astype(np.int64).sum()) for c in chains]
    assert res[3]["score"].tolist() == plain  # no penalties asked for
    invariants(world, chains, res)


def test_one_fill_several_collinear_fills_and_a_crossing_pair(world):
    _, _, hsps, W = world
    res = fill(world, W["collinear"])
    assert res[4]["n_hsps"].tolist() == [3] and res[4]["n_fill"].tolist() == [3] and res[2].tolist() == [W["collinear"][0][0], F.NONE, F.NONE, F.NONE, W["collinear"][0][1]]
    assert int(res[3]["fill_bases"][0]) == int((res[0]["len"][1:4] + 1).sum()) >= 180
    invariants(world, W["collinear"], res)
    res = fill(world, W["crossing"])
    assert res[4]["n_hsps"].tolist() == [2] and res[4]["n_fill"].tolist() == [1]
    a, b = res[5]
    assert not M.precedes(K.as_seg(res[5]), None, 0, 1) and not M.precedes(K.as_seg(res[5]), None, 1, 0)
    assert int(res[0]["score"][1]) == max(int(a["score"]), int(b["score"]))  # of two that cross, the better one
    invariants(world, W["crossing"], res)
    one = fill(world, W["limits"])
    assert one[4]["n_fill"].tolist() == [1] and one[3]["fills"].tolist() == [1]


def test_min_fill_at_and_above_the_fills_score(world):
    _, _, _, W = world
    score = int(fill(world, W["limits"])[5]["score"][0])
    assert fill(world, W["limits"], min_fill=score)[4]["n_fill"].tolist() == [1]
    res = fill(world, W["limits"], min_fill=score + 1)
    assert res[4]["n_fill"].tolist() == [0] and res[4]["n_hsps"].tolist() == [1] and res[0].size == 2


def test_each_of_the_three_flags(world):
    _, _, _, W = world
    assert fill(world, W["limits"], max_side=100)[4]["flags"].tolist() == [0]
    res = fill(world, W["limits"], max_side=99)
    assert res[4]["flags"].tolist() == [F.LONG] and res[4]["cells"].tolist() == [0] and res[0].size == 2
    assert fill(world, W["limits"], max_cells=6000)[4]["flags"].tolist() == [0]
    assert fill(world, W["limits"], max_cells=5999)[4]["flags"].tolist() == [F.LARGE]
    assert fill(world, W["homopolymer"], thresh=91, max_link_hsps=39)[4][["flags", "n_hsps", "n_fill"]].tolist() == [(0, 39, 1)]
    res = fill(world, W["homopolymer"], thresh=91, max_link_hsps=38)
    assert res[4][["flags", "n_hsps", "n_fill"]].tolist() == [(F.CROWDED, 39, 0)] and res[5].size == 0 and res[0].size == 2


def test_an_empty_chain_a_one_member_chain_and_chains_that_share_an_hsp(world):
    _, _, hsps, W = world
    c = W["collinear"][0]
    chains = [[], [c[0]], c, [], c]
    res = fill(world, chains)
    assert res[1].tolist() == [0, 0, 1, 6, 6, 11] and res[3]["fills"].tolist() == [0, 0, 3, 0, 3]
    assert np.array_equal(res[0][1:6], res[0][6:11]) and res[4].size == 2 and res[5]["link"].tolist() == [0, 0, 0, 1, 1, 1]
    invariants(world, chains, res)
    assert fill(world, [])[1].tolist() == [0]


def test_the_score_charges_the_penalties_between_consecutive_entries(world):
    _, _, _, W = world
    res = fill(world, W["collinear"], diag_pen=2, anti_pen=1)
    out = res[0]
    pen = sum(M.penalty(out, k, k + 1, 2, 1) for k in range(out.size - 1))
    assert pen > 0 and int(res[3]["score"][0]) == int(out["score"].astype(np.int64).sum()) - pen


def test_what_the_contract_refuses(world):
    t, q, hsps, W = world
    c = W["collinear"][0]
    with pytest.raises(ValueError, match="overlaps"):
        fill(world, [[c[1], c[0]]])
    h = hsps.copy()
    h[c[1]]["ref_start"] = t.size - 5
    with pytest.raises(ValueError, match="inside the block"):
        F.fill(t, q, SUB, h, *S.csr([c]))
    big = SUB.copy()
    big[0] = 4000
    with pytest.raises(ValueError, match="headroom"):
        F.fill(t, q, big, hsps, *S.csr([c]), max_side=1 << 20)


# ---- the GPU test's regimes, with the model in the engine's place -------------------------------------------------------------

def test_the_gpu_cases_hold_their_regimes(world):
    t, q, hsps, W = world
    K.regime_sizes(fill(world, W["sizes"], **K.ONE))
    K.regime_tiny(fill(world, W["tiny"], **K.ONE))
    K.regime_past_stitch(fill(world, W["past_stitch"]))
    K.regime_skinny(fill(world, W["skinny"]), hsps, W["skinny"])
    K.regime_edges(fill(world, W["edges"]), hsps, W["edges"])
    K.regime_diagonals(fill(world, W["diagonals"], **K.ONE), hsps, W["diagonals"])
    K.hand_regimes(lambda chains, **kw: fill(world, chains, **kw), W, hsps)
    K.regime_separators(fill(world, W["separators"]), t, q, hsps, W["separators"])
    K.regime_lengths(fill(world, W["lengths"], **K.SMALL))


@pytest.mark.parametrize("k", range(3))
def test_the_gpu_random_sets_hold_their_regimes(world, k):
    _, _, _, W = world
    for chains in W["random"]:
        res = fill(world, chains, **K.RANDOM_PARAMS[k])
        K.regime_random(res, k)
        invariants(world, chains, res)


def test_the_checker_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/cpp/fill_check_main.c), never loaded into Python."""
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    exe = str(tmp_path / "fill_check_san")
    subprocess.check_call([cc, "-g", "-O1", "-std=c99", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "cpp", "fill_check.c"), os.path.join(HERE, "cpp", "fill_check_main.c"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"checksum" in r.stdout and not r.stderr, (r.returncode, r.stdout[-200:], r.stderr[-500:])
