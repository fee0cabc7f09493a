"""CPU: the model of sa_net_subset (tests/net_subset_model.py; contract in include/segalign_amd.h) held to the
consequences the header states, on random sets made with hsp_chain_gap_model.chain_all (hsp_chain_all_model under penalties) and
net_model.net, and on hand-worked cases, one per clause.

In the random sets the query is written from the HSPs (every HSP's target bases copied to its query range, later ones over earlier
ones) and every score field is the HSP's code sum, so that consequence (c) is tested under its own premise."""
import numpy as np
import pytest

import hsp_chain_gap_model as GM
import hsp_chain_model as M
import net_model as N
import net_subset_model as NS
from gapped_model import SUB

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SUB64 = np.asarray(SUB, dtype=np.int64).reshape(64)
THRESHOLDS = [(s, f) for s in (1, 5, 25) for f in (1, 3, 12)]
TABLE = {"pos": [1, 10, 100], "q_gap": [30, 60, 200], "t_gap": [20, 50, 300], "both_gap": [60, 90, 400]}
SEEDS = range(10)
TALLY = ("cut_left", "cut_right", "cut_both", "split", "two_children", "depth2", "whole_chain")


def code_sum(t, q, rs, qs, n):
    return int(SUB64[t[rs:rs + n].astype(np.int64) * 8 + q[qs:qs + n].astype(np.int64)].sum())


def random_input(seed, costs):
    """-> (t codes, q codes, hsps, members, first, chain records, penalties)."""
    rng = np.random.default_rng(900 + seed)
    n = int(rng.integers(60, 140))
    rows = []
    for k in range(n):
        d = int(rng.integers(0, 4)) * 90 + int(rng.integers(-3, 4))
        qs = 20 + k * 6 + int(rng.integers(0, 30))
        rows.append((qs + 400 + d, qs, int(rng.integers(4, 40)), 0))
    h = M.make(rows)[rng.permutation(n)]
    t = ACGT[rng.integers(0, 4, 2200)]
    q = ACGT[rng.integers(0, 4, 1400)]
    for x in h:
        rs, qs, b = int(x["ref_start"]), int(x["query_start"]), int(x["len"]) + 1
        q[qs:qs + b] = t[rs:rs + b]
    t, q = NS.encode(t), NS.encode(q)
    h["score"] = [code_sum(t, q, int(x["ref_start"]), int(x["query_start"]), int(x["len"]) + 1) for x in h]
    pen = dict(diag_pen=int(rng.integers(0, 3)), anti_pen=int(rng.integers(0, 2)), gap_costs=costs)
    g = rng.choice(np.array([5, 2], dtype=np.uint32), size=n)
    _, _, chains, members, _ = GM.chain_all(h, g, max_gap=60, min_score=0, **pen)
    first = np.concatenate([chains["first_member"], [members.size]]).astype(np.uint32)
    return t, q, h, members["hsp_index"].astype(np.uint32), first, chains, pen


_cache = {}


def runs():
    """Every (seed, table, axis, thresholds) once: [(input, axis, thresholds, fills, the model's answer)]."""
    if not _cache:
        out = []
        for seed in SEEDS:
            for costs in (None, TABLE):
                inp = random_input(seed, costs)
                t, q, h, mem, first, chains, pen = inp
                assert 1 <= chains.size <= 60
                for axis in ("target", "query"):
                    bs, be = NS.blocks(h, mem, axis)
                    for ms, mf in THRESHOLDS:
                        fills, _ = N.net(first, bs, be, chains["score"], chains["group"], min_space=ms, min_fill=mf)
                        out.append((inp, axis, (ms, mf), fills, NS.subset(t, q, SUB, h, mem, first, fills, axis=axis, **pen)))
        _cache["runs"] = out
    return _cache["runs"]


def test_the_sets_reach_every_regime_ten_times():
    tally = dict.fromkeys(TALLY, 0)
    for inp, axis, th, fills, (hs, ch, st) in runs():
        chains = inp[5]
        one = ch[ch["n_members"] == 1]
        tally["cut_left"] += int(np.count_nonzero(ch["clipped"] & 1))
        tally["cut_right"] += int(np.count_nonzero(ch["clipped"] & 2))
        tally["cut_both"] += int(np.count_nonzero(one["clipped"] == 3))
        tally["split"] += st["splits"]
        tally["depth2"] += int(np.count_nonzero(fills["depth"] >= 2))
        kids = fills[fills["parent"] >= 0]
        bs, be = NS.blocks(inp[2], inp[3], axis)
        gaps = [(int(k["parent"]), NS.gap_of(k, NS.clipped(fills[int(k["parent"])], bs, be))) for k in kids]
        tally["two_children"] += len(gaps) - len(set(gaps))
        tally["whole_chain"] += sum(1 for c in ch if int(c["clipped"]) == 0 and int(c["n_members"]) == int(chains["n_members"][int(c["chain"])]))
    assert all(v >= 10 for v in tally.values()), tally


def test_a_hulls_of_a_group_are_disjoint_with_the_split_flag():
    without = 0
    for inp, axis, th, fills, (hs, ch, st) in runs():
        assert NS.hulls_disjoint(ch, axis), (axis, th)
        t, q, h, mem, first, chains, pen = inp
        if th == (1, 1):
            without += not NS.hulls_disjoint(NS.subset(t, q, SUB, h, mem, first, fills, axis=axis, split=False, **pen)[1], axis)
    assert without >= 10  # and the flag is what makes them so


def test_b_the_runs_pass_the_stitch_entrys_validation():
    for inp, axis, th, fills, (hs, ch, st) in runs():
        t, q = inp[0], inp[1]
        mem, first = NS.csr(ch)
        assert mem.size == hs.size and first[0] == 0 and np.all(first[1:] > first[:-1])
        rs, qs, n = hs["ref_start"].astype(np.int64), hs["query_start"].astype(np.int64), hs["len"].astype(np.int64) + 1
        assert np.all(rs + n <= t.size) and np.all(qs + n <= q.size)
        inner = np.ones(hs.size - 1, dtype=bool)
        inner[first[1:-1] - 1] = False  # the pairs that straddle two runs
        assert np.all((rs + n)[:-1][inner] <= rs[1:][inner]) and np.all((qs + n)[:-1][inner] <= qs[1:][inner])


def test_c_a_whole_unjoined_chain_in_one_run_scores_the_chains_score():
    seen = 0
    for inp, axis, th, fills, (hs, ch, st) in runs():
        chains = inp[5]
        for c in ch:
            k = int(c["chain"])
            if int(c["clipped"]) or int(c["n_members"]) != int(chains["n_members"][k]):
                continue
            if int(chains["joined"][k]) < 0:  # (a joined chain: test_c_does_not_apply_to_a_joined_chain)
                assert int(c["score"]) == int(chains["score"][k])
                seen += 1
    assert seen >= 100


def test_d_the_kept_bases_partition_the_blocks_at_thresholds_1():
    done = 0
    for inp, axis, th, fills, (hs, ch, st) in runs():
        if th != (1, 1):
            continue
        t, q, h, mem, first, chains, pen = inp
        key = "ref_start" if axis == "target" else "query_start"
        own = [(int(c["group"]), x) for c in ch for m in hs[int(c["first_member"]):int(c["first_member"]) + int(c["n_members"])]
               for x in range(int(m[key]), int(m[key]) + int(m["len"]) + 1)]
        bs, be = NS.blocks(h, mem, axis)
        union = {(int(chains["group"][c]), x) for c in range(chains.size) for b in range(int(first[c]), int(first[c + 1])) for x in range(bs[b], be[b])}
        assert len(own) == len(set(own)) and set(own) == union
        done += 1
    assert done == 2 * 2 * len(SEEDS)


def test_a_cut_member_scores_its_kept_columns_and_moves_both_coordinates():
    for inp, axis, th, fills, (hs, ch, st) in runs()[::7]:
        t, q, h, mem = inp[:4]
        at = 0
        for f in fills:
            for j in range(int(f["n_blocks"])):
                src, x = h[int(mem[int(f["first_block"]) + j])], hs[at]
                d = int(x["ref_start"]) - int(src["ref_start"])
                assert d >= 0 and int(x["query_start"]) - int(src["query_start"]) == d and d + int(x["len"]) <= int(src["len"])
                if int(x["len"]) == int(src["len"]):
                    assert int(x["score"]) == int(src["score"])
                else:
                    assert int(x["score"]) == code_sum(t, q, int(x["ref_start"]), int(x["query_start"]), int(x["len"]) + 1)
                at += 1
        assert at == hs.size


# ---- hand-worked cases ----
T0 = NS.encode(ACGT[np.random.default_rng(1).integers(0, 4, 1000)])
Q0 = T0.copy()


def hand(chains, scores, hsp_scores=None, t=T0, q=Q0, sub=SUB, net_kw={}, **kw):
    """Chains of (start, bases) HSPs on the main diagonal of two equal sequences; -> (hsps, fills, out_hsps, sub-chains, stats)."""
    rows = [(s, s, n, 0) for c in chains for s, n in c]
    h = M.make(rows)
    sub64 = np.asarray(sub, dtype=np.int64).reshape(64)
    h["score"] = [int(sub64[t[s:s + n].astype(np.int64) * 9].sum()) for s, _, n, _ in rows] if hsp_scores is None else hsp_scores
    first = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
    mem = np.arange(h.size, dtype=np.uint32)
    bs, be = NS.blocks(h, mem, "target")
    fills, _ = N.net(first, bs, be, np.asarray(scores, dtype=np.int64), None, **net_kw)
    return (h, fills) + NS.subset(t, q, sub, h, mem, first, fills, **kw)


COMB = [(100, 20), (200, 20), (300, 20), (400, 20)]


@pytest.mark.parametrize("split,members", [(True, [2, 2, 1]), (False, [4, 1])])
def test_split_on_and_split_off(split, members):
    h, fills, hs, ch, st = hand([COMB, [(250, 30)]], [9, 1], split=split, anti_pen=1)
    assert ch["n_members"].tolist() == members and ch["run"].tolist() == ([0, 1, 0] if split else [0, 0]) and st["splits"] == int(split)
    whole = int(h["score"][:4].astype(np.int64).sum()) - 3 * 160
    if split:
        assert int(ch["score"][0]) + int(ch["score"][1]) == whole + 160  # the link over the child's gap is no longer paid
        assert ch[["ref_start", "ref_end"]].tolist() == [(100, 220), (300, 420), (250, 280)]
    else:
        assert int(ch["score"][0]) == whole and ch[["ref_start", "ref_end"]].tolist() == [(100, 420), (250, 280)]


@pytest.mark.parametrize("at,members", [(130, [1, 3, 1]), (330, [3, 1, 1])])
def test_a_child_in_the_first_and_in_the_last_gap(at, members):
    h, fills, hs, ch, st = hand([COMB, [(at, 30)]], [9, 1])
    assert ch["n_members"].tolist() == members and st["splits"] == 1 and NS.hulls_disjoint(ch)


def test_a_gap_below_min_space_gives_no_split():
    h, fills, hs, ch, st = hand([COMB, [(230, 30)]], [9, 1], net_kw=dict(min_space=81))
    assert fills.size == 1 and ch["n_members"].tolist() == [4] and st["splits"] == 0
    h, fills, hs, ch, st = hand([COMB, [(230, 30)]], [9, 1], net_kw=dict(min_space=80))
    assert fills.size == 2 and st["splits"] == 1


def test_a_cut_members_score_is_clamped_to_int32_in_the_hsp_only():
    big = np.full(64, 3_000_000, dtype=np.int64)
    h, fills, hs, ch, st = hand([[(100, 50)], [(120, 800)]], [9, 1], sub=big, hsp_scores=[7, 8])
    assert st["cut_members"] == 1 and int(hs["len"][1]) + 1 == 770 and int(hs["score"][1]) == 2 ** 31 - 1
    assert int(ch["score"][1]) == 770 * 3_000_000 > 2 ** 31 and int(ch["clipped"][1]) == 1 and int(hs["score"][0]) == 7
    h, fills, hs, ch, st = hand([[(100, 50)], [(120, 800)]], [9, 1], sub=-big, hsp_scores=[7, 8])
    assert int(hs["score"][1]) == -2 ** 31 and int(ch["score"][1]) == -770 * 3_000_000


def test_c_does_not_apply_to_a_joined_chain():
    h = M.make([(100, 100, 50, 1000), (200, 200, 50, 900), (160, 300, 30, 500)])
    _, _, chains, members, _ = GM.chain_all(h, None, diag_pen=1)
    assert chains["n_members"].tolist() == [2, 1] and chains["joined"].tolist() == [-1, 0] and chains["score"].tolist() == [1900, 360]
    mem = members["hsp_index"].astype(np.uint32)
    first = np.array([0, 2, 3], dtype=np.uint32)
    bs, be = NS.blocks(h, mem, "target")
    fills, _ = N.net(first, bs, be, chains["score"])
    hs, ch, st = NS.subset(T0, Q0, SUB, h, mem, first, fills, diag_pen=1)
    assert fills["parent"].tolist() == [-1, 0] and ch["score"].tolist() == [1000, 900, 500] and ch["chain"].tolist() == [0, 0, 1]
    assert int(ch["score"][2]) != int(chains["score"][1])  # 500, not 360: the link the chain was cut at is not in the fill


@pytest.mark.parametrize("edit,clause", [
    (lambda a: a["fills"]["start"].__setitem__(0, 500), "fill extent"),
    (lambda a: a["fills"]["chain"].__setitem__(0, 2), "fill chain"),
    (lambda a: a["fills"]["n_blocks"].__setitem__(0, 5), "fill blocks"),
    (lambda a: a["fills"]["first_block"].__setitem__(1, 3), "fill blocks"),
    (lambda a: a["fills"]["start"].__setitem__(0, 120), "fill edge blocks"),
    (lambda a: a["fills"]["parent"].__setitem__(1, 1), "fill parent"),
    (lambda a: (a["fills"]["end"].__setitem__(0, 120), a["fills"]["n_blocks"].__setitem__(0, 1)), "fill gap"),
    (lambda a: a["first"].__setitem__(0, 1), "first"),
    (lambda a: a["hsps"]["ref_start"].__setitem__(1, 110), "collinear"),
    (lambda a: a["hsps"]["len"].__setitem__(3, 900), "member outside the block"),
    (lambda a: a.__setitem__("diag_pen", (1 << 20) + 1), "penalty"),
    (lambda a: a.__setitem__("gap_costs", {"pos": [2, 2], "q_gap": [1, 2], "t_gap": [1, 2], "both_gap": [1, 2]}), "pos"),
])
def test_every_validation_clause(edit, clause):
    h, fills, _, _, _ = hand([COMB, [(250, 30)]], [9, 1])
    a = dict(hsps=h.copy(), members=np.arange(5, dtype=np.uint32), first=np.array([0, 4, 5], dtype=np.uint32), fills=fills.copy(), diag_pen=0,
             gap_costs=None)
    NS.validate(T0, Q0, **a)
    edit(a)
    with pytest.raises(ValueError, match=clause):
        NS.validate(T0, Q0, **a)


def test_the_rendering_of_the_chains_file():
    h, fills, hs, ch, st = hand([COMB, [(250, 30)]], [9, 1])
    text = NS.render_chains(hs, ch, True, ["tA", "tB"], [0, 290], ["q1"], [0])
    lines = text.splitlines()
    assert len(lines) == 3 + 5 and lines[0] == "#chain 0 fill=0 run=0 score=%d tA 101 220 q1 101 220 -" % int(ch["score"][0])
    assert lines[3] == "#chain 1 fill=0 run=1 score=%d tB 11 130 q1 301 420 -" % int(ch["score"][1])
    assert lines[4] == "tB\t11\t30\tq1\t301\t320\t-\t%d" % int(hs["score"][2])
