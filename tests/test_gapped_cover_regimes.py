"""CPU: the inputs of tests/gapped_cover_regimes.py are in the regimes they name, shown on the serial checkers and the index model alone,
so that tests/test_gpu_gapped_cover_regimes.py cannot pass quietly on an input that misses its target."""
import numpy as np
import pytest

import gapped_cover_regimes as CR
import gapped_greedy_model as GR
import gapped_trace_model as T


def states(reg):
    return reg.want()[2]["state"]


def test_rows_have_lengths_of_both_parities():
    h = CR.ladder().hsps
    assert np.all(h["len"] > 0) and set((h["len"] % 2).tolist()) == {0, 1}
    assert all(GR.anchor(x) != (int(x["ref_start"]), int(x["query_start"])) for x in h)


# ---- ends -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["runs", "path"])
def test_ends_probes_are_where_their_names_say(part):
    reg = CR.ends(part)
    cover, st = reg.cover_of(0), states(reg)
    assert st[0] == 1
    runs = reg.meta["runs"]
    for side in "LR":  # an I run and a D run on each side
        assert {T.OP_I, T.OP_D} <= {r[2] for r in runs if r[0] == side}
    inside = {"first", "last"}
    for name, (k, on) in reg.meta["probes"].items():
        a = GR.anchor(reg.hsps[k])
        assert on == (a in cover) == (name.split("_", 1)[1] in inside), name
        # every probe's own alignment is eligible, so "not covered" shows as "returned"; no probe covers another uncovered one
        assert reg.raw()[0][k]["score"] >= reg.thresh and st[k] == (2 if on else 1), name
    sides = {n.split("_")[0] for n in reg.meta["probes"]}
    assert sides == ({"L", "R"} if part == "runs" else {"path"})
    if part == "runs":
        assert {"L_in_I", "L_in_D", "R_in_I", "R_in_D", "L_end", "R_end", "L_before", "R_before"} <= set(reg.meta["probes"])
        for s in "LR":  # the end point is one past the last pair on its diagonal; the neighbours share t with the pair
            a = {n: GR.anchor(reg.hsps[reg.meta["probes"][s + "_" + n][0]]) for n in ("last", "end", "last_up", "last_down")}
            assert a["end"] == (a["last"][0] + 1, a["last"][1] + 1)
            assert a["last_up"] == (a["last"][0], a["last"][1] + 1) and a["last_down"] == (a["last"][0], a["last"][1] - 1)


# ---- carry ------------------------------------------------------------------------------------------------------------------------------

def test_carry_sides_have_three_chunks_and_a_probe_pair_in_each():
    reg = CR.carry()
    assert min(reg.meta["n_runs"].values()) >= 130
    recs, paths = reg.raw()
    assert (paths[0][0].size, paths[0][1].size) == (reg.meta["n_runs"]["L"], reg.meta["n_runs"]["R"])
    cover, st = reg.cover_of(0), states(reg)
    seen = set()
    for (side, chunk, walk, on), k in reg.meta["probes"].items():
        assert walk // 64 == chunk and on == (GR.anchor(reg.hsps[k]) in cover) and st[k] == (2 if on else 1)
        # the walk index counts from the far end: the left ops are in walk order, the right ops reversed
        ops = paths[0][0] if side == "L" else paths[0][1][::-1]
        assert int(ops[walk]) & 3 == T.OP_M
        seen.add((side, chunk, on))
    assert seen == {(s, c, on) for s in "LR" for c in (0, 1, 2) for on in (True, False)}


def test_carry_sides_of_63_64_and_65_runs():
    ext = CR.carry_edge_extents()
    assert sorted(ext) == [63, 64, 65]
    for n, (gap, e) in ext.items():
        reg = CR.carry(e, (0, 1), gap)
        assert reg.meta["n_runs"]["R"] == n == reg.raw()[1][0][1].size
        st, cover = states(reg), reg.cover_of(0)
        assert any(s == "R" and c == 0 for s, c, _, _ in reg.meta["probes"])
        for (side, chunk, walk, on), k in reg.meta["probes"].items():
            assert on == (GR.anchor(reg.hsps[k]) in cover) and st[k] == (2 if on else 1)


# ---- nesting ----------------------------------------------------------------------------------------------------------------------------

def test_nesting_tells_the_running_maximum_from_the_own_end():
    reg = CR.nesting()
    st = states(reg)
    assert st[0] == st[1] == 1
    recs, paths = reg.raw()
    assert [int(x) for x in paths[1][0]] == [997 << 2 | T.OP_M, 3 << 2 | T.OP_D]
    assert [int(x) for x in paths[1][1]] == [3 << 2 | T.OP_I, 997 << 2 | T.OP_M]
    ix = CR.Index(CR.accepted_segments(reg, [0, 1]))
    keys = ix.keys()
    assert keys.count((0, 2500)) == 2 and keys.count((0, 3500)) == 3  # equal keys with different ends: nested segments
    cover = reg.cover_of(0) | reg.cover_of(1)
    differ, agree_in, agree_out = [], [], []
    for k in reg.meta["probes"]:
        a = GR.anchor(reg.hsps[k])
        assert ix.covered(a) == (a in cover), a
        if a in cover:
            assert st[k] == 2
        (differ if ix.covered(a) != ix.covered_own_end(a) else agree_in if a in cover else agree_out).append(a[0])
    assert {3498, 3499, 3503, 3800, 4499} <= set(differ) and agree_in and agree_out, (differ, agree_in, agree_out)
    assert all(not ix.covered_own_end((t, t)) for t in differ)
    # at a batch size of 2 the probes come in later batches than both accepted alignments
    assert CR.batches(reg, 2)[0] == [0, 1]


# ---- merge ------------------------------------------------------------------------------------------------------------------------------

def test_merge_later_batches_repeat_keys_and_interleave():
    reg = CR.merge()
    st = states(reg)
    a, c, b, d = reg.meta["mains"]
    assert st[a] == st[c] == st[b] == st[d] == 1
    for B in (1, 2):
        where = [next(n for n, bt in enumerate(CR.batches(reg, B)) if k in bt) for k in (a, c, b, d)]
        assert where[0] < where[1] < where[2] < where[3]
    seg = {k: CR.accepted_segments(reg, [k]) for k in (a, c, b, d)}
    key = {k: {(d, tb): te for d, tb, te in seg[k] if te > tb + 1} for k in seg}
    resident = dict(key[a])
    resident.update(key[c])
    tied = [(kk, resident[kk], te) for kk, te in key[b].items() if kk in resident]
    assert any(old < new for _, old, new in tied) and any(old > new for _, old, new in tied), tied
    # where the later batches' keys fall among the resident ones: before the first, after the last and in between
    pos = set()
    for res, new in ((sorted(key[a]), key[c]), (sorted(resident), key[b]), (sorted({**resident, **key[b]}), key[d])):
        for kk in new:
            pos.add("before" if kk < res[0] else "after" if kk > res[-1] else "between")
    assert pos == {"before", "between", "after"}
    # probes that only the longer run of a tied pair covers
    anchors = reg.anchors()
    for kk, old, new in tied:
        if old != new:
            lo, hi = min(old, new), max(old, new)
            assert any(kk[0] == p[0] - p[1] and lo <= p[0] < hi for p in (anchors[k] for k in reg.meta["probes"])), kk
    assert {1, 2} <= set(st[reg.meta["probes"]].tolist())


# ---- ladder -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True])
def test_ladder_alternates_along_a_chain_of_dependencies(mirror):
    reg = CR.ladder(mirror)
    st = states(reg)
    pi = GR.priority(reg.hsps)
    assert pi == (list(range(CR.LADDER_N))[::-1] if mirror else list(range(CR.LADDER_N)))
    assert st[pi].tolist() == [1, 2] * (CR.LADDER_N // 2)
    anchors = reg.anchors()
    covers = [reg.cover_of(k) for k in range(CR.LADDER_N)]
    for n, k in enumerate(pi):
        on = [pi[m] for m in range(n) if anchors[k] in covers[pi[m]]]
        assert on == ([pi[n - 1]] if n else [])  # only on its predecessor's path: covered by it, or free because that one is covered
    assert CR.LADDER_N > 2 * 64 and all(r["score"] >= reg.thresh for r in reg.raw()[0])


# ---- fans -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rank", [None, 0, 1, 2])
def test_fan_in_edges(rank):
    reg = CR.fan(rank)
    st, m = states(reg), reg.meta
    anchors, pi = reg.anchors(), GR.priority(reg.hsps)
    assert pi[0] == m["top"] and pi[-1] == m["last"] and anchors[m["last"]] not in reg.cover_of(m["top"])
    owners = [k for k in range(reg.hsps.size) if k != m["last"] and anchors[m["last"]] in reg.cover_of(k)]
    eligible = [k for k in owners if reg.raw()[0][k]["score"] >= reg.thresh]
    assert len(eligible) >= 65 and set(m["owners"]) <= set(eligible)
    assert all(st[k] == 2 for k in m["owners"])
    accepted = [k for k in owners if st[k] == 1]
    if rank is None:
        assert accepted == [] and st[m["last"]] == 1
    else:
        assert accepted == [m["extra"]] and st[m["last"]] == 2
        among = sorted(eligible, key=pi.index).index(m["extra"])
        assert among == (0, len(eligible) // 2, len(eligible) - 1)[rank]


# ---- thresh -----------------------------------------------------------------------------------------------------------------------------

def test_thresh_states():
    reg = CR.thresh()
    st, m = states(reg), reg.meta
    score = reg.raw()[0]["score"]
    weak = [m["on_path"][0], m["on_path"][1], m["weak_first"], *m["dup"]]
    assert all(score[k] < reg.thresh for k in weak) and all(score[k] >= reg.thresh for k in (*m["strong"], m["strong_after"]))
    assert reg.want()[2]["below_thresh"] >= 2
    anchors = reg.anchors()
    # (a) duplicates below the threshold: none covers the other
    assert anchors[m["dup"][0]] == anchors[m["dup"][1]] and [st[k] for k in m["dup"]] == [0, 0]
    # (b) weak anchors on an accepted path are covered, in the coverer's batch and in a later one
    bt = CR.batches(reg, 2)
    for w, s, same in zip(m["on_path"], m["strong"], (True, False)):
        assert st[s] == 1 and anchors[w] in reg.cover_of(s) and st[w] == 2
        assert (next(n for n, x in enumerate(bt) if w in x) == next(n for n, x in enumerate(bt) if s in x)) == same
    # (c) a strong anchor on a weak alignment's path only
    pi = GR.priority(reg.hsps)
    before = [k for k in pi[:pi.index(m["strong_after"])] if anchors[m["strong_after"]] in reg.cover_of(k)]
    assert before == [m["weak_first"]] and st[m["weak_first"]] == 0 and st[m["strong_after"]] == 1


# ---- ties -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_ties_go_to_the_lower_index(seed):
    reg = CR.ties(seed)
    st = states(reg)
    anchors = reg.anchors()
    for g, grp in enumerate(reg.meta["groups"]):
        assert len(set(reg.hsps[grp]["score"].tolist())) == 1
        assert sorted(grp) != grp or g >= 3 or len(grp) == 2  # scattered
        for k in grp:
            assert all(anchors[k] in reg.cover_of(j) for j in grp)  # each on every other's path
            assert st[k] == (1 if k == min(grp) else 2)
        if g < 3:
            assert len({tuple(reg.hsps[k].tolist()) for k in grp}) == 1
        else:
            assert anchors[grp[0]] != anchors[grp[1]]
    assert any(min(grp) != grp[0] for grp in reg.meta["groups"][3:]) or seed  # the shuffle reverses at least one pair


# ---- gapanc -----------------------------------------------------------------------------------------------------------------------------

def test_gapanc_anchor_is_no_m_pair():
    reg = CR.gapanc()
    recs, paths = reg.raw()
    a = GR.anchor(reg.hsps[0])
    assert int(paths[0][1][0]) & 3 == T.OP_D  # the right side begins with a gap at the anchor
    pairs = GR.cover_set(recs[0], np.concatenate(paths[0][:2]), (-1, -1)) - {(-1, -1)}
    assert a not in pairs and a in reg.cover_of(0)
    assert states(reg).tolist() == [1, 2]
    assert (a[0] - a[1], a[0], a[0] + 1) in CR.accepted_segments(reg) and not CR.Index(
        [s for s in CR.accepted_segments(reg) if s != (a[0] - a[1], a[0], a[0] + 1)]).covered(a)
