"""CPU: tests/extend_model.py equals the oracle's ungapped extension -- scalar, and tiled at widths 8 and 64 -- on every anchor of every
parameter set of tests/extend_regimes.py, examined bases included, and every regime is in the state it names, read off the model
alone: tests/test_gpu_extend_regimes.py cannot pass quietly on an input that misses its edge."""
import numpy as np
import pytest

import extend_model as M
import extend_regimes as R
from helpers import Case


@pytest.fixture(scope="module")
def sets(oracle):
    return {s.name: s.resolve(oracle) for s in R.SETS + R.ENTROPY_SETS}


def hoxd(oracle):
    return tuple(int(x) for x in oracle.build_sub_mat(910))


def fact(e, key):
    return e.total if key == "total" else getattr(getattr(e, key[0]), key[1])


NAMES = [s.name for s in R.SETS + R.ENTROPY_SETS]


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_scalar_and_tiled(oracle, sets, name):
    s = sets[name]
    p, anchors = s.pair, s.pair.bulk()
    exts = M.extend_all(p.ref, p.qry, s.mat, anchors, s.xdrop, s.hspthresh)
    assert len(exts) == anchors.shape[0]
    for (r, q), e in zip(anchors.tolist(), exts):
        ok, rec, examined = oracle.extend_hit(p.ref, p.qry, s.mat, r, q, xdrop=s.xdrop, hspthresh=s.hspthresh, noentropy=True)
        want = tuple(int(x) & 0xFFFFFFFF for x in e.rec[:3]) + (e.total,) if e.passed else (r, q, 0, 0)
        assert (ok, rec, examined) == (e.passed, want, e.examined), (name, r, q, e.R, e.L)
        for w in (8, 64):
            ok_t, rec_t, _ = oracle.extend_hit(p.ref, p.qry, s.mat, r, q, xdrop=s.xdrop, hspthresh=s.hspthresh, noentropy=True, tiled=w)
            assert (ok_t, rec_t) == (ok, rec), (name, w, r, q)


@pytest.mark.parametrize("name", ["W", "F", "H hoxd70", "B both ends"])
def test_every_regime_is_in_the_state_it_names(sets, name):
    s = sets[name]
    p = s.pair
    assert p.ref.size <= 65536 and p.qry.size <= 65536
    exts = M.extend_all(p.ref, p.qry, s.mat, p.anchors(), s.xdrop, s.hspthresh)
    i, checked = 0, 0
    for g in p.regs:
        e = exts[i]
        i += len(g.anchors)
        for key, want in g.facts.items():
            assert fact(e, key) == want, (g, key, want, e.R, e.L)
            checked += 1
    assert checked > 2 * len(p.regs)


def test_wave_queue_inputs_hold_the_largest_call(sets):
    for name in ("W", "F"):
        assert sets[name].pair.bulk().shape[0] >= max(R.QUEUE_SIZES)


def test_both_walks_meet_a_real_sequence_end(sets):
    s = sets["B both ends"]
    p = s.pair
    seen = {"target start": set(), "query start": set()}
    for g in p.regs:
        e = first(p, s, g)
        r, q = g.anchors[0]
        assert e.L.edge and e.R.edge and e.L.last == e.L.best and e.R.last == e.R.best, g
        l, rr = e.L.stop - 1, e.R.stop
        if g.name.startswith("target start"):      # the left walk runs out of target, the right walk out of query
            assert r == l and q + rr == p.qry.size and q > l and r + rr < p.ref.size
        else:
            assert q == l and r + rr == p.ref.size and r > l and q + rr < p.qry.size
        assert e.passed == (100 * (l + rr) >= s.hspthresh)
        seen["target start" if g.name.startswith("target start") else "query start"].add((l, rr))
    want = {(a, b) for a in R.LIMS for b in R.LIMS}
    assert seen["target start"] == want and seen["query start"] == want


def names_of(p, word):
    return [g for g in p.regs if word in g.name]


def first(p, s, g):
    return M.extend_all(p.ref, p.qry, s.mat, [g.anchors[0]], s.xdrop, s.hspthresh)[0]


def test_runs_put_the_best_on_both_sides_of_every_window_and_lane_edge(sets):
    for name, need in (("W", {6, 7, 8, 510, 511, 512, 513, 1023, 1024, 1535}), ("H hoxd70", {7, 8, 511, 512, 513, 1024})):
        s = sets[name]
        right = {first(s.pair, s, g).R.pos for g in names_of(s.pair, "run") if "right" in g.name}
        left = {first(s.pair, s, g).L.pos for g in names_of(s.pair, "run") if "left" in g.name}
        assert need <= right and need <= left and {n + 1 for n in need if n > 500} <= left        # (the left side's windows start at k = 1)
        both = [first(s.pair, s, g) for g in names_of(s.pair, "both@")]
        assert {(e.L.pos, e.R.pos) for e in both} >= {(512, 511), (513, 510)} and all(e.L.pos > 0 and e.R.pos >= 0 for e in both)


def test_dips_of_xdrop_go_on_and_dips_of_xdrop_plus_one_stop(sets):
    for name in ("W", "H hoxd70"):
        s = sets[name]
        bottoms = {"R": set(), "L": set()}
        for g in names_of(s.pair, "dip"):
            e = first(s.pair, s, g)
            for side, x in (("R", e.R), ("L", e.L)):
                if (side, "dip") in g.facts:          # exactly xdrop: survived, and the best lies behind the dip
                    assert x.dip == s.xdrop and x.pos > x.dip_at and e.rec[2] > x.dip_at
                    bottoms[side].add(x.dip_at)
                if (side, "stop") in g.facts:         # xdrop + 1: stopped on the bottom itself, the best before the dip
                    assert not x.edge and x.pos < x.stop - 9 and x.dip <= s.xdrop
                    bottoms[side].add(-x.stop)
        # lane edges of the exact kernel (8m - 1 | 8m, left 8m | 8m + 1), its window edge, the packed filter's 16-base test points
        assert {23, 24, 511, 512, 15, 16, 17, 63, 64, 65} <= bottoms["R"] and {24, 25, 512, 513, 16, 17, 64, 65} <= bottoms["L"]
        assert {-23, -24, -511, -512, -15, -16} <= bottoms["R"] and {-24, -25, -512, -513, -16, -17} <= bottoms["L"]


def test_ties_report_the_earlier_position_and_their_twins_the_later(sets):
    for name in ("W", "H hoxd70"):
        s = sets[name]
        pairs = {"R": set(), "L": set()}
        for g in names_of(s.pair, "tie"):
            e = first(s.pair, s, g)
            for side, x in (("R", e.R), ("L", e.L)):
                if g.facts.get((side, "ties")):
                    assert x.ties[0] > x.pos and "twin" not in g.name
                    pairs[side].add((x.pos, x.ties[0]))
                elif (side, "ties") in g.facts:
                    assert x.ties == [] and "twin" in g.name
        lane = lambda k, side: (k - (side == "L")) // 8
        for side in "RL":
            lanes = {(lane(a, side), lane(b, side)) for a, b in pairs[side]}
            assert {(15, 16), (63, 64)} <= lanes and any(a + 1 == b and a < 15 for a, b in lanes)     # rows 0|1, windows 0|1, neighbours
            if name == "W":
                assert (31, 32) in lanes and any(a == b for a, b in lanes)


def test_sequence_ends_are_met_at_the_best(sets):
    s = sets["W"]
    p = s.pair
    for word, side in (("start both ends", "L"), ("start query ends", "L"), ("start target ends", "L"), ("end query ends", "R"),
                       ("end target ends", "R"), ("end both ends", "R"), ("E right", "R"), ("E left", "L")):
        lims = set()
        for g in names_of(p, word):
            e = first(p, s, g)
            x = e.R if side == "R" else e.L
            assert x.last == x.best and x.edge == (not word.startswith("E ")), g
            lims.add(x.stop - (side == "L"))
            r, q = g.anchors[0]
            if word == "start query ends":
                assert q == x.stop - 1 and r > q
            if word == "start target ends":
                assert r == x.stop - 1 and q > r
            if word == "end query ends":
                assert q + x.stop == p.qry.size and r + x.stop < p.ref.size
            if word == "end target ends":
                assert r + x.stop == p.ref.size and q + x.stop < p.qry.size
        assert lims == set(R.LIMS), word
    a = {tuple(x) for x in p.anchors().tolist()}
    assert (0, 0) in a and (p.ref.size, p.qry.size) in a
    assert any(r == p.ref.size and q < p.qry.size for r, q in a) and any(q == 0 and r > 0 for r, q in a)
    assert any(q == p.qry.size and r < p.ref.size for r, q in a) and any(r == 0 and q > 0 for r, q in a)


def test_thresholds_caps_and_switches(oracle, sets):
    s = sets["F"]
    p, h = s.pair, s.hspthresh
    tot = {}
    for g in names_of(p, "total"):
        e = first(p, s, g)
        assert e.passed == (e.total >= h) and e.total in (h - 1, h)
        tot.setdefault(e.total, []).append((e.R.best, e.L.best))
    assert all(any(a == 0 for a, b in v) and any(b == 0 for a, b in v) and any(b == h // 2 for a, b in v) for v in tot.values()) and len(tot) == 2
    # alive for exactly n bases: a candidate of the byte-coded filter whatever its total iff n >= long_cap
    for cap in R.CAPS:
        seen = set()
        for g in names_of(p, "alive"):
            e = first(p, s, g)
            n = int(g.name.split()[1])
            if n in (cap - 8, cap, cap + 8):
                other = e.L.stop - 1 if "right" in g.name else e.R.stop        # (the side that supplies the total is alive for a while too)
                assert M.is_candidate(e, h, cap) == (n >= cap or e.total >= h or other >= cap), (g, cap)
                seen.add((n, e.total, "right" in g.name))
        assert len(seen) == 12
        for g in names_of(p, "lone"):
            e = first(p, s, g)
            n = int(g.name.split()[1])
            assert e.total < h and M.is_candidate(e, h, cap) == (n >= cap), (g, cap)
    # the chunk-edge drop: at xdrop 700 / 600 the walk ends on the first base of a chunk, seven matches follow, the best stays
    for xdrop, word in ((700, "drop 701"), (600, "drop 601")):
        for g in names_of(p, word):
            e = M.extend_all(p.ref, p.qry, s.mat, [g.anchors[0]], xdrop, h)[0]
            x = e.R if g.name.endswith("R") else e.L
            k = x.stop - (not g.name.endswith("R"))
            assert not x.edge and k % 8 == 0 and x.pos == x.stop - (xdrop // 100 + 1) and x.dip == xdrop
            if e.total < h:
                assert e.total == h - 1 and not M.is_candidate(e, h, 128)
    # the switches of the three eligibility tests
    mx = lambda name: int(np.max(sets[name].mat))
    assert 7 * mx("F xdrop 700") == sets["F xdrop 700"].xdrop == sets["F xdrop 699"].xdrop + 1
    assert mx("F max 127") * 128 == 16256 and mx("F max 128") * 128 == 16384 and sets["F xdrop 16383"].xdrop + 1 == sets["F xdrop 16384"].xdrop == 16384
    assert int(np.min(sets["H separator below int16, xdrop 5000"].mat)) < -16383 and int(np.min(s.mat)) < -16383
    codes = {int(p.ref[g.anchors[0][0] + (15 if g.name.endswith("R") else -16)]) for g in names_of(p, "in island")}
    assert codes == {R.L, R.N, R.X}                                       # codes above 3 in the TARGET, inside the island
    assert np.all(p.qry < 4) and np.all(sets["W"].pair.qry < 4)         # (the reverse strand of the rev set holds ACGT alone)


def test_entropy_islands(oracle, sets):
    s = sets["F entropy 3099"]
    p = s.pair
    verdict = {}
    for k, a in p.entropy.items():
        on = oracle.extend_hit(p.ref, p.qry, s.mat, a[0], a[1], xdrop=s.xdrop, hspthresh=s.hspthresh, noentropy=False)
        off = oracle.extend_hit(p.ref, p.qry, s.mat, a[0], a[1], xdrop=s.xdrop, hspthresh=s.hspthresh, noentropy=True)
        verdict[k] = (on[0], off[0], off[1][3])
    assert verdict["band"] == (False, True, 3 * s.hspthresh) and verdict["above"] == (True, True, 3 * s.hspthresh + 1)
    assert verdict["balanced"][1:] == (True, s.hspthresh)


def test_chain_cases(sets):
    s = sets["F"]
    p = s.pair
    r, q, m = M.as_lists(p.ref, p.qry, s.mat)
    got = {}
    for name, anchors in p.chain_cases:
        exts = M.extend_all(p.ref, p.qry, s.mat, anchors, s.xdrop, s.hspthresh)
        assert all(e.passed for e in exts), name                   # every one a candidate
        recs = M.chain_records(p.ref, p.qry, s.mat, anchors, s.xdrop, s.hspthresh)
        every = M.records(exts)
        assert {tuple(x) for x in recs.tolist()} == {tuple(x) for x in every.tolist()}
        got[name] = (recs.size, len({tuple(x) for x in every.tolist()}), exts)
        assert len({int(b) >> 9 for a, b in anchors.tolist()}) == (2 if "windows" in name else 1)
    n = {k: v[0] for k, v in got.items()}
    assert n["b at right end"] == 1 and n["b past right end"] == 2 and got["b past right end"][1] == 1
    e = got["b at right end"][2]
    assert p.chain_cases[0][1][1][0] == p.chain_cases[0][1][0][0] + e[0].R.pos           # b exactly on a's best right end
    assert n["gap 256"] == 1 and n["gap 257"] == 2
    assert n["new best at gap + 96"] == 1 and n["new best at gap + 97"] == 2 and got["new best at gap + 97"][1] == 1
    assert n["strict"] == 2 and got["strict"][1] == 2                                     # two different records, both owed
    a, b = got["strict"][2][1], got["strict"][2][0]
    assert b.L.ties and b.L.ties[0] > 43 and a.rec[0] < b.rec[0]                          # b ties its best before a; a's own walk goes further
    assert n["best at a"] == 2 and got["best at a"][1] == 1
    assert n["windows 511|512"] == 2 and n["duplicates"] == 3
    for e_at in (63, 64, 65):
        k = "run beyond@%d" % e_at
        anchors = dict(p.chain_cases)[k]
        assert anchors.shape[0] == 130 and got[k][2][0].R.pos == e_at - 1 and 2 < n[k] < 130
        srt = [tuple(x) for x in anchors.tolist()]
        heads = [M.chain_is_head(r, q, m, srt[j], srt[j - 1], s.xdrop) for j in range(1, 130)]
        assert not any(heads)                                                             # one run: members are promoted, none is flagged
    # the two windows of the 511|512 case fall into different buckets of the 16384 the device picks for a small call
    (r1, q1), (r2, q2) = dict(p.chain_cases)["windows 511|512"].tolist()
    bucket = lambda r_, q_: ((((r_ - q_) * 2654435761) & 0xFFFFFFFF) ^ (((q_ >> 9) * 0x85EBCA6B) & 0xFFFFFFFF)) >> 14 & 16383
    assert q1 % 512 == 511 and bucket(r1, q1) != bucket(r2, q2)


def test_class_filter_pair(oracle):
    p = R.pair_c(hoxd(oracle))
    exts = M.extend_all(p.ref, p.qry, p.mat, p.anchors(), p.xdrop, p.hspthresh)
    kept = [e.total for g, e in zip(p.regs, exts) if g.facts.get("kept") is True]
    lost = [e.total for g, e in zip(p.regs, exts) if g.facts.get("kept") is False]
    assert kept and set(kept) == {p.hspthresh} and len(lost) >= 10 and all(t < p.hspthresh for t in lost) and p.hspthresh - 1 in lost
    # drops at every right offset up to 54 and every left offset up to 78 from some seed position: runs of >= 100 bases before and behind them
    assert sum(1 for g in p.regs if "long dip" in g.name) == 4 and all(g.facts["span"][1] >= 210 for g in p.regs if "long dip" in g.name)
    # what the table-direct calls are held to: the oracle's own output has every island at hspthresh and none at hspthresh - 1
    c = Case(p.target_ascii(), p.query_ascii(), chunk=60000, noentropy=True).oracle_setup(oracle)
    (s0, e0), = c.chunks()
    out = c.oracle_saf(c.host_seeds(s0, e0, False), False)[0][1:]
    have = {tuple(int(x) for x in r) for r in out.tolist()}
    starts = out["ref_start"].astype(np.int64)
    for g, e in zip(p.regs, exts):
        if g.facts.get("kept") is True:
            assert tuple(e.rec) in have, g
        elif g.facts.get("kept") is False:
            lo, n = g.facts["span"]
            assert not np.any((starts >= lo) & (starts < lo + n)), g
