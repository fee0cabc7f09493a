"""CPU: the model of sa_net_classify (tests/net_class_model.py; contract in include/segalign_amd.h) held to the consequences
the header states, on random sets made with hsp_chain_gap_model.chain_all and net_model.net with both strands in one net
(tests/net_class_cases.py), and on hand-worked cases, one per clause.  The package's two pure-numpy helpers, net_other_blocks and
net_select, are held to their twins in the model here too: they need no device."""
import numpy as np
import pytest

import net_class_cases as K
import net_class_model as NC
import net_model as N
import net_subset_model as NS
from segalign_amd import engine as E

SEEDS = range(12)
TALLY = ("top", "syn", "inv", "nonSyn", "oover", "ofar", "odup", "odup_is_ali", "dropped_with_kept_siblings", "dropped_subtree_depth2")
_cache = {}


def runs():
    """Every (seed, thresholds) once: [(input, blocks, fills, classes without a filter, filter, classes with it)]."""
    if not _cache:
        out = []
        for seed in SEEDS:
            inp = K.random_input(seed)
            assert 1 <= inp["score"].size <= 60 and 2 <= np.unique(inp["ogroup"]).size <= 4
            bl = K.blocks_of(inp)
            for j, (ms, mf) in enumerate(K.THRESHOLDS):
                fills, _ = N.net(inp["first"], bl[0], bl[1], inp["score"], inp["group"], min_space=ms, min_fill=mf)
                flt = K.filters_of(fills, np.random.default_rng(100 * seed + j))
                kw = dict(ogroup=inp["ogroup"], ostrand=inp["ostrand"])
                out.append((inp, bl, fills, NC.classify(inp["first"], *bl, fills, **kw), flt, NC.classify(inp["first"], *bl, fills, filter=flt, **kw)))
        _cache["runs"] = out
    return _cache["runs"]


def children_of(fills):
    kids = {}
    for k, f in enumerate(fills):
        kids.setdefault((int(f["group"]), int(f["parent"])), []).append(k)
    return kids


def height(k, fills, kids):
    below = kids.get((int(fills[k]["group"]), k), [])
    return 1 + max([height(c, fills, kids) for c in below], default=0)


def test_the_sets_reach_every_regime_ten_times():
    tally = dict.fromkeys(TALLY, 0)
    for inp, bl, fills, (cls, st), flt, (fcls, fst) in runs():
        for t, name in enumerate(NC.NAMES):
            tally[name] += st["n_type"][t]
        tally["oover"] += int(np.count_nonzero(cls["oover"]))
        tally["ofar"] += int(np.count_nonzero(cls["ofar"]))
        tally["odup"] += int(np.count_nonzero(cls["odup"]))
        tally["odup_is_ali"] += int(np.count_nonzero(cls["odup"] == fills["ali"]))
        kids = children_of(fills)
        for k, f in enumerate(fills):
            p = int(f["parent"])
            if fcls[k]["keep"] or (p >= 0 and not fcls[p]["keep"]):
                continue  # kept, or dropped with its parent
            tally["dropped_with_kept_siblings"] += any(fcls[s]["keep"] for s in kids[int(f["group"]), p])
            tally["dropped_subtree_depth2"] += height(k, fills, kids) >= 2
    assert all(v >= 10 for v in tally.values()), tally


def test_odup_lies_between_0_and_ali():
    for inp, bl, fills, (cls, st), flt, (fcls, fst) in runs():
        assert np.all(cls["odup"] <= fills["ali"])
        assert st["dup_bases"] == int(cls["odup"].astype(np.int64).sum()) and st["blocks"] == int(fills["n_blocks"].sum())


def test_the_odup_of_a_group_sum_to_the_sorted_event_sweeps_weighted_bases():
    for inp, bl, fills, (cls, st), flt, (fcls, fst) in runs():
        want = NC.sweep_dup(inp["first"], *bl, fills, inp["ogroup"], inp["ostrand"])
        got = {int(g): int(cls["odup"][cls["ogroup"] == g].astype(np.int64).sum()) for g in np.unique(cls["ogroup"])}
        assert got == want and len(want) == st["ogroups"]


def test_the_hull_contains_every_clipped_other_block():
    for inp, bl, fills, (cls, st), flt, (fcls, fst) in runs():
        for f, c in zip(fills, cls):
            strand = int(inp["ostrand"][int(f["chain"])])
            cl = NC.clipped_other(f, *bl, strand)
            assert all(int(c["ostart"]) <= s < e <= int(c["oend"]) for s, e in cl) and int(c["strand"]) == strand
            assert sum(e - s for s, e in cl) == int(f["ali"])  # a clip keeps as many bases on the other axis as on the axis
            assert (cl[0][0], cl[-1][1]) == (c["ostart"], c["oend"]) if not strand else (cl[-1][0], cl[0][1]) == (c["ostart"], c["oend"])


def test_the_filter_changes_keep_alone_and_without_it_every_fill_is_kept():
    for inp, bl, fills, (cls, st), flt, (fcls, fst) in runs():
        assert np.all(cls["keep"] == 1) and st["kept"] == fills.size
        for k in NC.FIELDS[:-1]:
            assert np.array_equal(cls[k], fcls[k])


def test_keep_is_subtree_closed_and_net_select_passes_the_subset_entrys_validation():
    kept_some = 0
    for inp, bl, fills, (cls, st), flt, (fcls, fst) in runs():
        assert NC.keep_closed(fills, fcls)
        sel, index = NC.select(fills, fcls["keep"])
        got, got_index = E.net_select(fills, fcls["keep"])
        assert np.array_equal(index, got_index) and all(np.array_equal(sel[k], got[k]) for k in N.FIELDS)
        assert sel.size == fst["kept"] and np.array_equal(sel["chain"], fills["chain"][index.astype(np.int64)])
        big = np.zeros(8000, dtype=np.uint8)
        NS.validate(big, big, inp["hsps"], inp["members"], inp["first"], sel, "target")
        kept_some += 0 < sel.size < fills.size
    assert kept_some >= 50


def test_net_select_refuses_a_keep_that_is_not_subtree_closed():
    n = K.Net([K.comb(2), [(120, 500, 10)]], [9, 1])
    assert n.fills["parent"].tolist() == [-1, 0]
    with pytest.raises(ValueError):
        E.net_select(n.fills, [0, 1])
    with pytest.raises(KeyError):
        NC.select(n.fills, [0, 1])


def test_net_other_blocks_equals_its_twin():
    for seed in (0, 5):
        inp = K.random_input(seed)
        for axis in ("target", "query"):
            want = NC.other_blocks(inp["hsps"], inp["members"], inp["first"], axis, inp["ostrand"], inp["size"])
            got = E.net_other_blocks(inp["hsps"], inp["members"], inp["first"], axis, inp["ostrand"], inp["size"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.uint32
            plain = E.net_other_blocks(inp["hsps"], inp["members"], inp["first"], axis)
            other = E.net_blocks(inp["hsps"], inp["members"], inp["first"], "query" if axis == "target" else "target")
            assert np.array_equal(plain[0], other[0]) and np.array_equal(plain[1], other[1])


# ---- hand-worked cases ----
PARENT = [(100, 1000, 20), (200, 1100, 20)]  # other hull [1000, 1120)


@pytest.mark.parametrize("ostart,over,far", [(1119, 1, 0), (1120, 0, 0), (1121, 0, 1), (900, 0, 80), (1050, 20, 0)])
def test_x_against_the_parent(ostart, over, far):
    n = K.Net([PARENT, [(130, ostart, 20)]], [9, 1])
    cls, st = n.classify()
    assert n.fills["parent"].tolist() == [-1, 0] and cls["type"].tolist() == [NC.TOP, NC.SYN]
    assert (int(cls["oover"][1]), int(cls["ofar"][1])) == (over, far) and (int(cls["ostart"][0]), int(cls["oend"][0])) == (1000, 1120)


def test_inv_and_nonsyn():
    cls, st = K.Net([PARENT, [(130, 1040, 20)]], [9, 1], ostrand=[0, 1]).classify()
    assert cls["type"].tolist() == [NC.TOP, NC.INV] and int(cls["oover"][1]) == 20 and cls["strand"].tolist() == [0, 1]
    cls, st = K.Net([PARENT, [(130, 1040, 20)]], [9, 1], ogroup=[5, 6]).classify()
    assert cls["type"].tolist() == [NC.TOP, NC.NONSYN] and int(cls["oover"][1]) == 0 and int(cls["ofar"][1]) == 0 and st["n_type"] == [1, 0, 0, 1]
    assert st["ogroups"] == 2 and cls["ogroup"].tolist() == [5, 6]


def test_two_fills_with_identical_other_intervals_and_triple_coverage():
    two = K.Net([[(100, 700, 30)], [(100, 700, 30)]], [5, 5], group=[0, 1])
    cls, st = two.classify()
    assert cls["odup"].tolist() == [30, 30] and st["dup_bases"] == 60 and two.fills["ali"].tolist() == [30, 30]
    three = K.Net([[(100, 700, 30)], [(100, 710, 30)], [(100, 720, 30)]], [5, 5, 5], group=[0, 1, 2])
    cls, st = three.classify()
    assert cls["odup"].tolist() == [20, 30, 20]  # [710, 730) of the first, all of the second, [720, 740) of the third


def test_abutting_blocks_and_equal_coordinates_in_two_ogroups_are_not_duplication():
    cls, st = K.Net([[(100, 700, 30)], [(100, 730, 30)], [(100, 670, 30)]], [5, 5, 5], group=[0, 1, 2]).classify()
    assert cls["odup"].tolist() == [0, 0, 0]
    cls, st = K.Net([[(100, 700, 30)], [(100, 700, 30)]], [5, 5], group=[0, 1], ogroup=[8, 9]).classify()
    assert cls["odup"].tolist() == [0, 0] and st["ogroups"] == 2
    cls, st = K.Net([[(100, 700, 30)], [(100, 729, 30)]], [5, 5], group=[0, 1]).classify()
    assert cls["odup"].tolist() == [1, 1]


@pytest.mark.parametrize("top,want_axis,want_other", [
    ([(100, 9000, 20)], (120, 160), (500, 540)),                     # cut on the left: the other interval loses its right end
    ([(150, 9000, 20)], (110, 150), (510, 550)),                     # cut on the right: it loses its left end
    ([(100, 9000, 20), (150, 9050, 20)], (120, 150), (510, 540)),    # both
])
def test_a_strand_1_block_cut_left_right_and_both(top, want_axis, want_other):
    n = K.Net([top, [(110, 500, 50)]], [9, 1], ostrand=[0, 1])
    low = [k for k, f in enumerate(n.fills) if int(f["chain"]) == 1]
    assert len(low) == 1 and (int(n.fills[low[0]]["start"]), int(n.fills[low[0]]["end"])) == want_axis
    cls, st = n.classify()
    assert (int(cls["ostart"][low[0]]), int(cls["oend"][low[0]])) == want_other
    plus, _ = K.Net([top, [(110, 500, 50)]], [9, 1]).classify()
    d = (want_axis[0] - 110, 160 - want_axis[1])
    assert (int(plus["ostart"][low[0]]), int(plus["oend"][low[0]])) == (500 + d[0], 550 - d[1])


BASE = dict(min_score=0, min_top_score=0, min_size=0, min_ali=0, max_far=1 << 31)


@pytest.mark.parametrize("name,at,keep_at,keep_off", [
    ("min_score", 40, [1, 1], [1, 0]),      # the child scores 40
    ("min_top_score", 90, [1, 1], [0, 0]),  # the top fill scores 90: it falls and takes its child with it
    ("min_size", 20, [1, 1], [1, 0]),       # the child is [130, 150)
    ("min_ali", 20, [1, 1], [1, 0]),
])
def test_each_lower_threshold_at_its_value_and_one_above(name, at, keep_at, keep_off):
    n = K.Net([PARENT, [(130, 1200, 20)]], [90, 40])
    assert n.classify(filter=dict(BASE, **{name: at}))[0]["keep"].tolist() == keep_at
    cls, st = n.classify(filter=dict(BASE, **{name: at + 1}))
    assert cls["keep"].tolist() == keep_off and st["kept"] == sum(keep_off)


def test_max_far_at_its_value_and_one_below_and_nonsyn_never_passes():
    n = K.Net([PARENT, [(130, 1200, 20)]], [90, 40])  # the child is 80 bases past the parent's hull
    assert n.classify()[0]["ofar"].tolist() == [0, 80]
    assert n.classify(filter=dict(BASE, max_far=80))[0]["keep"].tolist() == [1, 1]
    assert n.classify(filter=dict(BASE, max_far=79))[0]["keep"].tolist() == [1, 0]
    n = K.Net([PARENT, [(130, 1040, 20)]], [90, 40], ogroup=[1, 2])
    assert n.classify(filter=BASE)[0]["keep"].tolist() == [1, 0]
    assert n.classify(filter=dict(min_top_score=-(1 << 62), min_score=-(1 << 62)))[0]["keep"].tolist() == [1, 0]


def test_a_dropped_fill_takes_its_subtree_and_leaves_its_siblings():
    chains = [K.comb(3), [(112, 10_012, 4), (122, 10_022, 4)], [(117, 10_017, 3)], [(152, 10_052, 20)]]
    n = K.Net(chains, [90, 40, 30, 50])
    assert n.fills["parent"].tolist() == [-1, 0, 1, 0] and n.fills["depth"].tolist() == [0, 1, 2, 1]
    cls, st = n.classify(filter=dict(BASE, min_score=41))
    assert cls["keep"].tolist() == [1, 0, 0, 1] and st["kept"] == 2
    sel, index = NC.select(n.fills, cls["keep"])
    assert index.tolist() == [0, 3] and sel["parent"].tolist() == [-1, 0]


def edit_fill(field, k, v):
    return lambda a: a["fills"][field].__setitem__(k, v)


def edit_array(name, k, v):
    return lambda a: a[name].__setitem__(k, v)


@pytest.mark.parametrize("edit,clause", [
    (edit_array("first", 0, 1), "first"),
    (edit_array("first", 1, 4), "first"),
    (edit_array("block_end", 0, 100), "block"),
    (edit_array("block_start", 1, 110), "block order"),
    (edit_array("oblock_end", 0, 1000), "other block"),
    (edit_array("oblock_end", 0, 1 << 31), "other block"),
    (edit_array("oblock_end", 0, 1019), "other block length"),
    (lambda a: (a["oblock_start"].__setitem__(1, 990), a["oblock_end"].__setitem__(1, 1010)), "other block order"),
    (edit_array("ostrand", 0, 1), "other block order"),
    (edit_array("ostrand", 1, 2), "ostrand"),
    (edit_fill("start", 0, 500), "fill extent"),
    (edit_fill("chain", 0, 2), "fill chain"),
    (edit_fill("n_blocks", 0, 3), "fill blocks"),
    (edit_fill("n_blocks", 1, 0), "fill blocks"),
    (edit_fill("first_block", 1, 1), "fill blocks"),
    (edit_fill("start", 0, 120), "fill edge blocks"),
    (edit_fill("end", 0, 200), "fill edge blocks"),
    (edit_fill("parent", 1, 1), "fill parent"),
    (edit_fill("parent", 1, -2), "fill parent"),
    (edit_fill("depth", 1, 2), "fill depth"),
    (edit_fill("depth", 0, 1), "fill depth"),
    (lambda a: a.__setitem__("filter", dict(min_size=(1 << 31) + 1)), "parameter"),
    (lambda a: a.__setitem__("filter", dict(max_far=-1)), "parameter"),
    (lambda a: a.__setitem__("filter", dict(min_len=1)), "filter names"),
])
def test_every_validation_clause(edit, clause):
    n = K.Net([PARENT, [(130, 1040, 20)]], [9, 1])
    a = dict(first=n.first.copy(), block_start=n.bs.copy(), block_end=n.be.copy(), oblock_start=n.obs.astype(np.int64),
             oblock_end=n.obe.astype(np.int64), fills=n.fills.copy(), ostrand=np.zeros(2, dtype=np.uint8), filter=None)
    NC.validate(**a)
    edit(a)
    with pytest.raises(ValueError, match="^%s$" % clause):
        NC.validate(**a)


def test_the_rendering_of_the_class_file():
    n = K.Net([PARENT, [(130, 1200, 20)], [(100, 1000, 20)]], [90, 40, 7], group=[0, 0, 1])
    cls, st = n.classify(filter=dict(BASE, max_far=79))
    assert cls["keep"].tolist() == [1, 0, 1]
    net = "net tA 500\nfill 100 120 q + 1000 120 chain=0 score=90 ali=40\n fill 130 20 q + 1200 20 chain=1 score=40 ali=20\nnet tB 90\nfill 100 20 q + 1000 20 chain=2 score=7 ali=20\n"
    lines = NC.render_class(net, cls).splitlines()
    assert len(lines) == 5 and lines[0] == "net tA 500" and lines[3] == "net tB 90"
    assert lines[1] == "fill 100 120 q + 1000 120 chain=0 score=90 ali=40 type=top qover=0 qfar=0 qdup=20"
    assert lines[2] == " fill 130 20 q + 1200 20 chain=1 score=40 ali=20 type=syn qover=0 qfar=80 qdup=0"
    kept = NC.render_class(net, cls, kept_only=True).splitlines()
    assert kept == [lines[0], lines[1], lines[3], lines[4]]
    cls["keep"][2] = 0
    assert NC.render_class(net, cls, kept_only=True).splitlines() == [lines[0], lines[1]]  # a net line with no kept fill is left out
