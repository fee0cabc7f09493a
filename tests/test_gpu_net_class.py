"""GPU: sa_net_classify (include/segalign_amd.h) against the model of tests/net_class_model.py.  Every test first asserts
with the models that its input is in the regime it names, then compares every field of every record and every count.  The entry reads no
sequence: the hand-built tests state their blocks on both axes directly (tests/net_class_cases.py) and take the fills from
tests/net_model.py.  Only the pipeline tests, which go on to sa_net_subset, need a resident target and query."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_model as M
import net_class_cases as K
import net_class_model as NC
import net_model as N
import net_subset_model as NS
from gapped_model import SUB
from helpers import Case as Setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 1 << 31
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LEN = 70_000
BASE = dict(min_score=0, min_top_score=0, min_size=0, min_ali=0, max_far=TOP)
PARENT = [(100, 1000, 20), (200, 1100, 20)]  # other hull [1000, 1120)


def sequences():
    rng = np.random.default_rng(2222)
    return ACGT[rng.integers(0, 4, LEN)], ACGT[rng.integers(0, 4, LEN)]


@pytest.fixture(scope="module")
def E(engine):
    t, q = sequences()
    Setup(t, q, chunk=250_000, sub_mat=SUB).engine_setup(engine, num_gpu=1)
    yield engine
    engine.ShutdownProcessor()


def held(E, net, filter=None):
    """One engine call held against the model.  -> (the model's classes, stats)."""
    want, wst = net.classify(filter=filter)
    got, st = net.classify(E.NetClassify, filter=filter)
    assert got.dtype == E.NET_CLASS_DTYPE
    NC.same(got, want)
    NC.same_stats(st, wst)
    assert st["class_ms"] > 0 or not want.size
    return want, wst


# ---- sizes ----
def test_no_fill_and_one_fill(E):
    net = K.Net([K.comb(3)], [5])
    got, st = E.NetClassify(net.first, net.bs, net.be, net.obs, net.obe, net.fills[:0])
    assert got.size == 0 and got.dtype == E.NET_CLASS_DTYPE and (st["fills"], st["blocks"], st["events"], st["kept"]) == (0, 0, 0, 0)
    got, st = E.NetClassify([0], [], [], [], [], net.fills[:0])
    assert got.size == 0
    want, wst = held(E, net)
    assert want.size == 1 and want[["ostart", "oend", "odup", "type", "keep"]].tolist() == [(10_000, 10_090, 0, NC.TOP, 1)] and wst["blocks"] == 3


@pytest.mark.parametrize("blocks", [1, 2, 31, 32, 33, 63, 64, 65, 129, 1025])
def test_so_many_clipped_blocks_in_all(E, blocks):
    # two chains in two groups of the net whose other blocks overlap by five bases: 2 * blocks events straddle the wave and tile edges
    a, b = (blocks + 1) // 2, blocks // 2
    net = K.Net([K.comb(a)] + ([K.comb(b, ostart=10_005)] if b else []), [5, 4][:1 + (b > 0)], group=[0, 1][:1 + (b > 0)])
    want, wst = held(E, net)
    assert wst["blocks"] == blocks and wst["events"] == 2 * blocks and want["odup"].tolist() == ([5 * b] * 2 if b else [0])


def test_a_fill_of_1025_blocks_whose_1024_gaps_each_hold_a_child(E):
    # child k lies in gap k and claims, on the other axis, the second half of the parent's block k and one base past it
    chains = [K.comb(1025)] + [[(112 + 40 * k, 10_005 + 40 * k, 6)] for k in range(1024)]
    net = K.Net(chains, [10 ** 6] + list(range(1024)))
    want, wst = held(E, net)
    assert wst["fills"] == 1025 and wst["n_type"] == [1, 1024, 0, 0] and (net.fills["parent"][1:] == 0).all()
    assert int(want["odup"][0]) == 5 * 1024 and (want["odup"][1:] == 5).all() and (want["oover"][1:] == 6).all()


def test_70_identical_intervals(E):
    net = K.Net([[(100, 700, 30)]] * 70, [5] * 70, group=list(range(70)))
    want, wst = held(E, net)
    assert (want["odup"] == 30).all() and wst["dup_bases"] == 70 * 30 and np.array_equal(want["odup"], net.fills["ali"])


def test_ends_and_starts_tying_at_one_coordinate(E):
    # 80 abutting intervals, each in a group of its own: every inner coordinate holds one end and one start; then one that overlaps by a base
    net = K.Net([[(100, 700 + 30 * k, 30)] for k in range(80)], [5] * 80, group=list(range(80)))
    want, wst = held(E, net)
    assert wst["dup_bases"] == 0
    net = K.Net([[(100, 700 + 30 * k, 30)] for k in range(80)] + [[(100, 1299, 2)]], [5] * 81, group=list(range(81)))
    want, wst = held(E, net)
    assert want["odup"].tolist() == [0] * 19 + [1, 1] + [0] * 59 + [2]  # [1299, 1301) lies on the last base of one and the first of the next


@pytest.mark.parametrize("layers", [3, 5, 9])
def test_depth_3_and_deeper(E, layers):
    net = K.Net([[(100, 5000 + 10 * k, 200 - 20 * k)] for k in range(layers)], [5] * layers, group=list(range(layers)))
    want, wst = held(E, net)  # interval k = [5000 + 10 k, 5200 - 10 k): nested, the innermost under all of them
    assert want["odup"].tolist() == [180] + [200 - 20 * k for k in range(1, layers)]


def test_two_ogroups_whose_coordinates_coincide_and_sparse_ids(E):
    ids = [0xFFFFFFFF, 0, 0x80000000, 0xFFFFFFFF, 7]
    net = K.Net([[(100, 700, 30)]] * 5, [5] * 5, group=list(range(5)), ogroup=ids)
    want, wst = held(E, net)
    assert want["odup"].tolist() == [30, 0, 0, 30, 0] and wst["ogroups"] == 4 and want["ogroup"].tolist() == ids


def test_coordinates_up_to_2_to_the_31_minus_1(E):
    net = K.Net([[(TOP - 200, TOP - 300, 50), (TOP - 51, TOP - 51, 50)], [(TOP - 120, TOP - 31, 30)], [(TOP - 120, TOP - 31, 30)]], [9, 1, 1],
                group=[0, 0, 1], ostrand=[0, 1, 0])
    want, wst = held(E, net)
    assert net.fills["parent"].tolist() == [-1, 0, -1] and int(want["oend"][0]) == TOP - 1 and int(want["oend"][1]) == TOP - 1
    assert want["type"].tolist() == [NC.TOP, NC.INV, NC.TOP] and want["odup"].tolist() == [30, 30, 30] and int(want["oover"][1]) == 30


# ---- clipping on strand 1 ----
@pytest.mark.parametrize("kept", [1, 63, 64, 65])
@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_a_strand_1_block_cut_on_this_side_keeping_so_many_bases(E, side, kept):
    low = (1000, 7000, 300)  # [1000, 1300) on the axis, [7000, 7300) on the other, strand 1
    if side == "left":
        top, axis, other = [(900, 90_000, 400 - kept)], (1300 - kept, 1300), (7000, 7000 + kept)
    elif side == "right":
        top, axis, other = [(1000 + kept, 90_000, 400)], (1000, 1000 + kept), (7300 - kept, 7300)
    else:
        top, axis, other = [(900, 90_000, 200), (1100 + kept, 90_300, 400)], (1100, 1100 + kept), (7200 - kept, 7200)
    net = K.Net([top, [low], [(50, 7000, 300)]], [9, 1, 1], group=[0, 0, 1], ostrand=[0, 1, 0])  # a third chain in another group over it all
    k = int(np.flatnonzero(net.fills["chain"] == 1)[0])
    assert (int(net.fills["start"][k]), int(net.fills["end"][k])) == axis and int(net.fills["ali"][k]) == kept
    want, wst = held(E, net)
    assert (int(want["ostart"][k]), int(want["oend"][k])) == other and int(want["odup"][k]) == kept


# ---- classes ----
@pytest.mark.parametrize("ostart,over,far", [(1119, 1, 0), (1120, 0, 0), (1121, 0, 1), ((1 << 30) + 5000, 0, (1 << 30) + 5000 - 1120)])
def test_x_against_the_parent_and_a_far_distance(E, ostart, over, far):
    net = K.Net([PARENT, [(130, ostart, 20)]], [9, 1])
    want, wst = held(E, net)
    assert want["type"].tolist() == [NC.TOP, NC.SYN] and (int(want["oover"][1]), int(want["ofar"][1])) == (over, far)
    want, wst = held(E, net, filter=dict(BASE, max_far=far))
    assert want["keep"].tolist() == [1, 1]
    if far:
        assert held(E, net, filter=dict(BASE, max_far=far - 1))[0]["keep"].tolist() == [1, 0]


def test_a_child_before_its_parent_on_the_other_axis(E):
    want, wst = held(E, K.Net([[(100, 1 << 30, 20), (200, (1 << 30) + 100, 20)], [(130, 5, 20)]], [9, 1]))
    assert int(want["ofar"][1]) == (1 << 30) - 25


def test_inv_and_nonsyn(E):
    want, wst = held(E, K.Net([PARENT, [(130, 1040, 20)], [(160, 1040, 20)]], [9, 2, 1], ostrand=[0, 1, 0], ogroup=[5, 5, 6]), filter=BASE)
    assert want["type"].tolist() == [NC.TOP, NC.INV, NC.NONSYN] and want["keep"].tolist() == [1, 1, 0] and wst["n_type"] == [1, 0, 1, 1]
    want, wst = held(E, K.Net([K.comb_minus(3), [(112, 89_990, 8)]], [9, 1], ostrand=[1, 1]))
    assert want["type"].tolist() == [NC.TOP, NC.SYN] and (int(want["ostart"][0]), int(want["oend"][0])) == (89_910, 90_000)


# ---- the filter ----
def deep(fail_at):
    """A net 40 deep, one fill per level; the fill at level fail_at scores -1, every other one 1000 - its level."""
    net = K.Net(K.nested(40), [1000 - k for k in range(40)])
    assert net.fills["depth"].tolist() == list(range(40)) and net.fills["parent"].tolist() == list(range(-1, 39))
    net.fills["score"][fail_at] = -1
    return net


@pytest.mark.parametrize("fail_at", [0, 20, 39])
def test_nesting_40_deep_with_the_filter_failing_at_the_root_in_the_middle_and_at_a_leaf(E, fail_at):
    net = deep(fail_at)
    want, wst = held(E, net, filter=dict(BASE, min_score=0))
    assert want["keep"].tolist() == [1] * fail_at + [0] * (40 - fail_at)
    assert held(E, net)[0]["keep"].tolist() == [1] * 40  # without the flag


@pytest.mark.parametrize("name,at,keep_at,keep_off", [("min_score", 40, [1, 1], [1, 0]), ("min_top_score", 90, [1, 1], [0, 0]),
                                                      ("min_size", 20, [1, 1], [1, 0]), ("min_ali", 20, [1, 1], [1, 0])])
def test_each_lower_threshold_at_its_value_and_one_above(E, name, at, keep_at, keep_off):
    net = K.Net([PARENT, [(130, 1200, 20)]], [90, 40])
    assert held(E, net, filter=dict(BASE, **{name: at}))[0]["keep"].tolist() == keep_at
    assert held(E, net, filter=dict(BASE, **{name: at + 1}))[0]["keep"].tolist() == keep_off
    assert held(E, net, filter=dict(BASE, max_far=80))[0]["keep"].tolist() == [1, 1]
    assert held(E, net, filter=dict(BASE, max_far=79))[0]["keep"].tolist() == [1, 0]


def test_a_dropped_fill_takes_its_subtree_and_leaves_its_siblings(E):
    net = K.Net([K.comb(3), [(112, 10_012, 4), (122, 10_022, 4)], [(117, 10_017, 3)], [(152, 10_052, 20)]], [90, 40, 30, 50])
    want, wst = held(E, net, filter=dict(BASE, min_score=41))
    assert net.fills["parent"].tolist() == [-1, 0, 1, 0] and want["keep"].tolist() == [1, 0, 0, 1]


def test_scores_and_thresholds_at_plus_and_minus_2_to_the_62(E):
    net = K.Net([PARENT, [(130, 1040, 20)], [(300, 1300, 20)]], [9, 1, 0])
    net.fills["score"] = [1 << 62, -(1 << 62), -(1 << 62)]
    assert net.fills["parent"].tolist() == [-1, 0, -1]
    for flt, keep in [(dict(min_score=-(1 << 62), min_top_score=-(1 << 62)), [1, 1, 1]), (dict(min_score=-(1 << 62) + 1, min_top_score=-(1 << 62)), [1, 0, 0]),
                      (dict(min_score=-(1 << 62), min_top_score=1 << 62), [1, 1, 0]), (dict(min_score=-(1 << 62), min_top_score=(1 << 62) + 1), [0, 0, 0]),
                      (dict(min_score=1 << 62), [1, 0, 0])]:
        assert held(E, net, filter=dict(BASE, **flt))[0]["keep"].tolist() == keep


# ---- random sets through the pipeline, threads ----
PARAMS = [dict(min_space=1, min_fill=1), dict(min_space=5, min_fill=12), dict(min_space=25, min_fill=3)]
OGROUPS = np.array([11, 0, 4_000_000_000], dtype=np.uint32)
_sets = {}


def scatter(rng, n, diagonals, step=40, jitter=6, pitch=150):
    """n HSPs along a few diagonals `pitch` apart, near enough for a child's other hull to meet its parent's, in shuffled input order."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * pitch + int(rng.integers(-jitter, jitter + 1))
        q = 1000 + k * step // diagonals + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(5, 50)), int(rng.integers(-40, 3000))))
    return M.make(rows)[rng.permutation(n)]


class Pipe:
    pass


def pipeline(E, seed, k):
    """Per strand ChainHspsAll -> chain_csr; both strands as one CSR -> net_blocks / net_other_blocks -> (model) net and classes."""
    if (seed, k) not in _sets:
        rng = np.random.default_rng(7000 + seed)
        p = Pipe()
        hs, idx, first, score, key, strand = [], [], [np.zeros(1, dtype=np.uint32)], [], [], []
        for s in (0, 1):
            h = scatter(rng, int(rng.integers(500, 1501)), diagonals=8)
            g = (rng.integers(0, 2, h.size) * 8 + rng.integers(0, 3, h.size)).astype(np.uint32)  # target record * 8 + query record
            chains, members, _, _ = E.ChainHspsAll(h, g, max_gap=120, min_score=0, diag_pen=s, anti_pen=0)
            i, f = E.chain_csr(members)
            idx.append(i + np.uint32(sum(x.size for x in hs)))
            first.append(f[1:] + first[-1][-1])
            hs.append(h)
            score.append(chains["score"])
            key.append(chains["group"])
            strand.append(np.full(chains.size, s, dtype=np.uint8))
        p.h, p.idx, p.first = np.concatenate(hs), np.concatenate(idx), np.concatenate(first)
        p.score, key, p.ostrand = np.concatenate(score), np.concatenate(key), np.concatenate(strand)
        p.group, p.ogroup = key // 8, OGROUPS[key % 8]
        p.size = np.full(p.score.size, LEN, dtype=np.uint32)
        p.bs, p.be = E.net_blocks(p.h, p.idx, p.first, axis="target")
        p.obs, p.obe = E.net_other_blocks(p.h, p.idx, p.first, axis="target", strand=p.ostrand, size=p.size)
        want = NC.other_blocks(p.h, p.idx, p.first, "target", p.ostrand, p.size)
        assert np.array_equal(p.obs, want[0]) and np.array_equal(p.obe, want[1])
        p.fills, p.net_st = N.net(p.first, p.bs, p.be, p.score, p.group, **PARAMS[k])
        p.filter = K.filters_of(p.fills, np.random.default_rng(seed * 3 + k))
        p.want = NC.classify(p.first, p.bs, p.be, p.obs, p.obe, p.fills, p.ogroup, p.ostrand)
        p.want_f = NC.classify(p.first, p.bs, p.be, p.obs, p.obe, p.fills, p.ogroup, p.ostrand, p.filter)
        _sets[(seed, k)] = p
    return _sets[(seed, k)]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(6))
def test_random_sets_through_the_pipeline(E, seed, k):
    p = pipeline(E, seed, k)
    (cls, st), (fcls, fst) = p.want, p.want_f
    assert 100 <= p.score.size <= 2000 and p.net_st["max_depth"] >= 2 and all(n >= 5 for n in st["n_type"]) and st["ogroups"] == 3
    assert np.count_nonzero(cls["oover"]) >= 2 and np.count_nonzero(cls["ofar"]) >= 5 and st["dup_bases"] > 0
    assert 0 < fst["kept"] < st["fills"] and NC.keep_closed(p.fills, fcls) and np.all(cls["odup"] <= p.fills["ali"])
    fills, _ = E.NetChains(p.first, p.bs, p.be, p.score, p.group, **PARAMS[k])
    N.same(fills, p.fills)
    for flt, (want, wst) in ((None, p.want), (p.filter, p.want_f)):
        got, gst = E.NetClassify(p.first, p.bs, p.be, p.obs, p.obe, fills, p.ogroup, p.ostrand, flt)
        NC.same(got, want)
        NC.same_stats(gst, wst)
    # the syntenic net's alignments: the kept fills are a net of their own that sa_net_subset takes unchanged
    sel, index = E.net_select(fills, got["keep"])
    want_sel, want_index = NC.select(p.fills, fcls["keep"])
    assert np.array_equal(index, want_index) and all(np.array_equal(sel[f], want_sel[f]) for f in N.FIELDS)
    hs, ch, sst = E.NetSubset(p.h, p.idx, p.first, sel, False, 0)
    assert sst["fills"] == sel.size and np.array_equal(np.unique(ch["fill"]), np.arange(sel.size))
    assert NS.hulls_disjoint(ch)  # sa_net_subset's consequence (a)


def test_eight_threads_get_the_serial_results(E):
    jobs = [pipeline(E, s, (s + 1) % 3) for s in range(6)] + [pipeline(E, 0, 0), pipeline(E, 1, 1)]
    out, errors = [None] * 8, []

    def work(i):
        try:
            p = jobs[i]
            out[i] = E.NetClassify(p.first, p.bs, p.be, p.obs, p.obe, p.fills, p.ogroup, p.ostrand, p.filter if i % 2 else None)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(8):
        NC.same(out[i][0], (jobs[i].want_f if i % 2 else jobs[i].want)[0])


# ---- failures ----
CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import net_class_cases as K
from segalign_amd import engine as E
E.InitializeInterface(1)
net = K.Net([[(100, 1000, 20), (200, 1100, 20)], [(130, 1040, 20)]], [9, 1])
first, bs, be, obs, obe, fills = net.args()
kw = dict(ostrand=np.zeros(2, dtype=np.uint8))
%s
got, st = E.NetClassify(first, bs, be, obs, obe, fills, **kw)
assert got["type"].tolist() == [0, 1]
print("returned")
"""


@pytest.mark.parametrize("edit,words", [
    ("pass", None),
    ("obe = obe.copy(); obe[0] += 1", [b"chain 0, block 0", b"lengths on the two axes differ"]),
    ("kw['ostrand'][0] = 1", [b"chain 0 (ostrand 1)", b"ascend"]),
    ("kw['ostrand'][1] = 2", [b"ostrand[1] = 2"]),
    ("kw['filter'] = dict(max_far=(1 << 31) + 1)", [b"max_far", b"out of range"]),
    ("fills = fills.copy(); fills['depth'][1] = 2", [b"fill 1", b"depth 2"]),
])
def test_bad_input_fails_with_a_message(edit, words):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), edit)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if words is None:  # the unedited input returns: the failures below are the edits'
        assert r.returncode == 0 and b"returned" in r.stdout, r.stderr
        return
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"NetClassify" in r.stderr and all(w in r.stderr for w in words), r.stderr
