"""GPU: sa_lift_intervals (include/segalign_amd.h) against the model of tests/lift_model.py.  Every test first asserts with
the model that its input is in the regime it names, then compares every field of every record, hit and block and every count.  The entry
reads no sequence: the hand-built tests state their blocks on both axes directly (tests/lift_cases.py).  Only the pipeline tests that go
through sa_net_subset need a resident target and query."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_model as M
import lift_cases as LC
import lift_model as L
import net_class_cases as K
import net_subset_model as NS
from gapped_model import SUB
from helpers import Case as Setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 1 << 31
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LEN = 70_000
A = [(100, 1000, 20), (200, 1100, 20)]  # [100, 120) and [200, 220), on the other axis [1000, 1020) and [1100, 1120)


@pytest.fixture(scope="module")
def E(engine):
    rng = np.random.default_rng(2323)
    Setup(ACGT[rng.integers(0, 4, LEN)], ACGT[rng.integers(0, 4, LEN)], chunk=250_000, sub_mat=SUB).engine_setup(engine, num_gpu=1)
    yield engine
    engine.ShutdownProcessor()


def held(E, chains, intervals, iv_group=None, ratio=(95, 100), multiple=False, blocks=False):
    """One engine call held against the model.  -> the model's (records, hits, blocks, stats)."""
    want = chains.lift(intervals, iv_group=iv_group, min_match=ratio, multiple=multiple, blocks=blocks)
    got = chains.lift(intervals, E.LiftIntervals, iv_group=iv_group, min_match=ratio, multiple=multiple, blocks=blocks)
    assert got[0].dtype == E.LIFT_RECORD_DTYPE and got[1].dtype == E.LIFT_HIT_DTYPE and (got[2] is None or got[2].dtype == E.LIFT_BLOCK_DTYPE)
    L.same(got, want)
    L.same_stats(got[3], want[3])
    assert got[3]["lift_ms"] > 0 and (got[3]["prep_ms"] > 0 or got[3]["chains"] == 0)
    return want


def held_under_every_flag(E, chains, intervals, iv_group=None, ratio=(95, 100)):
    """-> the model's answer with both flags."""
    for multiple, blocks in LC.FLAGS:
        want = held(E, chains, intervals, iv_group, ratio, multiple, blocks)
    return want


# ---- sizes ----
def test_no_interval_no_chain_and_one_chain_of_one_block(E):
    c = LC.Chains([A])
    rec, hits, blocks, st = E.LiftIntervals(*c.args(), [], [], multiple=True, blocks=True)
    assert rec.size == 0 and hits.size == 0 and blocks.size == 0 and (st["intervals"], st["chains"], st["blocks"], st["hits"]) == (0, 1, 2, 0)
    none = LC.Chains([])
    rec, hits, blocks, st = held_under_every_flag(E, none, [(5, 9), (100, 200)])
    assert rec["status"].tolist() == [0, 0] and rec["chain"].tolist() == [L.NONE] * 2 and st["candidates"] == 0 and hits.size == 0
    rec, hits, blocks, st = held_under_every_flag(E, LC.Chains([[(100, 1000, 20)]]), [(90, 100), (100, 120), (105, 106), (119, 140), (120, 140)])
    assert rec["status"].tolist() == [0, 2, 2, 1, 0] and hits["interval"].tolist() == [1, 2] and blocks.size == 2


# ---- the candidate range ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1025])
def test_so_many_candidates_all_touching_and_qualifying(E, n):
    # chain k starts k bases before the last one and holds the whole interval: the hit order is the reverse of the chain order
    c = LC.Chains([[(2000 - k, 500_000 + 4000 * k, 200 + k)] for k in range(n)])
    rec, hits, blocks, st = held_under_every_flag(E, c, [(2000, 2100), (2050, 2051)])
    assert st["candidates"] == 2 * n and rec["n_touch"].tolist() == [n, n] and rec["n_qualify"].tolist() == [n, n]
    assert hits["chain"].tolist() == list(range(n - 1, -1, -1)) * 2 and rec["chain"].tolist() == [n - 1] * 2  # ties of mapped: the first in hit order
    assert rec["first_hit"].tolist() == [0, n] and blocks.size == 2 * n


def long_range(n):
    """n candidates of which only the last touches [2000, 2100): one early chain whose hull spans everything with the interval in its
    gap, n - 2 small chains that end before the interval, and the chain that holds it."""
    chains = [[(100, 900_000, 10), (5000, 904_900, 10)]] if n > 1 else []
    chains += [[(200 + k, 100_000 + 10 * k, 5)] for k in range(n - 2)]
    return LC.Chains(chains + [[(1990, 500_000, 200)]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1025])
def test_so_many_candidates_of_which_only_the_last_touches(E, n):
    rec, hits, blocks, st = held_under_every_flag(E, long_range(n), [(2000, 2100)])
    assert st["candidates"] == n and rec["n_touch"].tolist() == [1] and rec["chain"].tolist() == [n - 1] and hits.size == 1
    assert (int(rec["ostart"][0]), int(rec["oend"][0])) == (500_010, 500_110)


def test_one_early_chain_spans_the_group_over_300_chains_the_interval_does_not_meet(E):
    rec, hits, blocks, st = held_under_every_flag(E, long_range(302), [(2000, 2100), (1200, 1300), (150, 203)])
    assert st["candidates"] == 302 + 301 + 4 and rec["n_touch"].tolist() == [1, 0, 3] and rec["status"].tolist() == [2, 0, 1]


# ---- chains of many blocks ----
@pytest.mark.parametrize("n", [1, 2, 64, 65, 1025])
def test_a_chain_of_so_many_blocks_cut_in_its_first_its_last_and_one_block(E, n):
    c = LC.Chains([K.comb(n)])  # blocks [100 + 40 k, 110 + 40 k)
    last = 100 + 40 * (n - 1)
    iv = [(105, last + 10), (100, last + 5), (103, 107), (last + 3, last + 7), (95, last + 15), (104, last + 6)]
    rec, hits, blocks, st = held_under_every_flag(E, c, iv, ratio=(0, 1))
    assert rec["n_blocks"].tolist() == [n, n, 1, 1, n, n] and rec["mapped"].tolist() == [10 * n - 5, 10 * n - 5, 4, 4, 10 * n, 10 * n - 8]
    assert rec["first_block"].tolist() == [0, 0, 0, n - 1, 0, 0] and blocks.size == 4 * n + 2
    assert (int(rec["ostart"][0]), int(rec["oend"][1]), int(rec["ostart"][3])) == (10_005, 10_000 + 40 * (n - 1) + 5, 10_000 + 40 * (n - 1) + 3)


# ---- edges of touching and of the threshold ----
def test_abutting_intervals_one_base_of_overlap_and_an_interval_in_a_gap(E):
    rec, hits, blocks, st = held_under_every_flag(E, LC.Chains([A]), [(120, 200), (119, 201), (119, 200), (120, 201), (130, 150), (99, 100), (220, 221)],
                                                  ratio=(0, 1))
    assert rec["status"].tolist() == [0, 2, 2, 2, 0, 0, 0] and rec["mapped"].tolist() == [0, 2, 1, 1, 0, 0, 0] and st["candidates"] == 5
    assert rec["n_blocks"].tolist() == [0, 2, 1, 1, 0, 0, 0] and (int(rec["ostart"][1]), int(rec["oend"][1])) == (1019, 1101)


@pytest.mark.parametrize("block,iv,ratio,status", [
    ((0, TOP - 1), (0, TOP - 1), (1 << 20, 1 << 20), 2), ((1, TOP - 1), (0, TOP - 1), (1 << 20, 1 << 20), 1),
    ((0, 1 << 29), (0, 1 << 30), (1 << 19, 1 << 20), 2), ((0, (1 << 29) - 1), (0, 1 << 30), (1 << 19, 1 << 20), 1),
    ((2047, TOP - 1), (0, TOP - 1), ((1 << 20) - 1, 1 << 20), 2), ((2048, TOP - 1), (0, TOP - 1), ((1 << 20) - 1, 1 << 20), 1),
    ((100, 120), (100, 140), (1, 2), 2), ((100, 120), (100, 141), (1, 2), 1)])
def test_the_threshold_at_its_value_and_one_off_it(E, block, iv, ratio, status):
    c = LC.Chains([[(block[0], block[0], block[1] - block[0])]])
    mapped, length = min(block[1], iv[1]) - max(block[0], iv[0]), iv[1] - iv[0]
    assert (mapped * ratio[1] >= ratio[0] * length) == (status == 2) and abs(mapped * ratio[1] - ratio[0] * length) <= ratio[1]
    rec, hits, blocks, st = held_under_every_flag(E, c, [iv], ratio=ratio)
    assert rec["status"].tolist() == [status] and int(rec["mapped"][0]) == mapped


def test_num_0_and_num_equal_to_den(E):
    for ratio, status in (((0, 7), [2, 0, 2, 2]), ((7, 7), [1, 0, 2, 1])):
        rec = held_under_every_flag(E, LC.Chains([A]), [(119, 150), (130, 150), (100, 120), (100, 121)], ratio=ratio)[0]
        assert rec["status"].tolist() == status


# ---- clipping on strand 1 ----
@pytest.mark.parametrize("kept", [1, 63, 64, 65])
@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_a_strand_1_block_cut_on_this_side_keeping_so_many_bases(E, side, kept):
    c = LC.Chains([[(1000, 7000, 300)], [(900, 90_000, 50), (1400, 90_500, 50)]], ostrand=[1, 0])  # the second chain's hull covers it all
    iv, other = {"left": ((1300 - kept, 1400), (7000, 7000 + kept)), "right": ((950, 1000 + kept), (7300 - kept, 7300)),
                 "both": ((1100, 1100 + kept), (7200 - kept, 7200))}[side]
    rec, hits, blocks, st = held_under_every_flag(E, c, [iv], ratio=(0, 1))
    assert (int(rec["ostart"][0]), int(rec["oend"][0]), int(rec["mapped"][0]), int(rec["strand"][0])) == other + (kept, 1) and st["candidates"] == 2
    assert blocks.tolist() == [(max(iv[0], 1000), min(iv[1], 1300)) + other]


def test_strand_1_chains_of_several_blocks(E):
    c = LC.Chains([K.comb_minus(70)], ostrand=[1])  # blocks [100 + 40 k, 110 + 40 k), on the other axis [89 990 - 40 k, 90 000 - 40 k)
    rec, hits, blocks, st = held_under_every_flag(E, c, [(105, 100 + 40 * 69 + 3), (143, 187), (100, 110)], ratio=(0, 1))
    assert (int(rec["ostart"][0]), int(rec["oend"][0])) == (89_990 - 40 * 69 + 7, 89_995) and (int(rec["ostart"][1]), int(rec["oend"][1])) == (89_913, 89_957)
    assert np.all(np.diff(blocks["ostart"][:70].astype(np.int64)) < 0)


# ---- order, ties, groups ----
def test_ties_of_mapped_and_of_hull_start(E):
    c = LC.Chains([[(100, 1000, 20)], [(90, 2000, 30)], [(100, 3000, 20)], [(100, 4000, 25)]], ogroup=[5, 6, 5, 0xFFFFFFFF])
    rec, hits, blocks, st = held_under_every_flag(E, c, [(100, 120), (100, 110), (118, 126)])
    assert rec["status"].tolist() == [3, 3, 1] and rec["chain"].tolist() == [1, 1, 3] and hits["chain"].tolist() == [1, 0, 2, 3] * 2
    assert rec["ogroup"].tolist() == [6, 6, 0xFFFFFFFF]


def test_empty_chains_among_the_candidates(E):
    c = LC.Chains([[], [(100, 1000, 20)], [], [(90, 2000, 30)], []] + [[]] * 70 + [[(50, 3000, 100)]])
    rec, hits, blocks, st = held_under_every_flag(E, c, [(100, 120), (60, 70), (0, 5)])
    assert rec["n_touch"].tolist() == [3, 1, 0] and hits["chain"].tolist() == [75, 3, 1, 75] and st["candidates"] == 3 + 1 + 0


def test_groups_up_to_2_to_the_32_minus_1_a_group_without_a_chain_and_equal_coordinates_in_different_groups(E):
    ids = [0xFFFFFFFF, 0, 0x80000000, 0xFFFFFFFF, 7]
    c = LC.Chains([[(100, 700 + 100 * k, 30)] for k in range(5)], group=ids, ogroup=[9, 8, 7, 6, 5])
    rec, hits, blocks, st = held_under_every_flag(E, c, [(100, 130)] * 7, iv_group=ids + [5, 0xFFFFFFFE])
    assert rec["status"].tolist() == [3, 2, 2, 3, 2, 0, 0] and rec["chain"].tolist() == [0, 1, 2, 0, 4, L.NONE, L.NONE]
    assert rec["n_touch"].tolist() == [2, 1, 1, 2, 1, 0, 0] and st["candidates"] == 7


def test_coordinates_up_to_2_to_the_31_minus_1(E):
    c = LC.Chains([[(TOP - 200, TOP - 300, 50), (TOP - 51, TOP - 51, 50)], [(TOP - 120, TOP - 31, 30)]], ostrand=[0, 1])
    rec, hits, blocks, st = held_under_every_flag(E, c, [(TOP - 60, TOP - 1), (TOP - 2, TOP - 1), (TOP - 180, TOP - 100), (0, TOP - 1)], ratio=(1, 4))
    assert rec["status"].tolist() == [2, 2, 3, 1] and int(rec["oend"][0]) == TOP - 1 and int(blocks["oend"].max()) == TOP - 1


# ---- the blocks ----
@pytest.mark.parametrize("n", [0, 1, 64, 65, 1025])
def test_so_many_output_blocks_in_all(E, n):
    a = n // 2
    c = LC.Chains([K.comb(max(n, 1))])
    iv = [(100 + 40 * a, 100 + 40 * n)] + ([(100, 100 + 40 * a)] if a else []) if n else [(100, 110)]
    rec, hits, blocks, st = held(E, c, iv, iv_group=None if n else [1], ratio=(0, 1), multiple=True, blocks=True)
    assert st["out_blocks"] == n == blocks.size and hits["out_block"].tolist() == ([0, n - a][:hits.size])
    assert held(E, c, iv, iv_group=None if n else [1], ratio=(0, 1), multiple=True, blocks=False)[2] is None


# ---- random sets, flags, consequence (e) ----
@pytest.mark.parametrize("seed", range(3))
def test_random_nets_under_every_flag_combination(E, seed):
    case = LC.random_case(seed)
    for ratio in ((95, 100), (51, 100)):
        answers = []
        for multiple, blocks in LC.FLAGS:
            want = LC.run(case, ratio=ratio, multiple=multiple, blocks=blocks)
            got = LC.run(case, E.LiftIntervals, ratio=ratio, multiple=multiple, blocks=blocks)
            assert all(n >= 5 for n in want[3]["n_status"]) and set(case["kw"]["ostrand"].tolist()) == {0, 1}
            L.same(got, want)
            L.same_stats(got[3], want[3])
            answers.append(got)
        base, both = answers[0], answers[3]  # consequence (e)
        for k in L.RECORD_FIELDS:
            if k != "first_hit":
                assert all(np.array_equal(a[0][k], base[0][k]) for a in answers)
        pick = both[1][np.isin(both[1]["interval"], np.flatnonzero(base[0]["status"] == L.MAPPED))]
        assert pick.size == base[1].size > 0 and all(np.array_equal(pick[k], base[1][k]) for k in L.HIT.names if k != "out_block")


# ---- through the pipeline ----
OGROUPS = np.array([11, 0, 4_000_000_000], dtype=np.uint32)
PARAMS = [dict(ratio=(95, 100), multiple=False, blocks=True), dict(ratio=(51, 100), multiple=True, blocks=False)]
_sets = {}


def scatter(rng, n, diagonals, step=40, jitter=6, pitch=150):
    """n HSPs along a few diagonals `pitch` apart, in shuffled input order."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * pitch + int(rng.integers(-jitter, jitter + 1))
        q = 1000 + k * step // diagonals + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(5, 50)), int(rng.integers(-40, 3000))))
    return M.make(rows)[rng.permutation(n)]


class Pipe:
    pass


def pipeline(E, seed):
    """Per strand ChainHspsAll -> chain_csr; both strands as one CSR -> net_blocks / net_other_blocks, and 2 000 intervals over them."""
    if seed not in _sets:
        rng = np.random.default_rng(2370 + seed)
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
        p.group, p.ogroup = (key // 8).astype(np.uint32), OGROUPS[key % 8]
        p.bs, p.be = E.net_blocks(p.h, p.idx, p.first, axis="target")
        p.obs, p.obe = E.net_other_blocks(p.h, p.idx, p.first, axis="target", strand=p.ostrand, size=np.full(p.score.size, LEN, dtype=np.uint32))
        p.iv = LC.intervals_over(rng, p.first, p.bs, p.be, p.group, 2000)
        _sets[seed] = p
    return _sets[seed]


def lift_all(fn, p, ratio, multiple, blocks):
    return fn(p.first, p.bs, p.be, p.obs, p.obe, p.iv[0], p.iv[1], group=p.group, ogroup=p.ogroup, ostrand=p.ostrand, iv_group=p.iv[2],
              min_match=ratio, multiple=multiple, blocks=blocks)


@pytest.mark.parametrize("k", range(2))
@pytest.mark.parametrize("seed", range(6))
def test_random_sets_through_all_chains(E, seed, k):
    p = pipeline(E, seed)
    want = lift_all(L.lift, p, **PARAMS[k])
    assert 100 <= p.score.size <= 2000 and all(n >= 20 for n in want[3]["n_status"])  # overlapping chains: DUPLICATED occurs
    assert want[3]["candidates"] > want[3]["touches"] > 2000 and int(want[0]["n_touch"].max()) >= 3
    got = lift_all(E.LiftIntervals, p, **PARAMS[k])
    L.same(got, want)
    L.same_stats(got[3], want[3])


@pytest.mark.parametrize("seed", range(6))
def test_random_sets_through_the_sub_chains_of_the_net(E, seed):
    p = pipeline(E, seed)
    fills, _ = E.NetChains(p.first, p.bs, p.be, p.score, p.group)
    hs, ch, _ = E.NetSubset(p.h, p.idx, p.first, fills, False, 0)
    assert NS.hulls_disjoint(ch) and ch.size >= 50
    smem, sfirst = E.subset_csr(ch)
    bs, be = E.net_blocks(hs, smem, sfirst, axis="target")
    strand = p.ostrand[ch["chain"]]
    obs, obe = E.net_other_blocks(hs, smem, sfirst, axis="target", strand=strand, size=np.full(ch.size, LEN, dtype=np.uint32))
    kw = dict(group=ch["group"], ogroup=p.ogroup[ch["chain"]], ostrand=strand, iv_group=p.iv[2])
    for ratio, multiple, blocks in (((51, 100), True, True), ((95, 100), False, False)):
        want = L.lift(sfirst, bs, be, obs, obe, p.iv[0], p.iv[1], min_match=ratio, multiple=multiple, blocks=blocks, **kw)
        assert want[3]["n_status"][L.DUPLICATED] == 0 and all(want[3]["n_status"][s] >= 20 for s in (0, 1, 2))  # consequence (c)
        got = E.LiftIntervals(sfirst, bs, be, obs, obe, p.iv[0], p.iv[1], min_match=ratio, multiple=multiple, blocks=blocks, **kw)
        L.same(got, want)
        L.same_stats(got[3], want[3])


def test_eight_threads_get_the_serial_results(E):
    jobs = [(pipeline(E, s % 6), PARAMS[s % 2]) for s in range(8)]
    want = [lift_all(L.lift, p, **kw) for p, kw in jobs]
    out, errors = [None] * 8, []

    def work(i):
        try:
            out[i] = lift_all(E.LiftIntervals, jobs[i][0], **jobs[i][1])
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(8):
        L.same(out[i], want[i])
        L.same_stats(out[i][3], want[i][3])


# ---- failures ----
CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
E.InitializeInterface(1)
first, bs, be = np.array([0, 2]), np.array([100, 200]), np.array([120, 220])
obs, obe = np.array([1000, 1100]), np.array([1020, 1120])
ivs, ive = np.array([119, 130]), np.array([201, 150])
kw = dict(min_match=(1, 50))
flags = None
%s
if flags is None:
    rec, hits, blocks, st = E.LiftIntervals(first, bs, be, obs, obe, ivs, ive, **kw)
    assert rec["status"].tolist() == [2, 0] and hits.size == 1
else:
    import ctypes as C
    out = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    n = [C.c_size_t(0), C.c_size_t(0)]
    a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (first, bs, be, obs, obe, ivs, ive)]
    E.lib().sa_lift_intervals(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data, None, None, None, 1, None,
                              a[5].ctypes.data, a[6].ctypes.data, 2, None, flags, C.byref(out[0]), C.byref(out[1]), C.byref(n[0]),
                              C.byref(out[2]), C.byref(n[1]), None)
print("returned")
"""


@pytest.mark.parametrize("edit,words", [
    ("pass", None),
    ("flags = 3", None),
    ("ive[1] = 130", [b"interval 1", b"start >= end"]),
    ("ive[0] = 1 << 31", [b"interval 0", b"2^31"]),
    ("kw['min_match'] = (3, 2)", [b"num = 3", b"den = 2"]),
    ("kw['min_match'] = (0, 0)", [b"den = 0"]),
    ("kw['min_match'] = (1, (1 << 20) + 1)", [b"den = 1048577"]),
    ("flags = 4", [b"flags = 4"]),
    ("obe[0] += 1", [b"chain 0, block 0", b"lengths on the two axes differ"]),
    ("kw['ostrand'] = [1]", [b"chain 0 (ostrand 1)", b"ascend"]),
    ("bs[1] = 119", [b"chain 0", b"overlap or descend at block 1"]),
])
def test_bad_input_fails_with_a_message(edit, words):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), edit)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if words is None:  # the unedited input returns: the failures below are the edits'
        assert r.returncode == 0 and b"returned" in r.stdout, r.stderr
        return
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"LiftIntervals" in r.stderr and all(w in r.stderr for w in words), r.stderr
