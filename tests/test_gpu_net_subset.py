"""GPU: sa_net_subset (include/segalign_amd.h) against the model of tests/net_subset_model.py.  Every test first asserts
with the models that its input is in the regime it names, then compares every field of every output HSP and sub-chain and the counts.

One target and one query are built piece by piece: random bases, the query a copy with substitutions (no indels, so any diagonal may
carry an HSP), with a separator and an N put where one case looks for them.  The chains are hand-built HSPs on them; the fills come
from tests/net_model.py, so every case is a whole net of its own and all cases share the one pair of sequences."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import hsp_chain_model as M
import net_model as N
import net_subset_model as NS
import stitch_model as S
from gapped_model import SUB
from helpers import Case as Setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LEN = 70_000
SEP_AT, N_AT = 60_050, 60_030  # a separator in the query, an N in the target
D = 137  # the diagonal offset of the hand-built HSPs: query_start = ref_start + D


def revcomp(a):
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return comp[a[::-1]]


def sequences():
    rng = np.random.default_rng(2121)
    t = ACGT[rng.integers(0, 4, LEN)]
    q = np.concatenate([ACGT[rng.integers(0, 4, D)], t])[:LEN].copy()  # q[x + D] = t[x], then substitutions
    hit = rng.random(LEN) < 0.08
    q[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    q[SEP_AT + D] = ord("&")
    t = t.copy()
    t[N_AT] = ord("N")
    return t, q


class World:
    pass


@pytest.fixture(scope="module")
def world(engine):
    E = engine
    w = World()
    w.E = E
    w.t, w.q = sequences()
    Setup(w.t, w.q, chunk=250_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(revcomp(w.q), 0, w.q.size, 1)
    w.ref = E.copy_ref_codes()
    w.codes = {(buf, rev): E.copy_query_codes(buf, rev) for buf in (0, 1) for rev in (False, True)}
    assert np.array_equal(w.ref, NS.encode(w.t)) and np.array_equal(w.codes[(0, False)], NS.encode(w.q))
    assert np.array_equal(w.codes[(1, True)], w.codes[(0, False)]) and not np.array_equal(w.codes[(0, True)], w.codes[(0, False)])
    yield w
    E.ShutdownProcessor()


_T, _Q = (NS.encode(x) for x in sequences())


def code_sum(rs, qs, n):
    return int(np.asarray(SUB, dtype=np.int64).reshape(64)[_T[rs:rs + n].astype(np.int64) * 8 + _Q[qs:qs + n].astype(np.int64)].sum())


class Net:
    """Chains of hand-built HSPs, their net on one axis from net_model, and the subset model's answer for the forward query."""

    def __init__(self, chains, scores, groups=None, axis="target", d=D, hsp_scores=None, **net_kw):
        # chains: [[(ref_start, bases) or (ref_start, bases, shift), ...], ...]; query_start = ref_start + d + shift (d: one value, or
        # one per chain)
        ds = d if isinstance(d, list) else [d] * len(chains)
        rows = [(x[0], x[0] + ds[c] + (x[2] if len(x) > 2 else 0), x[1], 0) for c, ch in enumerate(chains) for x in ch]  # M.make takes bases
        self.hsps = M.make(rows)
        self.hsps["score"] = [code_sum(r, q, n) for r, q, n, _ in rows] if hsp_scores is None else hsp_scores
        self.members = np.arange(len(rows), dtype=np.uint32)
        self.first = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
        self.axis = axis
        key = "ref_start" if axis == "target" else "query_start"
        self.bs = self.hsps[key].astype(np.uint32)
        self.be = (self.bs + self.hsps["len"] + 1).astype(np.uint32)
        self.scores = np.asarray(scores, dtype=np.int64)
        self.groups = None if groups is None else np.asarray(groups, dtype=np.uint32)
        self.fills, self.net_st = N.net(self.first, self.bs, self.be, self.scores, self.groups, **net_kw)
        self._want = {}

    def want(self, **kw):
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in self._want:
            self._want[key] = NS.subset(_T, _Q, SUB, self.hsps, self.members, self.first, self.fills, axis=self.axis, **kw)
        return self._want[key]


def held(w, net, rev=False, buf=0, **kw):
    """One engine call held against the model.  -> (the model's out_hsps, chains, stats)."""
    assert np.array_equal(w.codes[(buf, rev)], _Q)
    hs, ch, st = net.want(**kw)
    g_hs, g_ch, g_st = w.E.NetSubset(net.hsps, net.members, net.first, net.fills, rev, buf, axis=net.axis, **kw)
    assert g_hs.dtype == w.E.SEG_DTYPE and g_ch.dtype == w.E.SUBSET_CHAIN_DTYPE
    NS.same(g_hs, g_ch, hs, ch)
    for k in NS.COUNTS:
        assert g_st[k] == st[k], (k, g_st[k], st[k])
    assert g_st["subset_ms"] > 0
    return hs, ch, st


# ---- sizes ----
def test_no_fill(world):
    net = Net([[(100, 50)]], [5])
    hs, ch, st = world.E.NetSubset(net.hsps, net.members, net.first, net.fills[:0], False, 0)
    assert hs.size == 0 and ch.size == 0 and hs.dtype == world.E.SEG_DTYPE and ch.dtype == world.E.SUBSET_CHAIN_DTYPE
    assert (st["fills"], st["runs"], st["members"]) == (0, 0, 0)
    hs, ch, st = world.E.NetSubset(net.hsps[:0], [], [0], net.fills[:0], False, 0)
    assert hs.size == 0 and ch.size == 0


def test_one_fill_that_is_its_whole_chain(world):
    net = Net([[(100, 50), (160, 30), (200, 1)]], [5])
    hs, ch, st = held(world, net, diag_pen=3, anti_pen=2)
    assert ch.size == 1 and st["cut_members"] == 0 and int(ch["clipped"][0]) == 0 and np.array_equal(hs, net.hsps)
    assert int(ch["score"][0]) == int(net.hsps["score"].astype(np.int64).sum()) - 2 * (2 * 10 + 2 * 10)  # anti_pen over both gaps, no diagonal step


# ---- cut members ----
KEPT = [1, 2, 63, 64, 65, 129, 4097]


def cuts(L):
    """Three lower chains of one HSP each with L kept bases: cut on the left only, on the right only and on both sides."""
    x, y, z = 1000, 1000 + L + 200, 1000 + 2 * L + 500
    chains = [[(x, 50)], [(x + 20, 30 + L)],            # the first covers the second's first 30 bases
              [(y + L, 50)], [(y, L + 30)],              # ... its last 30
              [(z, 40), (z + 40 + L, 40)], [(z + 10, L + 60)]]  # the gap of L bases is all that is left of it
    return Net(chains, [9, 1, 9, 1, 9, 1])


@pytest.mark.parametrize("L", KEPT)
def test_cut_members_of_this_kept_length(world, L):
    net = cuts(L)
    hs, ch, st = net.want(split=True)
    mine = {int(c["chain"]): c for c in ch if int(c["chain"]) in (1, 3, 5)}
    assert [int(mine[c]["clipped"]) for c in (1, 3, 5)] == [1, 2, 3]  # left only, right only, both sides of one member
    assert all(int(hs["len"][int(mine[c]["first_member"])]) + 1 == L for c in (1, 3, 5))
    assert st["cut_members"] == 3 and st["bases_rescored"] == 3 * L and st["splits"] == 1 and st["runs"] == 7
    assert all(int(mine[c]["score"]) == code_sum(int(mine[c]["ref_start"]), int(mine[c]["query_start"]), L) for c in (1, 3, 5))
    held(world, net, split=True)
    held(world, net, split=False)


def test_a_separator_and_an_n_inside_a_cut_member(world):
    net = Net([[(SEP_AT - 100, 70)], [(SEP_AT - 60, 200)]], [9, 1])
    hs, ch, st = net.want()
    cut = hs[int(ch["first_member"][1])]
    assert st["cut_members"] == 1 and int(cut["ref_start"]) == SEP_AT - 30 < N_AT < SEP_AT < int(cut["ref_start"]) + int(cut["len"])
    assert _T[N_AT] == 5 and _Q[SEP_AT + D] == 7 and int(ch["score"][1]) == code_sum(SEP_AT - 30, SEP_AT - 30 + D, 170)  # as the matrix has them
    held(world, net)


# ---- blocks, gaps and children ----
def comb(teeth, x=2000, tooth=4, gap=6):
    return [(x + (tooth + gap) * k, tooth) for k in range(teeth)]


def child(k, x=2000, tooth=4, gap=6):
    """A one-HSP chain inside gap k of comb()."""
    return [(x + (tooth + gap) * k + tooth + 1, gap - 2)]


@pytest.mark.parametrize("blocks", [1, 2, 64, 65, 1025])
def test_one_fill_of_so_many_blocks(world, blocks):
    net = Net([comb(blocks)], [5])
    hs, ch, st = held(world, net, diag_pen=1, anti_pen=1, gap_costs="loose")
    assert ch.size == 1 and int(ch["n_members"][0]) == blocks and st["splits"] == 0


@pytest.mark.parametrize("blocks,gaps", [(2, [0]), (64, [0]), (64, [62]), (65, [0, 63]), (65, [63]), (1025, list(range(1024)))])
def test_children_in_the_first_the_last_and_every_gap(world, blocks, gaps):
    net = Net([comb(blocks)] + [child(k) for k in gaps], [10 ** 6] + [5] * len(gaps))
    hs, ch, st = net.want(diag_pen=2, gap_costs="medium")
    assert st["fills"] == 1 + len(gaps) and st["splits"] == len(gaps) and st["runs"] == 1 + 2 * len(gaps)
    top = ch[ch["fill"] == 0]
    bounds = [0] + [k + 1 for k in gaps] + [blocks]
    assert top["run"].tolist() == list(range(len(gaps) + 1)) and top["n_members"].tolist() == [b - a for a, b in zip(bounds, bounds[1:])]
    assert NS.hulls_disjoint(ch)
    held(world, net, diag_pen=2, gap_costs="medium")
    hs, ch, st = held(world, net, diag_pen=2, gap_costs="medium", split=False)  # the split flag off on the same input
    assert st["splits"] == 0 and st["runs"] == st["fills"] and (len(gaps) == 0 or not NS.hulls_disjoint(ch))


def test_two_children_in_one_gap_cut_once(world):
    net = Net([[(3000, 50), (3200, 50), (3300, 50)], [(3060, 40)], [(3120, 60)]], [9, 2, 3])
    hs, ch, st = held(world, net)
    assert net.fills["parent"].tolist() == [-1, 0, 0] and st["splits"] == 1 and ch["n_members"].tolist() == [1, 2, 1, 1]


def test_nesting_three_deep(world):
    net = Net([[(4000, 50), (5000, 50)], [(4100, 50), (4800, 50)], [(4200, 50), (4600, 50)], [(4300, 50)]], [9, 8, 7, 6])
    hs, ch, st = held(world, net, anti_pen=1)
    assert net.fills["depth"].tolist() == [0, 1, 2, 3] and st["runs"] == 7 and NS.hulls_disjoint(ch)


def test_a_gap_below_min_space_holds_no_child_and_gives_no_split(world):
    net = Net([[(3000, 50), (3090, 50)], [(3055, 30)]], [9, 5], min_space=41)
    hs, ch, st = held(world, net)
    assert net.fills.size == 1 and st["splits"] == 0 and st["runs"] == 1


# ---- the query axis ----
def test_the_query_axis_on_the_reverse_strand_of_buffer_1(world):
    # two diagonals: the chains overlap on the query where they do not on the target
    chains = [[(6000, 80), (6200, 80)], [(6700, 300)], [(6800 + 130, 30)]]
    net = Net(chains, [9, 4, 5], axis="query", d=[D + 700, D + 100, D])
    hs, ch, st = net.want()
    assert net.fills["chain"].tolist() == [0, 1, 1] and net.fills["parent"].tolist() == [-1, 0, -1]
    assert st["cut_members"] == 2 and st["splits"] >= 1 and NS.hulls_disjoint(ch, "query") and not np.array_equal(net.bs, net.hsps["ref_start"])
    held(world, net, rev=True, buf=1)
    assert not NS.hulls_disjoint(Net(chains, [9, 4, 5], d=[D + 700, D + 100, D]).want()[1], "query")  # the target net of the same chains


# ---- sums ----
def test_run_sums_below_zero_and_past_2_to_the_33(world):
    up = Net([comb(9)], [5], hsp_scores=[2 ** 31 - 1] * 9)
    hs, ch, st = held(world, up)
    assert int(ch["score"][0]) == 9 * (2 ** 31 - 1) > 2 ** 33
    down = Net([comb(9), child(3)], [5, 1], hsp_scores=[-2 ** 31] * 9 + [7])
    hs, ch, st = held(world, down, diag_pen=5)
    assert ch["score"].tolist() == [4 * -2 ** 31, 5 * -2 ** 31, 7]
    mixed = Net([comb(64)], [5], hsp_scores=[(-1) ** k * (2 ** 31 - 1 - k) for k in range(64)])
    held(world, mixed)


def test_penalties_at_2_to_the_20(world):
    net = Net([[(7000, 40), (9000, 40), (20000, 40, 3000)], [(7500, 40)]], [9, 1])  # the last link takes a diagonal step as well
    hs, ch, st = held(world, net, diag_pen=1 << 20, anti_pen=1 << 20, gap_costs="medium")
    assert ch["n_members"].tolist() == [1, 2, 1] and int(ch["score"][1]) < -2 ** 33 and st["splits"] == 1
    hs, ch, st = held(world, net, diag_pen=1 << 20, anti_pen=1 << 20, gap_costs="medium", split=False)
    assert int(ch["score"][0]) < -2 ** 33 - 2 ** 31


TABLE = {"pos": [1, 50, 2000], "q_gap": [10, 400, 500], "t_gap": [20, 300, 3000], "both_gap": [1, 2, 2_000_000]}


@pytest.mark.parametrize("costs", ["medium", TABLE])
def test_gap_cost_tables(world, costs):
    # the links: a gap in the query only (0, 20), none (0, 0), in the target only (30, 0), in both (5, 5), then the child's gap and a long
    # link in both past the last break point
    chains = [[(7000, 40), (7040, 40, 20), (7080, 40, 20), (7150, 40, -10), (7195, 40, -10), (9000, 40), (14000, 40, 900)], [(7300, 40)]]
    net = Net(chains, [9, 1])
    h = net.hsps
    gaps = [(int(h["ref_start"][k + 1]) - int(h["ref_start"][k]) - 40, int(h["query_start"][k + 1]) - int(h["query_start"][k]) - 40) for k in range(6)]
    assert gaps[:4] == [(0, 20), (0, 0), (30, 0), (5, 5)] and gaps[5] == (4960, 5860)
    hs, ch, st = held(world, net, gap_costs=costs)
    plain = net.want()[1]
    assert ch["n_members"].tolist() == [5, 2, 1] and np.all(ch["score"][:2] < plain["score"][:2]) and ch["score"][2] == plain["score"][2]


# ---- the pipeline on random sets ----
PARAMS = [dict(min_space=1, min_fill=1), dict(min_space=5, min_fill=12), dict(min_space=25, min_fill=3)]
PENS = [dict(), dict(diag_pen=1, anti_pen=0, gap_costs="loose"), dict(diag_pen=2, anti_pen=1)]
_sets = {}


def scatter(rng, n, diagonals, step=40, jitter=6):
    """n HSPs along a few diagonals, in shuffled input order (as tests/test_gpu_net.py builds them)."""
    rows = []
    for k in range(n):
        d = int(rng.integers(0, diagonals)) * 700 + int(rng.integers(-jitter, jitter + 1))
        q = 1000 + k * step // diagonals + int(rng.integers(0, step))
        rows.append((q + 20000 + d, q, int(rng.integers(5, 50)), int(rng.integers(-40, 3000))))
    return M.make(rows)[rng.permutation(n)]


class Pipe:
    pass


def pipeline(E, seed, k):
    """ChainHspsAll -> chain_csr -> net_blocks -> (model) net, once per (seed, parameter set)."""
    if (seed, k) not in _sets:
        rng = np.random.default_rng(5000 + seed)
        p = Pipe()
        p.h = scatter(rng, int(rng.integers(1500, 4001)), diagonals=10)
        p.g = rng.choice(np.array([3, 1, 900_000], dtype=np.uint32), size=p.h.size)
        p.pen = PENS[k]
        p.chains, members, _, _ = E.ChainHspsAll(p.h, p.g, max_gap=120, min_score=0, **p.pen)
        p.idx, p.first = E.chain_csr(members)
        p.bs, p.be = E.net_blocks(p.h, p.idx, p.first, axis="target")
        p.fills, p.net_st = N.net(p.first, p.bs, p.be, p.chains["score"], p.chains["group"], **PARAMS[k])
        p.want = NS.subset(_T, _Q, SUB, p.h, p.idx, p.first, p.fills, **p.pen)
        _sets[(seed, k)] = p
    return _sets[(seed, k)]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("seed", range(6))
def test_random_sets_through_the_pipeline(world, seed, k):
    E = world.E
    p = pipeline(E, seed, k)
    hs, ch, st = p.want
    assert 200 <= p.chains.size <= 2000 and p.net_st["max_depth"] >= 2
    both = sum(1 for c in ch if int(c["clipped"]) == 3 and int(c["n_members"]) == 1)
    assert st["cut_members"] >= 10 and st["splits"] >= 10 and both >= 1 and np.any(ch["clipped"] == 1) and np.any(ch["clipped"] == 2)
    got_f, _ = E.NetChains(p.first, p.bs, p.be, p.chains["score"], p.chains["group"], **PARAMS[k])
    N.same(got_f, p.fills)
    g_hs, g_ch, g_st = E.NetSubset(p.h, p.idx, p.first, got_f, False, 0, **p.pen)
    NS.same(g_hs, g_ch, hs, ch)
    assert all(g_st[c] == st[c] for c in NS.COUNTS)
    assert NS.hulls_disjoint(g_ch)  # consequence (a), at any thresholds
    # consequence (c): a fill that is its whole chain in one run, the chain not joined, scores what the chain scores
    whole = [c for c in g_ch if int(c["clipped"]) == 0 and int(c["n_members"]) == int(p.chains["n_members"][int(c["chain"])])
             and int(p.chains["joined"][int(c["chain"])]) < 0]
    assert len(whole) >= 10 and all(int(c["score"]) == int(p.chains["score"][int(c["chain"])]) for c in whole)
    if k == 0:  # consequence (d): the kept bases partition the union of the blocks
        own = {(int(c["group"]), x) for c in g_ch for m in g_hs[int(c["first_member"]):int(c["first_member"]) + int(c["n_members"])]
               for x in range(int(m["ref_start"]), int(m["ref_start"]) + int(m["len"]) + 1)}
        union = {(int(p.chains["group"][c]), x) for c in range(p.chains.size) for b in range(int(p.first[c]), int(p.first[c + 1]))
                 for x in range(int(p.bs[b]), int(p.be[b]))}
        assert own == union and len(own) == int(g_hs["len"].astype(np.int64).sum()) + g_hs.size
    # consequence (b): the output stitches, and the records keep single coverage of the axis
    mem, first = E.subset_csr(g_ch)
    assert np.array_equal(mem, NS.csr(ch)[0]) and np.array_equal(first, NS.csr(ch)[1])
    recs, ops, _ = E.StitchChains(g_hs, mem, first, False, 0)
    assert recs.size >= g_ch.size and np.array_equal(np.unique(recs["chain"]), np.arange(g_ch.size))
    rec_group = g_ch["group"][recs["chain"]]
    for g in np.unique(rec_group):
        mine = recs[rec_group == g]
        order = np.argsort(mine["ref_start"], kind="stable")
        assert np.all(mine["ref_end"][order][:-1] <= mine["ref_start"][order][1:])
    S.check_invariants(world.ref, world.codes[(0, False)], SUB, recs, ops)
    # reciprocal best: the sub-chains netted on the other axis
    qs, qe = E.net_blocks(g_hs, mem, first, axis="query")
    want_q, _ = N.net(first, qs, qe, g_ch["score"], g_ch["group"], **PARAMS[k])
    got_q, _ = E.NetChains(first, qs, qe, g_ch["score"], g_ch["group"], **PARAMS[k])
    N.same(got_q, want_q)
    assert 0 < want_q.size and np.unique(want_q["chain"]).size < g_ch.size  # the query axis drops some


def test_eight_threads_get_the_serial_results(world):
    E = world.E
    jobs = [pipeline(E, s, (s + 1) % 3) for s in range(6)] + [pipeline(E, 0, 0), pipeline(E, 1, 1)]
    out, errors = [None] * 8, []

    def work(i):
        try:
            p = jobs[i]
            out[i] = E.NetSubset(p.h, p.idx, p.first, p.fills, False, 0, **p.pen)
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(8):
        NS.same(out[i][0], out[i][1], jobs[i].want[0], jobs[i].want[1])


# ---- failures ----
CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_gpu_net_subset as T
from segalign_amd import engine as E
w = T.World()
t, q = T.sequences()
T.Setup(t, q, chunk=250_000, sub_mat=T.SUB).engine_setup(E, num_gpu=1)
net = T.Net([[(3000, 50), (3200, 50), (3300, 50)], [(3060, 40)]], [9, 2])
fills = net.fills.copy()
kw = {}
%s
E.NetSubset(net.hsps, net.members, net.first, fills, False, 0, **kw)
print("returned")
"""


@pytest.mark.parametrize("edit,words", [
    ("pass", None),
    ("fills['n_blocks'][0] = 4", [b"fill 0", b"blocks leave chain 0"]),
    ("fills['end'][0] = 3050; fills['n_blocks'][0] = 1", [b"fill 1", b"does not lie in a gap of its parent 0"]),
    ("kw = dict(diag_pen=(1 << 20) + 1)", [b"diag_pen", b"out of range"]),
    ("kw = dict(gap_costs={'pos': [2, 2], 'q_gap': [1, 2], 't_gap': [1, 2], 'both_gap': [1, 2]})", [b"gap costs", b"pos[1]"]),
])
def test_bad_input_fails_with_a_message(edit, words):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), edit)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if words is None:  # the unedited input returns: the failures below are the edits'
        assert r.returncode == 0 and b"returned" in r.stdout, r.stderr
        return
    assert r.returncode == 1 and b"returned" not in r.stdout
    assert b"NetSubset" in r.stderr and all(w in r.stderr for w in words), r.stderr
