"""GPU: sa_trim_chains (include/segalign_amd.h) against the model of tests/chain_trim_model.py: every field of every
trimmed HSP, chain and link, each regime asserted with the model first.  One target and one query are built so that the members and
their overlaps are known: a member is a stretch the query copies from the target with mismatches, and where a test needs a certain
crossover the columns of the overlap are set by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_trim_model as T
import hsp_chain_model as M
import hsp_chain_overlap_model as O
import stitch_model as S
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
OVERLAPS = [1, 63, 64, 65, 128, 129, 4096]
N = 400_000


def revcomp(a):
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return comp[a[::-1]]


def other(x):
    """Another base for every base."""
    return ACGT[(np.searchsorted(ACGT, x) + 1) % 4]


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.t, self.q = ACGT[self.rng.integers(0, 4, N)], ACGT[self.rng.integers(0, 4, N)]
        self.rows, self.at = [], 1000

    def member(self, r, s, b, rate=0.15):
        self.rows.append((r, s, b - 1, 1000 + len(self.rows)))  # the input score is arbitrary: an untouched member returns it
        self.q[s:s + b] = np.where(self.rng.random(b) < rate, other(self.t[r:r + b]), self.t[r:r + b])
        return len(self.rows) - 1

    def chain(self, bases, links, rate=0.15):
        """Members of bases[k] bases; links[k] = (kind, o, gap): the overlap on both axes alike ("both"), on the target only ("t", the
        query gap is gap), on the query only ("q"), or on both by unequal amounts ("uneq": o on the target, o // 2 on the query)."""
        r = s = self.at
        out = []
        for k, b in enumerate(bases):
            out.append(self.member(r, s, b, rate))
            if k == len(links):
                break
            kind, o, gap = links[k]
            r, s = {"both": (r + b - o, s + b - o), "t": (r + b - o, s + b + gap), "q": (r + b + gap, s + b - o),
                    "uneq": (r + b - o, s + b - o // 2)}[kind]
        self.at = max(r, s) + bases[-1] + 50
        assert self.at < N - 100
        return out

    def set_columns(self, m, lo, hi, match):
        """Columns lo .. hi of member m all match or all mismatch."""
        r, s = self.rows[m][0], self.rows[m][1]
        self.q[s + lo:s + hi] = self.t[r + lo:r + hi] if match else other(self.t[r + lo:r + hi])


def build_world():
    b = Builder(77)
    W = {}
    W["sizes"] = [b.chain([2 * o + 1 + 40, 2 * o + 1 + 9], [(kind, o, 5)]) for o in OVERLAPS for kind in ("t", "q", "both", "uneq")]
    W["none"] = [b.chain([30, 40, 50], [("t", 0, 0), ("q", 0, 7)]), b.chain([25], [])]
    # x = o: j matches in the overlap, i does not; x = 0: the other way round; both on a target-only overlap of 70 (two chunks)
    c = b.chain([200, 200], [("t", 70, 3)])
    b.set_columns(c[0], 130, 200, True)
    b.set_columns(c[1], 0, 70, False)
    W["x_is_o"] = [c]
    c = b.chain([200, 200], [("t", 70, 3)])
    b.set_columns(c[0], 130, 200, False)
    b.set_columns(c[1], 0, 70, True)
    W["x_is_0"] = [c]
    # ties: both members match in every shared column, S is flat; and a plateau that starts in the second chunk
    c = b.chain([300, 300], [("t", 100, 2)])
    b.set_columns(c[0], 200, 300, True)
    b.set_columns(c[1], 0, 100, True)
    W["flat"] = [c]
    c = b.chain([300, 300], [("t", 100, 2)])
    b.set_columns(c[0], 200, 300, True)
    b.set_columns(c[1], 0, 100, True)
    b.set_columns(c[1], 0, 80, False)  # S rises up to x = 80 and is flat from there: the lowest x of the plateau is 80
    W["plateau"] = [c]
    # a member of 7 bases cut at both ends down to one base
    c = b.chain([40, 7, 40], [("t", 3, 6), ("t", 3, 4)])
    b.set_columns(c[0], 37, 40, True)
    b.set_columns(c[1], 0, 3, False)
    b.set_columns(c[1], 4, 7, False)
    b.set_columns(c[2], 0, 3, True)
    W["one_base"] = [c]
    rng = b.rng
    W["random"] = []
    for _ in range(40):
        bases = [int(x) for x in rng.integers(3, 300, int(rng.integers(2, 40)))]
        links = [(["t", "q", "both", "uneq"][int(rng.integers(0, 4))], int(rng.integers(0, (min(x, y) - 1) // 2 + 1)) * int(rng.integers(0, 2)),
                  int(rng.integers(0, 30))) for x, y in zip(bases, bases[1:])]
        W["random"].append(b.chain(bases, links))
    return b.t, b.q, M.make([(r, s, n + 1, sc) for r, s, n, sc in b.rows]), W


class World:
    pass


@pytest.fixture(scope="module")
def world(engine):
    E = engine
    w = World()
    w.E = E
    w.t, w.q, w.hsps, w.chains = build_world()
    Case(w.t, w.q, chunk=250_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(revcomp(w.q), 0, w.q.size, 1)
    w.ref = E.copy_ref_codes()
    w.codes = {(buf, rev): E.copy_query_codes(buf, rev) for buf in (0, 1) for rev in (False, True)}
    assert np.array_equal(w.codes[(0, False)], w.codes[(1, True)])
    yield w
    E.ShutdownProcessor()


def run(w, chains, rev=False, buf=0, **kw):
    """One engine call held against the model, field for field.  -> the model's (out, chains, links), the engine's stats."""
    members, first = S.csr(chains)
    out, ch, links = T.trim(w.ref, w.codes[(buf, rev)], SUB, w.hsps, members, first, **kw)
    g_out, g_ch, g_links, st = w.E.TrimChains(w.hsps, members, first, rev, buf, links=True, **kw)
    for got, want in ((g_out, out), (g_ch, ch), (g_links, links)):
        assert got.size == want.size
        for f in want.dtype.names:
            assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8])
    assert (st["chains"], st["members"], st["links"]) == (len(chains), members.size, links.size)
    assert (st["trimmed_links"], st["bases_cut"]) == (int((links["o"] > 0).sum()), int(links["o"].sum()))
    assert st["cut_members"] == int(sum(1 for k in range(out.size) if O.node(out, k)[:3] != O.node(w.hsps, int(members[k]))[:3]))
    only = w.E.TrimChains(w.hsps, members, first, rev, buf, **kw)  # without the links
    assert np.array_equal(only[0], g_out) and np.array_equal(only[1], g_ch)
    return out, ch, links, st


def test_every_overlap_size_on_every_axis(world):
    out, ch, links, _ = run(world, world.chains["sizes"])
    assert links["o"].tolist() == [o for o in OVERLAPS for _ in range(4)]
    gaps = list(zip(links["gap_r"].tolist(), links["gap_q"].tolist()))
    for k, o in enumerate(OVERLAPS):
        assert gaps[4 * k:4 * k + 4] == [(0, o + 5), (o + 5, 0), (0, 0), (0, o - o // 2)]
    both = links[2::4]
    assert np.all(both["x"] == 0)  # the same columns in both members: S is flat
    rest = np.concatenate([links[0::4], links[1::4], links[3::4]])
    assert ((rest["x"] > 0) & (rest["x"] < rest["o"])).sum() >= 8 and (rest["x"] > 64).any() and (rest["x"] > 2048).any()


def test_the_winners_at_both_ends_and_the_lowest_x_among_equals(world):
    w = world
    _, _, links, _ = run(w, w.chains["x_is_o"] + w.chains["x_is_0"] + w.chains["flat"] + w.chains["plateau"])
    assert [tuple(int(v) for v in l)[:2] for l in links] == [(70, 70), (70, 0), (100, 0), (100, 80)]
    m = w.chains["plateau"][0]
    a = T.columns(w.ref, w.codes[(0, False)], SUB, *[v + 200 for v in O.node(w.hsps, m[0])[:2]], 100)
    b = T.columns(w.ref, w.codes[(0, False)], SUB, *O.node(w.hsps, m[1])[:2], 100)
    s = [sum(a[:x]) + sum(b[x:]) for x in range(101)]
    assert s[80] == max(s) and s[79] < s[80] and s[80:] == [s[80]] * 21


def test_a_member_cut_at_both_ends_down_to_one_base(world):
    out, ch, links, st = run(world, world.chains["one_base"])
    assert [tuple(int(v) for v in l)[:2] for l in links] == [(3, 3), (3, 0)]
    mid = O.node(world.hsps, world.chains["one_base"][0][1])
    assert O.node(out, 1)[:3] == (mid[0] + 3, mid[1] + 3, 1) and st["cut_members"] == 1
    assert out[0] == world.hsps[world.chains["one_base"][0][0]] and out[2] == world.hsps[world.chains["one_base"][0][2]]


def test_chains_without_overlaps_come_back_bit_for_bit(world):
    out, ch, links, st = run(world, world.chains["none"], diag_pen=2, anti_pen=1)
    members, _ = S.csr(world.chains["none"])
    assert np.array_equal(out, world.hsps[members].astype(out.dtype)) and np.all(links["o"] == 0) and st["cut_members"] == 0
    assert int(ch["score"][1]) == int(world.hsps["score"][members[3]]) and int(ch["score"][0]) == int(world.hsps["score"][members[:3]].sum()) - 2 * 7 - 7


@pytest.mark.parametrize("kw", [dict(), dict(diag_pen=3, anti_pen=2), dict(gap_costs="loose", anti_pen=1)])
def test_random_chains_under_every_penalty(world, kw):
    out, ch, links, st = run(world, world.chains["random"], **kw)
    assert (links["o"] > 0).sum() > 100 and ((links["x"] > 0) & (links["x"] < links["o"])).sum() > 30
    assert sum(1 for c in world.chains["random"] if len(c) > 2) > 20 and st["cut_members"] > 150
    first = S.csr(world.chains["random"])[1]
    for c in range(len(first) - 1):
        for k in range(int(first[c]), int(first[c + 1]) - 1):
            assert M.precedes(out, None, k, k + 1)


def test_the_other_strand_and_the_second_buffer(world):
    w = world
    chains = w.chains["random"][:12] + w.chains["one_base"]
    want = run(w, chains)
    got = run(w, chains, rev=True, buf=1)  # buffer 1 holds the reverse complement: its minus strand is buffer 0's plus strand
    assert all(np.array_equal(a, b) for a, b in zip(want[:3], got[:3]))
    # and a strand the members were not made for: other columns, other crossovers, still the model's
    small = [c for c in w.chains["random"] if all(O.node(w.hsps, i)[1] + O.node(w.hsps, i)[2] <= w.q.size for i in c)][:12]
    other_strand = run(w, small, rev=True, buf=0)
    assert not np.array_equal(other_strand[2]["x"], run(w, small)[2]["x"])


def test_the_trimmed_chains_stitch_as_the_stitch_model_says(world):
    w = world
    chains = w.chains["random"][:15] + w.chains["one_base"] + w.chains["sizes"][:8]
    out, ch, links, _ = run(w, chains)
    first = S.csr(chains)[1]
    members = np.arange(out.size, dtype=np.uint32)
    recs, ops, slinks, cnt = S.stitch(w.ref, w.codes[(0, False)], SUB, out, members, first)
    g_recs, g_ops, g_links, st = w.E.StitchChains(out, members, first, False, 0, links=True)
    assert g_recs.size == recs.size and all(np.array_equal(g_recs[f], recs[f]) for f in S.RECORD_DTYPE.names) and np.array_equal(g_ops, ops)
    assert np.array_equal(g_links["dt"], links["gap_r"]) and np.array_equal(g_links["dq"], links["gap_q"])


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_chain_trim as W
import stitch_model as S
from gapped_model import SUB
from helpers import Case
from segalign_amd import engine as E
t, q, hsps, chains = W.build_world()
if %d:
    Case(t, q, chunk=250_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
else:
    E.InitializeInterface(1)
h = hsps.copy()
members, first = S.csr(chains["one_base"])
what = %r
if what == "stitch":
    E.StitchChains(h, members, first, False, 0)
else:
    if what == "outside":
        h[members[2]]["ref_start"] = t.size - 5
    if what == "half":
        h[members[1]]["len"] = 5
    if what == "far":
        h = S.make([(1000, 1000, 9999, 1), (1000 + 10000 - 4097, 1000 + 10000 - 4097, 9999, 1)])
        members, first = np.array([0, 1], dtype=np.uint32), np.array([0, 2], dtype=np.uint32)
    if what == "index":
        members = members.copy(); members[0] = h.size
    if what == "first":
        first = first.copy(); first[0] = 1
    if what == "buffer":
        E.TrimChains(h, members, first, False, 7)
    E.TrimChains(h, members, first, False, 0, diag_pen=(1 << 21) if what == "diag_pen" else 0)
print("returned")
"""


@pytest.mark.parametrize("what,proc,message", [("stitch", 1, b"StitchChains"), ("outside", 1, b"inside the block"), ("half", 1, b"overlaps the next"),
                                               ("far", 1, b"overlaps the next"), ("index", 1, b"not in the input"), ("first", 1, b"first[0]"),
                                               ("diag_pen", 1, b"diag_pen"), ("buffer", 1, b"TrimChains"), ("no processor", 0, b"TrimChains")])
def test_what_is_refused_ends_the_process_with_a_message(what, proc, message):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), proc, what)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout, (r.returncode, r.stderr[-300:])
    assert message in r.stderr, r.stderr[-300:]


def test_the_far_overlap_is_accepted_at_4096(world):
    c = world.chains["sizes"][4 * OVERLAPS.index(4096):4 * OVERLAPS.index(4096) + 4]
    _, _, links, _ = run(world, c)
    assert links["o"].tolist() == [4096] * 4
