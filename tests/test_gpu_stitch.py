"""GPU: sa_stitch_chains (include/segalign_amd.h) against the model of tests/stitch_model.py, which runs the serial link
checker tests/cpp/stitch_check.c.  Every test compares every field of every record, link and op, and first asserts with the model that its
input is in the regime it names.

One target and one query are built piece by piece, so the members and the links between them are known: a member is a stretch both
sequences share, a link a stretch of dt target bases against dq query bases that are a mutated copy with indels of them."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import stitch_model as S
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
EDGES = [126, 127, 128, 254, 255, 256, 510, 511, 512, 1086, 1087, 1088, 2047, 2048]
UNIT = np.full(64, -1, dtype=np.int32)
UNIT[[0, 9, 18, 27]] = 1


def revcomp(a):
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return comp[a[::-1]]


class Builder:
    """Target and query grown side by side."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.t, self.q, self.nt, self.nq, self.hsps = [], [], 0, 0, []

    def bases(self, n):
        return ACGT[self.rng.integers(0, 4, n)]

    def put(self, t, q):
        self.t.append(np.asarray(t, dtype=np.uint8))
        self.q.append(np.asarray(q, dtype=np.uint8))
        self.nt += len(t)
        self.nq += len(q)

    def member(self, n, seq=None):
        s = self.bases(n) if seq is None else seq
        self.hsps.append((self.nt, self.nq, n - 1, 0))
        self.put(s, s)
        return len(self.hsps) - 1

    def mutated(self, t, dq, sub_rate=0.1):
        """A copy of t with substitutions, then bases dropped or inserted at random places until dq are left."""
        q = t.copy()
        hit = self.rng.random(q.size) < sub_rate
        q[hit] = self.bases(int(hit.sum()))
        if q.size > dq:
            q = q[np.sort(self.rng.choice(q.size, dq, replace=False))]
        while q.size < dq:
            at = int(self.rng.integers(0, q.size + 1))
            q = np.concatenate([q[:at], self.bases(min(dq - q.size, int(self.rng.integers(1, 9)))), q[at:]])
        return q

    def link(self, dt, dq):
        t = self.bases(dt)
        self.put(t, self.mutated(t, dq))

    def chain(self, links, member=24):
        """Members of `member` bases with a (dt, dq) link, or a ready (t, q) pair of pieces, between each two: -> the chain's HSP indices."""
        out = [self.member(member)]
        for l in links:
            if isinstance(l[0], (int, np.integer)):
                self.link(*l)
            else:
                self.put(*l)
            out.append(self.member(member))
        self.put(self.bases(7), self.bases(11))  # unrelated sequence between chains
        return out


def ascii_(s):
    return np.frombuffer(s, dtype=np.uint8)


def build_world():
    b = Builder(2024)
    W = {}
    W["small"] = [b.chain([(dt, dq)]) for dt in (0, 1, 2) for dq in (0, 1, 2)]
    W["edges"] = [b.chain([(dt, dq)]) for dt in EDGES for dq in (1, 70)]
    W["transposed"] = [b.chain([(1, 2048)]), b.chain([(70, 2048)])]
    sq = b.bases(2048)
    W["square"] = [b.chain([(sq, b.mutated(b.mutated(sq, 2010, 0.04), 2048, 0.04))])]  # bases dropped, then others inserted
    for name, swap in (("d_runs", False), ("i_runs", True)):
        W[name] = []
        for n in (70, 130, 300):
            pre, extra, suf = b.bases(40), b.bases(n), b.bases(40)
            long_, short = np.concatenate([pre, extra, suf]), np.concatenate([pre, suf])
            W[name].append(b.chain([(short, long_) if swap else (long_, short)]))
    W["homopolymer"] = [b.chain([(ascii_(b"A" * 50), ascii_(b"A" * 45))], member=12)]
    W["period5"] = [b.chain([(ascii_(b"ACGTT" * 20), ascii_(b"ACGTT" * 17))]), b.chain([(ascii_(b"ACGTT" * 13), ascii_(b"ACGTT" * 20 + b"AC"))])]
    W["break"] = [b.chain([(100, 90)])]
    tsep, qsep = b.bases(60), b.bases(60)
    tsep2 = tsep.copy()
    tsep2[31] = ord("&")
    qsep2 = qsep.copy()
    qsep2[17] = ord("&")
    W["separators"] = [b.chain([(50, 50), (tsep2, b.mutated(tsep, 55)), (40, 44)]), b.chain([(qsep, qsep2), (30, 30)])]
    W["shapes"] = [b.chain([]), b.chain([(30, 26)]), b.chain([(int(b.rng.integers(0, 25)), int(b.rng.integers(0, 25))) for _ in range(64)]),
                   b.chain([(int(b.rng.integers(0, 12)), int(b.rng.integers(0, 12))) for _ in range(299)], member=8)]
    c = b.chain([(40, 35), (60, 66), (20, 20)])
    W["shared"] = [c, c[1:], [c[0], c[2]], [c[0], c[3]], c[:2]]
    sizes = np.array([0, 1, 5, 20, 60, 130, 260, 520])
    weight = np.array([2, 2, 4, 6, 6, 3, 1.5, 0.5])
    for k, n in enumerate((200, 300, 400, 600, 800, 1000)):
        links = []
        for _ in range(n):
            dt = int(b.rng.choice(sizes, p=weight / weight.sum()))
            dt = int(b.rng.integers(dt // 2, dt + 1))
            links.append((dt, max(0, dt + int(b.rng.integers(-min(dt, 12), 13)))))
        cuts = np.sort(b.rng.choice(np.arange(1, n), n // 40, replace=False)).tolist()
        W["random%d" % k] = [b.chain(links[a:e], member=int(b.rng.integers(8, 40))) for a, e in zip([0] + cuts, cuts + [n])]
    t, q = np.concatenate(b.t), np.concatenate(b.q)
    return t, q, S.make(b.hsps), W


def setup(E, t, q, sub=SUB):
    Case(t, q, chunk=250_000, sub_mat=sub).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(revcomp(q), 0, q.size, 1)


class World:
    pass


@pytest.fixture(scope="module")
def world(engine):
    E = engine
    w = World()
    w.E = E
    w.t, w.q, w.hsps, w.chains = build_world()
    setup(E, w.t, w.q)
    w.ref = E.copy_ref_codes()
    w.codes = {(buf, rev): E.copy_query_codes(buf, rev) for buf in (0, 1) for rev in (False, True)}
    assert np.array_equal(w.codes[(0, False)], w.codes[(1, True)])
    w.sub = SUB
    yield w
    E.ShutdownProcessor()


COUNTS = ("links", "swept", "long_links", "dead_links", "low_links", "cells", "records")


def run(w, chains, rev=False, buf=0, **kw):
    """One engine call held against the model, field for field.  -> (the model's records, ops, links, the engine's stats)."""
    members, first = S.csr(chains)
    recs, ops, links, cnt = S.stitch(w.ref, w.codes[(buf, rev)], w.sub, w.hsps, members, first, **kw)
    g_recs, g_ops, g_links, st = w.E.StitchChains(w.hsps, members, first, rev, buf, links=True, **kw)
    assert g_links.size == links.size
    for f in S.LINK_DTYPE.names:
        assert np.array_equal(g_links[f], links[f]), (f, np.flatnonzero(g_links[f] != links[f])[:8])
    assert g_recs.size == recs.size
    for f in S.RECORD_DTYPE.names:
        assert np.array_equal(g_recs[f], recs[f]), (f, np.flatnonzero(g_recs[f] != recs[f])[:8])
    assert np.array_equal(g_ops, ops)
    for k in COUNTS:
        assert st[k] == cnt[k], k
    S.check_invariants(w.ref, w.codes[(buf, rev)], w.sub, g_recs, g_ops, kw.get("gap_open", 400), kw.get("gap_extend", 30))
    only_r, only_o, _ = w.E.StitchChains(w.hsps, members, first, rev, buf, **kw)  # without the links
    assert np.array_equal(only_r, g_recs) and np.array_equal(only_o, g_ops)
    return recs, ops, links, st


def gap_runs(ops, op):
    return sorted((ops[(ops & 3) == op] >> 2).tolist())


def test_sides_of_0_1_and_2(world):
    recs, ops, links, _ = run(world, world.chains["small"])
    assert sorted(zip(links["dt"].tolist(), links["dq"].tolist())) == [(a, b) for a in (0, 1, 2) for b in (0, 1, 2)]
    assert np.all(links["flags"] == 0) and recs.size == 9 and np.all(recs["n_members"] == 2)
    for l in links:
        if l["dt"] == 0 or l["dq"] == 0:
            k = int(l["dt"]) + int(l["dq"])
            assert int(l["score"]) == (-(400 + 30 * k) if k else 0)


def test_every_instance_edge(world):
    recs, ops, links, st = run(world, world.chains["edges"])
    assert links["dt"].tolist() == [dt for dt in EDGES for _ in (1, 70)] and links["dq"].tolist() == [1, 70] * len(EDGES)
    ks = [S.instance(int(dt)) for dt in links["dt"]]
    assert [ks.count(k) for k in S.INSTANCES] == [4, 6, 6, 6, 6]  # 126, 127 | 128 .. 255 | 256 .. 511 | 512 .. 1087 | 1088 .. 2048
    assert np.all(links["flags"] == 0) and st["trace_bytes"] > 0


def test_the_transposes_and_the_square(world):
    recs, ops, links, _ = run(world, world.chains["transposed"] + world.chains["square"])
    assert list(zip(links["dt"].tolist(), links["dq"].tolist())) == [(1, 2048), (70, 2048), (2048, 2048)]
    assert np.all(links["flags"] == 0) and int(links[2]["cells"]) == 2049 * 2049
    assert int(recs[2]["matches"]) > 1400 and int(recs[2]["gap_opens"]) > 10  # a real alignment of the mutated copy


@pytest.mark.parametrize("name,op", [("d_runs", S.OP_D), ("i_runs", S.OP_I)])
def test_single_long_gap_runs(world, name, op):
    recs, ops, links, _ = run(world, world.chains[name])
    for k, n in enumerate((70, 130, 300)):
        o = S.record_ops(recs, ops, k)
        assert gap_runs(o, op) == [n] and gap_runs(o, 3 - op) == [] and (o & 3).tolist() == [0, op, 0]
        assert (int(recs[k]["gap_opens"]), int(recs[k]["gap_bases"]), int(recs[k]["mismatches"])) == (1, n, 0)


def test_a_homopolymer(world):
    recs, ops, links, _ = run(world, world.chains["homopolymer"])
    assert (int(links[0]["dt"]), int(links[0]["dq"])) == (50, 45)
    assert (ops & 3).tolist().count(S.OP_D) == 1 and gap_runs(ops, S.OP_D) == [5] and int(recs[0]["mismatches"]) == 0
    for kw in (dict(gap_open=0, gap_extend=1), dict(gap_open=0, gap_extend=0), dict(gap_open=91, gap_extend=91)):
        run(world, world.chains["homopolymer"] + world.chains["small"], **kw)


@contextlib.contextmanager
def restarted(w, sub=SUB, **options):
    """The engine shut down and set up again with another matrix or other options; the module's set-up comes back afterwards."""
    E = w.E
    E.ShutdownProcessor()
    for k, v in options.items():
        E.set_option(k, v)
    try:
        setup(E, w.t, w.q, sub)
        w.sub = sub
        yield
    finally:
        E.ShutdownProcessor()
        for k in options:
            E.reset_option(k)
        w.sub = SUB
        setup(E, w.t, w.q)


def test_a_period_5_repeat_under_a_unit_matrix(world):
    with restarted(world, UNIT):
        for kw in (dict(gap_open=1, gap_extend=1), dict(gap_open=0, gap_extend=1), dict(gap_open=3, gap_extend=0)):
            chains = world.chains["period5"] + world.chains["homopolymer"] + world.chains["shapes"][:3]
            recs, ops, links, _ = run(world, chains, **kw)
            # the repeat fits in many ways that score alike: the unit of the gap can sit anywhere, the tie rules decide
            runs = gap_runs(S.record_ops(recs, ops, 0), S.OP_D)
            assert sum(runs) == 15 and (len(runs) == 1 or kw["gap_open"] == 0) and int(recs[0]["mismatches"]) == 0
            assert gap_runs(S.record_ops(recs, ops, 0), S.OP_I) == []
    run(world, world.chains["small"])  # back under the module's matrix


def test_max_link_at_the_side_and_one_below(world):
    c = world.chains["break"]
    recs, _, links, _ = run(world, c, max_link=100)
    assert links["flags"].tolist() == [0] and recs.size == 1 and (int(links[0]["dt"]), int(links[0]["dq"])) == (100, 90)
    recs, _, links, st = run(world, c, max_link=99)
    assert links["flags"].tolist() == [S.LONG] and recs["flags"].tolist() == [S.LONG, 0] and st["swept"] == 0 and st["batches"] == 0
    recs, _, links, _ = run(world, world.chains["transposed"], max_link=2047)  # the query side counts too
    assert links["flags"].tolist() == [S.LONG, S.LONG]


def test_min_link_score_at_the_score_and_one_above(world):
    c = world.chains["break"]
    _, _, links, _ = run(world, c)
    s = int(links[0]["score"])
    recs, _, links, _ = run(world, c, min_link_score=s)
    assert links["flags"].tolist() == [0] and recs.size == 1
    recs, _, links, st = run(world, c, min_link_score=s + 1)
    assert links["flags"].tolist() == [S.LOW] and int(links[0]["score"]) == s and recs["flags"].tolist() == [S.LOW, 0] and st["low_links"] == 1


def test_a_separator_in_either_range(world):
    recs, _, links, st = run(world, world.chains["separators"])
    assert links["flags"].tolist() == [0, S.DEAD, 0, S.DEAD, 0]
    assert recs["n_members"].tolist() == [2, 2, 1, 2] and recs["flags"].tolist() == [S.DEAD, 0, S.DEAD, 0] and st["dead_links"] == 2
    # the target's separator lies in the second link of chain 0, the query's in the first link of chain 1
    l1, l3 = links[1], links[3]
    m = world.hsps[world.chains["separators"][0][1]]
    re_ = int(m["ref_start"]) + int(m["len"]) + 1
    assert np.any(world.ref[re_:re_ + int(l1["dt"])] == 7)
    m = world.hsps[world.chains["separators"][1][0]]
    qe = int(m["query_start"]) + int(m["len"]) + 1
    assert np.any(world.codes[(0, False)][qe:qe + int(l3["dq"])] == 7)


@pytest.mark.parametrize("buf,rev", [(1, True), (0, True), (1, False)])
def test_the_other_strand_and_buffer(world, buf, rev):
    # (1, True) is the strand the HSPs were built on; on the two others the same coordinates name unrelated sequence, which is as valid
    chains = world.chains["small"] + world.chains["edges"][::3] + world.chains["d_runs"] + world.chains["random0"]
    recs, _, links, _ = run(world, chains, rev=rev, buf=buf)
    if (buf, rev) == (1, True):
        assert int(recs["matches"].sum()) > 5 * int(recs["mismatches"].sum())
    else:
        assert int(recs["matches"].sum()) < 2 * int(recs["mismatches"].sum()) + int(recs["gap_bases"].sum())


def test_chains_of_1_2_65_and_300_members(world):
    recs, _, links, _ = run(world, world.chains["shapes"])
    assert [len(c) for c in world.chains["shapes"]] == [1, 2, 65, 300]
    assert recs["n_members"].tolist() == [1, 2, 65, 300] and links.size == 0 + 1 + 64 + 299


def test_chains_that_share_an_hsp(world):
    chains = world.chains["shared"] + [[]] + world.chains["shared"][::-1]
    recs, _, links, _ = run(world, chains)
    assert recs["chain"].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]
    assert len(set(np.concatenate(chains).tolist())) == 4 and sum(len(c) for c in chains) == 26


def test_a_trace_budget_of_one_mib_gives_identical_results(world):
    chains = world.chains["square"] + world.chains["edges"][::3] + world.chains["random1"]
    members, first = S.csr(chains)
    want = world.E.StitchChains(world.hsps, members, first, False, 0, links=True)
    assert {S.instance(int(l["dt"])) for l in want[2] if l["dt"] + l["dq"]} == set(S.INSTANCES)
    assert want[3]["batches"] == 5  # one per instance
    with restarted(world, gapped_trace_mb=1):
        _, _, links, st = run(world, chains)
        got = world.E.StitchChains(world.hsps, members, first, False, 0, links=True)
    sq = int(np.flatnonzero(links["dt"] == 2048)[0])
    assert S.instance(2048) == 33 and (2048 + 2048) * 64 * 5 * 4 > (1 << 20)  # the square's trace area alone is above the budget
    assert got[3]["batches"] > 5 and got[3]["trace_bytes"] == want[3]["trace_bytes"] and int(links[sq]["flags"]) == 0
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    assert world.E.StitchChains(world.hsps, members, first, False, 0)[2]["batches"] == 5  # back on the default budget


@pytest.mark.parametrize("k", range(6))
def test_random_sets(world, k):
    chains = world.chains["random%d" % k]
    n = sum(len(c) - 1 for c in chains)
    assert n == (200, 300, 400, 600, 800, 1000)[k]
    kw = [dict(), dict(gap_open=200, gap_extend=60), dict(max_link=200), dict(min_link_score=0), dict(gap_open=0, gap_extend=45),
          dict(max_link=64, min_link_score=-500)][k]
    recs, _, links, st = run(world, chains, **kw)
    assert len({S.instance(int(l["dt"])) for l in links}) >= 3  # mixed sizes
    assert int(recs["gap_opens"].sum()) > n // 20
    if "max_link" in kw:
        assert st["long_links"] > 0
    if "min_link_score" in kw:
        assert st["low_links"] > 0
    assert st["swept"] > n // 2


def test_eight_concurrent_callers_get_the_serial_results(world):
    names = ["random0", "edges", "shapes", "random2", "small", "d_runs", "random1", "separators"]
    jobs = []
    for k, name in enumerate(names):
        members, first = S.csr(world.chains[name])
        jobs.append((members, first, bool(k % 2), k % 2, dict(gap_open=400 - 30 * k, max_link=(0, 300)[k % 2])))

    def call(members, first, rev, buf, kw):
        return world.E.StitchChains(world.hsps, members, first, rev, buf, links=True, **kw)[:3]

    serial = [call(*j) for j in jobs]
    results = [None] * len(jobs)

    def work(i):
        for _ in range(3):
            r = call(*jobs[i])
            if results[i] is None or all(np.array_equal(a, b) for a, b in zip(results[i], r)):
                results[i] = r
            else:
                results[i] = "differs"
    th = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(len(jobs)):
        assert results[i] != "differs" and all(np.array_equal(a, b) for a, b in zip(results[i], serial[i])), i


def test_empty_inputs(world):
    E = world.E
    for members, first in (([], [0]), ([], [0, 0, 0])):
        recs, ops, links, st = E.StitchChains(world.hsps, members, first, False, 0, links=True)
        assert recs.size == ops.size == links.size == 0 and st["records"] == 0 and st["batches"] == 0


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
from gapped_model import SUB
from helpers import Case
rng = np.random.default_rng(1)
t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4000)]
Case(t, t.copy(), sub_mat=SUB).engine_setup(E, num_gpu=1)
h = np.array(%s, dtype=E.SEG_DTYPE)
r = E.StitchChains(h, %s, %s, False, 0, **%s)
print("returned", len(r[0]))
"""


@pytest.mark.parametrize("what,hsps,members,first,kw", [
    ("does not end before", [(100, 100, 19, 0), (119, 130, 9, 0)], [0, 1], [0, 2], {}),          # one target base of overlap
    ("inside the block", [(100, 100, 19, 0), (3990, 3000, 19, 0)], [0, 1], [0, 2], {}),
    ("not in the input", [(100, 100, 19, 0)], [0, 1], [0, 2], {}),
    ("gap_extend", [(100, 100, 19, 0)], [0], [0, 1], dict(gap_extend=-1)),
    ("headroom", [(100, 100, 19, 0)], [0], [0, 1], dict(gap_extend=1 << 17)),
])
def test_bad_input_fails_with_a_message(what, hsps, members, first, kw):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), hsps, members, first, kw)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout, (r.returncode, r.stderr[-300:])
    assert b"StitchChains" in r.stderr and what.encode() in r.stderr

