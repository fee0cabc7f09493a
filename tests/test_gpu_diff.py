"""GPU: sa_diff_alignments (include/segalign_amd.h) against the model of tests/diff_model.py.  Every test compares every
field of every event, every summary and the pair counts, and first asserts with the model that its input is in the regime it names.

One target and one query are built side by side.  Their first part is the same sequence in both with differences planted at known
places, so a span on its diagonal differs exactly there; behind it lie a pair made from a plan of edits, the pieces the three producers
align, and a tail that ends both sequences together.  Each case runs at chunk 64 and at the default, C below being the one in force."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import diff_model as D
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CHUNKS = ((64, 64), (0, D.DEFAULT_CHUNK))  # (the parameter, the C it means)
M, I, Dl = D.OP_M, D.OP_I, D.OP_D

MAIN = 215_000
ONE = 9_300        # the only difference of main[1_000, 17_600)
RUN0, RUN1 = 22_300, 30_800  # main differs in every base of [RUN0, RUN1) and in none of [18_000, RUN0) and [RUN1, 35_000)
CODES = 36_000     # the hand-written pairs
PAIRS = ["AA", "AG", "AC", "AA", "AC", "AN", "AT", "AA", "aA", "NA", "RA", "&A", "AA", "Aa", "AN", "AR", "A&", "AA", "aa", "NN", "&&", "AA"]
GAPS = 37_000      # spans with gaps, on a stretch without differences
NEIGHBOURS = 40_000  # main[NEIGHBOURS + 99] and [+ 100] differ
SMALL0, SMALL1 = 41_000, 60_000
BIG = 10_000       # the span of 200 000 columns starts here


def revcomp(a):
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return comp[a[::-1]]


def other_base(rng, b):
    """A base that differs from every base of b."""
    return ACGT[(np.searchsorted(ACGT, b) + rng.integers(1, 4, b.size)) % 4]


def edited(rng, t, rate=0.04):
    """A query made from t by a plan of substitutions (always to another base), insertions and deletions, at least two unchanged
    bases between them and at either end.  -> (query, runs for the ops, the plan as (kind, target offset, query offset, length))."""
    q, runs, plan, at, keep = [], [], [], 0, 0

    def flush():
        nonlocal keep
        if keep:
            runs.append((keep, M))
            keep = 0
    nq = 0
    while at < t.size:
        if at >= 2 and at + 12 < t.size and keep >= 2 and rng.random() < rate:
            kind, n = int(rng.integers(0, 3)), int(rng.integers(1, 6))
            if kind == 0:  # substitution of n bases: M columns
                q.append(other_base(rng, t[at:at + n]))
                plan.append((D.SUB, at, nq, n))
                flush()
                runs.append((n, M))
                at, nq = at + n, nq + n
            elif kind == 1:
                q.append(ACGT[rng.integers(0, 4, n)])
                plan.append((D.INS, at, nq, n))
                flush()
                runs.append((n, I))
                nq += n
            else:
                plan.append((D.DEL, at, nq, n))
                flush()
                runs.append((n, Dl))
                at += n
            q.append(t[at:at + 2])  # two unchanged bases behind every edit
            keep, at, nq = 2, at + 2, nq + 2
        else:
            q.append(t[at:at + 1])
            keep, at, nq = keep + 1, at + 1, nq + 1
    flush()
    merged = []
    for n, c in runs:  # adjacent M runs are one entry
        if merged and merged[-1][1] == c == M:
            merged[-1] = (merged[-1][0] + n, M)
        else:
            merged.append((n, c))
    return np.concatenate(q), merged, plan


class World:
    pass


def build_world():
    rng = np.random.default_rng(77)
    w = World()
    t = ACGT[rng.integers(0, 4, MAIN)]
    q = t.copy()
    for p in (0, ONE, NEIGHBOURS + 99, NEIGHBOURS + 100):
        q[p:p + 1] = other_base(rng, t[p:p + 1])
    q[RUN0:RUN1] = other_base(rng, t[RUN0:RUN1])
    t[CODES:CODES + len(PAIRS)] = np.frombuffer("".join(p[0] for p in PAIRS).encode(), dtype=np.uint8)
    q[CODES:CODES + len(PAIRS)] = np.frombuffer("".join(p[1] for p in PAIRS).encode(), dtype=np.uint8)
    T, Q = [t], [q]
    size = lambda x: sum(len(a) for a in x)

    def put(a, b):
        at = (size(T), size(Q))
        T.append(np.asarray(a, dtype=np.uint8))
        Q.append(np.asarray(b, dtype=np.uint8))
        return at

    def spacer():  # unrelated sequence that ends in a record separator: no alignment of a producer reaches across
        put(np.append(ACGT[rng.integers(0, 4, 150)], ord("&")).astype(np.uint8), np.append(ACGT[rng.integers(0, 4, 260)], ord("&")).astype(np.uint8))

    spacer()
    # planted truth
    tp = ACGT[rng.integers(0, 4, 6_000)]
    qp, w.plan_runs, w.plan = edited(rng, tp)
    w.plan_at = put(tp, qp)
    spacer()
    # what the gapped entries align: HSPs (ref_start, query_start, len, score)
    w.hsps = []
    for _ in range(3):  # an edited middle between two shared flanks, the anchor in the first flank
        mid = ACGT[rng.integers(0, 4, 700)]
        fl, fr = ACGT[rng.integers(0, 4, 200)], ACGT[rng.integers(0, 4, 200)]
        at = put(np.concatenate([fl, mid, fr]), np.concatenate([fl, edited(rng, mid, 0.03)[0], fr]))
        w.hsps.append((at[0] + 50, at[1] + 50, 99, 0))
        spacer()
    for swap in (False, True):  # ten bases that one sequence lacks, the anchor in their middle: a gap run on either side of it
        l, x, r = ACGT[rng.integers(0, 4, 300)], np.full(10, ord("A"), dtype=np.uint8), ACGT[rng.integers(0, 4, 300)]
        l[-1], r[0] = ord("G"), ord("C")  # no base beside the ten can pair with one of them, so each side opens its gap at the anchor
        long_, short = np.concatenate([l, x, r]), np.concatenate([l, r])
        at = put(short, long_) if swap else put(long_, short)
        ar, aq = at[0] + 300 + (0 if swap else 5), at[1] + 300 + (5 if swap else 0)
        w.hsps.append((ar - 20, aq - 20, 40, 0))
        spacer()
    # what the stitch aligns: members both share, between them links of a target piece against an edited copy
    w.members, w.first = [], [0]
    for links in ([(20, 0.1), (0, 0), (35, 0.05)], [(60, 0.08)], [(5, 0.5), (90, 0.06), (12, 0.0), (300, 0.04)]):
        for k in range(len(links) + 1):
            m = ACGT[rng.integers(0, 4, 30)]
            at = put(m, m)
            w.members.append(len(w.hsps))
            w.hsps.append((at[0], at[1], 29, 0))
            if k < len(links) and links[k][0]:
                lt = ACGT[rng.integers(0, 4, links[k][0])]
                put(lt, edited(rng, lt, links[k][1])[0])
        w.first.append(len(w.members))
        spacer()
    # the tail: shared, with a difference in its first and in its last base
    tail = ACGT[rng.integers(0, 4, 300)]
    qt = tail.copy()
    qt[[0, 299]] = other_base(rng, tail[[0, 299]])
    w.tail_at = put(tail, qt)
    w.t, w.q = np.concatenate(T), np.concatenate(Q)
    w.rng = rng
    return w


@pytest.fixture(scope="module")
def world(engine):
    E = engine
    w = build_world()
    w.E = E
    Case(w.t, w.q, chunk=250_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(revcomp(w.q), 0, w.q.size, 1)
    w.ref = E.copy_ref_codes()
    w.codes = {(buf, rev): E.copy_query_codes(buf, rev) for buf in (0, 1) for rev in (False, True)}
    assert w.ref.size == w.t.size and w.codes[(0, False)].size == w.q.size
    assert np.array_equal(w.codes[(0, False)], w.codes[(1, True)])
    yield w
    E.ShutdownProcessor()


def same(got, want, names):
    assert got.size == want.size, (got.size, want.size)
    for f in names:
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8])


def check(w, spans, ops, chunk=None, rev=False, buf=0, per_base=False, model=None):
    """One engine call per chunk (both of CHUNKS unless one parameter is given) held against the model.  -> the model's result."""
    ops = np.asarray(ops, dtype=np.uint32)
    ev, sm, pairs = model or D.diff(w.ref, w.codes[(buf, rev)], spans, ops, per_base)
    for c in ((64, 0) if chunk is None else (chunk,)):
        g_ev, g_sm, st = w.E.DiffAlignments(spans, ops, rev, buf, per_base=per_base, chunk=c)
        same(g_ev, ev, D.EVENT_DTYPE.names)
        same(g_sm, sm, D.SUMMARY_DTYPE.names)
        assert np.array_equal(st["pairs"], pairs)
        assert st["spans"] == len(spans) and st["events"] == ev.size and st["columns"] == int(sm["columns"].astype(np.int64).sum())
        assert st["ops"] == int(np.asarray(spans["n_ops"], dtype=np.int64).sum()) and st["work_items"] == D.work_items(spans, ops, c)
    return ev, sm, pairs


def diag(p, runs):
    """A span that starts on main's diagonal at p."""
    return (p, p, runs)


def test_nothing_and_single_columns(world):
    w = world
    ev, sm, st = w.E.DiffAlignments(np.zeros(0, dtype=D.SPAN_DTYPE), [], False)
    assert ev.size == sm.size == 0 and st["spans"] == st["events"] == st["work_items"] == 0 and not st["pairs"].any()
    ev, sm, _ = check(w, *D.pack([diag(500, [])]))
    assert ev.size == 0 and sm.size == 1 and int(sm[0]["columns"]) == 0
    ev, sm, _ = check(w, *D.pack([diag(500, [(1, M)])]))
    assert ev.size == 0 and int(sm[0]["matches"]) == 1
    ev, sm, _ = check(w, *D.pack([diag(ONE, [(1, M)])]))
    assert ev.size == 1 and int(sm[0]["matches"]) == 0 and int(ev[0]["len"]) == 1


@pytest.mark.parametrize("param,C", CHUNKS)
def test_one_run_of_every_edge_length_with_one_mismatch(world, param, C):
    al, want = [], []
    for L in (1, 63, 64, 65, 127, 128, 129, C - 1, C, C + 1, 2 * C + 1):
        for col in sorted({0, 63, 64, L - 1}):
            if col < L:
                al.append(diag(ONE - col, [(L, M)]))
                want.append(col)
    spans, ops = D.pack(al)
    ev, sm, _ = check(world, spans, ops, chunk=param)
    assert ev["column"].tolist() == want and np.all(ev["len"] == 1) and np.all(sm["n_events"] == 1)  # the regime: one mismatch each
    assert np.all(sm["matches"] + 1 == sm["columns"])


@pytest.mark.parametrize("param,C", CHUNKS)
def test_mismatch_runs_across_steps_chunks_and_entries(world, param, C):
    assert RUN1 - RUN0 > 2 * C + 300
    al = [diag(RUN0 - 61, [(200, M)]),               # columns 61 .. 199: across the step edge at 64
          diag(RUN1 - (C + 3), [(2 * C, M)]),        # columns 0 .. C + 2: across the chunk edge at C
          diag(RUN1 - 103, [(100, M), (100, M)]),    # columns 0 .. 102: across the edge of two adjacent M entries at 100
          diag(RUN0 - 60, [(C + 32, M), (200, M)]),  # columns 60 .. C + 231: across the step edge, the chunk edge at C and the entry edge
          diag(RUN0 - (C - 5), [(3 * C, M)])]        # columns C - 5 .. 3 C - 1: starts in item 0 and ends in item 2
    spans, ops = D.pack(al)
    ev, sm, _ = check(world, spans, ops, chunk=param)
    assert np.all(sm["n_events"] == 1) and np.all(ev["kind"] == D.SUB)
    got = list(zip(ev["column"].tolist(), (ev["column"].astype(np.int64) + ev["len"]).tolist()))
    assert got == [(61, 200), (0, C + 3), (0, 103), (60, C + 232), (C - 5, 3 * C)]


@pytest.mark.parametrize("param,C", CHUNKS)
def test_a_run_that_spans_a_middle_item(world, param, C):
    n = RUN1 - RUN0
    assert n > 2 * C + 10
    p = RUN0 - (C - 5)  # the run starts at column C - 5 of item 0
    L = (C - 5) + n + 20
    ev, sm, _ = check(world, *D.pack([diag(p, [(L, M)])]), chunk=param)
    assert ev.size == 1 and int(ev[0]["column"]) == C - 5 and int(ev[0]["len"]) == n
    assert (C - 5) // C == 0 and (C - 5 + n - 1) // C >= 2


def test_all_difference_and_none(world):
    ev, sm, _ = check(world, *D.pack([diag(RUN0, [(RUN1 - RUN0, M)]), diag(18_100, [(4_000, M)])]))
    assert ev.size == 1 and int(ev[0]["len"]) == RUN1 - RUN0 == int(sm[0]["columns"]) and int(sm[0]["matches"]) == 0
    assert int(sm[1]["n_events"]) == 0 and int(sm[1]["matches"]) == 4_000


def test_gap_entries(world):
    g = GAPS
    al = [diag(g, [(50, M), (3, I), (4, I), (50, M)]),            # two adjacent I entries: one event
          diag(g + 200, [(50, M), (3, I), (4, Dl), (50, M)]),     # I next to D: two events
          diag(g + 400, [(2, Dl), (70, M), (5, I)]),              # gaps as the first and as the last entry
          diag(g + 600, [(2, I), (3, Dl), (1, I), (1, I), (6, Dl)]),  # gaps only
          diag(g + 800, [(3, Dl), (3, Dl), (2, Dl), (70, M), (1, I)])]
    ev, sm, _ = check(world, *D.pack(al))
    kinds = lambda k: [(int(e["kind"]), int(e["len"])) for e in ev[ev["span"] == k] if e["kind"] >= D.INS]
    assert kinds(0) == [(D.INS, 7)] and int(sm[0]["ins_runs"]) == 1 and int(sm[0]["ins_bases"]) == 7
    assert kinds(1) == [(D.INS, 3), (D.DEL, 4)]
    assert kinds(2) == [(D.DEL, 2), (D.INS, 5)] and int(ev[ev["span"] == 2][0]["column"]) == 0
    assert kinds(3) == [(D.INS, 2), (D.DEL, 3), (D.INS, 2), (D.DEL, 6)] and int(sm[3]["columns"]) == 13 and int(sm[3]["matches"]) == 0
    assert kinds(4) == [(D.DEL, 8), (D.INS, 1)]
    e = ev[(ev["span"] == 0) & (ev["kind"] == D.INS)][0]
    assert (int(e["ref_pos"]), int(e["query_pos"]), int(e["tcode"])) == (g + 50, g + 50, D.NO_CODE)


def test_classes_and_codes(world):
    ev, sm, pairs = check(world, *D.pack([diag(CODES, [(len(PAIRS), M)])]))
    got = [(int(e["column"]), int(e["len"]), int(e["kind"])) for e in ev]
    assert got[:4] == [(1, 2, D.SUB), (4, 1, D.SUB), (5, 1, D.OTHER), (6, 1, D.SUB)]  # TS next to TV: one; SUB, OTHER, SUB: three
    assert got[4:] == [(8, 4, D.OTHER), (13, 4, D.OTHER), (18, 3, D.OTHER)]
    assert (int(sm[0]["transitions"]), int(sm[0]["transversions"]), int(sm[0]["others"])) == (1, 3, 12)
    for c in (4, 5, 6, 7):  # every special code on either side
        assert pairs[c * 8 + 0] == 1 and pairs[0 * 8 + c] == (2 if c == 5 else 1)
    ev, sm, _ = check(world, *D.pack([diag(CODES, [(len(PAIRS), M)])]), per_base=True)
    assert [(int(e["column"]), int(e["len"])) for e in ev[:3]] == [(1, 1), (2, 1), (4, 1)]


def test_a_difference_on_both_sides_of_a_span_boundary(world):
    n = NEIGHBOURS
    spans, ops = D.pack([diag(n, [(100, M)]), diag(n + 100, [(100, M)])])
    ev, sm, _ = check(world, spans, ops)
    assert ev.size == 2 and ev["column"].tolist() == [99, 0] and ev["len"].tolist() == [1, 1] and ev["ref_pos"].tolist() == [n + 99, n + 100]
    ev, _, _ = check(world, *D.pack([diag(n, [(100, M), (100, M)])]))  # the same ops as one span: one event
    assert ev.size == 1 and int(ev[0]["len"]) == 2


def test_empty_spans_between_full_ones_and_unused_ops(world):
    n = NEIGHBOURS
    ops = np.array([D.op(100, M), D.op(7, I), D.op(9, 3), D.op(0, M), D.op(100, M), D.op(3, Dl)], dtype=np.uint32)  # [2] and [3] belong to no span
    spans = D.make_spans([(5, 5, 0, 0), (n, n, 0, 2), (0, 0, 2, 0), (9, 9, 4, 0), (n + 100, n + 107, 4, 2), (1, 1, 6, 0)])
    ev, sm, _ = check(world, spans, ops)
    assert [int(sm[k]["n_events"]) for k in (0, 2, 3, 5)] == [0] * 4 and int(sm[1]["n_events"]) >= 2 and int(sm[4]["n_events"]) > 10
    assert sm["first_event"].tolist()[2:5] == [int(sm[1]["n_events"])] * 3 and int(sm[5]["first_event"]) == ev.size


def small_spans(rng, n, lo, hi):
    al = []
    for _ in range(n):
        runs = [(int(rng.integers(1, 40)), int(rng.choice([M, M, I, Dl]))) for _ in range(int(rng.integers(1, 4)))]
        p = int(rng.integers(lo, hi))
        al.append((p, p + int(rng.integers(-3, 4)), runs))
    return al


def test_many_small_spans_beside_one_of_200_000_columns(world):
    rng = np.random.default_rng(5)
    big = (BIG, BIG, [(100_000, M), (3, I), (50_000, M), (2, Dl), (49_995, M)])
    al = small_spans(rng, 1000, SMALL0, SMALL1) + [big] + small_spans(rng, 1000, SMALL0, SMALL1)
    spans, ops = D.pack(al)
    ev, sm, _ = check(world, spans, ops)
    assert len(spans) == 2001 and int(sm[1000]["columns"]) == 200_000 and np.all(spans["n_ops"][:1000] <= 3)
    assert int(sm[1000]["n_events"]) > 10_000 and int(sm[1000]["matches"]) > 100_000


def test_the_first_and_the_last_base_of_both_sequences(world):
    w = world
    tr, tq = w.tail_at
    assert tr + 300 == w.ref.size and tq + 300 == w.codes[(0, False)].size
    al = [(0, 0, [(100, M)]), (tr, tq, [(300, M)]), (0, 0, [(1, Dl), (1, I), (50, M)]), (tr + 297, tq + 298, [(2, M), (1, Dl)]),
          (tr + 298, tq + 297, [(2, M), (1, I)])]
    ev, sm, _ = check(w, *D.pack(al))
    assert int(ev[0]["column"]) == 0 and int(ev[0]["ref_pos"]) == 0  # base 0 differs
    e = ev[ev["span"] == 1]
    assert e["column"].tolist() == [0, 299] and int(e[1]["ref_pos"]) == w.ref.size - 1 and int(e[1]["query_pos"]) == tq + 299


def test_the_reverse_strand_and_a_second_buffer(world):
    rng = np.random.default_rng(6)
    n = world.q.size
    al = small_spans(rng, 300, 100, min(world.t.size, n) - 200) + [(200, 200, [(3_000, M), (4, I), (500, M)]), (0, n - 120, [(120, M)])]
    spans, ops = D.pack(al)
    a = check(world, spans, ops, rev=True, buf=0)
    b = check(world, spans, ops, rev=False, buf=1)  # buffer 1 holds the reverse complement
    assert a[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    c = check(world, spans, ops, rev=False, buf=0)
    assert not np.array_equal(a[2], c[2])


def test_per_base_and_no_events(world):
    w = world
    al = [diag(RUN0 - 10, [(500, M)]), diag(CODES - 5, [(40, M)]), diag(GAPS, [(50, M), (3, I), (4, I), (50, M)])]
    spans, ops = D.pack(al)
    runs = check(w, spans, ops)
    each = check(w, spans, ops, per_base=True)
    assert each[0].size > runs[0].size + 480 and np.all(each[0]["len"][each[0]["kind"] == D.SUB] == 1)
    assert each[0][each[0]["kind"] == D.INS]["len"].tolist() == [7] and np.array_equal(each[2], runs[2])
    for c, _ in CHUNKS:
        ev, sm, st = w.E.DiffAlignments(spans, ops, False, 0, events=False, chunk=c)
        assert ev.size == 0 and st["emit_ms"] == 0 and st["events"] == runs[0].size
        same(sm, runs[1], D.SUMMARY_DTYPE.names)
        assert np.array_equal(st["pairs"], runs[2])


def test_planted_edits_are_the_events(world):
    w = world
    spans, ops = D.pack([(w.plan_at[0], w.plan_at[1], w.plan_runs)])
    ev, sm, _ = check(w, spans, ops)
    assert len(w.plan) > 100 and {k for k, *_ in w.plan} == {D.SUB, D.INS, D.DEL}
    want = [(k, w.plan_at[0] + r, w.plan_at[1] + q, n) for k, r, q, n in w.plan]
    assert [(int(e["kind"]), int(e["ref_pos"]), int(e["query_pos"]), int(e["len"])) for e in ev] == want
    assert int(sm[0]["others"]) == 0 and int(sm[0]["ins_runs"]) == sum(k == D.INS for k, *_ in w.plan)


def test_the_three_producers_end_to_end(world):
    w, E = world, world.E
    hsps = np.array(w.hsps, dtype=E.SEG_DTYPE)
    strict = 0
    for fn in (E.GappedAlign, E.GappedAlignGreedy):
        recs, paths, ops, _ = fn(hsps[:5], False, 0)
        assert recs.size >= 4
        spans = E.diff_spans(recs, paths)
        ev, sm, _ = check(w, spans, ops)
        assert np.array_equal(sm["matches"], paths["matches"])
        assert np.array_equal(sm["transitions"] + sm["transversions"] + sm["others"], paths["mismatches"])
        assert np.array_equal(sm["ins_bases"] + sm["del_bases"], paths["gap_bases"])
        assert np.all(sm["ins_runs"] + sm["del_runs"] <= paths["gap_opens"])
        strict += int((sm["ins_runs"] + sm["del_runs"] < paths["gap_opens"]).sum())
        assert int(sm["ins_runs"].sum()) > 0 and int(sm["del_runs"].sum()) > 0 and int(sm["transitions"].sum()) > 0
    assert strict >= 1  # gap runs that meet at an anchor, in the model's count as in the engine's
    recs, ops, _ = E.StitchChains(hsps, w.members, w.first, False, 0)
    assert recs.size == 3 and np.all(recs["flags"] == 0)
    ev, sm, _ = check(w, E.diff_spans(recs), ops)
    assert np.array_equal(sm["matches"], recs["matches"])
    assert np.array_equal(sm["transitions"] + sm["transversions"] + sm["others"], recs["mismatches"])
    assert np.array_equal(sm["ins_bases"] + sm["del_bases"], recs["gap_bases"])
    assert np.array_equal(sm["ins_runs"] + sm["del_runs"], recs["gap_opens"]) and int(recs["gap_opens"].sum()) > 0


def test_eight_concurrent_callers_get_the_serial_results(world):
    w = world
    rng = np.random.default_rng(8)
    jobs = []
    for k in range(8):
        al = small_spans(rng, 200 + 50 * k, SMALL0, SMALL1) + [diag(RUN0 - 100 * k, [(6_000 + k, M)])]
        spans, ops = D.pack(al)
        jobs.append((spans, ops, bool(k % 2), k % 2, dict(per_base=bool(k & 2), chunk=(0, 64, 256)[k % 3])))

    def call(spans, ops, rev, buf, kw):
        ev, sm, st = w.E.DiffAlignments(spans, ops, rev, buf, **kw)
        return ev, sm, st["pairs"]

    serial = [call(*j) for j in jobs]
    for j, s in zip(jobs, serial):
        m = D.diff(w.ref, w.codes[(j[3], j[2])], j[0], j[1], j[4]["per_base"])
        assert all(np.array_equal(a, b) for a, b in zip(s, m))
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


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from segalign_amd import engine as E
from gapped_model import SUB
from helpers import Case
import diff_model as D
rng = np.random.default_rng(1)
t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4000)]
Case(t, t.copy(), sub_mat=SUB).engine_setup(E, num_gpu=1)
r = E.DiffAlignments(D.make_spans(%s), np.array(%s, dtype=np.uint32), False, 0, **%s)
print("returned", len(r[0]))
"""


@pytest.mark.parametrize("what,spans,ops,kw", [
    ("has code 3", [(10, 10, 0, 2)], [D.op(5, M), D.op(5, 3)], {}),
    ("a zero run", [(10, 10, 0, 2)], [D.op(5, M), D.op(0, I)], {}),
    ("overlap", [(10, 10, 0, 2), (50, 50, 1, 1)], [D.op(5, M), D.op(5, M)], {}),
    ("leave the array", [(10, 10, 1, 2)], [D.op(5, M), D.op(5, M)], {}),
    ("inside the block", [(3990, 100, 0, 1)], [D.op(11, M)], {}),
    ("inside the block", [(100, 3990, 0, 2)], [D.op(5, Dl), D.op(11, I)], {}),
    ("chunk", [(10, 10, 0, 1)], [D.op(5, M)], dict(chunk=96)),
    ("chunk", [(10, 10, 0, 1)], [D.op(5, M)], dict(chunk=32)),
])
def test_bad_input_fails_with_a_message(what, spans, ops, kw):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), spans, ops, kw)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout, (r.returncode, r.stderr[-300:])
    assert b"DiffAlignments" in r.stderr and what.encode() in r.stderr
