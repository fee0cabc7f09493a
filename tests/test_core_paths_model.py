"""CPU: the rules of tests/core_paths_model.py on hand-made cases, and -- with the oracle -- that every input of
tests/test_gpu_core_paths.py is in the regime it names: the iterations of every chunk, which chunks are empty, which have hits and no
record, where the records lie, and the hits per iteration on either side of hit_batch."""
import numpy as np
import pytest

import core_paths_model as CM
import probe_model as PM
from helpers import Case

P = lambda *a: np.array(a, dtype=np.int64)


# ---- the rules on hand-made cases --------------------------------------------------------------------------------------------------------
def test_general_plan_equals_the_probe_models_where_that_one_plans():
    rng = np.random.default_rng(1)
    for _ in range(300):
        prefix = np.cumsum(rng.integers(0, 9, int(rng.integers(1, 40))))
        mh = int(rng.integers(1, 60))
        n, ends = PM.plan_from_words(prefix, mh, False)
        got = CM.plan_general(prefix, mh)
        if n != PM.OVERFLOW:
            assert got == ends and len(got) == n, (prefix, mh)
        else:
            assert len(got) in (int(prefix[-1]) // mh + 2, int(prefix[-1]) // mh + 1) and got[-1] == prefix[-1]
    assert CM.plan_general(P(1, 63), 9) == [1] * 8 + [63]                        # nine iterations: beyond the table-direct limit
    assert CM.plan_general(P(), 5) == [] and CM.plan_general(P(0, 0), 5) == []


def test_batches_on_hand_made_segment_ends():
    B = CM.batches
    ends = list(range(10, 180, 10))                                              # 17 segments of 10 hits
    assert B(ends[:8], False) == [(0, 8, 80)]
    assert B(ends[:9], False) == [(0, 8, 80), (8, 1, 10)]
    assert B(ends[:16], False) == [(0, 8, 80), (8, 8, 80)]
    assert B(ends, False) == [(0, 8, 80), (8, 8, 80), (16, 1, 10)]
    assert B(ends, True) == [(0, 17, 170)]                                       # a table-direct call is one batch
    assert B(list(range(1, 601)), True) == [(0, 512, 512), (512, 88, 88)]
    # hit_batch: a batch ends in front of the segment that would take it PAST the limit
    assert B([10, 20], False, 20) == [(0, 2, 20)]
    assert B([10, 20], False, 19) == [(0, 1, 10), (1, 1, 10)]
    assert B([30, 40], False, 5) == [(0, 1, 30), (1, 1, 10)]                     # ... unless it is the batch's first
    assert B([10, 20, 25, 60], False, 15) == [(0, 1, 10), (1, 2, 15), (3, 1, 35)]
    assert B([10, 20], True, 5) == [(0, 2, 20)]                                  # (no hit list in a table-direct call: no limit)
    # batches without hits are not counted, and leave the segment numbering alone
    assert B([0, 0, 7], False) == [(0, 3, 7)]
    assert B([0] * 8 + [5], False) == [(8, 1, 5)]
    assert B([4] + [4] * 8, False) == [(0, 8, 4)]
    assert B([], False) == []


def test_slices_route_and_owner():
    assert [CM.slices(n, 100) for n in (0, 99, 100, 101, 200, 201, 300)] == [0, 0, 0, 2, 2, 3, 3]
    r = CM.route
    assert r(0) == CM.ROUTE_NONE and r(0, raw=True) == CM.ROUTE_NONE
    assert r(5) == CM.ROUTE_SPEC_CHAIN and r(5, segments=512) == CM.ROUTE_SPEC_CHAIN
    assert r(5, segments=513) == CM.ROUTE_LIBRARY_SORTS
    assert r(5, refused=True) == CM.ROUTE_LIBRARY_SORTS and r(5, sliced=True) == CM.ROUTE_LIBRARY_SORTS
    assert r(CM.DEDUP_TOTAL) == CM.ROUTE_SPEC_CHAIN and r(CM.DEDUP_TOTAL + 1) == CM.ROUTE_LIBRARY_SORTS
    assert r(5, spec_dedup=0) == CM.ROUTE_CHAIN_AFTER_SYNC and r(5, spec_dedup=0, refused=True) == CM.ROUTE_LIBRARY_SORTS
    assert r(5, no_small_dedup=1) == CM.ROUTE_LIBRARY_SORTS
    assert r(5, td=False) == CM.ROUTE_CHAIN_AFTER_SYNC and r(5, td=False, batches=3, segments=17) == CM.ROUTE_CHAIN_AFTER_SYNC
    assert r(5, batches=2) == CM.ROUTE_CHAIN_AFTER_SYNC
    assert r(5, raw=True, td=False) == CM.ROUTE_RAW
    assert r(5, rm=True) == CM.ROUTE_RM_SORT and r(5, rm=True, coverage=True) == CM.ROUTE_RM_COVERAGE
    assert r(5, rm=True, td=False, no_small_dedup=1, spec_dedup=0) == CM.ROUTE_RM_SORT
    assert CM.spec_tried() and not CM.spec_tried(td=False) and not CM.spec_tried(spec_dedup=0) and not CM.spec_tried(rm=True)
    iters = [0, 2, 3, 0, 0, 2]
    assert [CM.owner(g, iters) for g in range(7)] == [1, 1, 2, 2, 2, 5, 5]
    with pytest.raises(AssertionError):
        CM.owner(7, iters)


# ---- the inputs, with the oracle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(oracle):
    made = {}

    def get(inp):
        if inp.name not in made:
            made[inp.name] = Case(inp.target, inp.query, chunk=inp.chunk, hspthresh=inp.hspthresh).oracle_setup(oracle)
        return made[inp.name]
    return get


def oracle_chunk(c, s, e, rev=False, max_hits=1 << 30):
    """-> (seed words, hits, iterations, records) of one chunk"""
    seeds = c.host_seeds(s, e, rev)
    if seeds.size == 0:
        return 0, 0, 0, 0
    w, st = c.oracle_saf(seeds, rev, max_hits=max_hits)
    return int(seeds.size), int(st["num_hits"]), int(st["num_iter"]), int(w.size - 1)


@pytest.mark.parametrize("make", [CM.single, CM.sixteen, CM.split, CM.split_last, CM.late], ids=lambda f: f.__name__)
def test_model_plans_equal_the_oracles_hits_and_iterations(cases, make):
    inp = make()
    c = cases(inp)
    ch = inp.chunks()
    assert ch == c.chunks() and 50000 <= inp.target.size <= 200000 and 5000 <= inp.chunk <= 25000
    for rev in (False, True):
        iters, ends, hits = inp.plan(0, len(ch) - 1, rev)
        for j, (s, e) in enumerate(ch):
            _, h, it, _ = oracle_chunk(c, s, e, rev)
            assert (h, it if h else 0) == (hits[j], iters[j]), (inp, rev, j)
        assert ends == sorted(ends) and (not ends or ends[-1] == sum(hits))


def test_single_chunk_input(cases):
    inp = CM.single()
    c = cases(inp)
    s, e = inp.chunks()[0]
    _, h, it, rec = oracle_chunk(c, s, e)
    assert it == 2 and 2000 < h < 10000 and rec >= 50
    # 9, 16 and 17 iterations: 2, 2 and 3 batches of the general path
    for want, nb in ((9, 2), (16, 2), (17, 3)):
        mh = inp.max_hits_for(0, want)
        iters, ends, _ = inp.plan(0, 0, max_hits=mh)
        assert oracle_chunk(c, s, e, max_hits=mh)[2] == want == iters[0]
        b = CM.batches(ends, False)
        assert len(b) == nb and [x[1] for x in b] == [8] * (want // 8) + ([want % 8] if want % 8 else []), (want, b)
        assert all(x[2] > 0 for x in b)
    # hit_batch on either side of the second segment's end
    _, ends, _ = inp.plan(0, 0)
    assert len(ends) == 2 and 0 < ends[0] < ends[1] == h
    assert len(CM.batches(ends, False, ends[1])) == 1 and len(CM.batches(ends, False, ends[1] - 1)) == 2
    # four chunks of three iterations each: the second batch begins inside the third chunk
    mh4 = CM.four_chunk_max_hits(inp)
    iters, ends, hits = inp.plan(0, 3, max_hits=mh4)
    assert iters == [3, 3, 3, 3]
    b = CM.batches(ends, False)
    assert [x[:2] for x in b] == [(0, 8), (8, 4)] and CM.owner(7, iters) == CM.owner(8, iters) == 2
    for j, (s4, e4) in enumerate(inp.chunks()[:4]):
        assert oracle_chunk(c, s4, e4, max_hits=mh4)[1:3] == (hits[j], 3)


def test_sixteen_chunk_input(cases):
    inp = CM.sixteen()
    c = cases(inp)
    ch = inp.chunks()
    assert len(ch) == 16
    rows = [oracle_chunk(c, s, e) for (s, e) in ch]
    assert all(r[1] > 0 and r[2] == 2 for r in rows)
    assert sum(r[3] for r in rows) >= 50 and sum(r[3] > 0 for r in rows) >= 12
    assert sum(r[1] for r in rows) < 40000
    assert len(CM.batches(inp.plan(0, 15)[1], True)) == 1 and len(inp.plan(0, 15)[1]) == 32


def test_split_inputs(cases):
    for inp, lone in ((CM.split(), False), (CM.split_last(), True)):
        c = cases(inp)
        ch = inp.chunks()
        assert len(ch) == 16
        rows = [oracle_chunk(c, s, e) for (s, e) in ch]
        seeded = [j for j in range(16) if rows[j][0]]
        assert [j for j in range(16) if not rows[j][0]] == list(CM.SPLIT_EMPTY) and seeded[-1] == CM.SPLIT_LAST
        barren = [j for j in seeded if rows[j][3] == 0]
        with_records = [j for j in seeded if rows[j][3] > 0]
        assert all(rows[j][1] > 100 for j in seeded)
        if lone:
            assert with_records == [CM.SPLIT_LAST] and rows[CM.SPLIT_LAST][3] >= 20
        else:
            assert barren == list(CM.SPLIT_BARREN) and sum(rows[j][3] for j in with_records) >= 50
            # a chunk without records lies between two with records, and so does a chunk without seeds
            assert with_records[0] < barren[0] < with_records[1] and any(a < e < b for e in CM.SPLIT_EMPTY for a, b in zip(with_records, with_records[1:]))
    # some chunks in three planned iterations and others in two: the first segment of chunk c is not 2 c
    inp = CM.split()
    c = cases(inp)
    mh = CM.uneven_max_hits(inp, 0, 15)
    iters, ends, hits = inp.plan(0, 15, max_hits=mh)
    assert set(iters) == {0, 2, 3} and len(ends) <= CM.MAX_SEGS_TD
    first = np.concatenate([[0], np.cumsum(iters)])
    assert any(first[j] != 2 * j for j in range(16))
    for j, (s, e) in enumerate(inp.chunks()):
        if hits[j]:
            assert oracle_chunk(c, s, e, max_hits=mh)[1:3] == (hits[j], iters[j]), j


def test_late_input(cases):
    """17 iterations in three batches of which the first two hold as many hits; the hits of the unrelated front fill a fifth of the first
    batch and none of the second, which therefore holds more candidates"""
    inp = CM.late()
    c = cases(inp)
    s, e = inp.chunks()[0]
    _, h, it, rec = oracle_chunk(c, s, e)
    assert it == 2 and rec >= 50
    mh = inp.max_hits_for(0, 17)
    iters, ends, _ = inp.plan(0, 0, max_hits=mh)
    assert oracle_chunk(c, s, e, max_hits=mh)[1:3] == (h, 17) and iters == [17]
    b = CM.batches(ends, False)
    assert [x[:2] for x in b] == [(0, 8), (8, 8), (16, 1)] and all(x[2] > 0 for x in b)
    k = inp.text_query.keys(False)[:CM.LATE_NOISE - len(CM.SHAPE)]
    front = int(PM.word_prefix(inp.world.table, k[k >= 0])[-1])              # hits of the windows that lie wholly in the unrelated part
    assert b[0][2] // 5 < front < b[0][2] and b[1][2] >= b[0][2] - mh
    assert oracle_chunk(c, 0, CM.LATE_NOISE - len(CM.SHAPE))[3] == 0             # ... which leave no record


def test_the_forced_capacities_are_test_options(engine):
    """cand_cap, ent_cap, out_cap and hit_batch are listed, flagged test-only like l2_cap, and deployment options are not"""
    o = engine.options()
    assert all(o[k] is True for k in ("cand_cap", "ent_cap", "out_cap", "hit_batch", "l2_cap", "chain_cap", "spec_recs"))
    assert not any(o[k] for k in ("slots", "chunks_per_call", "no_td", "no_chain", "fin_batch"))
