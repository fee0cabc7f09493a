"""GPU: the call core (segalign_amd/csrc/core.hip saf_core) branch by branch -- batches of the general path, lists that
overflow and rerun (each list alone, in a first and in a later batch), the sliced chain, every way the survivors reach the host, the
split of the output per chunk, the raw and the repeat-masker routes -- on small inputs.  Every case compares every returned vector, the
header's hit count, num_hits and num_iter with the oracle by exact equality, and asserts through sa_get_last_call_trace that the branch
it names was TAKEN, against the rules of tests/core_paths_model.py (tests/test_core_paths_model.py shows on the CPU that every input is in
its regime).

The device lists of a slot only grow, so a forced capacity (options cand_cap, ent_cap, out_cap, l2_cap) overflows only on a freshly
initialised processor: every constrained case gets one, the trace -- not the option -- proves the overflow, and the call is repeated in
the same slot, where it must return the same vectors without a rerun.  The counts that place a capacity come from an unconstrained call of
the same range on a fresh processor and must be the same in a second one; they place the capacity only, the reference is the oracle."""
import numpy as np
import pytest

import core_paths_model as CM
import extend_model as XM
import extend_regimes as XR
from helpers import Case, seg_equal
from segalign_amd import synth
from test_gpu_rm_mask import as_list

pytestmark = pytest.mark.gpu

_cases, _counts = {}, {}


@pytest.fixture
def E(engine):
    try:
        yield engine
    finally:
        engine.set_max_hits(0)
        engine.set_count_examined(False)
        engine.ShutdownProcessor()
        engine.reset_option(None)


def case_of(oracle, inp):
    if inp.name not in _cases:
        _cases[inp.name] = Case(inp.target, inp.query, chunk=inp.chunk, hspthresh=inp.hspthresh).oracle_setup(oracle)
    return _cases[inp.name]


def fresh(E, c, opts=None, max_hits=0):
    """a freshly initialised processor under `opts`: new slots, new lists"""
    E.ShutdownProcessor()
    E.reset_option(None)
    for k, v in (opts or {}).items():
        E.set_option(k, v)
    c.engine_setup(E)
    for k, v in (opts or {}).items():
        assert E.get_option(k) == v, (k, v)
    for k in ("cand_cap", "ent_cap", "out_cap", "hit_batch"):          # unset: 0, the sizing of a real call
        assert E.get_option(k) == (opts or {}).get(k, 0) and E.options()[k] is True, k
    E.set_max_hits(max_hits)
    return E


class Call:
    """chunks first .. last of a strand of an input in one call, on the path `mode` (2 table-direct; 0 general: the device-seeded entries
    under no_td; "host": general, through the drop-in entry with the host's seed words under no_td -- without the option that entry
    verifies the vector on the device and looks it up table-direct too)"""

    def __init__(self, oracle, inp, first=0, last=0, rev=False, mode=2, max_hits=0, hit_batch=0):
        self.inp, self.first, self.last, self.rev, self.mode, self.max_hits, self.hit_batch = inp, first, last, rev, mode, max_hits, hit_batch
        self.c = case_of(oracle, inp)
        self.K = last - first + 1
        self.key = (inp.name, first, last, rev, mode, max_hits)
        self.base = {} if mode == 2 else {"no_td": 1}
        mh = max_hits or (1 << 30)
        self.iters, self.ends, self.hits = inp.plan(first, last, rev, mh)
        self.wants, self.o_iter, self.o_examined = [], 0, 0
        for (s, e) in inp.chunks()[first:last + 1]:
            seeds = self.c.host_seeds(s, e, rev)
            if seeds.size == 0:
                self.wants.append(None)
                continue
            w, st = self.c.oracle_saf(seeds, rev, max_hits=mh)
            self.wants.append(w)
            self.o_iter += int(st["num_iter"])
            self.o_examined += int(st["num_examined"])
        self.records = sum(w.size - 1 for w in self.wants if w is not None)

    def options(self, opts=None):
        o = dict(self.base, **(opts or {}))
        if self.hit_batch:
            o["hit_batch"] = self.hit_batch
        return o

    def run(self, E):
        """-> (vector of every chunk, statistics, trace)"""
        s, e = self.inp.call(self.first, self.last)
        if self.mode == "host":
            assert self.K == 1
            outs = [E.SeedAndFilter(self.c.host_seeds(s, e, self.rev), self.rev, 0)]
        elif self.K == 1:
            outs = [E.SeedAndFilterRange(s, e, self.rev, 0)]
        else:
            outs = E.SeedAndFilterChunks(s, e, self.rev, 0)
            assert all(o.size == 0 for o in outs[self.K:])
            outs = outs[:self.K]
        return outs, E.last_call_stats(), E.last_call_trace()

    def hold(self, E, opts=None, what=None, **route):
        """one call: vectors, hit counts and iterations against the oracle; segments, batches, spec_tried and the route against the model"""
        outs, st, tr = self.run(E)
        what = (self.key, opts, what)
        for j, (o, w) in enumerate(zip(outs, self.wants)):
            if w is None:
                assert o.size == 0, (what, j)                            # a chunk without seeds: NULL, count 0
            else:
                assert seg_equal(o, w), (what, j, o.size, w.size)       # header (hit count, record count) and every record
        assert st["num_hits"] == sum(self.hits) and st["num_iter"] == self.o_iter, (what, st)
        td = self.mode == 2
        assert st["lookup_path"] == (2 if td else 0), (what, st)
        b = CM.batches(self.ends, td, self.hit_batch)
        assert (tr["segments"], tr["batches"]) == (len(self.ends), len(b)), (what, tr, b)
        opts = opts or {}
        kind = dict(td=td, batches=len(b), segments=len(self.ends), spec_dedup=opts.get("spec_dedup", 1), no_small_dedup=opts.get("no_small_dedup", 0))
        assert bool(tr["spec_tried"]) == CM.spec_tried(**kind), (what, tr)
        assert tr["route"] == CM.route(st["num_survivors"], **kind, **route), (what, tr, route)
        assert tr["reruns"] >= (tr["rerun_last_batch"] >= 0) and (tr["reruns"] == 0) == (tr["overflowed"] == 0) == (tr["rerun_first_batch"] < 0), tr
        assert bool(st["path_flags"] & E.PATH_LIST_REGROWN) == (tr["reruns"] > 0), (what, st, tr)
        return outs, st, tr

    def counts(self, E):
        """the counts of one unconstrained call on a fresh processor, the same in a second one"""
        if self.key not in _counts:
            seen = []
            for _ in range(2):
                fresh(E, self.c, self.options(), self.max_hits)
                _, st, tr = self.hold(E, what="unconstrained")
                assert tr["reruns"] == 0
                seen.append({"cand": st["num_candidates"], "ent": st["num_entropy"], "surv": st["num_survivors"], "fwd": st["num_forwarded"],
                             "l2": tr["l2_max"]})
            assert seen[0] == seen[1], seen
            _counts[self.key] = seen[0]
        return _counts[self.key]

    def constrained(self, E, opts, over, later=False, **route):
        """the call under forced capacities on a fresh processor: the lists of `over` (OVER_*; 0: none) overflow and the batch reruns;
        repeated in the same slot it returns the same vectors without a rerun"""
        fresh(E, self.c, self.options(opts), self.max_hits)
        outs, st, tr = self.hold(E, opts, "fresh", **route)
        if over:
            assert tr["overflowed"] == over and tr["reruns"] >= 1, (self.key, opts, tr)
            if later:
                assert tr["rerun_first_batch"] >= 1 and tr["rerun_last_batch"] >= 1, (self.key, opts, tr)
        else:
            assert tr["reruns"] == 0 and tr["overflowed"] == 0, (self.key, opts, tr)
        outs2, st2, tr2 = self.hold(E, opts, "again", **route)
        assert tr2["reruns"] == 0 and all(seg_equal(a, b) for a, b in zip(outs, outs2)), (self.key, opts, tr2)
        return st, tr


def named(n):
    """every named call has a few hundred to a few thousand candidates and at least 50 records"""
    assert 200 <= n["cand"] <= 9999 and n["surv"] >= 50, n


LISTS = {"cand_cap": ("cand", CM.OVER_CANDIDATES, 1), "ent_cap": ("ent", CM.OVER_ENTROPY, 1), "out_cap": ("surv", CM.OVER_SURVIVORS, 1),
         "l2_cap": ("l2", CM.OVER_SECOND_LEVEL, CM.L2_NSUB)}


# ---- a. each list alone, at its count and one below ------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", [0, 1], ids=["at the count", "one below"])
@pytest.mark.parametrize("opt", list(LISTS))
def test_each_list_alone_table_direct(oracle, E, opt, below):
    call = Call(oracle, CM.single())
    assert call.records >= 50
    n = call.counts(E)
    named(n)
    field, bit, unit = LISTS[opt]
    assert n[field] >= 2, (opt, n)
    call.constrained(E, {opt: (n[field] - below) * unit}, bit if below else 0)


def test_all_four_lists_at_their_smallest(oracle, E):
    call = Call(oracle, CM.single())
    fresh(E, call.c, {"cand_cap": 1, "ent_cap": 1, "out_cap": 1, "l2_cap": CM.L2_NSUB})
    outs, st, tr = call.hold(E, what="smallest")
    assert 1 <= tr["reruns"] <= 4 and tr["overflowed"] & CM.OVER_SECOND_LEVEL and tr["overflowed"] & CM.OVER_CANDIDATES, tr
    outs2, _, tr2 = call.hold(E, what="smallest, again")
    assert tr2["reruns"] == 0 and seg_equal(outs[0], outs2[0])


@pytest.mark.parametrize("below", [0, 1], ids=["at the count", "one below"])
@pytest.mark.parametrize("opt", ["cand_cap", "ent_cap", "out_cap"])
def test_each_list_alone_drop_in_entry_with_host_seeds(oracle, E, opt, below):
    call = Call(oracle, CM.single(), mode="host")
    n = call.counts(E)
    named(n)
    field, bit, _ = LISTS[opt]
    assert n[field] >= 2 and n["l2"] == 0 and n["fwd"] == 0, (opt, n)
    call.constrained(E, {opt: n[field] - below}, bit if below else 0)


# ---- b. several batches on the general path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want,nb", [(9, 2), (16, 2), (17, 3)])
def test_batches_of_eight_iterations(oracle, E, want, nb):
    inp = CM.single()
    call = Call(oracle, inp, mode=0, max_hits=inp.max_hits_for(0, want))
    assert call.iters == [want] and call.o_iter == want and call.records >= 50
    fresh(E, call.c, call.options(), call.max_hits)
    _, _, tr = call.hold(E)
    assert tr["batches"] == nb and tr["segments"] == want and tr["route"] == CM.ROUTE_CHAIN_AFTER_SYNC


@pytest.mark.parametrize("less,nb", [(0, 1), (1, 2)], ids=["exactly hit_batch: one batch", "one hit less: two"])
def test_hit_batch_cuts_in_front_of_the_segment_that_passes_it(oracle, E, less, nb):
    inp = CM.single()
    ends = inp.plan(0, 0)[1]
    call = Call(oracle, inp, mode=0, hit_batch=ends[1] - less)
    fresh(E, call.c, call.options())
    _, _, tr = call.hold(E)
    assert tr["batches"] == nb and tr["segments"] == 2


def test_batches_that_straddle_a_chunk_border(oracle, E):
    inp = CM.single()
    call = Call(oracle, inp, 0, 3, mode=0, max_hits=CM.four_chunk_max_hits(inp))
    assert call.iters == [3, 3, 3, 3] and call.records >= 50
    fresh(E, call.c, call.options(), call.max_hits)
    _, _, tr = call.hold(E)
    assert tr["batches"] == 2 and tr["segments"] == 12
    Call(oracle, inp, 0, 3, rev=True, mode=0, max_hits=call.max_hits).hold(E)      # (the other strand in the same slot)


def late_call(oracle):
    inp = CM.late()
    call = Call(oracle, inp, mode=0, max_hits=inp.max_hits_for(0, 17))
    assert call.iters == [17] and call.records >= 50
    return call


def test_survivor_list_overflows_in_a_later_batch(oracle, E):
    """out_cap = the call's survivors - 1: the last batch with survivors overflows, and the records of the batches before it come
    through the regrown list"""
    call = late_call(oracle)
    n = call.counts(E)
    named(n)
    st, tr = call.constrained(E, {"out_cap": n["surv"] - 1}, CM.OVER_SURVIVORS, later=True)
    assert tr["batches"] == 3 and tr["reruns"] == 1 and st["num_survivors"] == n["surv"]


def test_candidate_list_overflows_in_a_later_batch_only(oracle, E):
    call = late_call(oracle)
    n = call.counts(E)
    cap, tr = n["cand"], None
    while cap > 1:                                  # halving from the call's total until a batch overflows: it must not be the first
        cap //= 2
        fresh(E, call.c, call.options({"cand_cap": cap}), call.max_hits)
        _, st, tr = call.hold(E, {"cand_cap": cap})
        if tr["reruns"]:
            break
    assert tr["rerun_first_batch"] >= 1 and tr["rerun_last_batch"] >= 1 and tr["overflowed"] == CM.OVER_CANDIDATES, (cap, tr)
    assert st["num_candidates"] == n["cand"] and st["num_survivors"] == n["surv"] and st["num_entropy"] == n["ent"]
    _, _, tr2 = call.hold(E, {"cand_cap": cap}, "again")
    assert tr2["reruns"] == 0


@pytest.mark.parametrize("opt,field,bit", [("out_cap", "surv", CM.OVER_SURVIVORS), ("cand_cap", "cand", CM.OVER_CANDIDATES)])
def test_examined_counts_survive_a_rerun_in_a_later_batch(oracle, E, opt, field, bit):
    """under sa_set_count_examined(1) (general path, no chain shortcut) the scored positions of the batches before the rerun and of the
    rerun's first attempt must not be counted twice, nor lost"""
    call = late_call(oracle)
    E.set_count_examined(True)
    seen = []
    for _ in range(2):
        fresh(E, call.c, call.options(), call.max_hits)
        _, st, tr = call.hold(E, what="counting")
        assert tr["reruns"] == 0 and tr["batches"] == 3
        seen.append((st["num_examined"], st["num_examined_filter"], st["num_candidates"], st["num_survivors"]))
    assert seen[0] == seen[1] and seen[0][0] == call.o_examined > 0 and seen[0][1] > 0
    # the last batch that has any: one record below the call's total overflows there
    fresh(E, call.c, call.options({opt: seen[0][3] - 1 if opt == "out_cap" else seen[0][2] // 2}), call.max_hits)
    _, st, tr = call.hold(E, what="counting, constrained")
    assert tr["overflowed"] == bit and tr["rerun_first_batch"] >= 1, tr
    assert (st["num_examined"], st["num_examined_filter"]) == seen[0][:2] and st["num_examined"] == call.o_examined


# ---- c. sliced chain -------------------------------------------------------------------------------------------------------------------
def test_chain_slices(oracle, E):
    call = Call(oracle, CM.single())
    n = call.counts(E)["cand"]
    fresh(E, call.c, {"no_chain": 1})
    # (without the shortcut every passing hit is a survivor: the call's first segment -- all but its last seed word -- holds more than
    #  the per-segment chain takes, by the oracle's count)
    o_surv = int(call.c.oracle_saf(call.c.host_seeds(*call.inp.call(0, 0), False), False)[1]["num_survivors"])
    assert o_surv - (call.ends[1] - call.ends[0]) > CM.DEDUP_SEG_MAX
    plain, st, tr = call.hold(E, what="no_chain", refused=True)
    assert tr["slices"] == 0 and tr["route"] == CM.ROUTE_LIBRARY_SORTS and tr["spec_refused"] and st["num_survivors"] == o_surv
    for cap, want in ((n, 0), (n - 1, 2), (-(-n // 3) - 1, 4)):
        assert CM.slices(n, cap) == want
        fresh(E, call.c, {"chain_cap": cap})
        outs, st, tr = call.hold(E, {"chain_cap": cap}, sliced=want > 0)
        assert st["num_candidates"] == n and tr["slices"] == want and bool(st["path_flags"] & E.PATH_CHAIN_SLICED) == (want > 0), (cap, tr)
        assert tr["route"] == (CM.ROUTE_LIBRARY_SORTS if want else CM.ROUTE_SPEC_CHAIN) and tr["spec_tried"] == 1
        assert seg_equal(outs[0], plain[0])


def test_sliced_chain_of_a_sixteen_chunk_call_drops_the_speculative_records(oracle, E):
    call = Call(oracle, CM.sixteen(), 0, 15)
    assert call.records >= 50
    n = call.counts(E)
    named(n)
    fresh(E, call.c, {"chain_cap": n["cand"] - 1})
    _, st, tr = call.hold(E, {"chain_cap": n["cand"] - 1}, sliced=True)
    assert tr["spec_tried"] == 1 and tr["route"] == CM.ROUTE_LIBRARY_SORTS and tr["slices"] == 2 and st["path_flags"] & E.PATH_CHAIN_SLICED


def test_rerun_first_then_slices(oracle, E):
    call = Call(oracle, CM.single())
    n = call.counts(E)["cand"]
    opts = {"chain_cap": n - 1, "cand_cap": n - 1}
    fresh(E, call.c, opts)
    _, st, tr = call.hold(E, opts, sliced=True)
    assert tr["reruns"] == 1 and tr["overflowed"] == CM.OVER_CANDIDATES and tr["slices"] == 2 and st["path_flags"] & E.PATH_CHAIN_SLICED, tr


# ---- d. output routes ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["one chunk", "sixteen chunks"])
def routed(request, oracle):
    return Call(oracle, CM.single()) if request.param == "one chunk" else Call(oracle, CM.sixteen(), 0, 15)


def test_speculative_chain_with_one_and_two_copies(oracle, E, routed):
    call = routed
    surv = call.counts(E)["surv"]
    assert 50 <= surv <= 16384 and call.records >= 50
    for recs, second in ((surv, 0), (surv - 1, 1), (1, surv - 1)):
        fresh(E, call.c, {"spec_recs": recs})
        # (the slot's pinned output buffer first takes the records of another range: a record the call under test fails to fetch is then
        #  another call's, not -- by luck of a fresh allocation -- the one the test before left there)
        other = Call(oracle, call.inp, call.first + 1, max(call.last, call.first + 1))
        assert other.records >= 50
        other.hold(E, {"spec_recs": recs}, "another range first")
        _, st, tr = call.hold(E, {"spec_recs": recs})
        assert tr["route"] == CM.ROUTE_SPEC_CHAIN and tr["second_copy"] == second and not tr["spec_refused"], (recs, tr)


@pytest.mark.parametrize("opts,route,flag,refused", [
    ({"dedup_seg_max": 1}, CM.ROUTE_LIBRARY_SORTS, True, True),
    ({"spec_dedup": 0}, CM.ROUTE_CHAIN_AFTER_SYNC, False, False),
    ({"spec_dedup": 0, "dedup_seg_max": 1}, CM.ROUTE_LIBRARY_SORTS, True, False),
    ({"no_small_dedup": 1}, CM.ROUTE_LIBRARY_SORTS, False, False)], ids=lambda o: " ".join("%s=%s" % kv for kv in o.items()) if isinstance(o, dict) else None)
def test_chain_after_the_sync_and_library_sorts(oracle, E, routed, opts, route, flag, refused):
    call = routed
    # (dedup_seg_max = 1: more records than segments, so some segment holds two survivors or more)
    assert call.records > len(call.ends)
    fresh(E, call.c, opts)
    _, st, tr = call.hold(E, opts, refused="dedup_seg_max" in opts)
    assert tr["route"] == route and bool(st["path_flags"] & E.PATH_DEDUP_FALLBACK) == flag and bool(tr["spec_refused"]) == refused, (opts, st, tr)
    assert tr["second_copy"] == 0


# ---- e. the per-chunk split ------------------------------------------------------------------------------------------------------------
ROUTES = [({}, CM.ROUTE_SPEC_CHAIN), ({"spec_dedup": 0}, CM.ROUTE_CHAIN_AFTER_SYNC), ({"no_small_dedup": 1}, CM.ROUTE_LIBRARY_SORTS)]


@pytest.mark.parametrize("opts,route", ROUTES, ids=["speculative chain", "chain after the sync", "library sorts"])
@pytest.mark.parametrize("make,uneven", [(CM.split, False), (CM.split_last, False), (CM.split, True)],
                         ids=["empty and barren chunks", "all records in the last seeded chunk", "three and two iterations"])
def test_split_of_the_output_per_chunk(oracle, E, make, uneven, opts, route):
    inp = make()
    mh = CM.uneven_max_hits(inp, 0, 15) if uneven else 0
    call = Call(oracle, inp, 0, 15, max_hits=mh)
    fresh(E, call.c, opts, mh)
    outs, st, tr = call.hold(E, opts)
    assert tr["route"] == route and not st["path_flags"] & E.PATH_GENERAL_FALLBACK
    if uneven:
        first = np.concatenate([[0], np.cumsum(call.iters)])
        assert set(call.iters) == {0, 2, 3} and any(first[j] != 2 * j for j in range(16)) and tr["segments"] == first[-1]
    sizes = [o.size for o in outs]
    assert [j for j in range(16) if sizes[j] == 0] == list(CM.SPLIT_EMPTY)            # NULL, count 0
    assert sum(s == 1 for s in sizes) >= 5                                            # header only
    for j in range(16):                                                               # ... and what a call of its own returns
        one = Call(oracle, inp, j, j, max_hits=mh)
        if one.wants[0] is None:
            s, e = inp.call(j, j)
            assert E.SeedAndFilterRange(s, e, False, 0).size == 0
        else:
            o, _, _ = one.hold(E, opts)
            assert seg_equal(o[0], outs[j]), j


# ---- f. raw route ------------------------------------------------------------------------------------------------------------------------
def raw_setup(E, oracle, s, opts):
    E.ShutdownProcessor()
    E.reset_option(None)
    for k, v in list(s.options.items()) + list(opts.items()):
        E.set_option(k, v)
    E.InitializeInterface(1)
    E.GenerateShapePos(CM.SHAPE)
    E.InitializeProcessor(True, 250000, 19, s.mat, s.xdrop, s.hspthresh, s.noentropy)
    t, q = s.pair.target_ascii(), s.pair.query_ascii(s.rev, oracle)
    keep = E.SendRefWriteRequest(t, 0, t.size)
    E.SendQueryWriteRequest(q, 0, q.size, 0)
    return keep


def rows(recs):
    return sorted((int(a), int(b), int(l), int(s)) for a, b, l, s in zip(recs["ref_start"], recs["query_start"], recs["len"], recs["score"]))


@pytest.mark.parametrize("opt,field,bit", [("cand_cap", "num_candidates", CM.OVER_CANDIDATES), ("out_cap", "num_survivors", CM.OVER_SURVIVORS)])
def test_raw_route_reruns(oracle, E, opt, field, bit):
    s = {x.name: x for x in XR.SETS}["W"].resolve(oracle)
    anchors = s.pair.bulk()
    want = rows(XM.records(XM.extend_all(s.pair.ref, s.pair.qry, s.mat, anchors, s.xdrop, s.hspthresh)))
    seen = []
    for _ in range(2):
        keep = raw_setup(E, oracle, s, {"no_chain": 1})
        plain = rows(E.ExtendHits(anchors, s.rev, 0))
        st, tr = E.last_call_stats(), E.last_call_trace()
        assert tr["route"] == CM.ROUTE_RAW and tr["reruns"] == 0 and (tr["segments"], tr["batches"]) == (1, 1)
        seen.append((st["num_candidates"], st["num_survivors"], st["num_entropy"]))
    assert seen[0] == seen[1] and plain == want and st[field] >= 2
    keep = raw_setup(E, oracle, s, {"no_chain": 1, opt: st[field] - 1})
    got = rows(E.ExtendHits(anchors, s.rev, 0))
    st2, tr = E.last_call_stats(), E.last_call_trace()
    assert tr["route"] == CM.ROUTE_RAW and tr["reruns"] >= 1 and tr["overflowed"] == bit and st2["path_flags"] & E.PATH_LIST_REGROWN, tr
    assert got == plain == want and (st2["num_candidates"], st2["num_survivors"]) == seen[0][:2]
    again = rows(E.ExtendHits(anchors, s.rev, 0))
    assert again == want and E.last_call_trace()["reruns"] == 0
    del keep


# ---- g. repeat masker -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rm_input(oracle):
    unit = synth.random_dna(600, 77)                      # tests/test_gpu_rm_mask.py's block: a diverged repeat family, both orientations
    t = synth.random_dna(200000, 15)
    rng = np.random.default_rng(3)
    for i in range(90):
        p = int(rng.integers(0, t.size - 700))
        cp = synth.mutate(unit, 500 + i, 0.05)
        t[p:p + cp.size] = cp if i % 3 else synth.reverse_complement(cp)
    t = synth.soft_mask(t, 5, 0.04)
    return Case(t, t, chunk=30000).oracle_setup(oracle)


RM_RANGE, RM_WINDOW = (30000, 36000), (90000, 200000)     # (a range whose candidates fit the list's first size: the unconstrained call must not rerun)


def rm_fresh(E, c, opts):
    fresh(E, c, opts)
    E.RmSendQueryWriteRequest()


def rm_want(c, oracle, s, e):
    seeds = c.host_seeds(s, e, False)
    w, st = oracle.seed_and_filter(c.o_ref, c.o_ref, c.o_index, c.o_pos, seeds, c.sub_mat, seed_size=c.seed_size, xdrop=c.xdrop,
                                   hspthresh=c.hspthresh, noentropy=c.noentropy, rm=(False, RM_WINDOW[0], RM_WINDOW[1]))
    return seeds, w, st


@pytest.mark.parametrize("opt,field,bit", [("cand_cap", "num_candidates", CM.OVER_CANDIDATES), ("out_cap", "num_survivors", CM.OVER_SURVIVORS)])
def test_repeat_masker_routes_rerun(oracle, E, rm_input, opt, field, bit):
    c = rm_input
    seeds, want, ost = rm_want(c, oracle, *RM_RANGE)
    assert want.size - 1 >= 50
    try:
        seen = []
        for _ in range(2):
            rm_fresh(E, c, {})
            got = E.RmSeedAndFilter(seeds, False, *RM_WINDOW)
            st, tr = E.last_call_stats(), E.last_call_trace()
            assert seg_equal(got, want) and st["num_hits"] == ost["num_hits"] and st["num_iter"] == ost["num_iter"]
            assert tr["route"] == CM.ROUTE_RM_SORT and tr["reruns"] == 0 and not tr["spec_tried"]
            seen.append((st["num_candidates"], st["num_survivors"]))
        assert seen[0] == seen[1] and st[field] >= 2
        ivl_want = oracle.rm_coverage_intervals(want[1:], c.target.size, 1)
        assert ivl_want.size >= 2                       # (one run of covered positions per repeat copy of the range)
        # route 5: the drop-in entry; route 6: the interval entry over the same chunk, records added to the coverage array on the device
        rm_fresh(E, c, {opt: st[field] - 1})
        got = E.RmSeedAndFilter(seeds, False, *RM_WINDOW)
        st5, tr = E.last_call_stats(), E.last_call_trace()
        assert seg_equal(got, want) and tr["route"] == CM.ROUTE_RM_SORT and tr["reruns"] >= 1 and tr["overflowed"] == bit, tr
        assert seg_equal(E.RmSeedAndFilter(seeds, False, *RM_WINDOW), want) and E.last_call_trace()["reruns"] == 0
        rm_fresh(E, c, {})
        ivl, tot = E.RmMaskInterval(RM_RANGE[0], RM_RANGE[1], RM_WINDOW[0], RM_WINDOW[1], 1, 1)
        st6, tr = E.last_call_stats(), E.last_call_trace()
        assert tr["route"] == CM.ROUTE_RM_COVERAGE and tr["reruns"] == 0 and as_list(ivl) == as_list(ivl_want)
        assert tot["num_hsps"] == want.size - 1 and tot["num_hits"] == ost["num_hits"]
        # (the interval entry looks its seeds up table-direct: its own counts place its capacity)
        cap = (st6["num_candidates"] if opt == "cand_cap" else st6["num_survivors"]) - 1
        rm_fresh(E, c, {opt: cap})
        ivl, tot = E.RmMaskInterval(RM_RANGE[0], RM_RANGE[1], RM_WINDOW[0], RM_WINDOW[1], 1, 1)
        tr = E.last_call_trace()
        assert tr["route"] == CM.ROUTE_RM_COVERAGE and tr["reruns"] >= 1 and tr["overflowed"] == bit, tr
        assert as_list(ivl) == as_list(ivl_want) and tot["num_hsps"] == want.size - 1
        ivl, _ = E.RmMaskInterval(RM_RANGE[0], RM_RANGE[1], RM_WINDOW[0], RM_WINDOW[1], 1, 1)
        assert as_list(ivl) == as_list(ivl_want) and E.last_call_trace()["reruns"] == 0
    finally:
        E.RmClearQuery()
