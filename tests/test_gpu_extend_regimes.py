"""GPU: sa_extend_hits -- the extension stage as a call runs it: the X-drop filter in its packed, fast and exact forms, the candidate list,
the chain shortcut, the 512-bases-per-step exact kernel, the entropy kernel -- on the hand-built pairs of tests/extend_regimes.py, held to
tests/extend_model.py field for field (with the entropy factor on: to the oracle).  tests/test_extend_regimes.py shows on the CPU that
the model equals the oracle on every anchor and that each regime is in the state it names.  Every comparison is of integers, for equality.

Per parameter set and option set one bulk call of every anchor: with the chain shortcut off the MULTISET of records is the model's (a
filter that loses one anchor of an island shows), with it on the set is and the count is not larger.  Every regime's anchor is also sent
alone; under the byte-coded filter the number of candidates is the model's too (the filter is an upper bound: too high a bound changes no
record, only this count; the packed filter is held from below only).  One processor set-up per (parameter set, options) comes from the
module-scoped fixture `stage`.  The class filter, which sa_extend_hits never runs, gets the islands through table-direct calls at the end."""
import numpy as np
import pytest

import extend_model as M
import extend_regimes as R
from helpers import Case
from test_gpu_filter_audit import audit_case

pytestmark = pytest.mark.gpu

SHAPE = "TTT0T00TT00T0T0TTTT"
NAMES = [s.name for s in R.SETS]


class Stage:
    """One processor set-up per (parameter set, options), shared by the tests that ask for the same one in a row, and the model's Ext of
    every anchor of a set, computed once.  Options are resolved by InitializeProcessor, so another key means another set-up; every
    option is reset whenever a set-up is left."""

    def __init__(self, E, oracle):
        self.E, self.oracle, self.key, self.keep, self.models = E, oracle, None, None, {}

    def model(self, name):
        """-> the set, the model's Ext of every anchor of pair.bulk() (the pair's own anchors first)"""
        if name not in self.models:
            s = {x.name: x for x in R.SETS + R.ENTROPY_SETS}[name].resolve(self.oracle)
            self.models[name] = (s, M.extend_all(s.pair.ref, s.pair.qry, s.mat, s.pair.bulk(), s.xdrop, s.hspthresh))
        return self.models[name]

    def close(self):
        if self.key is not None:
            self.key = self.keep = None
            self.E.ShutdownProcessor()
        self.E.set_count_examined(False)
        self.E.reset_option(None)

    def use(self, name, opts):
        """the engine with parameter set `name` resident under its own options + opts"""
        E, key = self.E, (name, tuple(sorted(opts.items())))
        E.set_count_examined(False)
        if key == self.key:
            return E
        self.close()
        s, _ = self.model(name)
        p = s.pair
        try:
            for k, v in list(s.options.items()) + list(opts.items()):
                E.set_option(k, v)
            E.InitializeInterface(1)
            E.GenerateShapePos(SHAPE)
            E.InitializeProcessor(True, 250000, 19, s.mat, s.xdrop, s.hspthresh, s.noentropy)
            self.key = key
            t, q = p.target_ascii(), p.query_ascii(s.rev, self.oracle)
            self.keep = E.SendRefWriteRequest(t, 0, t.size)
            E.SendQueryWriteRequest(q, 0, q.size, 0)
            assert np.array_equal(E.copy_ref_codes(), p.ref) and np.array_equal(E.copy_query_codes(0, s.rev), p.qry)
        except BaseException:
            self.close()
            raise
        return E


@pytest.fixture(scope="module")
def stage(engine, oracle):
    st = Stage(engine, oracle)
    yield st
    st.close()


def rows(recs):
    return sorted((int(a), int(b), int(l), int(s)) for a, b, l, s in zip(recs["ref_start"], recs["query_start"], recs["len"], recs["score"]))


def expected_mode(s, opts):
    if opts.get("no_fast_filter"):
        return 0
    return s.modes[1] if opts.get("no_packed_filter") else s.modes[0]


@pytest.mark.parametrize("opt", R.OPTION_SETS, ids=[o[0] for o in R.OPTION_SETS])
@pytest.mark.parametrize("name", NAMES)
def test_bulk_call_equals_the_model(stage, name, opt):
    s, exts = stage.model(name)
    opts = opt[1]
    anchors = s.pair.bulk()
    want = rows(M.records(exts))
    engine = stage.use(name, opts)
    assert engine.filter_mode() == expected_mode(s, opts)
    got = rows(engine.ExtendHits(anchors, s.rev, 0))
    st = engine.last_call_stats()
    if opts.get("no_chain"):
        assert got == want
    else:
        assert set(got) == set(want) and len(got) <= len(want)
    if expected_mode(s, opts) != 3:      # the byte-coded filter is exact: its candidates are the model's
        assert st["num_candidates"] == sum(M.is_candidate(e, s.hspthresh, s.long_cap) for e in exts)


@pytest.mark.parametrize("opts", [{}, {"no_packed_filter": 1}, {"no_fast_filter": 1, "no_chain": 1}], ids=["default", "byte-coded", "exact filter"])
@pytest.mark.parametrize("name", NAMES)
def test_single_anchor_calls_equal_the_model(stage, name, opts):
    s, exts = stage.model(name)
    p = s.pair
    index = {tuple(a): i for i, a in reversed(list(enumerate(p.bulk().tolist())))}
    packed = expected_mode(s, opts) == 3
    engine = stage.use(name, opts)
    for g in p.singles():
        e = exts[index[g.anchors[0]]]
        got = engine.ExtendHits(np.array([g.anchors[0]], dtype=np.uint32), s.rev, 0)
        assert rows(got) == rows(M.records([e])), (g, e.R, e.L)
        cand = int(engine.last_call_stats()["num_candidates"])
        if packed:
            assert cand >= int(e.passed), g       # (an upper bound looked at every 16 bases: it may forward more, and never loses a passing anchor)
        else:
            assert cand == int(M.is_candidate(e, s.hspthresh, s.long_cap)), (g, e.R, e.L)


@pytest.mark.parametrize("name", NAMES)
def test_examined_bases_equal_the_model(stage, name):
    s, exts = stage.model(name)
    engine = stage.use(name, {})
    engine.set_count_examined(True)
    try:
        got = rows(engine.ExtendHits(s.pair.bulk(), s.rev, 0))
        st = engine.last_call_stats()
    finally:
        engine.set_count_examined(False)
    assert got == rows(M.records(exts))                        # (counting runs the byte-coded filter and no chain)
    assert st["num_examined"] == sum(e.examined for e in exts)


@pytest.mark.parametrize("name", [s.name for s in R.SETS if s.chain_exact])
def test_chain_cases_leave_exactly_the_records_of_their_runs(stage, name):
    """every chain regime as a call of its own, where nothing else shares its buckets: which members the shortcut skips is known"""
    s, _ = stage.model(name)
    p = s.pair
    group_max = int(s.options.get("chain_group_max", 1024))
    engine = stage.use(name, {})
    for case, anchors in p.chain_cases:
        got = rows(engine.ExtendHits(anchors, s.rev, 0))
        every = M.records(M.extend_all(p.ref, p.qry, s.mat, anchors, s.xdrop, s.hspthresh))
        if anchors.shape[0] > group_max:                 # a bucket above the sort's capacity is left unsorted: every entry a run head
            want = rows(every)
        else:
            want = rows(M.chain_records(p.ref, p.qry, s.mat, anchors, s.xdrop, s.hspthresh))
        assert got == want, (case, len(got), len(want))
        assert set(got) == set(rows(every))


@pytest.mark.parametrize("options", R.QUEUE_OPTIONS, ids=lambda o: " ".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("name", ["W", "F"])
def test_wave_queue_sizes(stage, name, options):
    """bulk calls of 1, 63, 64, 65 and 64 * 4 * 3 + 1 anchors of mixed walk lengths with four waves (eight for the packed filter) and
    finalise batches of 1, 48 and 64 lanes: the same records under every setting"""
    s, exts = stage.model(name)
    anchors = s.pair.bulk()
    mixed = np.random.default_rng(7).permutation(anchors.shape[0])          # long and short walks side by side in every buffer
    engine = stage.use(name, dict(options, no_chain=1))
    for n in R.QUEUE_SIZES:
        idx = mixed[:n]
        got = rows(engine.ExtendHits(anchors[idx], s.rev, 0))
        assert got == rows(M.records([exts[i] for i in idx])), n


@pytest.mark.parametrize("opt", R.OPTION_SETS, ids=[o[0] for o in R.OPTION_SETS])
@pytest.mark.parametrize("name", [s.name for s in R.ENTROPY_SETS])
def test_entropy_on_equals_the_oracle(oracle, stage, name, opt):
    s, _ = stage.model(name)
    p, opts = s.pair, opt[1]
    anchors = p.bulk()
    ok, recs = oracle.extend_hits_pass(p.ref, p.qry, s.mat, anchors, xdrop=s.xdrop, hspthresh=s.hspthresh, noentropy=False)
    want = rows(recs[ok])
    engine = stage.use(name, opts)
    got = rows(engine.ExtendHits(anchors, False, 0))
    if opts.get("no_chain"):
        assert got == want
    else:
        assert set(got) == set(want) and len(got) <= len(want)
    if hasattr(p, "entropy") and s.hspthresh == 3099:
        for k, a in p.entropy.items():
            one = engine.ExtendHits(np.array([a], dtype=np.uint32), False, 0)
            v, r, _ = oracle.extend_hit(p.ref, p.qry, s.mat, a[0], a[1], xdrop=s.xdrop, hspthresh=s.hspthresh, noentropy=False)
            assert (one.size == 1) == v and (not v or rows(one) == [r]) and (k == "balanced" or v == (k == "above")), k


# ---- the class filter on the same islands: table-direct calls, every filter level audited ----------------------------------------------
@pytest.fixture
def audited(engine, stage):
    stage.close()
    engine.set_option("audit_cap", 1 << 22)
    yield engine
    engine.ShutdownProcessor()
    engine.reset_option(None)


@pytest.mark.parametrize("env_opt,mode", [({}, 2), ({"no_ctx": 1}, 1), ({"no_td": 1}, 0), ({"l2_right_state": 1}, 2)],
                         ids=["context", "no_ctx", "no_td", "l2_right_state"])
def test_class_filter_on_the_islands(oracle, audited, env_opt, mode):
    """near-threshold, dip and tie islands with the drops on the ends of the class filter's six-base fields and its four-base tail: the
    output equals the oracle's, no audited reject passes, every island at hspthresh is in the output and none at hspthresh - 1 is"""
    p = R.pair_c(tuple(int(x) for x in oracle.build_sub_mat(910)))
    for k, v in env_opt.items():
        audited.set_option(k, v)
    c = Case(p.target_ascii(), p.query_ascii(), chunk=60000, noentropy=True).oracle_setup(oracle).engine_setup(audited)
    assert np.array_equal(c.o_ref, p.ref) and np.array_equal(c.o_q, p.qry) and np.array_equal(c.sub_mat, p.mat)
    assert audited.lookup_mode() == mode
    rejected = audit_case(oracle, audited, c, strands=(False,))
    assert rejected > 0 or mode == 0          # (the audit list is the table-direct calls')
    (s0, e0), = c.chunks()
    got = audited.SeedAndFilterRange(s0, e0, False, 0)[1:]
    have = set(rows(got))
    starts = np.sort(got["ref_start"].astype(np.int64))
    exts = M.extend_all(p.ref, p.qry, p.mat, p.anchors(), p.xdrop, p.hspthresh)
    for g, e in zip(p.regs, exts):
        if g.facts.get("kept") is True:
            assert e.total == p.hspthresh and tuple(e.rec) in have, g
        elif g.facts.get("kept") is False:
            lo, n = g.facts["span"]
            assert e.total < p.hspthresh and not np.any((starts >= lo) & (starts < lo + n)), g
