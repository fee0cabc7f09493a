"""GPU: the two X-drop filter levels of a table-direct call -- extend_filter_cls_kernel and extend_filter_packed_kernel<SRC_CAND>, and
extend_filter_packed_kernel<SRC_TD> without context table -- hit for hit against tests/filter_model.py (DESIGN.md 4.5''').

Every call runs with audit_cap and fwd_keep set and is compared by EXACT equality, every hit of it:
  * the hand-over list (engine.get_forwards), sorted by hidx, equals the model's level-1 records field for field -- ref_loc, query_loc,
    hidx, state, meta --; num_forwarded is their number, the sub-list counters add up to it and l2_max is the largest of them;
  * the audit list (engine.get_audit) equals the model's level-1 rejects and level-2 rejects together, and did not overflow;
  * num_candidates equals the model's count;
  * the returned vector still equals the oracle's.
tests/test_filter_model.py shows on the CPU which regimes the worlds of tests/filter_regimes.py are in.  Launch geometry, fin_batch, the
wave partition and the query-copy form are no inputs of the model: the verdicts under them are the same ones."""
import numpy as np
import pytest

import filter_model as F
import filter_regimes as R
from helpers import Case, seg_equal

pytestmark = pytest.mark.gpu

AUDIT_CAP = 1 << 22
FIELDS = ("ref_loc", "query_loc", "hidx", "state", "meta")
MODEL_INPUTS = ("ctx_skip_seed", "l2_right_state", "long_cap")


@pytest.fixture(scope="module")
def worlds(oracle):
    return R.worlds(tuple(int(x) for x in oracle.build_sub_mat(910)))


@pytest.fixture
def E(engine):
    engine.ShutdownProcessor()
    engine.reset_option(None)
    try:
        yield engine
    finally:
        engine.ShutdownProcessor()
        engine.reset_option(None)


def open_world(E, oracle, w, options, xdrop=None, with_oracle=True, chunk=None):
    """a fresh processor on the world under these options -> Case"""
    E.set_option("audit_cap", AUDIT_CAP)
    E.set_option("fwd_keep", 1)
    for k, v in options.items():
        E.set_option(k, v)
    c = Case(w.target, w.query, shape=w.shape_text, chunk=chunk or max(w.query.size, 1 << 16), xdrop=w.xdrop if xdrop is None else xdrop,
             hspthresh=w.hspthresh, noentropy=True, sub_mat=w.mat)
    if with_oracle:
        c.oracle_setup(oracle)
        assert np.array_equal(c.o_ref, w.tc) and np.array_equal(c.o_q, w.qc) and np.array_equal(c.o_qrc, w.qrc), w
    c.engine_setup(E)
    assert E.lookup_mode() == (1 if options.get("no_ctx") else 2), (w, options)
    assert E.get_option("fwd_keep") == 1 and E.get_option("audit_cap") == AUDIT_CAP
    return c


def first_diff(got, want):
    for f in FIELDS:
        d = np.flatnonzero(got[f] != want[f])
        if d.size:
            return "%s: %d differ, first at record %d: %#x != %#x (hidx %d)" % (f, d.size, d[0], got[f][d[0]], want[f][d[0]], want["hidx"][d[0]])
    return None


def sub_list_counts(fwd, options):
    """what every sub-list must hold, from the launch rule of the class filter: one wave per chunk of 4096 hits unless ctx_waves asks for
    fewer, whole workgroups of ctx_threads (1024) lanes, wave w of W takes the chunks [w n / W, (w + 1) n / W) and appends to sub-list
    w mod 256.  (DESIGN.md 4.5''' names this partition as part of what is pinned: the sub-list a record lands in decides where level 2
    finds it; a retuned launch moves this function with it.)"""
    n = (fwd.size + 4095) // 4096
    waves = min(n, options.get("ctx_waves") or n)
    wpb = min(1024, max(64, (options.get("ctx_threads") or 1024) & ~63)) // 64
    W = (waves + wpb - 1) // wpb * wpb
    counts = np.zeros(F.L2_NSUB, dtype=np.int64)
    for wid in range(W):
        lo, hi = wid * n // W * 4096, (wid + 1) * n // W * 4096
        counts[wid % F.L2_NSUB] += int(np.count_nonzero(fwd[lo:hi]))
    return counts


def hold_call(E, c, w, rev, start, end, options, xdrop=None, vectors=True, rm=None, chunks=None):
    """one call against the model, everything it reports; rm: (first, last) target position of the repeat masker's window -- the call
    then goes through RmSeedAndFilter with the host seed words of the range; chunks: the (start, end) of the chunks of ONE
    SeedAndFilterChunks call over [start, end)"""
    kw = {k: E.get_option(k) for k in MODEL_INPUTS if k in options}      # (as resolved: long_cap stops at 128, the pad of the packed copies)
    if xdrop is not None:
        kw["xdrop"] = xdrop
    ctx = not options.get("no_ctx")
    if rm is not None:
        kw["rm_window"] = tuple(rm)
    v = w.verdicts(rev, start, end, ctx=ctx, **kw)
    if chunks is not None:
        outs = E.SeedAndFilterChunks(start, end, rev, 0)
    elif rm is None:
        got = E.SeedAndFilterRange(start, end, rev, 0)
    else:
        seeds = c.host_seeds(start, end, rev)
        got = E.RmSeedAndFilter(seeds, rev, rm[0], rm[1])
    st, tr = E.last_call_stats(), E.last_call_trace()
    what = (w, rev, start, end, options)
    assert st["num_hits"] == v.num_hits, what
    assert st["lookup_path"] == (2 if ctx else 1) or v.num_hits == 0, what
    if v.num_hits:                              # (a call without hits never starts the filters: the lists are the call's before)
        pairs, n = E.get_audit(AUDIT_CAP)
        assert n == pairs.shape[0] and n < AUDIT_CAP, "audit list overflowed"
        assert np.array_equal(F.pairs(pairs[:, 0], pairs[:, 1]), v.audit), (what, n, v.audit.shape[0])
        assert st["num_candidates"] == v.cand.shape[0], what
        if ctx:
            rec, nrec, counts = E.get_forwards()
            assert nrec == rec.size == st["num_forwarded"] == v.forwards.size, (what, nrec, rec.size, st["num_forwarded"], v.forwards.size)
            assert int(counts.sum()) == nrec and int(counts.max()) == tr["l2_max"], what
            assert np.array_equal(counts, sub_list_counts(v.l1["fwd"], options)), (what, np.flatnonzero(counts))
            rec = rec[np.argsort(rec["hidx"], kind="stable")]
            assert first_diff(rec, v.forwards) is None, (what, first_diff(rec, v.forwards))
    if vectors and not (rev and np.any(w.qc == R.X)):        # (other IUPAC letters in the query: the reference's minus strand is shifted, hazard H14)
        if chunks is not None:
            for (s0, e0), out in zip(chunks, outs):
                assert seg_equal(out, c.oracle_saf(c.host_seeds(s0, e0, rev), rev)[0]), (what, s0, e0)
        elif rm is not None:
            want = c.O.seed_and_filter(c.o_ref, c.o_qrc if rev else c.o_q, c.o_index, c.o_pos, seeds, c.sub_mat, seed_size=c.seed_size, xdrop=c.xdrop,
                                       hspthresh=c.hspthresh, noentropy=c.noentropy, rm=(rev, rm[0], rm[1]))[0]
        else:
            want = c.oracle_saf(c.host_seeds(start, end, rev), rev)[0] if end > start else got
        assert chunks is not None or seg_equal(got, want), what
    return v, (counts if v.num_hits and ctx else None)


# ---- every world, both strands, both context layouts --------------------------------------------------------------------------------------
WORLDS = ("H", "S", "codes", "field1", "repeat", "self", "synth", "stage", "H22")


@pytest.mark.parametrize("skip", [1, 0], ids=["skip_seed", "whole_window"])
@pytest.mark.parametrize("name", WORLDS)
def test_every_verdict_of_a_world_equals_the_model(oracle, E, worlds, name, skip):
    """the plus strand of the world and the minus strand of its flipped twin (the same islands seen from the other side), under
    ctx_skip_seed 1 and 0"""
    options = {} if skip else {"ctx_skip_seed": 0}
    total = 0
    for w, rev in ((worlds[name], False), (worlds[name].flipped(), True)):
        E.ShutdownProcessor()
        c = open_world(E, oracle, w, options)
        for r in (rev, not rev):
            v, _ = hold_call(E, c, w, r, 0, w.end, options)
            total += v.num_hits
    assert total > 0


# ---- the options -----------------------------------------------------------------------------------------------------------------------
OPTION_SETS = [{"cls_one_copy": 2}, {"l2_right_state": 1}, {"ctx_waves": 1}, {"ctx_threads": 64}, {"fin_batch": 1}, {"fin_batch": 64},
               {"packed_waves": 8}, {"l2_blocks": 1}, {"long_cap": 64}, {"long_cap": 192}, {"long_cap": 192, "l2_right_state": 1},
               {"l2_right_state": 1, "ctx_skip_seed": 0, "cls_one_copy": 2}]


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: " ".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("name", ["H", "S", "synth"])
def test_verdicts_under_every_option_set(oracle, E, worlds, name, options):
    """options that are no model inputs leave every verdict as it was; those that are (ctx_skip_seed, l2_right_state, long_cap) give
    the model's verdicts under them"""
    w = worlds[name]
    c = open_world(E, oracle, w, options)
    assert all(E.get_option(k) == (min(v, 128) if k == "long_cap" else v) for k, v in options.items())
    for rev in (False, True):
        hold_call(E, c, w, rev, 0, w.end, options)


@pytest.mark.parametrize("xdrop", [0, 16383])
@pytest.mark.parametrize("name", ["H", "S"])
def test_verdicts_at_the_ends_of_the_xdrop_range(oracle, E, worlds, name, xdrop):
    """xdrop 0: a side is alive only while it never falls; 16383: no context can drop, every hit is forwarded and walked to long_cap"""
    w = worlds[name]
    c = open_world(E, oracle, w, {}, xdrop=xdrop)
    for rev in (False, True):
        v, _ = hold_call(E, c, w, rev, 0, w.end, {}, xdrop=xdrop)
        if xdrop == 16383:
            assert v.forwards.size == v.num_hits == v.cand.shape[0]


def test_one_call_of_eight_chunks(oracle, E, worlds):
    """SeedAndFilterChunks: the hits of a multi-chunk call are one stream in position order, whatever the chunk grid; every chunk's
    vector is the oracle's"""
    w = worlds["synth"]
    c = open_world(E, oracle, w, {}, chunk=8000)
    ch = c.chunks()
    assert len(ch) == 8
    for rev in (False, True):
        v, _ = hold_call(E, c, w, rev, ch[0][0], ch[-1][1], {}, chunks=ch)
        assert v.num_hits > 4096


def test_repeat_masker_window_skips_hits_in_both_levels(oracle, E, worlds):
    """a block against itself through RmSeedAndFilter with a window that leaves out part of the hits: a skipped hit is neither forwarded
    nor audited, every other verdict is the model's; a window that holds every hit gives the verdicts of the plain call"""
    w = worlds["self"]
    c = open_world(E, oracle, w, {})
    E.RmSendQueryWriteRequest()
    try:
        plain = w.verdicts(False)
        for win in ((800, 1700), (0, w.target.size), (1000, 900)):
            v, _ = hold_call(E, c, w, False, 0, w.end, {}, rm=win)
            skipped = int(np.count_nonzero(v.l1["skip"]))
            assert v.num_hits == plain.num_hits and v.audit.shape[0] + v.cand.shape[0] == v.num_hits - skipped
            assert (skipped == 0) == (win[1] == w.target.size) and (skipped == v.num_hits) == (win[0] > win[1])
            if not skipped:
                assert np.array_equal(v.forwards, plain.forwards) and np.array_equal(v.audit, plain.audit)
    finally:
        E.RmClearQuery()


# ---- without context table: the packed filter on every hit (SRC_TD) ------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{"no_ctx": 1}, {"no_ctx": 1, "long_cap": 64}, {"no_ctx": 1, "packed_waves": 8, "fin_batch": 1}],
                         ids=["default", "long_cap=64", "packed_waves=8 fin_batch=1"])
@pytest.mark.parametrize("name", ["H", "S", "repeat", "synth"])
def test_packed_filter_without_context_table(oracle, E, worlds, name, options):
    """lookup mode 1: the audit list is the model's packed rejects and num_candidates the model's count -- the packed form held from
    above as well as from below; `repeat` brings a run of more than 64 hits and rows of one-hit records to the cursor's window"""
    w = worlds[name]
    c = open_world(E, oracle, w, options)
    for rev in (False, True):
        hold_call(E, c, w, rev, 0, w.end, options)


# ---- the stream: calls of every size around the buffer and chunk cuts ------------------------------------------------------------------
@pytest.mark.parametrize("options", [{}, {"ctx_waves": 1}, {"ctx_waves": 2}, {"no_ctx": 1}], ids=["default", "ctx_waves=1", "ctx_waves=2", "no_ctx"])
def test_calls_of_every_size(oracle, E, worlds, options):
    """calls of 1, 63, 64, 65, 4095, 4096, 4097 and 8193 hits (the stream is cut into buffers of 64 and chunks of 4096 hits); one wave
    walks 1, 2 or 3 chunks: an odd and an even number of buffers"""
    w = worlds["synth"]
    c = open_world(E, oracle, w, options)
    for n in R.STREAM_SIZES:
        rng = w.range_with(False, n)
        assert rng is not None, n
        v, _ = hold_call(E, c, w, False, rng[0], rng[1], options)
        assert v.num_hits == n


def test_forwards_in_one_sub_list_only_and_with_gaps_between(oracle, E, worlds):
    """one chunk under ctx_threads 64 (one wave): sub-list 0 alone; one chunk in a workgroup of sixteen waves: the LAST wave has it, sub-list
    15 alone; three chunks on sixteen waves: three sub-lists with empty ones between and the last used one at the end.  Totals of 1, 64
    and 65 forwards.  (hold_call compares all 256 counters with the launch rule every time.)"""
    w = worlds["synth"]
    ex = w.hits_before(False)
    one_chunk = int(np.searchsorted(ex, 4000))
    c = open_world(E, oracle, w, {"ctx_threads": 64})
    v, counts = hold_call(E, c, w, False, 0, one_chunk, {"ctx_threads": 64})
    assert 0 < v.num_hits <= 4096 and counts[0] == v.forwards.size > 0 and not counts[1:].any()
    E.ShutdownProcessor()
    E.reset_option(None)
    c = open_world(E, oracle, w, {})
    v, counts = hold_call(E, c, w, False, 0, one_chunk, {})
    assert counts[15] == v.forwards.size > 0 and np.count_nonzero(counts) == 1
    v, counts = hold_call(E, c, w, False, 0, w.end, {})
    used = np.flatnonzero(counts)
    assert (v.num_hits + 4095) // 4096 == 3 and used.tolist() == [5, 10, 15]
    full = w.verdicts(False)
    fwd_before = np.concatenate([[0], np.cumsum(full.l1["fwd"])])[ex]                # forwards of the hits in front of every position
    for n in (1, 64, 65):
        cut = np.flatnonzero(fwd_before == n)
        assert cut.size, n
        v, counts = hold_call(E, c, w, False, 0, int(cut[0]), {})
        assert v.forwards.size == n == counts.sum()


# ---- sub-lists shared between waves ---------------------------------------------------------------------------------------------------
def test_more_than_256_waves_share_the_sub_lists(oracle, E):
    """more than 2^20 + 4096 hits in one call: more than 256 waves, so wave 256 appends to sub-list 0 behind wave 0.  Sets and counts"""
    w = R.synth_world("big", np.array(oracle.build_sub_mat(910), dtype=np.int32), n=1_250_000, big=True, records=1, n_runs=0, mask_frac=0.0,
                      sub_rate=0.25, indel_every=60)
    c = open_world(E, oracle, w, {}, with_oracle=False)
    v, counts = hold_call(E, c, w, False, 0, w.end, {}, vectors=False)
    assert v.num_hits > (1 << 20) + 4096 and np.count_nonzero(counts) > 200
