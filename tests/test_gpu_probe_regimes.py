"""GPU: the front of a table-direct call -- probe_kernel, probe_partials_kernel, probe_compact_kernel with call_clear_kernel,
probe_plan_kernel (probe.hip), driven by td_front (front.hip) -- through the test entry sa_probe_call on the hand-built calls of
tests/probe_regimes.py, held to tests/probe_model.py: the per-position lookup, the records with their sentinel, every head-bit word of
the range the class filter may read, td_chunk, the bounds triples, the chunk plans, seg_end and the return value, all by exact
equality.  tests/test_probe_regimes.py shows on the CPU that every call is in the regime it names and that the model equals the oracle.
The plans are also tied to what a real call does with them: SeedAndFilterChunks on the same range under the same MAX_HITS against the
oracle, chunk by chunk (DESIGN.md 4.4')."""
import numpy as np
import pytest

import probe_model as PM
import probe_regimes as R
from helpers import seg_equal

pytestmark = pytest.mark.gpu

CALLS = R.all_calls()


@pytest.fixture(scope="module")
def sub_mat(oracle):
    return oracle.build_sub_mat(910)


@pytest.fixture
def E(engine):
    try:
        yield engine
    finally:
        engine.set_max_hits(0)
        engine.ShutdownProcessor()
        engine.reset_option(None)


def setup(E, sub_mat, world, chunk, rm=False, options=None, hspthresh=3000, noentropy=False):
    """the reference's call order (src/main.cpp:297-298,613-621) up to the table"""
    E.ShutdownProcessor()
    E.reset_option(None)
    for k, v in {**world.options, **(options or {})}.items():
        E.set_option(k, v)
    E.InitializeInterface(1)
    S = world.S
    assert E.GenerateShapePos(S.text) == S.weight
    E.InitializeProcessor(world.transition, chunk, S.span, sub_mat, 910, hspthresh, noentropy)
    keep = E.SendRefWriteRequest(world.target, 0, world.target.size)
    E.GenerateSeedPosTable(keep, 0, world.target.size, world.step, S.span, S.weight)
    if rm:
        E.RmSendQueryWriteRequest()
    return keep


def send(E, call):
    E.SendQueryWriteRequest(call.query.text, 0, call.query.size, call.buffer)


def hold(E, call):
    """one sa_probe_call against the model, field by field"""
    E.set_max_hits(call.max_hits)
    got = E.ProbeCall(call.start, call.end, call.rev, call.buffer, call.rm)
    assert got["status"] == E.PROBE_OK, (call, got)
    want = call.model(E.get_max_hits())
    mode = 1 if call.world.options.get("no_ctx") else 2
    assert got["lookup_mode"] == mode == E.lookup_mode(), (call, got["lookup_mode"])
    assert (got["start"], got["end"], got["chunk"]) == (call.start, call.clipped_end, call.grid_chunk), call
    bad = PM.differences(got, want)
    assert not bad, (call, bad)
    # every word of the returned range beyond the last hit is zero, and the range is the one the class filter may read
    if mode == 2:
        assert got["num_head_words"] == ((got["hits"] + 63) >> 6) * 2 + 16 <= got["head_words_after"], call
        assert not got["head_bits"][(got["hits"] + 31) >> 5:].any(), call
    else:
        assert got["num_head_words"] == 0 and got["head_bits"].size == 0 and got["regrown"] == 0, call
    return got


def poison(E, call):
    """Two other calls in the slot the call under test will get: a dense one of the same chunk count on the other query buffer, and the
    call's own range on the other strand.  What the call under test fails to write then holds another call's values, not -- by luck of
    a fresh allocation -- those of the test before.  -> the slot"""
    E.set_max_hits(0)
    if call.rm:
        return E.ProbeCall(call.start, call.end, not call.rev, 0, True)["slot"]
    pq = R.poison_query(call.world.shape_text)
    E.SendQueryWriteRequest(pq.text, 0, pq.size, 1 - call.buffer)
    n = min(call.end - call.start, pq.size)
    a = E.ProbeCall(0, n, False, 1 - call.buffer)        # (from position 0: the plain path of every kernel writes all there is to write)
    b = E.ProbeCall(call.start, call.end, not call.rev, call.buffer)
    assert a["status"] == b["status"] == E.PROBE_OK and a["slot"] == b["slot"] and (a["hits"] > 0 or not call.world.runs), call   # (a target that was not built need not hold the dense run)
    return a["slot"]


def run(E, sub_mat, call):
    setup(E, sub_mat, call.world, call.chunk, rm=call.rm)
    if not call.rm:
        send(E, call)
        assert np.array_equal(E.copy_query_codes(call.buffer, call.rev), call.query.codes(call.rev)), call
    slot = poison(E, call)
    got = hold(E, call)
    assert got["slot"] == slot, call
    return got


@pytest.mark.parametrize("name", list(CALLS))
def test_probe_call_equals_the_model(E, sub_mat, name):
    call = CALLS[name]
    got = run(E, sub_mat, call)
    for k, v in call.claims.items():           # (what the call was built for, as the entry reports it)
        if k in ("hits", "records", "ret", "K"):
            assert got[{"records": "num_records", "K": "num_chunks"}.get(k, k)] == v, (name, k)


def test_two_calls_of_one_thread_land_in_the_same_slot_and_a_small_call_behind_a_large_one_finds_nothing_stale(E, sub_mat):
    """call_clear_kernel's count: the head-bit words, the records and the td_chunk entries the second call returns lie inside what the
    first one wrote"""
    big = CALLS["head bits: runs of 1, 31, 32, 33 and 100 hits on the atomic path"]
    small = CALLS["head bits: tiles inside and across shared words, a zero-hit tile between two that share one"]
    small = R.Call(small.name, small.world, small.query, small.start, small.end, buffer=1)
    setup(E, sub_mat, big.world, big.chunk)
    send(E, big)
    send(E, small)
    first = hold(E, big)
    second = hold(E, small)
    assert first["slot"] == second["slot"]
    assert first["num_head_words"] > 100 * second["num_head_words"] and first["num_records"] > 100 * second["num_records"]
    assert second["head_words_before"] == first["head_words_after"] == second["head_words_after"]
    third = hold(E, big)                        # ... and the other way round
    assert third["slot"] == first["slot"] and third["regrown"] == 0


def test_head_bit_map_is_regrown_once_and_the_compaction_repeated(E, sub_mat):
    big, small = R.regrow_calls()
    setup(E, sub_mat, big.world, big.chunk)     # (a fresh processor: fresh slots)
    send(E, big)
    send(E, small)
    zero = hold(E, small)
    # the slot's first map; were it larger (a slot kept from an earlier test) the next call would not regrow and this test would say so here
    assert zero["head_words_before"] == 0 and zero["head_words_after"] == R.HEAD_WORDS_MIN and zero["regrown"] == 0
    need = big.facts()["head_words"]
    assert need > R.HEAD_WORDS_MIN
    first = hold(E, big)
    assert first["slot"] == zero["slot"] and first["head_words_before"] == R.HEAD_WORDS_MIN
    assert first["regrown"] == 1 and first["head_words_after"] >= need
    second = hold(E, big)
    assert second["slot"] == first["slot"] and second["regrown"] == 0 and second["head_words_before"] == first["head_words_after"]
    third = hold(E, small)
    assert third["regrown"] == 0


@pytest.mark.parametrize("name", ["lookup: no valid position", "lookup: valid positions whose run is empty"])
def test_call_without_hits_returns_nothing_and_the_probe_leaves_the_statistics_alone(E, sub_mat, name):
    call = CALLS[name]
    q = call.query
    setup(E, sub_mat, call.world, call.chunk)
    send(E, call)
    assert E.SeedAndFilterRange(q.marks["A"], q.marks["A"] + 50, False, 0).size >= 1
    before = E.last_call_stats()
    assert before["num_hits"] == 50 * R.UNITS["A"]
    got = hold(E, call)
    assert got["hits"] == 0 and got["num_records"] == 0 and got["records"]["prefix"][0] == 0 and got["td_chunk"].size == 0
    assert got["ret"] == (0 if "no valid" in name else 90 * got["words"])
    assert E.last_call_stats() == before        # the statistics of the calling thread are held
    out = E.SeedAndFilterRange(call.start, call.end, False, 0)
    assert out.size <= (0 if "no valid" in name else 1) and (out.size == 0 or out[0]["len"] == 0)    # nothing, or the bare header
    st = E.last_call_stats()
    assert st["num_hits"] == 0 and st["num_seeds"] == got["ret"]


TIED = [n for n, c in CALLS.items() if n.split(":")[0].endswith(("plans", "ordinary")) and not c.rm]


@pytest.mark.parametrize("name", TIED)
def test_a_real_call_under_the_same_plan_equals_the_oracle_chunk_by_chunk(E, oracle, sub_mat, name):
    """SeedAndFilterChunks on the range of a plan case under its MAX_HITS: the iteration ends are the scopes of the reference's
    de-duplication.  (hspthresh 500 without the entropy filter, so that most hits leave a record and equal records meet.)  A call the
    front refuses is halved or takes the general path: it must return the same."""
    call = CALLS[name]
    w, S = call.world, call.world.S
    setup(E, sub_mat, w, call.chunk, hspthresh=500, noentropy=True)
    send(E, call)
    got = hold(E, call)
    mh = E.get_max_hits()
    outs = E.SeedAndFilterChunks(call.start, call.end, call.rev, call.buffer)
    st = E.last_call_stats()
    ref, index, pos, ascii_, qcodes = R.oracle_side(oracle, call)
    b = np.minimum(call.start + np.arange(call.num_chunks + 1) * call.grid_chunk, call.clipped_end)
    records = 0
    for c in range(call.num_chunks):
        seeds = oracle.make_seeds(ascii_.tobytes(), 0, int(b[c]), int(b[c + 1]), S.span, S.weight, w.transition) if b[c + 1] > b[c] else np.zeros(0, np.uint64)
        if seeds.size == 0:
            assert outs[c].size == 0, (name, c)
            continue
        want, ost = oracle.seed_and_filter(ref, qcodes, index, pos, seeds, sub_mat, seed_size=S.span, hspthresh=500, noentropy=True, max_hits=mh)
        assert seg_equal(outs[c], want), (name, c, outs[c].size, want.size)
        assert ost["num_hits"] == int(got["plans"]["num_hits"][c]), (name, c)
        records += want.size - 1
    if got["ret"] != PM.REFUSED:
        assert st["num_hits"] == got["hits"] and st["num_seeds"] == got["ret"], (name, st)
    assert records > 0 or got["hits"] < 10, (name, "no record to tie the plan to")


def test_every_reason_for_which_the_entry_returns_nothing(E, sub_mat):
    w, q = R.world(), R.mixed_query()
    E.ShutdownProcessor()
    E.reset_option(None)
    E.InitializeInterface(1)
    assert E.ProbeCall(0, 100) == {"status": E.PROBE_NO_TABLE}                      # before InitializeProcessor
    assert E.GenerateShapePos(w.S.text) == w.S.weight
    E.InitializeProcessor(True, 1000, w.S.span, sub_mat, 910, 3000, False)
    assert E.ProbeCall(0, 100) == {"status": E.PROBE_NO_TABLE}                      # without a table
    setup(E, sub_mat, w, 1)
    assert E.ProbeCall(0, 100) == {"status": E.PROBE_EMPTY_RANGE}                   # no query: its length is 0, the clip leaves nothing
    E.SendQueryWriteRequest(q.text, 0, q.size, 0)
    assert E.ProbeCall(0, 100, buffer=2) == {"status": E.PROBE_NO_TABLE}            # a buffer that does not exist
    assert E.ProbeCall(100, 100) == {"status": E.PROBE_EMPTY_RANGE}
    assert E.ProbeCall(101, 100) == {"status": E.PROBE_EMPTY_RANGE}
    assert E.ProbeCall(q.size - w.S.span + 1, q.size) == {"status": E.PROBE_EMPTY_RANGE}   # wholly behind the last window
    assert E.ProbeCall(0, 257) == {"status": E.PROBE_TOO_MANY_CHUNKS}               # wga_chunk 1: 257 chunks
    assert E.ProbeCall(0, 256)["status"] == E.PROBE_OK
    assert E.ProbeCall(0, 100, rev=True, rm=True) == {"status": E.PROBE_EMPTY_RANGE}   # the target's minus strand is not there yet: length 0
    assert E.ProbeCall(0, 100, rm=True) == {"status": E.PROBE_NOT_ELIGIBLE}         # ... nor its packed copies (RmSendQueryWriteRequest makes them)
    E.RmSendQueryWriteRequest()
    assert E.ProbeCall(0, 100, rm=True)["status"] == E.PROBE_OK and E.ProbeCall(0, 100, rev=True, rm=True)["status"] == E.PROBE_OK
    setup(E, sub_mat, w, 1000, options={"no_td": 1})
    E.SendQueryWriteRequest(q.text, 0, q.size, 0)
    assert E.lookup_mode() == 0
    assert E.ProbeCall(0, 100) == {"status": E.PROBE_NOT_ELIGIBLE}                  # calls of this processor are not table-direct
