"""GPU: sa_rm_coverage_intervals (coverage.hip + coverage_finish in api_rm.hip: the difference array, the touched range, three prefix
scans per tile, the run slots) on the hand-built inputs of tests/coverage_regimes.py, held to tests/coverage_model.py as whole lists.
tests/test_coverage_regimes.py shows on the CPU that every input is in the regime it names and that the oracle equals the model on all of
them.  Pinned here: HSPs that run past the end of the block are clipped to it, not dropped; touched ranges that start at every word
alignment and end on either side of the scan's tiles and of its 256-tile trips; stacks at the uint8 wrap; M = 0 and 256; the run-slot cap
of a tiny block; inputs that count nothing; the difference array left zeroed behind every kind of call; eight callers at once; the second
upload batch."""
import threading

import numpy as np
import pytest

import coverage_regimes as R
from coverage_model import numpy_model
from helpers import Case
from segalign_amd import synth

pytestmark = pytest.mark.gpu

SMALL = R.small_regimes()


def as_list(iv):
    return [(int(a), int(b)) for a, b in zip(iv["query_start"], iv["len"])]


@pytest.fixture(scope="module")
def E(oracle, engine):
    """the entry takes a slot of the processor's pool: a small resident block is enough, its sequence plays no part"""
    t = synth.random_dna(3000, 21)
    Case(t, t, chunk=3000).oracle_setup(oracle).engine_setup(engine)
    yield engine
    engine.ShutdownProcessor()


def held(E, reg):
    for M in reg.Ms:
        assert as_list(E.RmCoverageIntervals(reg.hsps, reg.block_len, M)) == reg.want(M), (reg, M)


@pytest.mark.parametrize("reg", SMALL, ids=lambda r: r.name)
def test_small_regime_equals_the_model(E, reg):
    held(E, reg)


@pytest.mark.parametrize("first_mod4", R.FIRST_MOD4)
def test_touched_ranges_equal_the_model(E, first_mod4):
    for span in R.SPANS:
        held(E, R.touched(first_mod4, span))


def test_the_difference_array_is_left_zeroed(E):
    """an M = 0 call (no runs are extracted), a call that counts nothing and a past-the-end call (its -1 sits on the word behind the
    block), each followed by an M = 1 call on other HSPs in a block of the same length"""
    L = 3000
    clean = R.recs([(100, 40), (120, 40), (2000, 7), (L - 30, 12)])
    want = numpy_model(clean, L, 1)
    assert want == [(100, 60), (2000, 7), (L - 30, 12)]
    stack = R.recs([(90, 500)] * 3 + [(L - 50, 49)])
    assert E.RmCoverageIntervals(stack, L, 0).size == 0
    assert as_list(E.RmCoverageIntervals(clean, L, 1)) == want
    assert E.RmCoverageIntervals(R.recs([(110, 0), (L - 1, 0)]), L, 1).size == 0
    assert as_list(E.RmCoverageIntervals(clean, L, 1)) == want
    past = R.recs([(95, 30), (L - 40, 20), (L - 35, 400), (L - 10, 0xFFFFFFFF), (L, 5)])  # (L-40, 20) runs on into the clipped ones
    assert as_list(E.RmCoverageIntervals(past, L, 1)) == numpy_model(past, L, 1) == [(95, 30)]
    assert as_list(E.RmCoverageIntervals(clean, L, 1)) == want
    assert as_list(E.RmCoverageIntervals(past, L, 2)) == numpy_model(past, L, 2) == [(L - 35, 15)]
    assert as_list(E.RmCoverageIntervals(clean, L, 2)) == numpy_model(clean, L, 2) == [(120, 20)]


def test_eight_threads_get_the_serial_results(E):
    regs = R.thread_regimes()
    serial = [[as_list(E.RmCoverageIntervals(r.hsps, r.block_len, M)) for M in r.Ms] for r in regs]
    out, errors = [None] * 8, []

    def work(i):
        try:
            r = regs[i]
            out[i] = [[as_list(E.RmCoverageIntervals(r.hsps, r.block_len, M)) for M in r.Ms] for _ in range(3)]
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i, r in enumerate(regs):
        assert serial[i] == [r.want(M) for M in r.Ms], r
        assert out[i] == [serial[i]] * 3, r


def test_the_second_upload_batch(E):
    """2^24 + 5 HSPs of len <= 3 in a block of 4096: the records go up in two batches (2^24 and 5), and the five of the second decide the
    tail of the answer (coverage_regimes.second_batch; tests/test_coverage_regimes.py shows that the answer without them, or with the
    first five read again in their place, differs at M = 1 and M = 2)"""
    reg = R.second_batch()
    assert reg.hsps.size == R.BATCH + 5 and reg.want(1)[-2:] == [(reg.block_len - 150, 3), (reg.block_len - 100, 2)]
    held(E, reg)
