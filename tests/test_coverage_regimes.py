"""CPU: the hand-built coverage inputs of tests/coverage_regimes.py.  Every input is shown, on tests/coverage_model.py, to be in the regime
it names, and the oracle (orc_rm_coverage_intervals, the reference's loops restated with the clipping at the block end) is held to the
model on every regime, as whole lists.  tests/test_gpu_coverage_regimes.py holds the device to the same model."""
import numpy as np
import pytest

import coverage_regimes as R
from coverage_model import numpy_model

SMALL = R.small_regimes()


def as_list(iv):
    return [(int(a), int(b)) for a, b in zip(iv["query_start"], iv["len"])]


def held(oracle, reg):
    for M in reg.Ms:
        assert as_list(oracle.rm_coverage_intervals(reg.hsps, reg.block_len, M)) == reg.want(M), (reg, M)


def test_the_regime_records_have_the_engines_and_the_oracles_layout(oracle):
    from segalign_amd import engine as E
    assert R.SEG == E.SEG_DTYPE == oracle.SEG_DTYPE


@pytest.mark.parametrize("reg", SMALL, ids=lambda r: r.name)
def test_small_regime_is_what_it_names(reg):
    assert reg.holds(reg), reg


@pytest.mark.parametrize("reg", SMALL, ids=lambda r: r.name)
def test_oracle_equals_the_model_on_small_regime(oracle, reg):
    held(oracle, reg)


@pytest.mark.parametrize("first_mod4", R.FIRST_MOD4)
def test_touched_ranges_are_what_they_name_and_the_oracle_equals_the_model(oracle, first_mod4):
    for span in R.SPANS:
        reg = R.touched(first_mod4, span)
        assert reg.holds(reg), reg
        held(oracle, reg)


def test_thread_regimes_are_what_they_name_with_their_own_block_lengths(oracle):
    regs = R.thread_regimes()
    assert len(regs) == 8 and len({r.block_len for r in regs}) == 8 and len({r.name for r in regs}) == 8
    for reg in regs:
        assert 1000 <= reg.block_len <= 600000 and reg.holds(reg), reg
        held(oracle, reg)


def test_the_second_batch_decides_the_answer_and_the_oracle_equals_the_model(oracle):
    """the answer for 2^24 + 5 HSPs differs from the answer without the last five, and with the first five in their place"""
    reg = R.second_batch()
    assert reg.holds(reg), reg
    held(oracle, reg)


def test_the_past_the_end_examples_by_hand(oracle):
    """block of 100, HSPs (80, 10) and (85, 30): one run 80..99, open at the block end -> nothing at M = 1; the overlap 85..89 at M = 2"""
    h = R.recs([(80, 10), (85, 30)])
    assert numpy_model(h, 100, 1) == [] == as_list(oracle.rm_coverage_intervals(h, 100, 1))
    assert numpy_model(h, 100, 2) == [(85, 5)] == as_list(oracle.rm_coverage_intervals(h, 100, 2))


def test_vectorised_model_equals_a_position_by_position_count():
    """the model's difference array against the plainest statement of the rules: one increment per counted position, a serial run walk"""
    rng = np.random.default_rng(77)
    for L, n, maxlen in ((1, 5, 4), (2, 9, 5), (50, 700, 60), (400, 40, 90)):
        h = R.recs([(int(a), int(b)) for a, b in zip(rng.integers(0, L + 3, n), rng.integers(0, maxlen, n))])
        count = [0] * L
        for a, b in zip(h["query_start"].tolist(), h["len"].tolist()):
            for j in range(a, min(a + b, L)):
                count[j] += 1
        for M in (0, 1, 2, 3, 200, 255, 256):
            runs, start = [], None
            for i in range(L):
                if (count[i] & 0xFF) >= M:
                    start = i if start is None else start
                elif start is not None:
                    runs.append((start, i - start))
                    start = None
            assert numpy_model(h, L, M) == runs, (L, M)
