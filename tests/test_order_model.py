"""CPU: tests/order_model.py (numpy: lexsort + head flags) against the oracle's ordering chain (oracle/segalign_oracle.c: comparison
functions, a stable merge sort and a loop), segment by segment, on the tie-rich generator of tests/test_gpu_thrust_order.py and on every
designed set of tests/order_regimes.py.  Two independent restatements of src/seed_filter.cu:47-108 and
repeat_masker_src/seed_filter.cu:45-135 agree before either is used to judge the GPU."""
import numpy as np
import pytest

import order_model as M
import order_regimes as R
from test_gpu_thrust_order import tie_rich


def same_as_oracle(oracle, recs, seg, nsegs, rm):
    m = M.order(recs, seg, nsegs, rm)
    assert int(m["counts"].sum()) == m["records"].size == m["seg"].size
    for g in range(nsegs):
        want = oracle.order_hsps(recs[seg == g], rm)
        got = m["segments"][g]["final"]
        assert got.shape == want.shape and np.all(got == want), (g, rm)
        assert m["counts"][g] == want.size
    return m


@pytest.mark.parametrize("rm", [False, True])
def test_model_equals_oracle_on_tie_rich_sets(oracle, rm):
    rng = np.random.default_rng(11 if rm else 7)
    dropped = 0
    for (n, diagonals, wrap) in ((40, 1, False), (300, 2, False), (1500, 3, False), (1500, 40, True), (2048 * 3 // 4, 5, False),
                                 (30000, 9, True), (200000, 400, False)):
        recs = tie_rich(rng, n, diagonals, span=600 if n < 10000 else 20000, wrap=wrap)
        nsegs = 1 if n < 1000 else 3
        seg = rng.integers(0, nsegs, recs.size).astype(np.uint32)
        m = same_as_oracle(oracle, recs, seg, nsegs, rm)
        dropped += recs.size - m["records"].size
    assert dropped > 1000


def test_model_equals_oracle_on_every_designed_set(oracle):
    for reg in R.all_regimes():
        for rm in (False, True):
            if reg.nsegs > 8 and rm:
                continue     # (the rm chain never meets these: path 0 only)
            m = same_as_oracle(oracle, reg.recs, reg.seg, reg.nsegs, rm)
            if rm is False or reg.rm_too:
                reg._model[rm] = m


def test_stage_lists_are_the_segments_end_to_end():
    reg = R.lib_seg_breaks(9000)
    for rm in (False, True):
        st, m = reg.stages(rm), reg.model(rm)
        assert len(st) == (3 if rm else 2)
        assert st[0]["sorted"].size == reg.recs.size and np.all(np.diff(st[0]["seg"].astype(np.int64)) >= 0)
        assert np.array_equal(st[-1]["sorted"], m["records"]) and np.array_equal(st[-1]["seg"], m["seg"])
