"""GPU: the drop-in entries (sa_seed_and_filter, sa_rm_seed_and_filter) take the table-direct path exactly for the seed vectors that
equal the seeder's own for the positions they span, and return the oracle's result on whichever path they take.

The cases are those of tests/dropin_cases.py (tests/test_dropin_cases.py shows on the CPU what each of them is): edits of the seeder's
vector that only one of the checks behind the decision can reject -- the host's, seed_verify_kernel's key / order / transition-word
tests, the probe's count of positions -- placed where the edit changes the result, next to exact vectors that must stay fast.  Every
case runs in the three lookup modes, on both strands, and is held to
  * the oracle's records on the same vector, bit for bit, and its num_hits and num_iter;
  * sa_call_stats.lookup_path == the lookup mode when dropin_cases.expected_fast says the vector is the seeder's, 0 otherwise.
A second group runs the reference-shaped path (seed_lookup -> scan -> plan -> expand_hits) on hand-built vectors at the 256-seed block
of expand_hits_kernel: 1 .. 513 words, the only hit-bearing word or a word with a bucket of more than 256 positions at the block's
edges, max_hits so that an iteration ends between words 255 and 256 or inside the heavy word.

Not covered (neither is reachable at test size): the grid-stride branch of seed_verify_kernel beyond 4096 x 256 groups, and the
32-bit wrap of the iteration plan (num_hits >= 2^32)."""
import pytest

import dropin_cases as D
from helpers import seg_equal
from test_gpu_lookup_paths import MODES, with_env

pytestmark = pytest.mark.gpu

_want = {}   # the oracle's answers, computed once and shared by the lookup modes


def reference(cfg, what, i, vector, rev, max_hits):
    key = (cfg.name, what, i)
    if key not in _want:
        _want[key] = cfg.answer(vector, rev, max_hits)
    return _want[key]


@pytest.fixture
def clean(engine):
    try:
        yield engine
    finally:
        engine.ShutdownProcessor()
        engine.set_max_hits(0)
        with_env({})


def run_cases(oracle, E, cfg, mode, call):
    n_fast = 0
    for i, case in enumerate(cfg.cases):
        want, st = reference(cfg, "case", i, case.vector, case.rev, case.max_hits)
        E.set_max_hits(case.max_hits or 0)
        got = call(case)
        es = E.last_call_stats()
        assert seg_equal(got, want), (cfg.name, mode, case, got[:3], want[:3])
        assert (es["num_hits"], es["num_iter"]) == (st["num_hits"], st["num_iter"]), (cfg.name, mode, case, es, st)
        fast = D.expected_fast(oracle, case.vector, cfg.codes(case.rev), cfg.shape, cfg.transition)
        assert es["lookup_path"] == (mode if fast else 0), (cfg.name, mode, case, fast, es)
        n_fast += fast
    assert 0 < n_fast < len(cfg.cases)


@pytest.mark.parametrize("mode,env", MODES)
@pytest.mark.parametrize("name", ["12of19", "12of19 notransition", "weight 8"])
def test_drop_in_call_is_fast_exactly_for_the_seeders_vector(oracle, clean, mode, env, name):
    with_env(env)
    E = clean
    cfg = D.configs(oracle)[name]
    cfg.case.engine_setup(E)
    assert E.lookup_mode() == mode
    run_cases(oracle, E, cfg, mode, lambda case: E.SeedAndFilter(case.vector, case.rev, 0))


@pytest.mark.parametrize("mode,env", MODES)
def test_repeat_masker_drop_in_call_is_fast_exactly_for_the_seeders_vector(oracle, clean, mode, env):
    with_env(env)
    E = clean
    cfg = D.configs(oracle)["repeat masker"]
    cfg.case.engine_setup(E)
    E.RmSendQueryWriteRequest()
    try:
        assert E.lookup_mode() == mode
        run_cases(oracle, E, cfg, mode, lambda case: E.RmSeedAndFilter(case.vector, case.rev, 0, cfg.case.target.size))
    finally:
        E.RmClearQuery()


@pytest.mark.parametrize("mode,env", [MODES[0], MODES[2]])   # rejected by the default mode's checks / no table-direct path at all
def test_reference_shaped_path_at_the_edges_of_its_256_seed_block(oracle, clean, mode, env):
    with_env(env)
    E = clean
    cfg = D.configs(oracle)["12of19"]
    cfg.case.engine_setup(E)
    assert E.lookup_mode() == mode
    vecs = D.edge_vectors(cfg)
    for i, v in enumerate(vecs):
        want, st = reference(cfg, "edge", i, v.vector, v.rev, v.max_hits)
        E.set_max_hits(v.max_hits or 0)
        got = E.SeedAndFilter(v.vector, v.rev, 0)
        es = E.last_call_stats()
        assert seg_equal(got, want), (mode, v.name, got[:3], want[:3])
        assert (es["num_hits"], es["num_iter"]) == (st["num_hits"], st["num_iter"]), (mode, v.name, es, st)
        assert not D.expected_fast(oracle, v.vector, cfg.codes(v.rev), cfg.shape, cfg.transition) and es["lookup_path"] == 0, (mode, v.name, es)
    assert len(vecs) > 100
