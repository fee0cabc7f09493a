"""CPU: every seed vector of tests/dropin_cases.py is in the regime it is named for.

The drop-in entries decide per call whether the host vector is the seeder's own (fast path: the table-direct call over the positions
it spans) or not (reference-shaped path on the uploaded words).  tests/test_gpu_dropin_paths.py asserts the path and the result of
every case; here, without a GPU:
  * the plain model `expected_fast` gives each case the value its family is named for;
  * a rejected case's answer (oracle) differs from the answer of the exact vector it was made from, in num_hits or in the records, so an
    engine that took the fast path for it fails the result comparison as well, not only the path assertion -- except for the two
    families of dropin_cases.EXEMPT, which only permute words at one or two neighbouring positions;
  * "only the count can reject": every group is the seeder's group for its position and positions ascend strictly;
    "only the verify kernel can reject": as many groups as [first, last] has seed positions;
  * the hand-built vectors for the reference-shaped path put their special word and their iteration boundary where they say."""
import numpy as np
import pytest

import dropin_cases as D
from helpers import seg_equal

CONFIGS = ("12of19", "12of19 notransition", "weight 8", "repeat masker")


@pytest.fixture(scope="module")
def cfgs(oracle):
    return D.configs(oracle)


def differs(a, b):
    return a[1]["num_hits"] != b[1]["num_hits"] or not seg_equal(a[0], b[0])


def test_the_pair_has_what_the_cases_need(oracle, cfgs):
    cfg = cfgs["12of19"]
    c = cfg.case
    assert 29000 <= c.query.size <= 31000 and 29000 <= c.target.size <= 31000
    assert np.any(c.query == ord("N")) and np.any((c.query >= ord("a")) & (c.query <= ord("t")))
    for rev in (False, True):
        lo, hi = cfg.window[rev]
        assert hi - lo == D.WINDOW
        G = cfg.G[rev]
        pos = (G[:, 0] & D.M32).astype(np.int64)
        assert np.any(np.diff(pos) > 19) and G.shape[0] > 2 * D.BLOCK + 300            # a run without seeds inside; room for every index
        want, st = cfg.answer(G, rev)
        assert want.size > 1 and st["num_hits"] > 1000, (rev, st)          # HSPs on this strand
    assert cfg.bucket[cfg.heavy_key] > D.BLOCK and cfg.heavy_key == 0     # the poly-A bucket


@pytest.mark.parametrize("name", CONFIGS)
def test_low_code_bits_give_the_seeders_key_where_a_seed_stands(cfgs, name):
    cfg = cfgs[name]
    for rev, G in cfg.G.items():
        for g in range(0, G.shape[0], 97):
            p = int(G[g, 0] & D.M32)
            assert cfg.key_of_low_bits(rev, p) == int(G[g, 0] >> D.S32)
            assert np.array_equal(cfg.group(int(G[g, 0] >> D.S32), p), G[g])


@pytest.mark.parametrize("name", CONFIGS)
def test_every_case_takes_the_path_it_is_named_for(oracle, cfgs, name):
    cfg = cfgs[name]
    seen = set()
    for case in cfg.cases:
        pos = (case.vector & D.M32).astype(np.int64)
        assert pos.min() >= 0 and pos.max() <= cfg.codes(case.rev).size - len(cfg.shape), case
        assert D.expected_fast(oracle, case.vector, cfg.codes(case.rev), cfg.shape, cfg.transition) == case.fast, case
        assert D.expected_fast(oracle, case.base, cfg.codes(case.rev), cfg.shape, cfg.transition), case
        assert case.fast == (case.family in D.EXACT)
        seen.add((case.family, case.rev))
    fams = set(D.ONLY_COUNT + D.ONLY_VERIFY + D.HOST + D.EXACT)
    if cfg.per == 1:
        fams -= {"one_word_short", "altered_transition_word", "swap_transition_words"}   # one word per position: an exact shorter vector / no such words
    else:
        fams -= {"one_word_short_exact"}
    assert seen == {(f, rev) for f in fams for rev in cfg.G}


@pytest.mark.parametrize("name", CONFIGS)
def test_a_wrongly_taken_fast_path_would_change_the_result(cfgs, name):
    cfg = cfgs[name]
    """The edited vector's answer differs from the answer of the exact vector it was made from AND from the answer of the seeder's
    vector over [first, last + 1) of the edited one, which is the call a wrongly taken fast path would run (the two are the same
    vector unless the edit moved the first or the last word)."""
    answers, consequential = {}, set()

    def answer_of(vector, case):
        key = (case.rev, case.max_hits, vector.tobytes())
        if key not in answers:
            answers[key] = cfg.answer(vector, case.rev, case.max_hits)   # (the fast path would run under the same max_hits)
        return answers[key]

    for case in cfg.cases:
        if case.fast:
            continue
        others = [case.base]
        first, last = int(case.vector[0] & D.M32), int(case.vector[-1] & D.M32)
        if first <= last:
            others.append(cfg.host_seeds(first, last + 1, case.rev))
        got = cfg.answer(case.vector, case.rev, case.max_hits)
        if all(differs(got, answer_of(o, case)) for o in others):
            consequential.add((case.family, case.rev))
        else:
            assert case.family in D.EXEMPT, case
    assert len(D.EXEMPT) <= 2
    # every family but the swap of two transition words of one position (same position, same hits, whatever the iterations) has a
    # case that matters on each strand; for the swap of two groups it is the pair on either side of the masked run
    fams = [f for f in D.ONLY_COUNT + D.ONLY_VERIFY + D.HOST if f != "swap_transition_words" and not (cfg.per == 1 and f in ("one_word_short", "altered_transition_word"))]
    assert consequential >= {(f, rev) for f in fams for rev in cfg.G}, consequential


@pytest.mark.parametrize("name", CONFIGS)
def test_what_only_one_check_can_reject(oracle, cfgs, name):
    cfg = cfgs[name]
    per = cfg.per
    seeder, row_of = {}, {}
    for rev in cfg.G:   # the seeder's groups of the whole strand, and where the group of a position stands among them
        seeder[rev] = cfg.host_seeds(0, cfg.codes(rev).size - len(cfg.shape) + 1, rev).reshape(-1, per)
        row_of[rev] = np.full(cfg.codes(rev).size, -1, dtype=np.int64)
        row_of[rev][(seeder[rev][:, 0] & D.M32).astype(np.int64)] = np.arange(seeder[rev].shape[0])
    for case in cfg.cases:
        if case.family in D.ONLY_COUNT:
            # nothing for the verify kernel to object to: the seeder's own groups at strictly ascending positions
            G = case.vector.reshape(-1, per)
            pos = (G[:, 0] & D.M32).astype(np.int64)
            assert np.all(np.diff(pos) > 0), case
            rows = row_of[case.rev][pos]
            assert np.all(rows >= 0) and np.array_equal(G, seeder[case.rev][rows]), case
        if case.family in D.ONLY_VERIFY:
            # nothing for the host or the count to object to
            assert case.vector.size % per == 0 and case.vector.size == case.base.size, case
            first, last = int(case.vector[0] & D.M32), int(case.vector[-1] & D.M32)
            assert (first, last) == (int(case.base[0] & D.M32), int(case.base[-1] & D.M32)), case
            assert int(cfg.valid_positions(case.rev)[first:last + 1].sum()) == case.vector.size // per, case


def test_vectors_for_the_reference_shaped_path(cfgs):
    cfg = cfgs["12of19"]
    heavy = int(cfg.bucket[cfg.heavy_key])
    vecs = D.edge_vectors(cfg)
    assert {v.n for v in vecs} == set(D.EDGE_SIZES)
    boundary = 0
    for v in vecs:
        hits = cfg.word_hits(v.vector)
        incl = np.cumsum(hits)
        assert v.vector.size == v.n
        want, st = cfg.answer(v.vector, v.rev, v.max_hits)
        assert st["num_hits"] == incl[-1]
        if v.kind == "lonely":
            assert hits[v.at] == 1 and incl[-1] == 1, v.name
        elif v.kind == "heavy":
            assert hits[v.at] == heavy == incl[-1] and v.max_hits < heavy and st["num_iter"] >= 3, v.name
        else:
            assert hits[v.at] == heavy and np.all(np.delete(hits, v.at) == 1), v.name
            if v.n > D.BLOCK and incl[D.BLOCK - 1] < v.max_hits <= incl[D.BLOCK]:   # the first iteration ends with word 255
                boundary += 1
                assert st["num_iter"] >= 2, v.name
            else:
                assert v.max_hits < heavy, v.name
    assert boundary == 2 * sum(len({0, D.BLOCK - 1, D.BLOCK, n - 1}) for n in D.EDGE_SIZES if n > D.BLOCK)
