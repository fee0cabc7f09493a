"""CPU: the inputs of tests/table_regimes.py are in the regimes they name, and tests/table_model.py equals the oracle on them -- the seed
table (oracle.generate_seed_pos_table) and the runs of the neighbourhood table (the buckets of the words oracle.make_seeds emits for a
position, in its order).  tests/test_gpu_table_regimes.py then holds the device tables to the model on the same inputs."""
import numpy as np
import pytest

import table_model as M
import table_regimes as R

TABLE_REGIMES = {**R.TWO_LEVEL_REGIMES, **R.THREE_LEVEL_REGIMES, **R.WEIGHT14_REGIMES, **R.NBR_REGIMES,
                 "sparse": lambda: R.nbr_density((1 << 18) - 1), "dense": lambda: R.nbr_density(1 << 18)}


def oracle_table(oracle, reg):
    S = reg.shape
    assert oracle.generate_shape_pos(S.text) == S.weight
    index, pos = oracle.generate_seed_pos_table(reg.target.tobytes(), 0, reg.target.size, reg.step, S.span, S.weight)
    return index, M.canonical(index, pos)


@pytest.mark.parametrize("name", [n for n in TABLE_REGIMES if n not in R.THREE_LEVEL_REGIMES and n not in R.WEIGHT14_REGIMES])
def test_model_equals_the_oracles_seed_table(oracle, name):
    reg = TABLE_REGIMES[name]()
    keys, pos = reg.entries
    index, opos = oracle_table(oracle, reg)
    assert np.array_equal(index, M.index_ends(keys, reg.shape.nkeys))
    assert M.index_equal(index, keys)
    assert np.array_equal(opos, pos)
    assert np.array_equal(M.encode(reg.target), oracle.encode(reg.target.tobytes()))


def test_model_equals_the_oracles_seed_table_at_weight_14(oracle):
    reg = R.WEIGHT14_REGIMES["14of22 fine 8193"]()
    keys, pos = reg.entries
    index, opos = oracle_table(oracle, reg)
    assert M.index_equal(index, keys)
    assert np.array_equal(opos, pos)


def test_index_equal_notices_a_wrong_table():
    keys = np.array([0, 0, 5, 9, 9, 9], dtype=np.int64)
    good = M.index_ends(keys, 16)
    assert M.index_equal(good, keys)
    for k in (0, 4, 5, 9, 15):
        bad = good.copy()
        bad[k] += 1
        assert not M.index_equal(bad, keys)
    assert M.index_equal(M.index_ends(keys[2:], 16), keys[2:]) and not M.index_equal(good, keys[2:])


@pytest.mark.parametrize("name", sorted(n for n in R.NBR_REGIMES if "dense" not in n))   # (the dense one is "runs w9" plus filler positions)
@pytest.mark.parametrize("transition", [True, False])
def test_model_runs_are_the_oracles_buckets_in_seed_word_order(oracle, name, transition):
    """the target is the query: the run of the key at position p = the oracle's buckets of the words make_seeds emits for p"""
    reg = R.NBR_REGIMES[name]()
    S = reg.shape
    keys, pos = reg.entries
    index, opos = oracle_table(oracle, reg)
    nbr_start, src = M.neighbourhood(keys, S, transition)
    assert int(nbr_start[-1]) == src.size == keys.size * len(S.masks(transition))
    ends = np.concatenate([[0], index.astype(np.int64)])
    n = reg.target.size - S.span
    words = oracle.make_seeds(reg.target.tobytes(), 0, 0, n, S.span, S.weight, transition)
    per = len(S.masks(transition))
    assert words.size % per == 0 and words.size > 0
    seen = set()
    for w in words.reshape(-1, per):
        k = int(w[0] >> np.uint64(32))
        if k in seen:
            continue
        seen.add(k)
        want = np.concatenate([opos[ends[int(x >> np.uint64(32))]:ends[int(x >> np.uint64(32)) + 1]] for x in w])
        got = pos[src[int(nbr_start[k]):int(nbr_start[k + 1])]]
        assert np.array_equal(got, want), (k, got, want)
    # (keys no position of the target holds: their runs come from transition buckets alone -- checked against the buckets directly)
    blen = np.diff(ends)
    for k in np.flatnonzero(np.diff(nbr_start.astype(np.int64)))[:2000].tolist():
        if k not in seen:
            want = np.concatenate([opos[ends[k ^ m]:ends[(k ^ m) + 1]] for m in S.masks(transition)])
            assert np.array_equal(pos[src[int(nbr_start[k]):int(nbr_start[k + 1])]], want)
    assert int(np.diff(nbr_start.astype(np.int64)).sum()) == int(sum(blen[np.arange(S.nkeys) ^ m].sum() for m in S.masks(transition)))


def test_context_record_against_a_base_by_base_statement():
    """context_records against the record spelled out one base at a time (kernels.h CtxRec), on a sequence with every kind of letter"""
    reg = R.nbr_ordinary()
    codes = reg.codes
    span = reg.shape.span
    pos = np.array([1, 2, 3, 57, 58, 59, 60, 200, 1033, codes.size - span - 55, codes.size - span - 54, codes.size - span - 1, codes.size - span])
    for skip in (span, 0):
        recs = M.context_records(codes, pos, span, skip)
        for p, rec in zip(pos.tolist(), recs):
            bits = 0
            for k in range(54):
                i = p + span + k
                c = int(codes[i]) if i < codes.size and codes[i] < 4 else 0
                bits |= c << (2 * k)
            lend = p + span - skip
            for k in range(58):
                i = lend - 1 - k
                c = int(codes[i]) if i >= 0 and codes[i] < 4 else 0
                bits |= (3 - c) << (108 + 2 * k)
            got = sum(int(w) << (32 * j) for j, w in enumerate(rec["w"]))
            assert rec["pos"] == p and got == bits, (p, skip)


@pytest.mark.parametrize("name", sorted(TABLE_REGIMES))
def test_regime_is_what_its_name_says(name):
    reg = TABLE_REGIMES[name]()
    f = reg.facts()
    for k, v in reg.claims.items():
        assert f[k] == v, (name, k, f[k], v)
    three = 2 * reg.shape.weight > 2 * R.TB_COARSE_BITS
    assert (reg.build in (R.THREE_LEVEL, R.GAVE_UP)) == three
    if three:
        assert (f.get("rel_groups_max", 0) < R.REL_GROUPS) == (reg.build == R.THREE_LEVEL), (name, f)
    if reg.build != R.GAVE_UP:
        assert f["parts_over"] == reg.unsorted, (name, f["parts_over"])


def test_capacity_regimes_hold_the_edge_buckets_far_apart():
    for reg in (R.coarse_cap(R.TB_FIN_CAP), R.coarse_cap(R.TB_FIN_CAP + 1), R.fine_cap(R.TB_FIN_CAP_FINE + 1), R.sizes_fit_w9()):
        keys, pos = reg.entries
        f = reg.facts()
        assert {2, R.LDS_SORT_MAX, R.LDS_SORT_MAX + 1, R.SORT_MAX} <= f["bucket_sizes"], reg
        u, c = np.unique(keys, return_counts=True)
        assert (c >= 2).sum() >= 200, reg                      # hundreds of buckets in which order can go wrong
        if reg is not R.sizes_fit_w9():
            # the two members of every pair come from different partition tiles: >= 8192 windows apart
            first = np.concatenate([[0], np.cumsum(c)[:-1]])
            pairs = first[c == 2]
            gap = (pos[pairs + 1].astype(np.int64) - pos[pairs]) // reg.step
            assert pairs.size >= 2 and gap.min() >= R.TB_PART_TILE, (reg, gap.min())
    for reg in (R.sizes_fit_w9(), R.one_partition(0), R.last_fine()):
        assert set(R.EDGE_SIZES) <= reg.facts()["bucket_sizes"], reg


def test_run_regimes_hold_the_named_run_lengths():
    for shape in (R.SHAPE_W9, R.SHAPE_W11_HOLES):
        reg = R.nbr_runs(shape)
        keys, _ = reg.entries
        nbr_start, _ = M.neighbourhood(keys, reg.shape, True)
        run = np.diff(nbr_start.astype(np.int64))
        for k, n in reg.want_runs.items():
            assert run[k] == n, (k, run[k], n)
        assert set(R.RUN_LENGTHS) <= set(run.tolist()) and (run == 0).any()
        if shape == R.SHAPE_W9:               # the dense form: the same runs, one position per key or more
            dense = R.nbr_runs(shape, fill_to=1 << 18)
            assert dense.entries[0].size >= dense.shape.nkeys
            drun = np.diff(M.neighbourhood(dense.entries[0], dense.shape, True)[0].astype(np.int64))
            assert all(drun[k] == n for k, n in dense.want_runs.items())
        # the piece patterns: own bucket empty with transition buckets full; every piece full; a piece above a wave's 64 lanes
        blen = np.diff(np.concatenate([[0], M.index_ends(keys, reg.shape.nkeys).astype(np.int64)]))
        pieces = np.array([[blen[k ^ m] for m in reg.shape.masks(True)] for k in reg.want_runs])
        assert ((pieces[:, 0] == 0) & (pieces[:, 1:].sum(axis=1) > 0)).any()
        assert (pieces > 0).all(axis=1).any() and (pieces > 64).any()
        assert ((pieces[:, 0] > 0) & (pieces[:, -1] > 0) & (pieces[:, 1:-1].sum(axis=1) == 0)).any()


def test_ordinary_regime_reaches_every_phase_and_line_offset():
    reg = R.nbr_ordinary()
    _, pos = reg.entries
    span = reg.shape.span
    anchor = pos.astype(np.int64) + span
    for a in (anchor, pos.astype(np.int64)):          # lend = pos (left_skip = seed_size) or the anchor
        assert np.unique(a % 384).size == 384         # (mod 384 fixes mod 4 as well: every phase copy, every offset in and across the lines)
    assert set(range(1, 61)) <= set(pos.tolist())
    assert (anchor > reg.target.size - 54).any()
    bad = np.flatnonzero(reg.codes >= 4)
    assert {4, 5, 6, 7} <= set(reg.codes[bad].tolist())
    near = np.abs(pos.astype(np.int64)[:, None] - bad[None, :])
    assert (near < 50).any()
