"""CPU: the calls of tests/probe_regimes.py are in the regimes they name, and tests/probe_model.py equals the oracle where the oracle can
speak -- the hits and the iteration count of every chunk (oracle.seed_and_filter on the seed words oracle.make_seeds emits for the chunk),
and the runs of the positions against the oracle's traced hit list, seed word by seed word.  tests/test_gpu_probe_regimes.py then holds
what sa_probe_call returns to the model on the same calls (DESIGN.md 4.4')."""
import numpy as np
import pytest

import probe_model as PM
import probe_regimes as R
import table_model as M

CALLS = R.all_calls()


# ---- every call is in the regime it names ----------------------------------------------------------------------------------------------
def check_claims(name, call):
    f = call.facts()
    m = call.model()
    pl = m["plans"]
    for k, v in call.claims.items():
        if k in ("skew", "len_mod4", "n", "K", "hits", "records", "valid", "tiles", "ret", "max_run", "tile_nonempty", "tile_hits", "tile_words",
                 "n_iter", "chunk_hits"):
            assert f[k] == v, (name, k, f[k], v)
        elif k in ("tile_words_1", "tile_base_1"):
            assert f[k[:-2]][1] == v, (name, k, f[k[:-2]][1], v)
        elif k == "hits_in":
            full = [t for t, h in enumerate(f["tile_hits"]) if h]
            assert full == [0 if v == "first" else f["tiles"] - 1] and f["hits"] > 0, (name, full)
        elif k == "dense":
            tw = np.array(f["tile_words"])
            assert tw.size == 5 and ((tw > R.HB_LDS_WORDS).all() if v else ((tw > 0) & (tw <= R.HB_LDS_WORDS)).all()), (name, tw)
            # the stretches of 1, 31, 32, 33 and 100 hits: four consecutive records in one word, in four words, across skipped words
            rec = m["records"]
            word = rec["prefix"][:-1].astype(np.int64) >> 5
            step = np.diff(word)
            assert {0, 1}.issubset(step.tolist()) and (step >= 3).any(), name
            assert {1, 31, 32, 33, 100} <= set(np.diff(rec["prefix"].astype(np.int64)).tolist()), name
        elif k == "first_hit":
            pre = m["records"]["prefix"].astype(np.int64)
            r = int(np.flatnonzero(pre == v)[0])
            assert pre[r - 1] < v and m["td_chunk"][1] == (r if v <= R.TD_CHUNK_HITS else r - 1), (name, r, m["td_chunk"])
            assert m["td_chunk"].size == 2
        elif k == "upto0":
            assert int(pl["upto"][0][0]) - int(pl["hit_base"][0]) == v, (name, pl["upto"][0], v)
        elif k == "zero_iter_chunks":
            for c in v:
                assert pl["n_iter"][c] == 0 and pl["n_iter"][:c].any() and pl["n_iter"][c + 1:].any(), (name, c)
        elif k == "segments":
            assert m["num_seg_end"] == v, (name, m["num_seg_end"])
        elif k == "refused":
            assert (m["ret"] == PM.REFUSED) == v, (name, m["ret"])
        elif k == "empty":
            h = np.array(f["chunk_hits"])
            full = np.flatnonzero(h)
            if "first" in v:
                assert h[0] == 0
            if "last" in v:
                assert h[-1] == 0
            if "middle" in v:
                assert (h[full[0]:full[-1]] == 0).any()
        elif k == "same_as_plus_of":
            plus = R.Call("plus", call.world, R.mixed_query(call.world.shape_text), call.start, call.end).model()
            assert np.array_equal(plus["t_cnt"], m["t_cnt"]) and plus["hits"] == m["hits"] > 0, name
        elif k == "words":
            assert m["words"] == v
        else:
            raise AssertionError("unknown claim %s of %s" % (k, name))
    return f


@pytest.mark.parametrize("name", list(CALLS))
def test_call_is_in_the_regime_it_names(name):
    call = CALLS[name]
    f = check_claims(name, call)
    assert f["n"] >= 1 and f["K"] >= 1 and f["K"] <= R.MAX_CHUNKS
    assert call.world.target.size <= 100000 and call.query.size <= 2200000
    if call.world.runs:                     # a built target: every run is the one it was built for
        t = call.world.table
        for k, pieces in call.world.runs.items():
            want = pieces if isinstance(pieces, int) else sum(pieces)
            assert t.run[k] == (want if call.world.transition else t.bucket[k]), (name, k)


def test_groups_hold_the_edges_they_are_named_after():
    g = {name: (c, c.facts()) for name, c in CALLS.items()}
    grid = [f for n, (c, f) in g.items() if n.startswith("grid:")]
    assert {(f["skew"], f["len_mod4"]) for f in grid} >= {(s, l) for s in range(4) for l in range(4)}
    for skew in (0, 3):
        assert {f["n"] for f in grid if f["skew"] == skew} >= {1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049}
    chunks = [(c, f) for n, (c, f) in g.items() if n.startswith("chunks:")]
    assert {c.chunk for c, f in chunks} >= {1, 2, 3, 5, 1023, 1024, 1025}
    assert {f["K"] for c, f in chunks} >= {1, 2, 255, 256}
    # chunk 5 from a multiple of four and from one past it: the boundaries fall on every element of a thread's four positions
    for skew in (0, 1):
        b = {((skew + 5 * k) & 3) for k in range(8)}
        assert b == {0, 1, 2, 3}
    sums = [f for n, (c, f) in g.items() if n.startswith("sums:")]
    assert {f["tiles"] for f in sums} == {R.PP_TILE, R.PP_TILE + 1, 2 * R.PP_TILE + 1}
    # the regrow call needs more words than a slot's first map has, from a few thousand positions
    big, small = R.regrow_calls()
    f = big.facts()
    assert f["head_words"] > max(4 * f["n"] + 64, R.HEAD_WORDS_MIN) and f["n"] < 5000 and f["hits"] > 32 * R.HEAD_WORDS_MIN
    assert small.facts()["head_words"] < 100


def test_letters_invalidate_exactly_the_windows_that_hold_them():
    q = R.letters_query()
    S = q.S
    keys = q.keys()
    bad = np.flatnonzero(M.encode(q.text)[:400 + S.span - 1] >= 4)
    assert bad.size == 7
    want = np.ones(400, dtype=bool)
    for p in bad.tolist():
        want[max(p - S.span + 1, 0):p + 1] = False           # the letter is the last base of the first of them and the first base of the last
    assert np.array_equal(keys[:400] >= 0, want)
    assert set(M.encode(q.text)[bad].tolist()) == {4, 5, 6, 7}


def test_plan_rule_on_hand_made_prefixes():
    """plan_from_words against iteration ends worked out by hand from src/seed_filter.cu:718-745"""
    P = lambda *a: np.array(a, dtype=np.int64)
    assert PM.plan_from_words(P(), 100, False) == (0, [])
    assert PM.plan_from_words(P(0, 0), 100, False) == (0, [])
    assert PM.plan_from_words(P(0, 3, 3, 7), 100, False) == (2, [3, 7])            # below MAX_HITS: before the last hit-bearing word / the word
    assert PM.plan_from_words(P(7, 7, 7), 100, False) == (2, [0, 7])               # all hits in the first word: hazard H5, an empty iteration
    assert PM.plan_from_words(P(3, 6, 9, 12), 6, False) == (4, [3, 6, 9, 12])      # a word boundary on every limit: each is left to the next
    assert PM.plan_from_words(P(3, 6, 9, 12), 7, False) == (3, [6, 9, 12])
    assert PM.plan_from_words(P(10, 11), 5, False) == (4, [0, 0, 0, 11])           # a first word above MAX_HITS
    assert PM.plan_from_words(P(1, 60), 10, False) == (8, [1, 1, 1, 1, 1, 1, 1, 60])
    assert PM.plan_from_words(P(1, 63), 9, False) == (PM.OVERFLOW, [])             # nine iterations
    assert PM.plan_from_words(P(5, 10), (1 << 32) - 11, False) == (2, [5, 10])
    assert PM.plan_from_words(P(5, 10), (1 << 32) - 10, False) == (PM.OVERFLOW, [])
    assert PM.plan_from_words(P(5, 10), (1 << 32) - 10, True) == (2, [5, 10])


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sub_mat(oracle):
    return oracle.build_sub_mat(910)


oracle_side = R.oracle_side


ORACLE_CALLS = [n for n, c in CALLS.items() if c.model()["hits"] <= 200000 and c.query.size <= 100000 and
                (n.split(":")[0].endswith(("plans", "ordinary", "lookup", "td_chunk", "chunks", "notransition")))]


@pytest.mark.parametrize("name", ORACLE_CALLS)
def test_model_chunks_equal_the_oracles_hits_and_iterations(oracle, sub_mat, name):
    call = CALLS[name]
    w, S = call.world, call.world.S
    ref, index, pos, ascii_, qcodes = oracle_side(oracle, call)
    m = call.model()
    mh = call.max_hits or R.DEFAULT_MAX_HITS
    b = np.minimum(call.start + np.arange(call.num_chunks + 1) * call.grid_chunk, call.clipped_end)
    for c in range(call.num_chunks):
        p = m["plans"][c]
        seeds = oracle.make_seeds(ascii_.tobytes(), 0, int(b[c]), int(b[c + 1]), S.span, S.weight, w.transition) if b[c + 1] > b[c] else np.zeros(0, np.uint64)
        assert seeds.size == int(p["num_valid"]) * m["words"], (name, c)
        if seeds.size == 0:
            assert p["n_iter"] == 0 and p["num_hits"] == 0
            continue
        _, st = oracle.seed_and_filter(ref, qcodes, index, pos, seeds, sub_mat, seed_size=S.span, max_hits=mh,
                                       rm=(call.rev, 0, w.target.size) if call.rm else None)
        assert st["num_hits"] == int(p["num_hits"]), (name, c, st, p)
        if p["n_iter"] == PM.OVERFLOW:      # (refused: the general path plans such a chunk, there is no plan of the front to compare)
            continue
        assert st["num_iter"] == int(p["n_iter"]), (name, c, st, p)


TRACED = ["plans: every chunk of the plan query in one call, zero-iteration chunks between planned ones", "ordinary: ordinary, one chunk",
          "ordinary: ordinary, minus strand", "12of19 ordinary: ordinary, minus strand", "lookup: query buffer 1",
          "notransition: notransition: one word per position", "12of19 plans: every chunk of the plan query in one call, below MAX_HITS"]


@pytest.mark.parametrize("name", TRACED)
def test_model_runs_equal_the_oracles_hit_list_word_by_word(oracle, sub_mat, name):
    """the hit list find_hits leaves is in seed word order (the entries of a word in reverse); the records' runs, concatenated, are the
    same list up to the order inside a word"""
    call = CALLS[name]
    w, S = call.world, call.world.S
    ref, index, pos, ascii_, qcodes = oracle_side(oracle, call)
    m = call.model()
    seeds = oracle.make_seeds(ascii_.tobytes(), 0, call.start, call.clipped_end, S.span, S.weight, w.transition)
    _, tr = oracle.seed_and_filter_traced(ref, qcodes, index, pos, seeds, sub_mat, seed_size=S.span, max_hits=1 << 30)
    hits = tr["hits"]
    assert hits.size == m["hits"] > 0
    keys, tpos = M.seed_entries(w.codes, S, w.step)
    assert np.array_equal(tpos, pos)
    _, src = M.neighbourhood(keys, S, w.transition)
    rec = m["records"]
    got_ref = np.concatenate([tpos[src[int(r["off"]):int(r["off"]) + int(n)]] for r, n in zip(rec[:-1], np.diff(rec["prefix"].astype(np.int64)))])
    got_q = np.repeat(rec["qpos"][:-1], np.diff(rec["prefix"].astype(np.int64)))
    # the word of every hit: the hits of the call in word order, the words from the plain bucket sizes
    qk = call.query.keys(call.rev)[call.start:call.clipped_end]
    sizes = w.table.bucket[qk[qk >= 0][:, None] ^ w.table.masks[None, :]].reshape(-1)
    word = np.repeat(np.arange(sizes.size), sizes)
    assert word.size == hits.size
    want = np.lexsort((hits["ref_start"], word))
    have = np.lexsort((got_ref, word))
    assert np.array_equal(hits["ref_start"][want], got_ref[have].astype(np.int64) + S.span)
    assert np.array_equal(hits["query_start"][want], got_q[have].astype(np.int64) + S.span)
