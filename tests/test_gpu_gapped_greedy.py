"""GPU: sa_gapped_align_greedy (skipping anchors that lie on earlier alignments) against the sequential rule of
tests/gapped_greedy_model.py, run over the serial path checker and over sa_gapped_align raw mode: records, paths and ops exactly, the
per-HSP accounting, batch independence, parameter corners, edge anchors and concurrency."""
import ctypes as C
import re
import threading

import numpy as np
import pytest

import gapped_greedy_model as GR
import gapped_model as G
import gapped_trace_model as T
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu

KEYS = [(0, False), (0, True), (1, False), (1, True)]


def setup(E):
    from segalign_amd import synth
    t, q0 = synth.make_pair(300_000, 41, 42, sub_rate=0.08, mask_frac=0.2, records=3, indel_every=400)
    _, q1 = synth.make_pair(300_000, 41, 43, sub_rate=0.12, mask_frac=0.2, records=3, indel_every=900)
    Case(t, q0, chunk=100_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(q1, 0, q1.size, 1)
    return (q0, q1)


@pytest.fixture(scope="module")
def gcase(engine):
    E = engine
    qs = setup(E)
    ref = E.copy_ref_codes()
    hsps, codes, raw = {}, {}, {}
    for buf, q in enumerate(qs):
        for rev in (False, True):
            segs = []
            for s in range(0, q.size - 19, 100_000):
                r = E.SeedAndFilterRange(s, min(s + 100_000, q.size - 19), rev, buf)
                if r.size > 1:
                    segs.append(r[1:])
            hsps[(buf, rev)] = np.concatenate(segs)
            codes[(buf, rev)] = E.copy_query_codes(buf, rev)
            recs, pth, ops, _ = E.GappedAlign(hsps[(buf, rev)], rev, buf, raw=True)
            raw[(buf, rev)] = (recs, GR.from_align(recs, pth, ops))
    yield E, ref, hsps, codes, raw
    E.ShutdownProcessor()


def sample(h, k):
    return h[np.linspace(0, h.size - 1, min(k, h.size)).astype(np.int64)] if h.size else h


def same(got, want_recs, want_paths):
    recs, paths, ops = got[:3]
    assert np.array_equal(recs, want_recs), (recs[:3], want_recs[:3])
    wp, wops = T.pack(want_paths)
    assert np.array_equal(paths, wp)
    assert np.array_equal(ops, wops)


def check_stats(st, want, n):
    assert st["returned"] == want["returned"]
    assert (st["covered"], st["below_thresh"]) == (want["covered"], want["below_thresh"])
    assert st["returned"] + st["covered"] + st["below_thresh"] == n
    assert st["skipped"] <= st["covered"]
    assert st["anchors"] == n - st["skipped"]


@pytest.mark.parametrize("key", KEYS, ids=["b0+", "b0-", "b1+", "b1-"])
def test_equals_the_model_over_the_checker(gcase, key):
    E, ref, hsps, codes, _ = gcase
    buf, rev = key
    h = sample(hsps[key], 160)  # all of them on a strand with fewer
    assert h.size == min(160, hsps[key].size) and h.size >= 60
    got = E.GappedAlignGreedy(h, rev, buf, max_extent=2000)
    sel, sel_paths, want = GR.from_checker(ref, codes[key], SUB, h, 3000, max_extent=2000)
    same(got, sel, sel_paths)
    check_stats(got[3], want, h.size)


@pytest.mark.parametrize("key", KEYS, ids=["b0+", "b0-", "b1+", "b1-"])
def test_all_hsps_equal_the_model_over_raw_align(gcase, key):
    E, ref, hsps, codes, raw = gcase
    buf, rev = key
    h = hsps[key]
    rrecs, rpaths = raw[key]
    got = E.GappedAlignGreedy(h, rev, buf)
    sel, sel_paths, want = GR.greedy(h, rrecs, rpaths, 3000)
    same(got, sel, sel_paths)
    st = got[3]
    check_stats(st, want, h.size)
    assert want["covered"] > 0 and sel.size < h.size
    # every returned record and path is raw mode's for its HSP
    recs, paths, ops = got[:3]
    for k in range(recs.size):
        i = int(recs[k]["hsp_index"])
        assert recs[k] == rrecs[i]
        lo, ro = T.record_ops(paths, ops, k)
        assert np.array_equal(lo, rpaths[i][0]) and np.array_equal(ro, rpaths[i][1])
    assert st["cover_segments"] > 0 and st["cover_ms"] > 0 and st["priority_batches"] >= 1


def test_batch_size_does_not_change_the_result(gcase):
    E, ref, hsps, codes, raw = gcase
    key = (0, False)
    h = hsps[key]
    small = h[:200]
    base = E.GappedAlignGreedy(h, False, 0)
    base_small = E.GappedAlignGreedy(small, False, 0)
    n_default = E.get_option("gapped_greedy_batch")
    assert h.size <= n_default or base[3]["priority_batches"] > 1
    E.ShutdownProcessor()
    try:
        for b in (1, 3, 64):
            E.set_option("gapped_greedy_batch", b)
            setup(E)
            hh = small if b == 1 else h
            want = base_small if b == 1 else base
            got = E.GappedAlignGreedy(hh, False, 0)
            for a, c in zip(got[:3], want[:3]):
                assert np.array_equal(a, c), b
            for k in ("covered", "below_thresh", "returned"):
                assert got[3][k] == want[3][k], (b, k)
            assert got[3]["priority_batches"] == -(-hh.size // b)
            if b == 1:
                assert got[3]["skipped"] == got[3]["covered"]
            E.ShutdownProcessor()
        E.set_option("gapped_greedy_batch", 1 << 20)
        setup(E)
        got = E.GappedAlignGreedy(h, False, 0)
        assert got[3]["skipped"] == 0 and got[3]["priority_batches"] == 1
        for a, c in zip(got[:3], base[:3]):
            assert np.array_equal(a, c)
    finally:
        E.ShutdownProcessor()
        E.lib().sa_reset_option(b"gapped_greedy_batch")
        setup(E)
    assert E.get_option("gapped_greedy_batch") == n_default
    assert E.GappedAlignGreedy(small, False, 0)[3]["priority_batches"] == -(-small.size // n_default)


def debug_line(text):
    """(priority batches, resolve passes, edges) from the line option debug makes sa_gapped_align_greedy print."""
    m = re.search(r"GappedAlignGreedy: \d+ HSPs, (\d+) priority batches, (\d+) resolve passes, (\d+) edges", text)
    assert m, text[-2000:]
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_edge_budget_splits_resolve_passes(gcase, capfd):
    """A cluster of duplicate anchors covers itself pairwise (quadratically many edges); a small gapped_greedy_edges resolves each batch
    in several passes and must give the same result."""
    E, ref, hsps, codes, raw = gcase
    h0 = hsps[(0, False)][:300]
    dup = np.repeat(h0[np.argmax(h0["score"]) : np.argmax(h0["score"]) + 1], 250)
    h = np.concatenate([h0, dup, h0[::7]])
    base = E.GappedAlignGreedy(h, False, 0)
    assert base[3]["covered"] >= dup.size - 1
    E.ShutdownProcessor()
    try:
        E.set_option("gapped_greedy_edges", 64)
        E.set_option("debug", 1)
        setup(E)
        capfd.readouterr()
        got = E.GappedAlignGreedy(h, False, 0)
        batches, passes, edges = debug_line(capfd.readouterr().err)
        assert passes > batches and edges > 0
        for a, c in zip(got[:3], base[:3]):
            assert np.array_equal(a, c)
        for k in ("covered", "below_thresh", "returned", "skipped"):
            assert got[3][k] == base[3][k], k
    finally:
        E.ShutdownProcessor()
        E.lib().sa_reset_option(b"gapped_greedy_edges")
        E.lib().sa_reset_option(b"debug")
        setup(E)
    E.ShutdownProcessor()
    try:  # in one pass the duplicates cover each other pairwise: at least n (n - 1) / 2 edges
        E.set_option("debug", 1)
        setup(E)
        capfd.readouterr()
        got = E.GappedAlignGreedy(h, False, 0)
        batches, passes, edges = debug_line(capfd.readouterr().err)
        assert passes == batches and edges >= dup.size * (dup.size - 1) // 2
        for a, c in zip(got[:3], base[:3]):
            assert np.array_equal(a, c)
    finally:
        E.ShutdownProcessor()
        E.lib().sa_reset_option(b"debug")
        setup(E)


@pytest.mark.parametrize("kw", [dict(max_band=100, max_extent=800), dict(gap_open=0, max_extent=600), dict(max_extent=120)],
                         ids=["K2", "free_open", "extent_cap"])
def test_parameter_corners(gcase, kw):
    E, ref, hsps, codes, _ = gcase
    key = (1, True)
    h = sample(hsps[key], 60)
    got = E.GappedAlignGreedy(h, True, 1, **kw)
    sel, sel_paths, want = GR.from_checker(ref, codes[key], SUB, h, 3000, **kw)
    same(got, sel, sel_paths)
    check_stats(got[3], want, h.size)


def test_anchors_at_block_ends_and_separators(gcase):
    E, ref, hsps, codes, _ = gcase
    q = codes[(0, False)]
    seps_t = np.nonzero(ref == 7)[0]
    seps_q = np.nonzero(q == 7)[0]
    rows = [(r, qq, ln, sc) for (r, qq, ln, sc) in [(0, 0, 0, 5), (0, 0, 1, 9), (1, 2, 4, 9), (ref.size - 1, q.size - 1, 0, 3),
                                                    (ref.size - 3, q.size - 5, 4, 7), (ref.size - 20, q.size - 20, 40, 7)]]
    for st, sq in zip(seps_t, seps_q):
        for off in (-3, -1, 0, 1, 2, 5):
            rows.append((int(st) + off, int(sq) + off, 0, off))
            rows.append((int(st) + off, int(sq) - off, 2, 4))
    rows += [(int(r), int(qq), int(ln), int(sc)) for r, qq, ln, sc in sample(hsps[(0, False)], 40).tolist()]
    h = np.array(rows, dtype=G.SEG_DTYPE)
    for rev in (False, True):
        got = E.GappedAlignGreedy(h, rev, 0, max_extent=700, gappedthresh=0)
        sel, sel_paths, want = GR.from_checker(ref, codes[(0, rev)], SUB, h, 0, max_extent=700)
        same(got, sel, sel_paths)
        check_stats(got[3], want, h.size)


def test_concurrent_callers_get_the_serial_results(gcase):
    E, ref, hsps, codes, _ = gcase
    jobs = []
    for k in range(6):
        key = KEYS[k % 4]
        jobs.append((hsps[key][k::5][:400], key[1], key[0], dict(max_extent=600 + 100 * k, gappedthresh=1000 + 500 * k)))
    serial = [E.GappedAlignGreedy(h, rev, buf, **kw)[:3] for h, rev, buf, kw in jobs]
    results = [None] * len(jobs)

    def run(i):
        h, rev, buf, kw = jobs[i]
        for _ in range(2):
            r = E.GappedAlignGreedy(h, rev, buf, **kw)[:3]
            if results[i] is None or all(np.array_equal(a, b) for a, b in zip(results[i], r)):
                results[i] = r
            else:
                results[i] = "differs"
    th = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(len(jobs)):
        assert results[i] != "differs" and all(np.array_equal(a, b) for a, b in zip(results[i], serial[i])), i


def test_empty_input_returns_null(gcase):
    E = gcase[0]
    out, paths, ops = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)
    n_ops = C.c_size_t(7)
    st = E.GappedGreedyStats()
    st.covered = 5
    p = E.GappedParams(400, 30, 9430, 3000, 0, 0)
    n = E.lib().sa_gapped_align_greedy(None, 0, 0, 0, C.byref(p), C.byref(out), C.byref(paths), C.byref(ops), C.byref(n_ops), C.byref(st))
    assert n == 0 and not out.value and not paths.value and not ops.value and n_ops.value == 0
    assert st.covered == 0 and st.align.extend.anchors == 0 and st.priority_batches == 0 and st.cover_segments == 0
    recs, pth, o, s = E.GappedAlignGreedy(np.zeros(0, dtype=E.SEG_DTYPE), False, 0)
    assert recs.size == pth.size == o.size == 0 and s["returned"] == 0
