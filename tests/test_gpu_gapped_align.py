"""GPU: sa_gapped_align (the alignment paths of the gapped extension) against sa_gapped_extend and the serial path checker
tests/cpp/gapped_trace_check.c: records bit for bit, ops exactly, the path invariants on every record, the selection mode, the
parameter corners, trace batching and concurrency."""
import ctypes as C
import threading

import numpy as np
import pytest

import gapped_model as G
import gapped_trace_model as T
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu


def setup(E):
    from segalign_amd import synth
    t, q0 = synth.make_pair(300_000, 41, 42, sub_rate=0.08, mask_frac=0.2, records=3, indel_every=400)
    _, q1 = synth.make_pair(300_000, 41, 43, sub_rate=0.12, mask_frac=0.2, records=3, indel_every=900)
    Case(t, q0, chunk=100_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(q1, 0, q1.size, 1)
    return (q0, q1)


@pytest.fixture(scope="module")
def acase(engine):
    E = engine
    qs = setup(E)
    ref = E.copy_ref_codes()
    hsps, codes = {}, {}
    for buf, q in enumerate(qs):
        for rev in (False, True):
            segs = []
            for s in range(0, q.size - 19, 100_000):
                r = E.SeedAndFilterRange(s, min(s + 100_000, q.size - 19), rev, buf)
                if r.size > 1:
                    segs.append(r[1:])
            hsps[(buf, rev)] = np.concatenate(segs)
            codes[(buf, rev)] = E.copy_query_codes(buf, rev)
    yield E, ref, hsps, codes
    E.ShutdownProcessor()


def sample(h, k):
    return h[np.linspace(0, h.size - 1, min(k, h.size)).astype(np.int64)] if h.size else h


def check_paths(ref, q, hsps, recs, paths, ops, gap_open=400, gap_extend=30, sub=SUB):
    """The path invariants of the contract on every record (sub: the matrix the engine was started with)."""
    assert paths.size == recs.size
    total = 0
    for k in range(recs.size):
        r, p = recs[k], paths[k]
        assert int(p["op_offset"]) == total
        total += int(p["n_left"]) + int(p["n_right"])
        lo, ro = T.record_ops(paths, ops, k)
        h = hsps[int(r["hsp_index"])]
        ar, aq = int(h["ref_start"]) + int(h["len"]) // 2, int(h["query_start"]) + int(h["len"]) // 2
        assert T.canonical(lo) and T.canonical(ro)
        assert T.consumed(lo) == (ar - int(r["ref_start"]), aq - int(r["query_start"]))
        assert T.consumed(ro) == (int(r["ref_end"]) - ar, int(r["query_end"]) - aq)
        sl, ml, xl = T.rescore(ref, q, sub, int(r["ref_start"]), int(r["query_start"]), lo, gap_open, gap_extend)
        sr, mr, xr = T.rescore(ref, q, sub, ar, aq, ro, gap_open, gap_extend)
        assert sl + sr == int(r["score"])
        assert (ml + mr, xl + xr) == (int(p["matches"]), int(p["mismatches"]))
        gaps = np.concatenate([lo, ro])
        gaps = gaps[(gaps & 3) != T.OP_M]
        assert (int(p["gap_opens"]), int(p["gap_bases"])) == (gaps.size, int((gaps >> 2).sum()))
    assert total == ops.size


def check_align(E, ref, q, hsps, rev, buf, raw=True, sub=SUB, **kw):
    recs, paths, ops, st = E.GappedAlign(hsps, rev, buf, raw=raw, **kw)
    ext, est = E.GappedExtend(hsps, rev, buf, raw=raw, **kw)
    assert recs.size == ext.size and np.array_equal(recs, ext)
    for k in ("anchors", "cells", "extent_capped", "band_capped", "returned"):
        assert st[k] == est[k], k
    mk = {k: v for k, v in kw.items() if k != "gappedthresh"}
    raw_want, want_paths = T.align(ref, q, sub, hsps, **mk)
    if raw:
        assert np.array_equal(recs, raw_want)
        sel_paths = want_paths
    else:
        sel, sel_paths = T.select(raw_want, want_paths, kw.get("gappedthresh", 3000))
        assert np.array_equal(recs, sel)
    wp, wops = T.pack(sel_paths)
    assert np.array_equal(paths, wp), (paths[:3], wp[:3])
    assert np.array_equal(ops, wops)
    check_paths(ref, q, hsps, recs, paths, ops, kw.get("gap_open", 400), kw.get("gap_extend", 30), sub)
    if recs.size:
        assert st["trace_batches"] >= 1 and st["trace_bytes"] > 0
    return recs, paths, ops, st


@pytest.mark.parametrize("buf", [0, 1])
@pytest.mark.parametrize("rev", [False, True])
def test_raw_paths_equal_the_checker(acase, buf, rev):
    E, ref, hsps, codes = acase
    h = sample(hsps[(buf, rev)], 40)
    assert h.size >= 20
    recs, paths, ops, _ = check_align(E, ref, codes[(buf, rev)], h, rev, buf, max_extent=1500)
    assert np.count_nonzero(paths["gap_opens"]) > 0  # the sample holds gapped alignments


def test_default_parameters(acase):
    E, ref, hsps, codes = acase
    h = sample(hsps[(0, False)], 3)
    recs, *_ = check_align(E, ref, codes[(0, False)], h, False, 0)
    assert recs["cells"].min() > 1000


def test_selection_mode_equals_gapped_extend(acase):
    E, ref, hsps, codes = acase
    for (buf, rev) in ((0, False), (1, True)):
        h = sample(hsps[(buf, rev)], 50)
        h = np.concatenate([h, h[::7]])
        for thresh in (3000, 0):
            recs, *_ = check_align(E, ref, codes[(buf, rev)], h, rev, buf, raw=False, gappedthresh=thresh, max_extent=1500)
        assert recs.size < h.size


@pytest.mark.parametrize("kw", [dict(max_band=100, max_extent=800), dict(max_band=2048, max_extent=800), dict(gap_open=0, max_extent=600),
                                dict(ydrop=300, max_extent=1500), dict(gap_open=50, gap_extend=5, ydrop=2000, max_extent=900)],
                         ids=["K2", "K33", "free_open", "ydrop_below_open", "small_gaps"])
def test_parameter_corners(acase, kw):
    E, ref, hsps, codes = acase
    h = sample(hsps[(1, True)], 16)
    check_align(E, ref, codes[(1, True)], h, True, 1, **kw)


def test_capped_sides(acase):
    E, ref, hsps, codes = acase
    h = sample(hsps[(1, False)], 20)
    recs, *_ = check_align(E, ref, codes[(1, False)], h, False, 1, max_extent=120)
    assert np.count_nonzero(recs["flags"] & G.EXTENT_CAP) > 0
    recs, *_ = check_align(E, ref, codes[(1, False)], h, False, 1, max_band=12, gap_open=0, gap_extend=10, max_extent=1000)
    assert np.count_nonzero(recs["flags"] & G.BAND_CAP) > 0


def test_anchors_at_block_ends_and_separators(acase):
    E, ref, hsps, codes = acase
    q = codes[(0, False)]
    seps_t = np.nonzero(ref == 7)[0]
    seps_q = np.nonzero(q == 7)[0]
    rows = [(r, qq, ln, 0) for (r, qq, ln) in [(0, 0, 0), (0, 0, 1), (1, 2, 4), (ref.size - 1, q.size - 1, 0), (ref.size - 3, q.size - 5, 4),
                                              (ref.size - 20, q.size - 20, 40), (ref.size + 50, q.size + 50, 0)]]
    for st, sq in zip(seps_t, seps_q):
        for off in (-3, -1, 0, 1, 2, 5):
            rows.append((int(st) + off, int(sq) + off, 0, 0))
            rows.append((int(st) + off, int(sq) - off, 2, 0))
    h = np.array(rows, dtype=G.SEG_DTYPE)
    recs, paths, ops, _ = check_align(E, ref, q, h, False, 0, max_extent=700)
    # no op consumes a separator: the consumed ranges hold none
    for r in recs:
        assert not np.any(ref[r["ref_start"]:r["ref_end"]] == 7) and not np.any(q[r["query_start"]:r["query_end"]] == 7)
    check_align(E, ref, codes[(0, True)], h, True, 0, max_extent=700)


def test_trace_budget_of_one_mib_gives_identical_results(acase):
    E, ref, hsps, codes = acase
    h = sample(hsps[(0, False)], 30)
    kw = dict(max_extent=3000)
    want = E.GappedAlign(h, False, 0, raw=True, **kw)
    assert want[3]["trace_batches"] == 1
    E.ShutdownProcessor()
    E.set_option("gapped_trace_mb", 1)
    try:
        setup(E)
        got = E.GappedAlign(h, False, 0, raw=True, **kw)
    finally:
        E.ShutdownProcessor()
        E.lib().sa_reset_option(b"gapped_trace_mb")
        setup(E)
    assert 1 < got[3]["trace_batches"] <= 2 * h.size and got[3]["trace_bytes"] == want[3]["trace_bytes"]
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    # the engine is back on its default budget
    assert E.GappedAlign(h[:4], False, 0, raw=True, **kw)[3]["trace_batches"] == 1


def test_concurrent_callers_get_the_serial_results(acase):
    E, ref, hsps, codes = acase
    jobs = []
    for k in range(6):
        key = [(0, False), (0, True), (1, False), (1, True)][k % 4]
        h = hsps[key][k::37][:30]
        jobs.append((k % 2 == 0, h, key[1], key[0], dict(max_extent=600 + 100 * k, raw=bool(k % 3), gappedthresh=1000)))

    def call(align, h, rev, buf, kw):
        if align:
            r = E.GappedAlign(h, rev, buf, **kw)
            return r[:3]
        return (E.GappedExtend(h, rev, buf, **kw)[0],)

    serial = [call(*j) for j in jobs]
    results = [None] * len(jobs)

    def run(i):
        for _ in range(3):
            r = call(*jobs[i])
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


def test_empty_input_returns_null(acase):
    E = acase[0]
    out, paths, ops = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)
    n_ops = C.c_size_t(7)
    st = E.GappedAlignStats()
    p = E.GappedParams(400, 30, 9430, 3000, 0, 0)
    n = E.lib().sa_gapped_align(None, 0, 0, 0, C.byref(p), 0, C.byref(out), C.byref(paths), C.byref(ops), C.byref(n_ops), C.byref(st))
    assert n == 0 and not out.value and not paths.value and not ops.value and n_ops.value == 0
    assert st.extend.anchors == 0 and st.trace_batches == 0
    recs, pth, o, s = E.GappedAlign(np.zeros(0, dtype=E.SEG_DTYPE), False, 0)
    assert recs.size == pth.size == o.size == 0 and s["returned"] == 0

