"""GPU: sa_gapped_extend (gapped y-drop extension of HSP anchors) against the serial checker tests/cpp/gapped_check.c, every field of
every raw record (cells and flags included), and its selection mode and concurrency."""
import ctypes as C
import threading

import numpy as np
import pytest

import gapped_model as G
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gcase(engine):
    from segalign_amd import synth
    E = engine
    t, q0 = synth.make_pair(300_000, 41, 42, sub_rate=0.08, mask_frac=0.2, records=3, indel_every=400)
    _, q1 = synth.make_pair(300_000, 41, 43, sub_rate=0.12, mask_frac=0.2, records=3, indel_every=900)
    c = Case(t, q0, chunk=100_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(q1, 0, q1.size, 1)
    ref = E.copy_ref_codes()
    hsps, codes = {}, {}
    for buf, q in ((0, q0), (1, q1)):
        for rev in (False, True):
            segs = []
            for s in range(0, q.size - 19, 100_000):
                r = E.SeedAndFilterRange(s, min(s + 100_000, q.size - 19), rev, buf)
                if r.size > 1:
                    segs.append(r[1:])
            allh = np.concatenate(segs)
            hsps[(buf, rev)] = allh
            codes[(buf, rev)] = E.copy_query_codes(buf, rev)
    yield E, ref, hsps, codes
    E.ShutdownProcessor()


def sample(h, k):
    return h[np.linspace(0, h.size - 1, min(k, h.size)).astype(np.int64)] if h.size else h


def check_raw(E, ref, qcodes, hsps, rev, buf, sub=SUB, **kw):
    """Every field of every raw record, and the call's statistics, against gapped_check.c (sub: the matrix the engine was started with)."""
    got, st = E.GappedExtend(hsps, rev, buf, raw=True, **kw)
    want = G.extend(ref, qcodes, sub, hsps, **{k: v for k, v in kw.items() if k != "gappedthresh"})
    assert got.size == want.size == hsps.size
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (kw, got[bad[:3]].tolist(), want[bad[:3]].tolist())
    assert st["anchors"] == hsps.size and st["cells"] == int(want["cells"].astype(np.uint64).sum())
    assert st["extent_capped"] == int(np.count_nonzero(want["flags"] & G.EXTENT_CAP))
    assert st["band_capped"] == int(np.count_nonzero(want["flags"] & G.BAND_CAP))
    return got


@pytest.mark.parametrize("buf", [0, 1])
@pytest.mark.parametrize("rev", [False, True])
def test_raw_records_equal_the_checker(gcase, buf, rev):
    E, ref, hsps, codes = gcase
    h = sample(hsps[(buf, rev)], 50)
    assert h.size >= 20
    got = check_raw(E, ref, codes[(buf, rev)], h, rev, buf, max_extent=1500)
    assert np.count_nonzero(got["score"] > 0) > h.size // 2


def test_default_parameters_equal_the_checker(gcase):
    E, ref, hsps, codes = gcase
    h = sample(hsps[(0, False)], 4)
    got = check_raw(E, ref, codes[(0, False)], h, False, 0)
    assert got["cells"].min() > 1000


def test_widest_band_instance(gcase):
    E, ref, hsps, codes = gcase
    h = sample(hsps[(1, True)], 6)
    check_raw(E, ref, codes[(1, True)], h, True, 1, max_extent=800, max_band=2048)


def test_ydrop_below_gap_open_and_free_gap_open(gcase):
    E, ref, hsps, codes = gcase
    h = sample(hsps[(0, True)], 25)
    got = check_raw(E, ref, codes[(0, True)], h, True, 0, ydrop=300, max_extent=1500)
    # no gap survives: every extent is a diagonal
    assert np.all((got["ref_end"] - got["ref_start"]) == (got["query_end"] - got["query_start"]))
    check_raw(E, ref, codes[(0, True)], h, True, 0, gap_open=0, max_extent=600)


def test_caps_set_their_flags(gcase):
    E, ref, hsps, codes = gcase
    h = sample(hsps[(1, False)], 25)
    got = check_raw(E, ref, codes[(1, False)], h, False, 1, max_extent=120)
    assert np.count_nonzero(got["flags"] & G.EXTENT_CAP) > 0
    got = check_raw(E, ref, codes[(1, False)], h, False, 1, max_band=12, gap_open=0, gap_extend=10, max_extent=1000)
    assert np.count_nonzero(got["flags"] & G.BAND_CAP) > 0


def test_anchors_at_block_ends_and_separators(gcase):
    E, ref, hsps, codes = gcase
    q = codes[(0, False)]
    seps_t = np.nonzero(ref == 7)[0]
    seps_q = np.nonzero(q == 7)[0]
    assert seps_t.size >= 2 and seps_q.size >= 2
    rows = []
    for (r, qq, ln) in [(0, 0, 0), (0, 0, 1), (1, 2, 4), (ref.size - 1, q.size - 1, 0), (ref.size - 3, q.size - 5, 4),
                        (ref.size - 20, q.size - 20, 40), (ref.size + 50, q.size + 50, 0)]:
        rows.append((r, qq, ln, 0))
    for st, sq in zip(seps_t, seps_q):
        for off in (-3, -1, 0, 1, 2, 5):
            rows.append((int(st) + off, int(sq) + off, 0, 0))
            rows.append((int(st) + off, int(sq) - off, 2, 0))
    h = np.array(rows, dtype=G.SEG_DTYPE)
    check_raw(E, ref, q, h, False, 0, max_extent=700)
    check_raw(E, ref, codes[(0, True)], h, True, 0, max_extent=700)


def test_empty_input_returns_null(gcase):
    E = gcase[0]
    out = C.c_void_p(1)
    st = E.GappedStats()
    p = E.GappedParams(400, 30, 9430, 3000, 0, 0)
    n = E.lib().sa_gapped_extend(None, 0, 0, 0, C.byref(p), 0, C.byref(out), C.byref(st))
    assert n == 0 and not out.value and st.anchors == 0
    recs, s = E.GappedExtend(np.zeros(0, dtype=E.SEG_DTYPE), False, 0)
    assert recs.size == 0 and s["returned"] == 0


def test_selection_mode_equals_the_contract(gcase):
    E, ref, hsps, codes = gcase
    for (buf, rev) in ((0, False), (1, True)):
        h = sample(hsps[(buf, rev)], 60)
        h = np.concatenate([h, h[::7]])  # duplicates: the same extent from several HSPs
        raw = G.extend(ref, codes[(buf, rev)], SUB, h, max_extent=1500)
        for thresh in (3000, 0):
            got, st = E.GappedExtend(h, rev, buf, gappedthresh=thresh, max_extent=1500)
            want = G.select(raw, thresh)
            assert got.size == want.size and np.array_equal(got, want)
            assert st["returned"] == got.size
        assert got.size < h.size


def test_concurrent_callers_get_the_serial_results(gcase):
    E, ref, hsps, codes = gcase
    jobs = []
    for k in range(6):
        key = [(0, False), (0, True), (1, False), (1, True)][k % 4]
        h = hsps[key][k::37][:40]
        jobs.append((h, key[1], key[0], dict(max_extent=600 + 100 * k, raw=bool(k % 2), gappedthresh=1000)))
    serial = [E.GappedExtend(h, rev, buf, **kw)[0] for (h, rev, buf, kw) in jobs]
    results = [None] * len(jobs)

    def run(i):
        h, rev, buf, kw = jobs[i]
        for _ in range(3):
            r = E.GappedExtend(h, rev, buf, **kw)[0]
            if results[i] is None or np.array_equal(results[i], r):
                results[i] = r
            else:
                results[i] = "differs"
    th = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(len(jobs)):
        assert isinstance(results[i], np.ndarray) and np.array_equal(results[i], serial[i]), i
