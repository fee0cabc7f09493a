"""CPU: every input of tests/order_regimes.py is in the regime it names, shown on the intermediates of tests/order_model.py alone, so that
tests/test_gpu_order_regimes.py cannot pass quietly on an input that misses its target."""
import numpy as np
import pytest

import order_model as M
import order_regimes as R


def pow2(m):
    p = 1
    while p < m:
        p <<= 1
    return p


def first_list_is_the_design(reg, rm=False):
    key = "sorted0_rm" if rm else "sorted0"
    st = reg.stages(rm)[0]
    assert np.array_equal(st["sorted"], reg.facts[key]), reg
    return st


@pytest.mark.parametrize("m", R.LDS_SIZES)
def test_lds_sizes(m):
    for reg in (R.size_distinct(m), R.size_tower(m)):
        st = first_list_is_the_design(reg)
        assert reg.recs.size == m and int(st["keep"].sum()) == reg.facts["m2"] == reg.model()["records"].size
    assert R.size_distinct(m).facts["m2"] == m and R.size_tower(m).facts["m2"] == 1
    assert not np.array_equal(R.size_distinct(m).recs, R.size_distinct(m).facts["sorted0"]) or m < 3      # shuffled
    if m > 1024:
        for m2 in (1025, 1024, 1023):
            if m2 < m:
                reg = R.size_across(m, m2)
                st = first_list_is_the_design(reg)
                assert int(st["keep"].sum()) == m2 == reg.model()["records"].size
        assert pow2(m) == 2048 and pow2(1025) == 2048 and pow2(1024) == pow2(1023) == 1024   # the second network at the same and at half the size


def test_lds_sizes_cover_pad_free_networks_and_the_capacity():
    assert {m for m in R.LDS_SIZES if pow2(m) == m} >= {1, 2, 64, 1024, 2048} and max(R.LDS_SIZES) == R.SEG_CAP


@pytest.mark.parametrize("T", R.LDS_THREADS)
@pytest.mark.parametrize("kind", ["drop", "chain", "corner"])
def test_lds_tile_edges(T, kind):
    reg = R.lds_tile_edge(T, kind)
    st = first_list_is_the_design(reg)
    s, keep = st["sorted"], st["keep"]
    assert reg.recs.size <= R.SEG_CAP and reg.facts["edges"] and reg.facts["edges"][0] == T
    assert not keep[reg.facts["drops"]].any() and keep[reg.facts["keeps"]].all()
    for e in reg.facts["edges"]:
        assert e % T == 0 and e < s.size
        assert int((~keep[e - T:e]).sum()) >= T // 4                     # the earlier tile's compaction moved slots
        pred = lambda i, j: bool(M.contained(s[i:i + 1], s[j:j + 1])[0])
        if kind == "drop":
            assert keep[e - 1] and not keep[e] and pred(e - 1, e)
        elif kind == "chain":
            # T - 1 dropped for T - 2; T contained in (contains) T - 1 but unrelated to T - 2: dropped by the input-neighbour rule only
            assert keep[e - 2] and not keep[e - 1] and not keep[e]
            assert pred(e - 2, e - 1) and pred(e - 1, e) and not pred(e - 2, e)
        else:
            # T inside T - 2 only: kept by the input-neighbour rule, dropped by compare-with-last-kept
            assert keep[e - 2] and not keep[e - 1] and keep[e]
            assert pred(e - 2, e - 1) and not pred(e - 1, e) and pred(e - 2, e)


def edge_classes(idx):
    idx = np.asarray(idx)
    return {"tile": bool(np.any(idx % R.TILE == 0)), "wave": bool(np.any((idx % R.WAVE == 0) & (idx % R.TILE != 0))),
            "thread": bool(np.any((idx % R.THREAD == 0) & (idx % R.WAVE != 0)))}


@pytest.mark.parametrize("n", R.LIB_SIZES)
def test_library_unique_edges_plain(n):
    seen_drop, seen_keep = [], []
    for v in (0, 1):
        reg = R.lib_edges(n, v)
        st = first_list_is_the_design(reg)
        s, keep = st["sorted"], st["keep"]
        assert s.size == n
        d, k = np.array(reg.facts["drops"]), np.array(reg.facts["keeps"])
        assert not keep[d].any() and keep[k].all()
        # the keeps are corner keeps: inside the record two places back, apart from the input neighbour
        assert M.contained(s[k - 2], s[k]).all() and not M.contained(s[k - 1], s[k]).any()
        seen_drop += [i for i in d if i % R.THREAD == 0]
        seen_keep += list(k)
    want = {"thread": True, "wave": True, "tile": n > R.TILE}
    assert edge_classes(seen_drop) == want and edge_classes(seen_keep) == want
    tiles = -(-n // R.TILE)
    assert (tiles <= 4) == (n <= 32768)      # the one-workgroup kernel up to 32768 records, the tiled kernels from 32769 on
    if n > R.TILE:                           # every pass / tile edge carries a verdict of each kind over the two variants
        for e in range(R.TILE, n, R.TILE):
            assert e in seen_drop and e in seen_keep


@pytest.mark.parametrize("n", R.LIB_SIZES)
def test_library_unique_edges_rm(n):
    d1, k1, d2, k2 = [], [], [], []
    for v in (0, 1):
        reg = R.lib_edges_rm(n, v)
        st = reg.stages(True)
        assert np.array_equal(st[0]["sorted"], reg.facts["sorted0_rm"]) and st[0]["sorted"].size == n
        f = reg.facts
        assert st[1]["sorted"].size == f["n1"] == int(st[0]["keep"].sum())
        assert not st[0]["keep"][f["drops1"]].any() and st[0]["keep"][f["keeps1"]].all()
        assert not st[1]["keep"][f["drops2"]].any() and st[1]["keep"][f["keeps2"]].all()
        # first pass: the drops are exact copies, the kept twins differ from their neighbour in the score alone
        s0, s1 = st[0]["sorted"], st[1]["sorted"]
        a = np.array(f["keeps1"])
        assert all(s0[i - 1][c] == s0[i][c] for i in a for c in ("ref_start", "query_start", "len")) and np.all(s0[a - 1]["score"] != s0[a]["score"])
        k = np.array(f["keeps2"])
        assert M.contained(s1[k - 2], s1[k]).all() and not M.contained(s1[k - 1], s1[k]).any()
        d1 += f["drops1"]; k1 += f["keeps1"]; k2 += f["keeps2"]
        d2 += [j for j in f["drops2"] if j % R.THREAD == 0]
        n1 = f["n1"]
    for got, size in ((d1, n), (k1, n), (d2, n1), (k2, n1)):      # both passes meet a drop and a keep at every class of edge they have
        assert edge_classes(got) == {"thread": True, "wave": True, "tile": size > R.TILE}, (n, got)


@pytest.mark.parametrize("nsegs", R.SEG_COUNTS)
def test_segment_mixes(nsegs):
    reg = R.seg_mix(nsegs)
    m = reg.model()
    assert np.array_equal(m["counts"], reg.facts["counts"]) and reg.recs.size <= R.TOTAL
    assert np.bincount(reg.seg, minlength=nsegs).max() <= R.SEG_CAP
    assert nsegs == 1 or np.any(np.diff(reg.seg.astype(np.int64)) < 0)                    # ids interleaved in the input
    if nsegs >= 8:
        assert reg.facts["empty"] == [0, nsegs // 2, nsegs - 1] and not m["counts"][reg.facts["empty"]].any()
    assert int(m["counts"].sum()) < reg.recs.size                                         # every used segment drops something
    used = reg.facts["used"]
    for a, b in zip(used, used[1:]):
        ra, rb = m["segments"][a]["final"], m["segments"][b]["final"]
        shared = np.intersect1d(ra, rb)
        assert shared.size >= 1                                                           # the same record, kept in both segments
        # a pair that would merge lies split between the neighbours: kept apart, dropped together
        both = M.chain(np.concatenate([reg.recs[reg.seg == a], reg.recs[reg.seg == b]]))["final"]
        assert both.size < ra.size + rb.size - shared.size


def test_segment_511_alone_and_the_full_call():
    reg = R.seg_last_only()
    assert reg.nsegs == 512 and set(reg.seg.tolist()) == {511} and np.array_equal(reg.model()["counts"], reg.facts["counts"])
    full = R.seg_full()
    assert full.recs.size == R.TOTAL and np.all(np.bincount(full.seg) == R.SEG_CAP) and full.nsegs == 64
    assert np.array_equal(full.model()["counts"], full.facts["counts"])


@pytest.mark.parametrize("kind", R.REFUSALS)
def test_refusal_inputs(kind):
    reg = R.refusal(kind)
    per = np.bincount(reg.seg, minlength=reg.nsegs)
    cap = reg.facts["seg_max"] or R.SEG_CAP
    over_seg, over_total = bool(per.max() > cap), reg.recs.size > R.TOTAL
    assert reg.facts["refused"] == (over_seg or over_total)
    if kind == "cap100-100":
        assert per.max() == 100 == cap
    if kind == "cap100-101":
        assert per.max() == 101 and cap == 100
    if kind == "default-2048":
        assert per.max() == 2048 == cap
    if kind == "default-2049":
        assert per.max() == 2049
    if kind == "one-oversized":
        assert int((per > cap).sum()) == 1 and reg.nsegs == 5 and per.min() >= 30
    if kind == "total-131073":
        assert reg.recs.size == R.TOTAL + 1 and not over_seg and reg.facts["on_device"] is True
    assert int(reg.model()["counts"].sum()) < reg.recs.size or kind == "total-131073"


@pytest.mark.parametrize("n", [9000, 40961])
def test_library_segment_breaks(n):
    reg = R.lib_seg_breaks(n)
    for rm in (False, True):
        for st in reg.stages(rm)[:-1]:
            assert np.array_equal(st["sorted"], reg.facts["sorted0"]) and np.array_equal(st["seg"], reg.facts["sorted_seg"])
            assert st["keep"].all()
            s = st["sorted"]
            for c in reg.facts["cuts"]:
                assert st["seg"][c] == st["seg"][c - 1] + 1                       # a break exactly here ...
                assert M.contained(s[c - 1:c], s[c:c + 1])[0]                     # ... and only the break keeps the record
    assert edge_classes(reg.facts["cuts"]) == {"thread": True, "wave": True, "tile": True}
    assert (40961 > 4 * R.TILE) and (9000 <= 4 * R.TILE)                          # tiled kernels and the one-workgroup kernel


def test_strip_stride_input():
    reg = R.lib_strip_stride()
    for rm in (False, True):
        m = reg.model(rm)
        assert m["records"].size == reg.facts["kept"] > 2048 * 256 and reg.nsegs == 3 and (m["counts"] == 200_000).all()


@pytest.mark.parametrize("kind", R.MAGNITUDES)
def test_magnitudes(kind):
    reg = R.magnitudes(kind)
    r = reg.recs
    assert reg.nsegs == 1 and r.size <= 4000
    e64 = r["ref_start"].astype(np.int64) + r["len"].astype(np.int64)
    if kind == "ends":
        assert np.any(e64 < (1 << 32)) and np.any(e64 == (1 << 32)) and np.any(e64 > (1 << 32))
    if kind == "diagonals":
        d = M.diag(r)
        assert set(d.tolist()) == {0, 0xFFFFFFFF} and np.any(r["query_start"] > r["ref_start"])
        s = reg.stages()[0]["sorted"]
        ds = M.diag(s)
        i = int(np.nonzero(ds == 0xFFFFFFFF)[0][0])
        assert ds[i - 1] == 0 and np.all(ds[:i] == 0) and np.all(ds[i:] == 0xFFFFFFFF)   # next to each other in the first sort
    if kind == "lens":
        assert np.any(r["len"] == 0) and np.any(r["len"] == 0xFFFFFFFF) and np.any(e64 >= (1 << 32))
    if kind == "scores":
        sc = set(r["score"].tolist())
        assert {-(1 << 31), -1, 0, (1 << 31) - 1} <= sc
        u = np.unique(r[["ref_start", "query_start", "len"]])
        assert u.size < r.size // 4                                                         # twins that differ in the score only
    for rm in (False, True):
        m = reg.model(rm)
        assert 0 < m["records"].size < r.size
