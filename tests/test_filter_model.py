"""CPU: tests/filter_model.py and the worlds of tests/filter_regimes.py (DESIGN.md 4.5''').

  * every world is in the regimes it names: each CLAIM below is a predicate on the model's per-hit results and holds for at least one hit;
  * the vectorised walk of the model equals its stated per-base walk, on every hit of every world;
  * the packed {T : N} int16 step of the class filter on a table entry {sum, sum - mx} equals the per-base walk, for all 4096 + 256
    fields under both matrices;
  * the model is an UPPER bound: every hit whose exact extension passes is a model candidate, with and without context table;
  * no regime leaves int16, at either level."""
import numpy as np
import pytest

import extend_model as XM
import filter_model as F
import filter_regimes as R
import image_model as IM

WORLDS = ("H", "S", "codes", "field1", "repeat", "self", "synth", "stage", "H22")
LAYOUTS = (1, 0)


@pytest.fixture(scope="module")
def worlds(oracle):
    return R.worlds(tuple(int(x) for x in oracle.build_sub_mat(910)))


def detail(w, skip=1, rev=False, **kw):
    return w.verdicts(rev, detail=True, ctx_skip_seed=skip, **kw)


# ---- the claims ----------------------------------------------------------------------------------------------------------------------
def side(v, s):
    """(N after every base, field ends, alive, T after every base, start score) of a side"""
    o = v.l1
    if s == "R":
        return o["NR_all"], F.R_ENDS, o["r_alive"], o["TR_all"], 0
    return o["NL_all"], F.L_ENDS, o["l_alive"], o["TL_all"], None


def drop_at(v, s, e, depth, w):
    """the side's deepest field-end drop is `depth` and lies at field end e (base index)"""
    N, ends, alive, _, _ = side(v, s)
    fe = N[:, list(ends)]
    return (N[:, e] == -depth) & (fe.min(axis=1) == -depth) & (alive == (depth <= w.xdrop))


def dip_inside(v, s, k, w):
    """more than xdrop below the best at base k, which is no field end, and the side is alive all the same"""
    N, ends, alive, _, _ = side(v, s)
    assert k not in ends
    return (N[:, k] < -w.xdrop) & alive


def best_where(v, s, at_end, t0):
    """the side's best lies above its start score t0 and is first attained at a field's last base (the step's N' = N + sum) or inside
    a field (N' = sum - mx)"""
    N, ends, _, T, _ = side(v, s)
    return (T.max(axis=1) > t0) & (np.isin(np.argmax(T, axis=1), ends) == at_end)


def best_after_drop(v, s, w):
    N, ends, alive, T, _ = side(v, s)
    fe = N[:, list(ends)] < -w.xdrop
    first = np.where(fe.any(axis=1), np.asarray(ends)[np.argmax(fe, axis=1)], 10 ** 6)
    return ~alive & (np.argmax(T, axis=1) > first) & (T.max(axis=1) > T[:, 0])


def claims_walks(w, v, P):
    o, h, x = v.l1, w.hspthresh, w.xdrop
    c = {}
    for s, fields in (("R", (5, 9)), ("L", (9, 10))):            # (field 10 of the left side: the four-base tail)
        ends = F.R_ENDS if s == "R" else F.L_ENDS
        for f in fields:
            e = ends[f - 1]
            c["%s: deepest drop == xdrop at the end of field %d: alive" % (s, f)] = drop_at(v, s, e, x, w)
            c["%s: deepest drop == xdrop + 1 at the end of field %d: dropped" % (s, f)] = drop_at(v, s, e, x + 1, w)
            c["%s: deeper than xdrop one base before the end of field %d, alive" % (s, f)] = dip_inside(v, s, e - 1, w)
            if e + 1 < (F.R_BASES if s == "R" else F.L_BASES):
                c["%s: deeper than xdrop one base behind the end of field %d, alive" % (s, f)] = dip_inside(v, s, e + 1, w)
        t0 = 0 if s == "R" else F.seed_bound(v.cls, P.left_skip)
        c["%s: best in the middle of a field" % s] = best_where(v, s, False, t0)
        c["%s: best at a field end" % s] = best_where(v, s, True, t0)
        c["%s: best behind the drop" % s] = best_after_drop(v, s, w)
    both = ~o["r_alive"] & ~o["l_alive"]
    c["both dropped, bestR + bestL == hspthresh: forwarded as flags 3"] = both & (o["bestR"] + o["bestL"] == h) & o["fwd"] & (o["flags"] == 3)
    c["both dropped, bestR + bestL == hspthresh - 1: rejected"] = both & (o["bestR"] + o["bestL"] == h - 1) & ~o["fwd"]
    for fl in (1, 2, 3):
        c["alive sides: flags %d" % fl] = (o["r_alive"].astype(int) | (o["l_alive"].astype(int) << 1)) == fl
    for d in (0, 1, 5, 6, 7, 53, 54):
        c["right context: the target ends %d bases behind the anchor" % d] = len(w.tc) - o["ref_loc"] == d
        c["right context: the query ends %d bases behind the anchor" % d] = len(w.qc) - o["query_loc"] == d
    for d in (0, 1, 5, 6, 57, 58):
        if d:                                                    # (position 0 of the target is never indexed: no seed starts there)
            c["left context: %d target bases in front of the seed" % d] = o["ref_loc"] - w.S.span == d
        c["left context: %d query bases in front of the seed" % d] = o["query_loc"] - w.S.span == d
    for ph in range(16):
        c["query_loc & 15 == %d" % ph] = (o["query_loc"] & 15) == ph
        c["left window phase %d" % ph] = ((len(w.qc) - o["query_loc"] + P.left_skip) & 15) == ph
    return c


def claims_level2(w, v, P):
    l2, h = v.l2, w.hspthresh
    c = {}
    for fl in (1, 2, 3):
        c["level 2: flags %d" % fl] = l2["flags"] == fl
    resumed = l2["flags"] == 2
    for i in (1, 2, 3, 4):
        c["level 2: resumed left walk drops at test point %d of its first window" % i] = resumed & ~l2["forward"] & (l2["endL"] == F.L_BASES + P.left_skip + 16 * i)
        c["level 2: right walk from the anchor drops at test point %d of its first window" % i] = (l2["flags"] != 2) & (l2["endR"] == 16 * i)
        c["level 2: right walk from the anchor drops at test point %d of its second window" % i] = (l2["flags"] != 2) & (l2["endR"] == 64 + 16 * i)
    c["level 2: alive at long_cap from the anchor"] = l2["forward"] & (l2["endR"] == 128)
    c["level 2: alive at long_cap, resumed"] = l2["forward"] & resumed & (l2["endL"] == F.L_BASES + P.left_skip + 64)
    settled = (l2["flags"] == 3) & ~l2["forward"] & ~v.l1["r_alive"][v.forwards["hidx"]] & ~v.l1["l_alive"][v.forwards["hidx"]]
    c["level 2: class bound passes, exact total == hspthresh - 1: rejected"] = settled & (l2["bestR"] + l2["bestL"] == h - 1) & ~l2["cand"]
    c["level 2: class bound passes, exact total == hspthresh: candidate"] = settled & (l2["bestR"] + l2["bestL"] == h) & l2["cand"]
    return c


def populated(c):
    return sorted(k for k, m in c.items() if not np.any(m))


def claims_level2_resumes(v, P):
    """what the defaults do not reach: the long_cap rule at 64 from the anchor and resumed, and under l2_right_state the RIGHT walk resumed
    behind its 54 context bases dropping at each test point of its first window, or alive at the rule.  (A second window behind a resume
    does not exist: 54 + 64 + 10 and 58 + left_skip + 64 + 10 reach every long_cap the option allows, 128 at the most.)"""
    l2 = v.l2
    c = {}
    if P.long_cap == 64:
        c["level 2: alive at long_cap 64 from the anchor"] = l2["forward"] & (l2["endR"] == 64)
        c["level 2: alive at long_cap 64, left walk resumed"] = l2["forward"] & (l2["flags"] == 2) & (l2["endL"] == F.L_BASES + P.left_skip + 64)
    if P.l2_right_state:
        right = l2["flags"] == 1
        for i in (1, 2, 3, 4):
            c["level 2: resumed right walk drops at test point %d of its first window" % i] = right & ~l2["forward"] & (l2["endR"] == F.R_BASES + 16 * i)
        c["level 2: resumed right walk alive at the long_cap rule"] = right & l2["forward"] & (l2["endR"] == F.R_BASES + 64)
    return c


@pytest.mark.parametrize("skip", LAYOUTS)
@pytest.mark.parametrize("name", ["H", "S"])
def test_main_worlds_are_in_every_regime_they_name(worlds, name, skip):
    """on the plus strand, and on the minus strand of the world with its query reverse-complemented -- the call the GPU module makes for
    the other strand's images"""
    for w, rev in ((worlds[name], False), (worlds[name].flipped(), True)):
        v = detail(w, skip, rev)
        P = w.params(ctx_skip_seed=skip)
        missing = populated(claims_walks(w, v, P)) + populated(claims_level2(w, v, P))
        assert not missing, (rev, missing)
        for kw in ({"long_cap": 64}, {"l2_right_state": 1}, {"long_cap": 64, "l2_right_state": 1}):
            missing = populated(claims_level2_resumes(detail(w, skip, rev, **kw), w.params(ctx_skip_seed=skip, **kw)))
            assert not missing, (rev, kw, missing)


@pytest.mark.parametrize("name", ["H", "S", "H22"])
def test_left_resume_offset_decides_a_verdict(worlds, name):
    """the resumed left walk starts 58 + left_skip bases behind the anchor: started at 58 -- the seed window walked over context bases
    that level 1 has scored already -- some record of the world gets another verdict, in either direction"""
    import copy
    w = worlds[name]
    for rev, ww in ((False, w), (True, w.flipped())):
        v = ww.verdicts(rev)
        P = ww.params()
        Q = copy.copy(P)
        Q.left_skip = 0
        own, _ = ww.strand(rev)
        early = F.level2(ww.tc, own, ww.mat, v.forwards, Q)["cand"]
        two = v.l2["flags"] == 2
        lost, won = np.any(two & v.l2["cand"] & ~early), np.any(two & ~v.l2["cand"] & early)
        assert (lost and won) if name != "H22" else (lost or won), (name, rev)      # (22-base window: one direction is enough here)


def test_threshold_islands_under_a_22_base_seed_window(worlds):
    """14of22: the left walk starts at 22 x the largest class score; both sides dropped with bestR + bestL at hspthresh (forwarded as flags
    3) and one below (rejected), and level 2 decides a passing class bound by the exact total"""
    w = worlds["H22"]
    assert w.S.span == 22 and w.S.weight == 14
    v = detail(w)
    P = w.params()
    assert F.seed_bound(v.cls, P.left_skip) == 2200
    o = v.l1
    both = ~o["r_alive"] & ~o["l_alive"]
    for total, fwd in ((w.hspthresh, True), (w.hspthresh - 1, False)):
        m = both & (o["bestR"] + o["bestL"] == total)
        assert np.any(m) and np.all(o["fwd"][m] == fwd) and np.all(o["bestL"][m] >= 2200), total
    c = claims_level2(w, v, P)
    for k in ("level 2: class bound passes, exact total == hspthresh - 1: rejected", "level 2: class bound passes, exact total == hspthresh: candidate"):
        assert np.any(c[k]), k
    v0 = detail(w, 0)                       # (whole-window layout: the window is walked, 22 matches score the same 2200)
    assert np.any(~v0.l1["r_alive"] & ~v0.l1["l_alive"] & (v0.l1["bestR"] + v0.l1["bestL"] == w.hspthresh) & v0.l1["fwd"])


def test_sparse_table_equals_the_dense_one(worlds):
    """the table of the 14of22 world is built on the keys that occur; on 12of19 worlds the same code gives table_model.neighbourhood's"""
    for name in ("H", "repeat", "synth"):
        w = worlds[name]
        d, sp = w.table, F.Table(w.tc, w.S, 1, True, sparse=True)
        ks = np.arange(0, w.S.nkeys, 5)
        assert np.array_equal(sp.src, d.src) and np.array_equal(sp.pos, d.pos)
        for k in (np.flatnonzero(d.run > 0), np.flatnonzero(d.bucket > 0), ks):
            assert np.array_equal(sp.run[k], d.run[k]) and np.array_equal(sp.bucket[k], d.bucket[k])
        k = np.flatnonzero(d.run > 0)
        assert np.array_equal(sp.nbr_start[k], d.nbr_start[k])
        for rev in (False, True):
            a, b = F.call_hits(d, w.strand(rev)[0], 0, w.end), F.call_hits(sp, w.strand(rev)[0], 0, w.end)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_first_fields_drop_in_the_world_built_for_them(worlds):
    """xdrop 351: six bases can drop, so the first field of either side can end exactly xdrop, and xdrop + 1, below its start"""
    w = worlds["field1"]
    for skip in LAYOUTS:
        v = detail(w, skip)
        for s in ("RL" if skip else "R"):      # (whole-window layout: the first left field lies inside the seed window, whose care positions match)
            ends = F.R_ENDS if s == "R" else F.L_ENDS
            for depth in (w.xdrop, w.xdrop + 1):
                assert np.any(drop_at(v, s, ends[0], depth, w)), (skip, s, depth)
            assert np.any(dip_inside(v, s, ends[0] - 1, w)) and np.any(dip_inside(v, s, ends[0] + 1, w)), (skip, s)


def test_codes_world_raises_the_class_scores_and_puts_every_code_into_a_context(worlds, oracle):
    w = worlds["codes"]
    v = detail(w)
    plain = IM.class_scores(w.mat, 0x0F, 0x0F)
    assert IM.presence(w.tc) & 0x70 == 0x70 and IM.presence(w.qc) & 0x70 == 0x70
    assert all(a >= b for a, b in zip(v.cls, plain)) and tuple(v.cls) != tuple(plain), (v.cls, plain)
    o = v.l1
    for code in (R.L, R.N, R.X):
        for seq, loc in ((w.tc, o["ref_loc"]), (w.qc, o["query_loc"])):
            at = np.flatnonzero(seq == code)
            d = at[None, :] - loc[:, None]
            assert np.any((d >= 0) & (d < F.R_BASES)) and np.any((d < -w.S.span) & (d >= -w.S.span - F.L_BASES)), code


def test_stream_regimes(worlds):
    """calls of every size around the cuts; a record of more than 128 hits; 64 one-hit records in one buffer; records that start on
    lane 0 and on lane 63; buffers in which all 64 hits are forwarded"""
    w = worlds["synth"]
    for n in R.STREAM_SIZES:
        assert w.range_with(False, n) is not None, n
    rp = worlds["repeat"]
    ex = rp.hits_before(False)
    cnt = np.diff(ex)
    assert cnt.max() > 128
    starts = ex[:-1][cnt > 0]
    assert np.any(starts % 64 == 0) and np.any(starts % 64 == 63)
    one = np.zeros(int(ex[-1]), dtype=bool)
    one[starts[cnt[cnt > 0] == 1]] = True
    assert any(one[b:b + 64].all() for b in range(0, one.size - 63, 64))
    # the stage at its capacity of 95: one wave (one chunk), 31 records pending -- one below the flush mark -- when a buffer brings 64
    for skip in LAYOUTS:
        st = worlds["stage"].verdicts(False, ctx_skip_seed=skip)
        assert st.num_hits == 128 and R.stage_peaks(st.l1["fwd"], st.num_hits) == [(0, 31), (31, 64)]
    sv = worlds["self"].verdicts(False)
    f = sv.l1["fwd"]
    assert sv.forwards.size > 0.99 * sv.num_hits - 10 and sum(f[b:b + 64].all() for b in range(0, f.size - 63, 64)) >= 40


# ---- the model against itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_vectorised_walk_equals_the_per_base_walk(worlds, name):
    w = worlds[name]
    for skip in LAYOUTS:
        v = detail(w, skip)
        o, P = v.l1, w.params(ctx_skip_seed=skip)
        own, other = w.strand(False)
        pick = np.arange(v.num_hits) if v.num_hits <= 2000 else np.random.default_rng(1).choice(v.num_hits, 2000, replace=False)
        xr, xl = F.class_strings(w.tc, own, other, o["ref_loc"][pick], o["query_loc"][pick], P.left_skip)
        t0 = F.seed_bound(v.cls, P.left_skip)
        for j, i in enumerate(pick):
            T, N, W, best, _ = F.walk_one(xr[j], v.cls, 0, F.R_ENDS)
            assert (T, N, W, best) == (o["TR"][i], o["NR"][i], o["WR"][i], o["bestR"][i])
            T, N, W, best, _ = F.walk_one(xl[j], v.cls, t0, F.L_ENDS)
            assert (T, N, W, best) == (o["TL"][i], o["NL"][i], o["WL"][i], o["bestL"][i])


def i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


@pytest.mark.parametrize("hoxd", [True, False])
def test_field_step_on_a_table_entry_equals_the_per_base_walk(worlds, hoxd):
    """all 4096 six-base fields and all 256 four-base tails: T' = T + sum, N' = min(N + sum, sum - mx) in int16, from several states"""
    w = worlds["H" if hoxd else "S"]
    cls = IM.class_scores(w.mat, IM.presence(w.tc), IM.presence(w.qc))
    states = [(0, 0), (1900, 0), (700, -300), (-900, -900), (2500, -910), (-14000, -14000)]
    for nb, count in ((6, 4096), (4, 256)):
        for f in range(count):
            xs = [(f >> (2 * k)) & 3 for k in range(nb)]
            run = np.cumsum([cls[x] for x in xs])
            total, mx = int(run[-1]), max(0, int(run.max()))
            for T0, N0 in states:
                T, best = T0, T0 - N0
                for x in xs:
                    T += cls[x]
                    best = max(best, T)
                assert (i16(T0 + total), min(i16(N0 + total), i16(total - mx))) == (T, T - best), (nb, f, T0, N0)


@pytest.mark.parametrize("name", WORLDS)
def test_every_hit_that_passes_is_a_model_candidate(oracle, worlds, name):
    """the upper-bound property on the model itself: the exact extension of every hit of the call (the oracle's find_hsps, which extend_model
    restates: compared on a few hundred hits), against the candidates with context table (both layouts, both resume forms) and without"""
    w = worlds[name]
    for rev in (False, True):
        own, _ = w.strand(rev)
        ref_loc, query_loc = F.call_hits(w.table, own, 0, w.end)
        if not ref_loc.size:
            continue
        hits = np.stack([ref_loc, query_loc], axis=1)
        ok, _ = oracle.extend_hits_pass(w.tc, own, w.mat, hits.astype(np.uint32), xdrop=w.xdrop, hspthresh=w.hspthresh, noentropy=True)
        if name in ("H", "field1"):
            ex = XM.extend_all(w.tc, own, w.mat, hits[:400], w.xdrop, w.hspthresh)
            assert [e.passed for e in ex] == ok[:400].tolist()
        passing = set(map(tuple, hits[ok].tolist()))
        for kw in ({}, {"ctx_skip_seed": 0}, {"l2_right_state": 1}, {"long_cap": 64}, {"ctx": False}, {"ctx": False, "long_cap": 64}):
            cand = set(map(tuple, w.verdicts(rev, **kw).cand.tolist()))
            assert passing <= cand, (name, rev, kw, sorted(passing - cand)[:3])


def test_no_regime_leaves_int16(worlds):
    """level 1 asserts its T and N inside int16 on every call (the kernel's adds wrap); level 2's adds saturate, and the model counts the
    steps it had to clamp away from the query's end and from record separators (code 7 scores -9100 a base): none, in any world under
    any option set the GPU module runs, xdrop 16383 included"""
    before = F.SATURATED
    for name in WORLDS:
        w = worlds[name]
        for rev in (False, True):
            for kw in ({}, {"ctx_skip_seed": 0}, {"l2_right_state": 1}, {"ctx": False}, {"xdrop": 0}, {"xdrop": 16383}):
                w.verdicts(rev, **kw)
    assert F.SATURATED == before


def test_alive_shares_of_random_flanks_fall_with_the_context_length(worlds):
    """the record next to DESIGN.md 4.5a's table (profiles/r28_filter_verdicts/alive_shares.txt) comes from this function; here only
    that a longer flank leaves fewer walks alive"""
    w = worlds["H"]
    s = F.alive_shares(IM.class_scores(w.mat, 0x0F, 0x0F), 910, (48, 54, 58, 64), n=1 << 16)
    assert s[48] > s[54] > s[58] > s[64] > 0
