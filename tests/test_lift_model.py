"""CPU: the model of sa_lift_intervals (tests/lift_model.py; contract in include/segalign_amd.h) against the header's
consequences (a) - (e) on random nets, and against hand-worked cases."""
import numpy as np
import pytest

import lift_cases as LC
import lift_model as L
import net_model as N
import net_subset_model as NS
from gapped_model import SUB
from test_net_subset_model import random_input as subset_input

SEEDS = range(6)
_cache = {}


def case(seed):
    if seed not in _cache:
        _cache[seed] = LC.random_case(seed)
    return _cache[seed]


def answer(seed, ratio, multiple, blocks):
    key = (seed, ratio, multiple, blocks)
    if key not in _cache:
        _cache[key] = LC.run(case(seed), ratio=ratio, multiple=multiple, blocks=blocks)
    return _cache[key]


def test_the_sets_reach_every_status_under_every_flag_combination_ten_times():
    for multiple, blocks in LC.FLAGS:
        tally = np.zeros(4, dtype=np.int64)
        hits = out = 0
        for seed in SEEDS:
            for ratio in ((95, 100), (51, 100)):
                rec, h, b, st = answer(seed, ratio, multiple, blocks)
                tally += st["n_status"]
                hits += st["hits"]
                out += st["out_blocks"]
                assert st["intervals"] == rec.size == 300 and sum(st["n_status"]) == 300 and (b is None) == (not blocks)
        print(multiple, blocks, tally.tolist(), hits, out)
        assert (tally >= 10).all() and hits >= 10 and (out >= 10) == blocks, (multiple, blocks, tally)
    c = case(0)
    assert set(c["kw"]["ostrand"].tolist()) == {0, 1} and set(c["kw"]["group"].tolist()) == {0, 1}
    assert max(int(case(s)["kw"]["ogroup"].max()) for s in SEEDS) > 1 << 31  # sparse ogroups


def test_a_mapped_is_the_number_of_the_intervals_bases_in_a_block_of_the_chain():
    for seed in SEEDS:
        c = case(seed)
        first, bs, be = (x.astype(np.int64) for x in c["args"][:3])
        rec, hits, _, st = answer(seed, (0, 1), True, False)  # num = 0: every touching chain has a hit
        assert st["hits"] == st["touches"] == int(rec["n_touch"].sum()) and st["touches"] > 100
        got = {(int(h["interval"]), int(h["chain"])): int(h["mapped"]) for h in hits}
        want = {}
        for iv in range(rec.size):
            bases = set(range(int(c["iv_start"][iv]), int(c["iv_end"][iv])))
            for ch in range(first.size - 1):
                if int(c["kw"]["group"][ch]) != int(c["iv_group"][iv]):
                    continue
                n = len(bases & {x for k in range(first[ch], first[ch + 1]) for x in range(bs[k], be[k])})
                if n:
                    want[iv, ch] = n
        assert got == want


def test_b_the_counts_nest_and_the_hull_holds_every_clipped_other_block():
    for seed in SEEDS:
        rec, hits, blocks, st = answer(seed, (51, 100), True, True)
        assert (rec["n_qualify"] <= rec["n_touch"]).all() and st["out_blocks"] == int(hits["n_blocks"].sum())
        for h in hits:
            b = blocks[int(h["out_block"]):int(h["out_block"]) + int(h["n_blocks"])]
            assert int(b["ostart"].min()) == int(h["ostart"]) and int(b["oend"].max()) == int(h["oend"])
            assert int((b["end"] - b["start"]).sum()) == int(h["mapped"]) and ((b["oend"] - b["ostart"]) == (b["end"] - b["start"])).all()
            c = case(seed)
            assert int(b["start"].min()) >= int(c["iv_start"][h["interval"]]) and int(b["end"].max()) <= int(c["iv_end"][h["interval"]])


@pytest.mark.parametrize("ratio", [(51, 100), (95, 100), (1, 1)])
def test_c_disjoint_hulls_and_a_majority_ratio_give_no_duplicated_interval(ratio):
    seen = [0, 0, 0, 0]
    for seed in SEEDS:
        t, q, h, mem, first, chains, pen = subset_input(seed, None)
        for ms, mf in ((1, 1), (5, 3)):
            bs, be = NS.blocks(h, mem, "target")
            fills, _ = N.net(first, bs, be, chains["score"], chains["group"], min_space=ms, min_fill=mf)
            hs, ch, _ = NS.subset(t, q, SUB, h, mem, first, fills, axis="target", split=True, **pen)
            assert NS.hulls_disjoint(ch, "target") and ch.size >= 2
            smem, sfirst = NS.csr(ch)
            sb = NS.blocks(hs, smem, "target") + NS.blocks(hs, smem, "query")
            rng = np.random.default_rng(seed)
            s = rng.integers(380, 1900, 400)
            e = s + rng.choice([1, 1, 7, 30, 120], 400)
            g = rng.choice(np.array([5, 2], dtype=np.uint32), 400)
            rec, _, _, st = L.lift(sfirst, *sb, s, e, group=ch["group"], iv_group=g, min_match=ratio)
            assert st["n_status"][L.DUPLICATED] == 0 and (rec["n_qualify"] <= 1).all()
            seen = [a + b for a, b in zip(seen, st["n_status"])]
    assert seen[L.MAPPED] >= 100 and seen[L.UNMAPPED] >= 10 and seen[L.DUPLICATED] == 0, seen


def test_d_an_interval_inside_one_block_comes_back_through_the_same_chain():
    n = 0
    for seed in SEEDS:
        c = case(seed)
        first, bs, be, obs, obe = c["args"]
        rec = answer(seed, (1, 1), False, False)[0]
        for iv in np.flatnonzero((rec["status"] == L.MAPPED) & (rec["n_touch"] == 1) & (rec["n_blocks"] == 1) & (rec["strand"] == 0)):
            r = rec[iv]
            s, e, k = int(c["iv_start"][iv]), int(c["iv_end"][iv]), int(r["first_block"])
            assert int(bs[k]) <= s and e <= int(be[k]) and int(r["oend"]) - int(r["ostart"]) == e - s == int(r["mapped"])
            ch = int(r["chain"])
            lo, hi = int(first[ch]), int(first[ch + 1])
            back = L.lift([0, hi - lo], obs[lo:hi], obe[lo:hi], bs[lo:hi], be[lo:hi], [r["ostart"]], [r["oend"]], min_match=(1, 1))[0][0]
            assert int(back["status"]) == L.MAPPED and (int(back["ostart"]), int(back["oend"])) == (s, e)
            n += 1
    assert n >= 50


def test_e_the_records_do_not_depend_on_the_flags():
    for seed in SEEDS:
        for ratio in ((95, 100), (51, 100)):
            base = answer(seed, ratio, False, False)
            both = answer(seed, ratio, True, True)
            for multiple, blocks in LC.FLAGS[1:]:
                got = answer(seed, ratio, multiple, blocks)[0].copy()
                if multiple:  # first_hit is the running count of the hits, which the flag changes
                    assert np.array_equal(got["first_hit"], np.cumsum(np.concatenate([[0], got["n_qualify"][:-1]])))
                    got["first_hit"] = base[0]["first_hit"]
                L.same((got, base[1], None), (base[0], base[1], None))
            mapped = np.flatnonzero(base[0]["status"] == L.MAPPED)
            pick = both[1][np.isin(both[1]["interval"], mapped)]
            assert pick.size == base[1].size == mapped.size
            for k in ("interval", "chain", "ostart", "oend", "mapped", "first_block", "n_blocks"):
                assert np.array_equal(pick[k], base[1][k])
            assert np.array_equal(base[0]["first_hit"], np.cumsum(np.concatenate([[0], (base[0]["status"] == L.MAPPED)[:-1]])))


# ---- hand-worked ----
A = [(100, 1000, 20), (200, 1100, 20)]  # [100, 120) and [200, 220), on the other axis [1000, 1020) and [1100, 1120)


def one(chains, iv, **kw):
    rec, hits, blocks, st = chains.lift([iv], **kw)
    return rec[0], hits, blocks, st


def test_abutting_intervals_touch_nothing_and_one_base_on_each_side_does():
    c = LC.Chains([A])
    r, hits, _, st = one(c, (120, 200))  # s = a block's end and e = a block's start
    assert int(r["status"]) == L.UNMAPPED and int(r["chain"]) == L.NONE and hits.size == 0 and st["candidates"] == 1
    assert r.tolist()[5:11] == (0, 0, 0, 0, 0, 0)
    r, hits, blocks, st = one(c, (119, 201), min_match=(0, 1), blocks=True)
    assert r.tolist()[:11] == (L.MAPPED, 1, 1, 0, 0, 0, 1019, 1101, 2, 0, 2)
    assert blocks.tolist() == [(119, 120, 1019, 1020), (200, 201, 1100, 1101)] and hits.tolist() == [(0, 0, 1019, 1101, 2, 0, 2, 0)]
    assert int(one(c, (119, 200))[0]["n_blocks"]) == 1 and int(one(c, (120, 201))[0]["first_block"]) == 1


def test_an_interval_in_a_gap_of_a_chain_whose_hull_covers_it():
    r, _, _, st = one(LC.Chains([A]), (130, 150))
    assert int(r["status"]) == L.UNMAPPED and int(r["n_touch"]) == 0 and st["candidates"] == 1 and st["touches"] == 0


def test_the_threshold_at_its_value_and_one_base_fewer():
    c = LC.Chains([A])
    assert int(one(c, (100, 140), min_match=(1, 2))[0]["status"]) == L.MAPPED  # 20 * 2 = 1 * 40
    r = one(c, (100, 141), min_match=(1, 2))[0]  # 40 < 41
    assert (int(r["status"]), int(r["n_touch"]), int(r["n_qualify"]), int(r["mapped"]), int(r["chain"])) == (L.PARTIAL, 1, 0, 20, 0)
    assert (int(r["ostart"]), int(r["oend"])) == (1000, 1020)


def test_num_0_and_num_equal_to_den():
    c = LC.Chains([A])
    assert int(one(c, (119, 150), min_match=(0, 7))[0]["status"]) == L.MAPPED
    assert int(one(c, (130, 150), min_match=(0, 7))[0]["status"]) == L.UNMAPPED  # qualifying needs a touch
    assert int(one(c, (100, 120), min_match=(7, 7))[0]["status"]) == L.MAPPED
    assert int(one(c, (100, 121), min_match=(7, 7))[0]["status"]) == L.PARTIAL


@pytest.mark.parametrize("iv,other", [((1100, 1300), (7000, 7200)), ((1000, 1200), (7100, 7300)), ((1100, 1200), (7100, 7200))])
def test_a_strand_1_block_cut_left_right_and_both(iv, other):
    c = LC.Chains([[(1000, 7000, 300)]], ostrand=[1])
    r, _, blocks, _ = one(c, iv, blocks=True)
    assert (int(r["ostart"]), int(r["oend"])) == other and int(r["strand"]) == 1 and blocks.tolist() == [iv + other]
    # two blocks, descending on the other axis: the hull is the last block's start and the first block's end
    c = LC.Chains([[(1000, 7000, 300), (1400, 6500, 100)]], ostrand=[1])
    r = one(c, (1290, 1410), min_match=(0, 1))[0]
    assert (int(r["ostart"]), int(r["oend"]), int(r["mapped"]), int(r["n_blocks"])) == (6590, 7010, 20, 2)


def test_equal_mapped_in_two_chains_and_equal_hull_starts():
    c = LC.Chains([[(100, 1000, 20)], [(90, 2000, 30)]], ogroup=[5, 6])
    r, hits, _, _ = one(c, (100, 120), multiple=True)
    assert (int(r["status"]), int(r["chain"]), int(r["ogroup"]), int(r["ostart"])) == (L.DUPLICATED, 1, 6, 2010)  # chain 1 starts first
    assert hits["chain"].tolist() == [1, 0] and one(c, (100, 120))[1].size == 0
    c = LC.Chains([[(100, 1000, 20)], [(100, 2000, 30)]])
    assert int(one(c, (100, 110))[0]["chain"]) == 0 and int(one(c, (100, 130), min_match=(0, 1))[0]["chain"]) == 1
    assert one(c, (100, 110), multiple=True)[1]["chain"].tolist() == [0, 1]


def test_groups_and_empty_chains():
    c = LC.Chains([[(100, 1000, 20)], [], [(100, 2000, 20)]], group=[4_000_000_000, 4_000_000_000, 3])
    rec, hits, _, st = c.lift([(100, 120)] * 3, iv_group=[3, 4_000_000_000, 5], multiple=True)
    assert rec["chain"].tolist() == [2, 0, L.NONE] and rec["first_hit"].tolist() == [0, 1, 2]
    assert st["candidates"] == 2  # the empty chain sorts first in its group and is passed over: its hull ends at 0


EDITS = [("first[0] = 1", "first"), ("first[0] = 0; first[1] = -1", "first"), ("bs[0] = 120", "block"), ("be[1] = 1 << 31", "block"), ("bs[1] = 119", "block order"),
         ("obs[0] = 1020", "other block"), ("obe[1] = 1 << 31; obs[1] = (1 << 31) - 20", "other block"), ("obe[0] = 1021", "other block length"),
         ("obs[1] = 1019; obe[1] = 1039", "other block order"), ("kw['ostrand'] = [1]", "other block order"), ("kw['ostrand'] = [2]", "ostrand"),
         ("kw['group'] = [1, 2]", "per chain"), ("obe = obe[:1]", "block arrays"), ("ivs[0] = 150", "interval"), ("ive[0] = 1 << 31", "interval end"),
         ("kw['iv_group'] = [0, 0]", "per interval"), ("kw['min_match'] = (3, 2)", "num"), ("kw['min_match'] = (0, 0)", "den"),
         ("kw['min_match'] = (1, (1 << 20) + 1)", "den"), ("kw['flags'] = 4", "flags")]


@pytest.mark.parametrize("edit,clause", EDITS)
def test_every_validation_clause(edit, clause):
    c = LC.Chains([A])
    env = dict(first=c.first.astype(np.int64), bs=c.bs.astype(np.int64), be=c.be.astype(np.int64), obs=c.obs.astype(np.int64),
               obe=c.obe.astype(np.int64), ivs=[100], ive=[150], kw={})
    L.validate(env["first"], env["bs"], env["be"], env["obs"], env["obe"], env["ivs"], env["ive"])
    exec(edit, {}, env)
    with pytest.raises(ValueError, match="^%s$" % clause):
        L.validate(env["first"], env["bs"], env["be"], env["obs"], env["obe"], env["ivs"], env["ive"], **env["kw"])


def test_the_limits():
    with pytest.raises(ValueError, match="^chains$"):
        L.validate(np.zeros((1 << 22) + 2, dtype=np.int64), [], [], [], [], [], [])
    with pytest.raises(ValueError, match="^intervals$"):
        L.validate([0], [], [], [], [], np.zeros((1 << 26) + 1, dtype=np.uint8), [])
    with pytest.raises(ValueError, match="^first$"):
        L.validate([0, (1 << 26) + 1], [], [], [], [], [], [])


def test_the_rendering_of_the_two_files():
    text = "chrA\t119\t201\tpeak1\t0\t+\n#a comment\n\nchrA\t130\t150\nchrA\t100\t141\tx\nchrA\t100\t110\n"
    lines = L.parse_bed(text)
    assert [x[1:] for x in lines] == [("chrA", 119, 201, "\tpeak1\t0\t+"), ("chrA", 130, 150, ""), ("chrA", 100, 141, "\tx"), ("chrA", 100, 110, "")]
    c = LC.Chains([A, [(95, 5000, 20)]], ogroup=[1, 0])
    rec = c.lift([(x[2], x[3]) for x in lines], min_match=(1, 2))[0]
    assert rec["status"].tolist() == [L.PARTIAL, L.UNMAPPED, L.PARTIAL, L.DUPLICATED]
    rec2 = c.lift([(x[2], x[3]) for x in lines], min_match=(0, 1))[0]
    assert rec2["status"].tolist() == [L.MAPPED, L.UNMAPPED, L.DUPLICATED, L.DUPLICATED]
    rec3 = LC.Chains([A], ogroup=[1]).lift([(x[2], x[3]) for x in lines], min_match=(1, 50))[0]
    lifted, unlifted = L.render_bed(lines, rec3, ["q0", "q1"], [0, 900], "-")
    assert lifted == "q1\t119\t201\tpeak1\t0\t+\t-\nq1\t100\t120\tx\t-\nq1\t100\t110\t-\n"
    assert unlifted == "#Deleted\nchrA\t130\t150\n"
    _, unlifted = L.render_bed(lines, rec, ["q0", "q1"], [0, 900], "+")
    assert unlifted == ("#Partially deleted\nchrA\t119\t201\tpeak1\t0\t+\n#Deleted\nchrA\t130\t150\n#Partially deleted\nchrA\t100\t141\tx\n"
                        "#Duplicated\nchrA\t100\t110\n")
