"""CPU: the continuation-pieces model (tests/gapped_pieces_model.py; contract in include/segalign_amd.h) held against
the existing serial checkers, the path invariants of joined sides, a hand-made case for every way a chain ends, and the cover sets
of the greedy rule stated over pieces."""
import numpy as np
import pytest

import gapped_greedy_model as GR
import gapped_model as G
import gapped_pieces_model as PM
import gapped_trace_model as T
from gapped_model import SUB


@pytest.fixture(scope="module")
def data():
    return PM.inputs()


def test_one_piece_equals_the_existing_checkers(data):
    _, _, tc, codes, hsps = data
    for key in PM.KEYS[:2]:
        for kw in (PM.CHAIN, PM.DRY, PM.BAND):
            recs, paths, sides = PM.align(tc, codes[key], SUB, hsps[key], 1, **kw)
            assert np.array_equal(recs, G.extend(tc, codes[key], SUB, hsps[key], **kw))  # field for field
            want, wpaths = T.align(tc, codes[key], SUB, hsps[key], **kw)
            assert np.array_equal(recs, want)
            for (lo, ro, c), (wlo, wro, wc) in zip(paths, wpaths):
                assert np.array_equal(lo, wlo) and np.array_equal(ro, wro) and c == wc
            assert not np.any(recs["flags"] & PM.CONTINUED)
            assert all(len(s[1]) == 1 and s[2] == PM.STOP_ONE for pair in sides for s in pair)


def check_sides(tc, qc, hsps, recs, paths, sides, gap_open=400, gap_extend=30, **_):
    """Every joined side re-scores to its score and consumes exactly its extents; a junction is M | anything."""
    for k in range(recs.size):
        r, (lo, ro, counts), (L, R) = recs[k], paths[k], sides[k]
        ar, aq = GR.anchor(hsps[k])
        assert T.consumed(lo) == (ar - int(r["ref_start"]), aq - int(r["query_start"])) == (L[0][1], L[0][2])
        assert T.consumed(ro) == (int(r["ref_end"]) - ar, int(r["query_end"]) - aq) == (R[0][1], R[0][2])
        sl, ml, xl = T.rescore(tc, qc, SUB, int(r["ref_start"]), int(r["query_start"]), lo, gap_open, gap_extend)
        sr, mr, xr = T.rescore(tc, qc, SUB, ar, aq, ro, gap_open, gap_extend)
        assert (sl, sr) == (L[0][0], R[0][0]) and sl + sr == int(r["score"])
        assert (ml + mr, xl + xr) == (counts["matches"], counts["mismatches"])
        gaps = np.concatenate([lo, ro])
        gaps = gaps[(gaps & 3) != T.OP_M]
        assert (counts["gap_opens"], counts["gap_bases"]) == (gaps.size, int((gaps >> 2).sum()))
        for joined, chain, _ in (L, R):
            assert bool(joined[4] & PM.CONTINUED) == (len(chain) > 1)
            for p in chain[:-1]:  # a continued piece ends, at its best cell, with an M step: walk order starts with M
                assert p["ops"].size and int(p["ops"][0]) & 3 == T.OP_M and T.canonical(p["ops"])


@pytest.mark.parametrize("pieces", [2, 3, 64])
def test_joined_sides_rescore_and_consume_their_extents(data, pieces):
    _, _, tc, codes, hsps = data
    for key, kw in ((PM.KEYS[0], PM.CHAIN), (PM.KEYS[1], PM.DRY), (PM.KEYS[2], PM.BAND), (PM.KEYS[3], PM.CHAIN)):
        recs, paths, sides = PM.align(tc, codes[key], SUB, hsps[key], pieces, **kw)
        check_sides(tc, codes[key], hsps[key], recs, paths, sides, **kw)
        assert np.any(recs["flags"] & PM.CONTINUED)


def test_shared_inputs_reach_every_stop_reason(data):
    """The inputs the GPU tests use: every way a chain ends occurs, and chains of 8 pieces and more."""
    _, _, tc, codes, hsps = data
    seen, longest, ends = {}, 0, set()
    for kw in (PM.CHAIN, PM.DRY, PM.BAND):
        for key in PM.KEYS:
            recs, _, sides = PM.align(tc, codes[key], SUB, hsps[key], 64, **kw)
            s, n = PM.stop_reasons(sides)
            longest = max(longest, n)
            for a, b in s.items():
                seen[a] = seen.get(a, 0) + b
            for r, (L, R) in zip(recs, sides):
                ends |= {PM.end_kind(tc, codes[key], r, d) for d, S in ((-1, L), (1, R)) if S[2] == PM.STOP_END}
    assert {PM.STOP_P, PM.STOP_BAND, PM.STOP_STUCK, PM.STOP_END} <= set(seen), seen
    assert {"separator", "block end"} <= ends and longest >= 8


def hand_case():
    """A 900-base target and a query that equals it except where noted below."""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=900).astype(np.uint8)
    q = t.copy()
    t[500] = q[500] = 7                                   # a separator
    q[700:] = (t[700:] + rng.integers(1, 4, size=200)) % 4  # every base differs from 700 on: the homology ends
    return t, q


def test_hand_made_chain_ends():
    t, q = hand_case()
    kw = dict(max_extent=50, gap_open=400, gap_extend=30, ydrop=2000)
    # (1) P reached: the chain from 100 rightwards is cut at 3 pieces of 50 bases, still extent-capped
    j, chain, stop = PM.side_chain(t, q, SUB, 100, 100, +1, 3, **kw)
    assert stop == PM.STOP_P and len(chain) == 3 and j[1:3] == (150, 150) and j[4] == PM.EXTENT_CAP | PM.CONTINUED
    assert j[0] == sum(int(SUB[int(x) * 8 + int(x)]) for x in t[100:250])
    # (2) a separator: with pieces to spare it runs to the separator at 500 and is no longer extent-capped
    j, chain, stop = PM.side_chain(t, q, SUB, 100, 100, +1, 64, **kw)
    assert stop == PM.STOP_END and j[1:3] == (400, 400) and len(chain) == 9 and j[4] == PM.CONTINUED
    assert chain[-1]["res"][1:3] == (0, 0) and chain[-1]["origin"] == (500, 500)  # the last piece starts at the separator: nothing
    # (3) the block's end: leftwards from 100 to position 0
    j, chain, stop = PM.side_chain(t, q, SUB, 100, 100, -1, 64, **kw)
    assert stop == PM.STOP_END and j[1:3] == (100, 100) and len(chain) == 3 and j[4] == PM.CONTINUED
    # (4) no progress: from 600 rightwards the homology ends at 700; the piece that starts there reaches 50 bases within a y-drop
    #     of 9000 (50 mismatches cost at most 6250) without ever scoring above 0
    kw4 = dict(kw, ydrop=9000)
    j, chain, stop = PM.side_chain(t, q, SUB, 600, 600, +1, 64, **kw4)
    assert stop == PM.STOP_STUCK and j[1:3] == (100, 100) and len(chain) == 3
    assert chain[-1]["res"][1:3] == (0, 0) and chain[-1]["res"][4] == PM.EXTENT_CAP and j[4] == PM.EXTENT_CAP | PM.CONTINUED
    # (5) the band cap in a later piece: free gaps and a wide y-drop let the live band of the piece in the unrelated part outgrow 20
    kw5 = dict(max_extent=50, gap_open=0, gap_extend=1, ydrop=400, max_band=20)
    j, chain, stop = PM.side_chain(t, q, SUB, 660, 660, +1, 64, **kw5)
    assert stop == PM.STOP_BAND and len(chain) >= 2 and j[4] & PM.BAND_CAP and j[4] & PM.CONTINUED, (stop, len(chain), j)
    # the score limit cannot be reached with 32-bit extents and this matrix; the rule is one comparison in side_chain
    assert PM.SCORE_LIMIT == 1 << 29


def test_cover_sets_over_pieces_equal_the_walk_from_the_record_start(data):
    _, _, tc, codes, hsps = data
    key = PM.KEYS[1]
    h = hsps[key][:6]
    recs, paths, sides = PM.align(tc, codes[key], SUB, h, 64, **PM.CHAIN)
    assert max(len(s[1]) for pair in sides for s in pair) >= 3
    for k in range(h.size):
        a = GR.anchor(h[k])
        lo, ro, _ = paths[k]
        assert PM.cover_set_pieces(sides[k], a) == GR.cover_set(recs[k], np.concatenate([lo, ro]), a)


def test_greedy_covers_an_anchor_on_a_later_piece(data):
    """Two anchors on one homology, several max_extent apart: with pieces the first alignment reaches and covers the second anchor;
    with one piece it ends before it and both are returned."""
    _, _, tc, codes, hsps = data
    h, qc = later_piece_pair(tc, codes, hsps)
    for pieces, returned, covered in ((1, 2, 0), (64, 1, 1)):
        sel, _, st = PM.greedy(tc, qc, SUB, h, 3000, pieces, **PM.CHAIN)
        assert (st["returned"], st["covered"]) == (returned, covered), pieces
    recs, _, sides = PM.align(tc, qc, SUB, h[:1], 64, **PM.CHAIN)
    b = GR.anchor(h[1])
    on = [k for k, p in enumerate(sides[0][1][1]) if b in PM.cover_set_pieces(((None, [], None), (None, [p], None)), (-1, -1))]
    assert on and min(on) >= 1  # the second anchor lies on a later piece of the right side only


def later_piece_pair(tc, codes, hsps):
    """-> (two HSPs, query codes): the first of the strand's anchors with the higher score, and one 5 to 20 kbp to its right."""
    key = PM.KEYS[0]
    h = hsps[key]
    for x in range(h.size):
        for y in range(h.size):
            d = int(h[y]["ref_start"]) - int(h[x]["ref_start"])
            if 5000 <= d <= 20000 and not np.any(tc[int(h[x]["ref_start"]):int(h[y]["ref_start"])] == 7):
                pair = h[[x, y]].copy()
                pair["score"] = (9000, 4000)
                return pair, codes[key]
    raise AssertionError("no such pair of anchors")
