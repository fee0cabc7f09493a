"""CPU: the sequential rule of sa_gapped_align_greedy (tests/gapped_greedy_model.py) on hand-worked cases, over the path checker on
small built sequences and over abstract records and paths."""
import numpy as np

import gapped_greedy_model as GR
import gapped_model as G
import gapped_trace_model as T

SUB = G.SUB
SEP = 7
THRESH = 3000


def rand_codes(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def hsp_list(rows):
    return np.array(rows, dtype=G.SEG_DTYPE)


def M(n):
    return (n << 2) | T.OP_M


def I(n):
    return (n << 2) | T.OP_I


def D(n):
    return (n << 2) | T.OP_D


def abstract(rows):
    """Records, paths and HSPs from (anchor_t, anchor_q, hsp_score, ref_start, query_start, score, ops in genome order); the HSP has
    len 0, so its anchor is (ref_start, query_start) of the HSP; all ops go to the left side."""
    hsps = hsp_list([(at, aq, 0, hs) for at, aq, hs, *_ in rows])
    recs = np.zeros(len(rows), dtype=G.GAPPED_DTYPE)
    paths = []
    for k, (_, _, _, r0, q0, score, ops) in enumerate(rows):
        o = np.array(ops, dtype=np.uint32)
        nt, nq = T.consumed(o)
        recs[k] = (r0, r0 + nt, q0, q0 + nq, score, k, 0, 0)
        paths.append((o, np.zeros(0, dtype=np.uint32), {"matches": 0, "mismatches": 0, "gap_opens": 0, "gap_bases": 0}))
    return hsps, recs, paths


def returned(sel):
    return sorted(int(r["hsp_index"]) for r in sel)


def test_three_hsps_on_one_alignment_give_one_record():
    t = rand_codes(3000, 1)
    q = t.copy()
    hsps = hsp_list([(500, 500, 40, 2000), (1500, 1500, 40, 2500), (2400, 2400, 40, 1800)])
    sel, paths, st = GR.from_checker(t, q, SUB, hsps, THRESH)
    assert returned(sel) == [1]  # the highest HSP score extends first and spans the whole identity
    assert (st["returned"], st["covered"], st["below_thresh"]) == (1, 2, 0)
    lo, ro, _ = paths[0]
    assert T.consumed(np.concatenate([lo, ro])) == (3000, 3000)


def test_identical_duplicates_give_one_record():
    t = rand_codes(1200, 2)
    q = t.copy()
    q[300] = (q[300] + 1) % 4
    hsps = hsp_list([(600, 600, 30, 2000)] * 3)
    sel, _, st = GR.from_checker(t, q, SUB, hsps, THRESH)
    assert returned(sel) == [0]
    assert (st["covered"], st["below_thresh"]) == (2, 0)


def test_duplicates_whose_path_starts_with_a_gap_at_the_anchor():
    # abstract: the path passes beside its own anchor point; the anchor point alone still covers the duplicate
    rows = [(100, 100, 50, 50, 50, 5000, [M(50), I(3), M(50)])] * 2
    hsps, recs, paths = abstract(rows)
    assert (100, 100) not in GR.cover_set(recs[0], np.concatenate([paths[0][0], paths[0][1]]), (-1, -1))
    sel, _, st = GR.greedy(hsps, recs, paths, THRESH)
    assert returned(sel) == [0] and st["covered"] == 1


def test_two_alignments_split_by_a_separator_both_return():
    a, b = rand_codes(800, 3), rand_codes(800, 4)
    t = np.concatenate([a, [SEP], b]).astype(np.uint8)
    q = t.copy()
    hsps = hsp_list([(400, 400, 30, 2000), (1200, 1200, 30, 2100)])
    sel, _, st = GR.from_checker(t, q, SUB, hsps, THRESH)
    assert returned(sel) == [0, 1]
    assert st["covered"] == 0
    assert int(sel[0]["ref_end"]) <= 800 and int(sel[1]["ref_start"]) >= 801


def test_tandem_repeat_shifted_diagonal_is_returned():
    # a period-10 repeat aligned to itself: the main diagonal and the diagonal shifted by one period both align, and the shifted
    # HSP's anchor lies inside the main alignment's extent box but off its path
    unit = rand_codes(10, 5)
    t = np.tile(unit, 60)
    q = t.copy()
    hsps = hsp_list([(290, 290, 20, 3000), (300, 290, 20, 2000)])
    sel, paths, st = GR.from_checker(t, q, SUB, hsps, THRESH)
    main = sel[np.array([int(r["hsp_index"]) for r in sel]) == 0][0]
    assert int(main["ref_start"]) <= 310 < int(main["ref_end"]) and int(main["query_start"]) <= 300 < int(main["query_end"])
    assert returned(sel) == [0, 1]
    assert st["covered"] == 0


def test_box_is_not_cover_abstract():
    rows = [(150, 150, 90, 100, 100, 9000, [M(100)]),  # diagonal 0 over t 100 .. 199
            (160, 150, 80, 140, 130, 6000, [M(50)])]   # anchor inside the box, on diagonal +10
    hsps, recs, paths = abstract(rows)
    sel, _, st = GR.greedy(hsps, recs, paths, THRESH)
    assert returned(sel) == [0, 1] and st["covered"] == 0


def test_chain_a_covers_b_covers_c_returns_a_and_c():
    rows = [(50, 50, 90, 0, 0, 9000, [M(100)]),                           # a: diagonal 0, t 0 .. 99
            (80, 80, 80, 50, 50, 8000, [M(60), D(5), M(40)]),             # b: anchor on a; its path leaves to diagonal 5 at t 115
            (130, 125, 70, 120, 115, 7000, [M(30)])]                      # c: anchor on b's second run, not on a
    hsps, recs, paths = abstract(rows)
    b_pts = GR.cover_set(recs[1], paths[1][0], (80, 80))
    a_pts = GR.cover_set(recs[0], paths[0][0], (50, 50))
    assert (130, 125) in b_pts and (130, 125) not in a_pts and (80, 80) in a_pts
    sel, _, st = GR.greedy(hsps, recs, paths, THRESH)
    assert returned(sel) == [0, 2]  # dropping whatever ANY higher-priority alignment covers would lose c
    assert (st["covered"], st["below_thresh"]) == (1, 0)
    assert list(st["state"]) == [1, 2, 1]


def test_below_threshold_alignment_covers_nothing():
    rows = [(50, 50, 99, 0, 0, THRESH - 1, [M(100)]),  # first in priority, but its alignment scores below the threshold
            (60, 60, 10, 40, 40, 5000, [M(30)])]
    hsps, recs, paths = abstract(rows)
    sel, _, st = GR.greedy(hsps, recs, paths, THRESH)
    assert returned(sel) == [1]
    assert (st["covered"], st["below_thresh"]) == (0, 1)


def test_covered_counts_even_below_threshold():
    rows = [(50, 50, 99, 0, 0, 9000, [M(100)]),
            (60, 60, 10, 55, 55, 100, [M(10)])]  # below the threshold, but its anchor lies on the first path: covered
    hsps, recs, paths = abstract(rows)
    sel, _, st = GR.greedy(hsps, recs, paths, THRESH)
    assert returned(sel) == [0]
    assert (st["covered"], st["below_thresh"]) == (1, 0)


def test_priority_ties_break_by_index_and_output_in_rule_3_order():
    rows = [(500, 500, 50, 450, 450, 6000, [M(100)]),
            (50, 50, 50, 0, 0, 6000, [M(100)]),
            (55, 55, 50, 0, 0, 6000, [M(100)])]  # same HSP score as 1, later index: covered by 1
    hsps, recs, paths = abstract(rows)
    sel, sel_paths, st = GR.greedy(hsps, recs, paths, THRESH)
    assert [int(r["hsp_index"]) for r in sel] == [1, 0]  # query_start order
    assert st["covered"] == 1
    pa, ops = T.pack(sel_paths)
    assert pa.size == 2 and ops.size == 2


def test_every_hsp_is_exactly_one_thing_on_a_built_pair():
    from segalign_amd import synth
    t, q = synth.make_pair(6000, 11, 12, sub_rate=0.08, mask_frac=0.0, records=1, indel_every=300)
    t, q = np.asarray(t, dtype=np.uint8), np.asarray(q, dtype=np.uint8)
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(40):
        s = int(rng.integers(0, min(t.size, q.size) - 40))
        rows.append((s, s, 19, int(rng.integers(1000, 3000))))
    hsps = hsp_list(rows)
    sel, _, st = GR.from_checker(t, q, SUB, hsps, THRESH)
    assert st["returned"] + st["covered"] + st["below_thresh"] == hsps.size
    assert sel.size == st["returned"]
