"""The contract of sa_chain_hsps_ovl / sa_chain_hsps_all_ovl (include/segalign_amd.h) in Python integers: the overlap of
a pair, the predecessor relation under an allowance, the gaps once the overlap is cut off the successor's head, and the overlap
charge.  chain() is the recurrence of hsp_chain_model over them, one node at a time; rank, ties and members are that model's, the gap
cost hsp_chain_gap_model's, the peel hsp_chain_all_model's.  Written from the header, not from the kernels."""
import numpy as np

import hsp_chain_all_model as MA
import hsp_chain_gap_model as G
import hsp_chain_model as M

MAX_OVERLAP = 4096


def validate(max_overlap, reserved=0):
    if not 0 <= max_overlap <= MAX_OVERLAP:
        raise ValueError("max_overlap")
    if reserved != 0:
        raise ValueError("reserved")
    return max_overlap


def node(h, k):
    """(rs, qs, bases, score) of HSP k as Python integers."""
    return int(h["ref_start"][k]), int(h["query_start"][k]), int(h["len"][k]) + 1, int(h["score"][k])


def overlap(h, j, i):
    """o(j, i) = max(0, re_j - rs_i, qe_j - qs_i)."""
    rj, qj, bj, _ = node(h, j)
    ri, qi, _, _ = node(h, i)
    return max(0, rj + bj - ri, qj + bj - qi)


def trimmed_gaps(h, j, i):
    """(gap_r, gap_q) once o bases are cut off i's head."""
    rj, qj, bj, _ = node(h, j)
    ri, qi, _, _ = node(h, i)
    o = overlap(h, j, i)
    return ri + o - (rj + bj), qi + o - (qj + bj)


def precedes(h, g, j, i, max_overlap, max_gap=0):
    """j < i of the contract on input indices; g: the groups or None."""
    if g is not None and int(g[j]) != int(g[i]):
        return False
    o = overlap(h, j, i)
    if o > max_overlap or 2 * o >= min(node(h, j)[2], node(h, i)[2]):
        return False
    gr, gq = trimmed_gaps(h, j, i)
    assert gr >= 0 and gq >= 0
    return not max_gap or (gr <= max_gap and gq <= max_gap)


def weight(h, k):
    """w = floor(65536 max(score, 0) / bases)."""
    _, _, b, s = node(h, k)
    return (65536 * max(s, 0)) // b


def charge(h, j, i):
    """c(j, i) = (o min(w_j, w_i)) >> 16."""
    return (overlap(h, j, i) * min(weight(h, j), weight(h, i))) >> 16


def link_penalty(h, j, i, diag_pen, anti_pen, t):
    """pen'(j, i) on the trimmed gaps: the diagonal term as it was, the antidiagonal term and the table (t None: none) on the gaps."""
    rj, qj, _, _ = node(h, j)
    ri, qi, _, _ = node(h, i)
    gr, gq = trimmed_gaps(h, j, i)
    p = diag_pen * abs((ri - qi) - (rj - qj)) + anti_pen * (gr + gq)
    return p + (G.gapcost(t, gr, gq) if t is not None else 0)


def value(h, j, i, fj, diag_pen, anti_pen, t):
    """What j offers i: f_j - pen' - c."""
    return fj - link_penalty(h, j, i, diag_pen, anti_pen, t) - charge(h, j, i)


def chain(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, gap_costs=None, max_overlap=0):
    """-> (f int64[n] and pred int32[n] in INPUT order (pred: input index or -1), members hsp_chain_model.MEMBER[])."""
    validate(max_overlap)
    t = G.validate(gap_costs) if gap_costs is not None else None
    h = np.asarray(hsps, dtype=M.SEG)
    n = h.size
    g = np.zeros(n, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    order = [int(x) for x in M.rank_order(h, g)]
    f, pred = [0] * n, [-1] * n  # by input index
    # the pair loop on plain lists of Python integers; the clauses are those of precedes(), trimmed_gaps(), link_penalty() and charge(),
    # which tests/test_hsp_chain_overlap_model.py holds this loop against through an exhaustive search
    RS, QS, B, W = zip(*[(node(h, k)[0], node(h, k)[1], node(h, k)[2], weight(h, k)) for k in range(n)]) if n else ((), (), (), ())
    GR = [int(x) for x in g]
    for a, i in enumerate(order):
        best, bj = 0, -1
        for j in order[:a]:  # ascending rank: strictly larger keeps the lowest rank
            if GR[j] != GR[i]:
                continue
            o = max(0, RS[j] + B[j] - RS[i], QS[j] + B[j] - QS[i])
            if o > max_overlap or 2 * o >= min(B[j], B[i]):
                continue
            gr, gq = RS[i] + o - RS[j] - B[j], QS[i] + o - QS[j] - B[j]
            if max_gap and (gr > max_gap or gq > max_gap):
                continue
            pen = diag_pen * abs((RS[i] - QS[i]) - (RS[j] - QS[j])) + anti_pen * (gr + gq) + (G.gapcost(t, gr, gq) if t is not None else 0)
            v = f[j] - pen - ((o * min(W[j], W[i])) >> 16)
            if v > best:
                best, bj = v, j
        f[i], pred[i] = int(h["score"][i]) + best, bj
    rank = {k: a for a, k in enumerate(order)}
    members = []
    for grp in np.unique(g):
        r = [k for k in order if g[k] == grp]
        end = max(r, key=lambda k: (f[k], -rank[k]))  # largest f, lowest rank among equals
        if f[end] < min_score:
            continue
        walk = []
        while end >= 0:
            walk.append(end)
            end = pred[end]
        members += [(k, int(grp), f[k]) for k in reversed(walk)]
    return np.array(f, dtype=np.int64), np.array(pred, dtype=np.int32), np.array(members, dtype=M.MEMBER)


def chain_rows(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, gap_costs=None, max_overlap=0):
    """chain() a row at a time in numpy int64, for inputs of tens of thousands of HSPs (tools/gapped_bench.py); the contract's bounds
    keep every value it uses inside int64.  Held against chain() by tests/test_hsp_chain_overlap_model.py."""
    validate(max_overlap)
    t = G.validate(gap_costs) if gap_costs is not None else None
    pre = G.arrays(t) if t is not None else None
    h = np.asarray(hsps, dtype=M.SEG)
    n = h.size
    g_in = np.zeros(n, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    order = M.rank_order(h, g_in)
    rs, qs = h["ref_start"][order].astype(np.int64), h["query_start"][order].astype(np.int64)
    ln = h["len"][order].astype(np.int64)
    re, qe, sc, gr = rs + ln + 1, qs + ln + 1, h["score"][order].astype(np.int64), g_in[order]
    w = (np.maximum(sc, 0) << 16) // (ln + 1)
    lim = np.minimum(ln >> 1, max_overlap)  # 2 o < bases is o <= len >> 1
    dg, f, pred = rs - qs, np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for i in range(n):
        hr, hq = rs[i] - re[:i], qs[i] - qe[:i]
        o = np.maximum(0, -np.minimum(hr, hq))
        ok = (gr[:i] == gr[i]) & (o <= np.minimum(lim[:i], lim[i]))
        if max_gap:
            ok &= (hr + o <= max_gap) & (hq + o <= max_gap)
        best = 0
        if ok.any():
            c = np.flatnonzero(ok)
            dt, dq = hr[c] + o[c], hq[c] + o[c]
            pen = diag_pen * np.abs(dg[i] - dg[c]) + anti_pen * (dt + dq)
            if t is not None:
                pen = pen + G.gapcost_rows(t, dt, dq, pre)
            v = f[c] - pen - ((o[c] * np.minimum(w[c], w[i])) >> 16)
            j = int(np.argmax(v))  # the first maximum: the lowest rank
            if v[j] > 0:
                best, pred[i] = int(v[j]), int(c[j])
        f[i] = sc[i] + best
    members = []
    for grp in np.unique(gr):  # ascending
        r = np.flatnonzero(gr == grp)
        end = int(r[np.argmax(f[r])])  # first maximum: lowest rank
        if f[end] < min_score:
            continue
        walk = []
        while end >= 0:
            walk.append(end)
            end = int(pred[end])
        members += [(int(order[k]), int(grp), int(f[k])) for k in reversed(walk)]
    f_in, pred_in = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    f_in[order] = f
    pred_in[order] = np.where(pred >= 0, order[np.maximum(pred, 0)], -1)
    return f_in, pred_in, np.array(members, dtype=M.MEMBER)


def chain_all(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, gap_costs=None, max_overlap=0):
    """hsp_chain_all_model.chain_all on this model's f and pred."""
    f, pred, _ = chain(hsps, groups, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap, gap_costs=gap_costs, max_overlap=max_overlap)
    return MA.chain_all(hsps, groups, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap, min_score=min_score, dp=(f, pred))
