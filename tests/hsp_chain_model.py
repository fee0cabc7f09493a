"""The contract of sa_chain_hsps (include/segalign_amd.h) in numpy: one vectorised row per node in canonical rank order.
Python integers are unbounded, numpy's int64 is the contract's; the inputs' limits keep every value inside +-2^56."""
import numpy as np

SEG = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])
MEMBER = np.dtype([("hsp_index", "<u4"), ("group", "<u4"), ("f", "<i8")])


def make(rows):
    """[(ref_start, query_start, bases, score), ...] -> SEG records (len = bases - 1)."""
    h = np.zeros(len(rows), dtype=SEG)
    for k, (r, q, b, s) in enumerate(rows):
        h[k] = (r, q, b - 1, s)
    return h


def rank_order(hsps, groups=None):
    """Input indices in canonical rank order: (group, ref_start, query_start, len, input index)."""
    h = np.asarray(hsps, dtype=SEG)
    g = np.zeros(h.size, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    return np.lexsort((np.arange(h.size), h["len"], h["query_start"], h["ref_start"], g))


def chain(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0):
    """-> (f int64[n] and pred int32[n] in INPUT order (pred: input index or -1), members MEMBER[])."""
    h = np.asarray(hsps, dtype=SEG)
    n = h.size
    g_in = np.zeros(n, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    order = rank_order(h, g_in)
    rs = h["ref_start"][order].astype(np.int64)
    qs = h["query_start"][order].astype(np.int64)
    span = h["len"][order].astype(np.int64) + 1
    re, qe = rs + span, qs + span
    sc = h["score"][order].astype(np.int64)
    g = g_in[order]
    dg, f = rs - qs, np.zeros(n, dtype=np.int64)
    pred = np.full(n, -1, dtype=np.int64)  # ranks
    for i in range(n):
        ok = (g[:i] == g[i]) & (re[:i] <= rs[i]) & (qe[:i] <= qs[i])
        if max_gap:
            ok &= (rs[i] - re[:i] <= max_gap) & (qs[i] - qe[:i] <= max_gap)
        best = 0
        if ok.any():
            v = f[:i] - (diag_pen * np.abs(dg[i] - dg[:i]) + anti_pen * ((rs[i] + qs[i]) - (re[:i] + qe[:i])))
            v = np.where(ok, v, np.int64(-1) << 62)
            j = int(np.argmax(v))  # the first maximum: the lowest rank
            if v[j] > 0:
                best, pred[i] = int(v[j]), j
        f[i] = sc[i] + best
    members = []
    for grp in np.unique(g):  # ascending
        r = np.flatnonzero(g == grp)
        end = int(r[np.argmax(f[r])])  # first maximum: lowest rank
        if f[end] < min_score:
            continue
        walk = []
        while end >= 0:
            walk.append(end)
            end = int(pred[end])
        for k in reversed(walk):
            members.append((int(order[k]), int(grp), int(f[k])))
    f_in, pred_in = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    f_in[order] = f
    pred_in[order] = np.where(pred >= 0, order[np.maximum(pred, 0)], -1)
    return f_in, pred_in, np.array(members, dtype=MEMBER)


def precedes(hsps, groups, j, i, max_gap=0):
    """The predecessor relation j < i of the contract on input indices."""
    h = np.asarray(hsps, dtype=SEG)
    g = np.zeros(h.size, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    re, qe = int(h["ref_start"][j]) + int(h["len"][j]) + 1, int(h["query_start"][j]) + int(h["len"][j]) + 1
    rs, qs = int(h["ref_start"][i]), int(h["query_start"][i])
    ok = g[j] == g[i] and re <= rs and qe <= qs
    if max_gap:
        ok = ok and rs - re <= max_gap and qs - qe <= max_gap
    return bool(ok)


def penalty(hsps, j, i, diag_pen, anti_pen):
    h = np.asarray(hsps, dtype=SEG)
    rs, qs = int(h["ref_start"][i]), int(h["query_start"][i])
    rj, qj, sp = int(h["ref_start"][j]), int(h["query_start"][j]), int(h["len"][j]) + 1
    return diag_pen * abs((rs - qs) - (rj - qj)) + anti_pen * ((rs + qs) - (rj + sp + qj + sp))


def tile_of(hsps, groups, tile):
    """Tile index (rank // tile) of every HSP in input order."""
    order = rank_order(hsps, groups)
    t = np.zeros(order.size, dtype=np.int64)
    t[order] = np.arange(order.size) // tile
    return t
