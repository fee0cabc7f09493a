"""The contract of sa_chain_hsps_costs / sa_chain_hsps_all_costs (include/segalign_amd.h): the piecewise-linear gap cost
of a link, in Python integers (slopes, g, gapcost), on top of hsp_chain_model's linear penalty; chain() evaluates it a row at a time in
int64.  Everything else (predecessor relation, rank, ties, members) is hsp_chain_model's, restated here only as far as the recurrence
needs it; the peel is hsp_chain_all_model's."""
import numpy as np

import hsp_chain_all_model as MA
import hsp_chain_model as M

POINTS = 16
POSITION = [1, 2, 3, 11, 111, 2111, 12111, 32111, 72111, 152111, 252111]
PRESETS = {
    "loose": {"pos": POSITION,
              "q_gap": [325, 360, 400, 450, 600, 1100, 3600, 7600, 15600, 31600, 56600],
              "t_gap": [325, 360, 400, 450, 600, 1100, 3600, 7600, 15600, 31600, 56600],
              "both_gap": [625, 660, 700, 750, 900, 1400, 4000, 8000, 16000, 32000, 57000]},
    "medium": {"pos": POSITION,
               "q_gap": [350, 425, 450, 600, 900, 2900, 22900, 57900, 117900, 217900, 317900],
               "t_gap": [350, 425, 450, 600, 900, 2900, 22900, 57900, 117900, 217900, 317900],
               "both_gap": [750, 825, 850, 1000, 1300, 3300, 23300, 58300, 118300, 218300, 318300]},
}


def table(t):
    """A preset's name or a dict {"pos", "q_gap", "t_gap", "both_gap"} -> the dict, its lists copied."""
    t = PRESETS[t] if isinstance(t, str) else t
    return {k: [int(x) for x in t[k]] for k in ("pos", "q_gap", "t_gap", "both_gap")}


def slopes(pos, c):
    """slope_k = floor(65536 (c[k+1] - c[k]) / (pos[k+1] - pos[k])); the last one repeats the one before it; n = 1: 0."""
    n = len(pos)
    s = [(65536 * (c[k + 1] - c[k])) // (pos[k + 1] - pos[k]) for k in range(n - 1)]
    return s + [s[-1] if s else 0]


def validate(t):
    """The contract's checks; ValueError names the clause that fails."""
    t = table(t)
    pos, n = t["pos"], len(t["pos"])
    if not 1 <= n <= POINTS:
        raise ValueError("n")
    if any(len(t[k]) != n for k in ("q_gap", "t_gap", "both_gap")):
        raise ValueError("lengths")
    if pos[0] < 1 or pos[-1] >= 2 ** 32 or any(pos[k] <= pos[k - 1] for k in range(1, n)):
        raise ValueError("pos")
    for name in ("q_gap", "t_gap", "both_gap"):
        c = t[name]
        if any(x < 0 or x > 2 ** 40 for x in c):
            raise ValueError(name + " range")
        if any(c[k] < c[k - 1] for k in range(1, n)):
            raise ValueError(name + " order")
        if any(s >= 2 ** 27 for s in slopes(pos, c)):
            raise ValueError(name + " slope")
    return t


def g(pos, c, x):
    """The piecewise-linear cost of a length x >= 1."""
    if x < pos[0]:
        return c[0]
    k = max(j for j in range(len(pos)) if pos[j] <= x)
    return c[k] + (((x - pos[k]) * slopes(pos, c)[k]) >> 16)


def gapcost(t, dt, dq):
    """The gap cost of a link with gaps dt, dq >= 0 under the table t."""
    if dt == 0 and dq == 0:
        return 0
    if dt == 0:
        return g(t["pos"], t["q_gap"], dq)
    if dq == 0:
        return g(t["pos"], t["t_gap"], dt)
    return g(t["pos"], t["both_gap"], dt + dq)


def link_penalty(h, j, i, diag_pen, anti_pen, t):
    """pen'(j, i) on input indices: hsp_chain_model.penalty plus the gap cost (t None: none)."""
    p = M.penalty(h, j, i, diag_pen, anti_pen)
    if t is None:
        return p
    sp = int(h["len"][j]) + 1
    dt = int(h["ref_start"][i]) - (int(h["ref_start"][j]) + sp)
    dq = int(h["query_start"][i]) - (int(h["query_start"][j]) + sp)
    return p + gapcost(t, dt, dq)


def arrays(t):
    """(pos int64[n], costs int64[3, n], slopes int64[3, n]) of a table, rows in the order q_gap, t_gap, both_gap."""
    names = ("q_gap", "t_gap", "both_gap")
    return (np.array(t["pos"], dtype=np.int64), np.array([t[k] for k in names], dtype=np.int64),
            np.array([slopes(t["pos"], t[k]) for k in names], dtype=np.int64))


def gapcost_rows(t, dt, dq, pre=None):
    """gapcost for int64 vectors of gaps >= 0 (the bound of the contract keeps every product below 2^60); held against gapcost() by
    tests/test_hsp_chain_gap_model.py.  pre: arrays(t), where the caller has them."""
    pos, c, s = pre if pre is not None else arrays(t)
    x = dt + dq
    k = np.maximum(np.searchsorted(pos, x, side="right") - 1, 0)
    at = np.where(dt == 0, 0, np.where(dq == 0, 1, 2)) * pos.size + k  # the row of the case, flat
    return np.where(x == 0, 0, c.ravel()[at] + ((np.maximum(x - pos[k], 0) * s.ravel()[at]) >> 16))


def chain(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, gap_costs=None):
    """hsp_chain_model.chain under pen': -> (f int64[n] and pred int32[n] in INPUT order (pred: input index or -1), members MEMBER[]).
    gap_costs: a preset's name, a table dict, or None, which is hsp_chain_model.chain itself."""
    if gap_costs is None:
        return M.chain(hsps, groups, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap, min_score=min_score)
    t = validate(gap_costs)
    h = np.asarray(hsps, dtype=M.SEG)
    n = h.size
    g_in = np.zeros(n, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    order = M.rank_order(h, g_in)
    rs = h["ref_start"][order].astype(np.int64)
    qs = h["query_start"][order].astype(np.int64)
    span = h["len"][order].astype(np.int64) + 1
    re, qe = rs + span, qs + span
    sc = h["score"][order].astype(np.int64)
    gr = g_in[order]
    dg, f = rs - qs, np.zeros(n, dtype=np.int64)
    pred = np.full(n, -1, dtype=np.int64)  # ranks
    pre = arrays(t)
    for i in range(n):
        dt, dq = rs[i] - re[:i], qs[i] - qe[:i]
        ok = (gr[:i] == gr[i]) & (dt >= 0) & (dq >= 0)
        if max_gap:
            ok &= (dt <= max_gap) & (dq <= max_gap)
        best = 0
        if ok.any():
            c = np.flatnonzero(ok)
            v = f[c] - (diag_pen * np.abs(dg[i] - dg[c]) + anti_pen * (dt[c] + dq[c]) + gapcost_rows(t, dt[c], dq[c], pre))
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
        for k in reversed(walk):
            members.append((int(order[k]), int(grp), int(f[k])))
    f_in, pred_in = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    f_in[order] = f
    pred_in[order] = np.where(pred >= 0, order[np.maximum(pred, 0)], -1)
    return f_in, pred_in, np.array(members, dtype=M.MEMBER)


def chain_all(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, gap_costs=None):
    """hsp_chain_all_model.chain_all on this model's f and pred."""
    f, pred, _ = chain(hsps, groups, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap, gap_costs=gap_costs)
    return MA.chain_all(hsps, groups, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap, min_score=min_score, dp=(f, pred))
