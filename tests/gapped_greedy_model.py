"""The sequential rule of sa_gapped_align_greedy (include/segalign_amd.h) in plain Python.

Per-HSP records and paths come either from the path checker (gapped_trace_model.align) or from given arrays: records as
sa_gapped_align raw mode returns them (GAPPED_DTYPE, record k for HSP k) and paths as (left ops, right ops in genome order, counts)."""
import numpy as np

import gapped_model as G
import gapped_trace_model as T


def anchor(h):
    """(a_r, a_q) of one SEG_DTYPE HSP."""
    return int(h["ref_start"]) + int(h["len"]) // 2, int(h["query_start"]) + int(h["len"]) // 2


def priority(hsps):
    """pi: HSP indices by (score descending, index ascending)."""
    return sorted(range(hsps.size), key=lambda k: (-int(hsps[k]["score"]), k))


def cover_set(rec, ops, a):
    """The (t, q) of the M pairs of a path walked from (ref_start, query_start), plus the anchor point a."""
    pts = {a}
    i, j = int(rec["ref_start"]), int(rec["query_start"])
    for x in ops.tolist():
        ln, op = x >> 2, x & 3
        if op == T.OP_M:
            pts.update(zip(range(i, i + ln), range(j, j + ln)))
            i += ln
            j += ln
        elif op == T.OP_I:
            j += ln
        else:
            i += ln
    return pts


def order(recs):
    """Selection rule (3): (query_start, ref_start, query_end, ref_end, -score, hsp_index)."""
    return sorted(range(recs.size), key=lambda k: (int(recs[k]["query_start"]), int(recs[k]["ref_start"]), int(recs[k]["query_end"]),
                                                   int(recs[k]["ref_end"]), -int(recs[k]["score"]), int(recs[k]["hsp_index"])))


def greedy(hsps, recs, paths, gappedthresh):
    """-> (records of A in rule (3) order, their paths, {"returned", "covered", "below_thresh"} and "state": per HSP 1 returned,
    2 covered, 0 below threshold)."""
    hsps = np.ascontiguousarray(hsps, dtype=G.SEG_DTYPE)
    covered = set()
    state = np.zeros(hsps.size, dtype=np.int8)
    acc = []
    for h in priority(hsps):
        a = anchor(hsps[h])
        if a in covered:
            state[h] = 2
            continue
        if int(recs[h]["score"]) < gappedthresh:
            continue
        state[h] = 1
        acc.append(h)
        lo, ro, _ = paths[h]
        covered |= cover_set(recs[h], np.concatenate([lo, ro]), a)
    sel = recs[acc] if acc else np.zeros(0, dtype=G.GAPPED_DTYPE)
    ordk = order(sel)
    sel = sel[ordk] if ordk else sel
    sel_paths = [paths[int(r["hsp_index"])] for r in sel]
    stats = {"returned": len(acc), "covered": int((state == 2).sum()), "below_thresh": int((state == 0).sum()), "state": state}
    return sel, sel_paths, stats


def from_checker(t, q, sub, hsps, gappedthresh, **kw):
    """greedy() over the records and paths of the C path checker."""
    recs, paths = T.align(t, q, sub, hsps, **kw)
    return greedy(hsps, recs, paths, gappedthresh)


def from_align(recs, pth, ops):
    """Per-record (left ops, right ops, counts) from sa_gapped_align's raw outputs."""
    out = []
    for k in range(recs.size):
        lo, ro = T.record_ops(pth, ops, k)
        p = pth[k]
        out.append((lo.copy(), ro.copy(), {c: int(p[c]) for c in ("matches", "mismatches", "gap_opens", "gap_bases")}))
    return out
