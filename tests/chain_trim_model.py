"""The contract of sa_trim_chains (include/segalign_amd.h) in Python integers: the overlap of two consecutive members,
the crossover that keeps the most of the shared columns, the cut members with their exact scores, and the exact chain scores.  The
relation and the gaps are hsp_chain_overlap_model's, the gap cost hsp_chain_gap_model's.  t and q are the codes of the resident target
block and query strand (a column scores sub[(t & 7) * 8 + (q & 7)], as in stitch_model).  Written from the header, not from the kernel."""
import numpy as np

import hsp_chain_gap_model as G
import hsp_chain_model as M
import hsp_chain_overlap_model as O

CHAIN = np.dtype([("score", "<i8"), ("trimmed_links", "<u4"), ("bases_cut", "<u4")])
LINK = np.dtype([("o", "<u4"), ("x", "<u4"), ("gap_r", "<u4"), ("gap_q", "<u4")])


def columns(t, q, sub, r0, q0, n):
    """The scores of the n columns from (r0, q0) on, as Python integers."""
    a, b = np.asarray(t[r0:r0 + n], dtype=np.int64) & 7, np.asarray(q[q0:q0 + n], dtype=np.int64) & 7
    return [int(v) for v in np.asarray(sub, dtype=np.int64).reshape(64)[a * 8 + b]]


def crossover(a, b):
    """x in 0 .. o that maximises sum(a[:x]) + sum(b[x:]); the lowest x among equals."""
    assert len(a) == len(b)
    best, bx, s = None, 0, sum(b)  # s = S(0)
    for x in range(len(a) + 1):
        if best is None or s > best:
            best, bx = s, x
        if x < len(a):
            s += a[x] - b[x]
    return bx


def validate(t, q, hsps, members, first):
    """The contract's checks; ValueError names the clause that fails."""
    h = np.asarray(hsps, dtype=M.SEG)
    if len(first) - 1 > 1 << 22 or (len(first) > 1 and (first[0] != 0 or any(first[c + 1] < first[c] for c in range(len(first) - 1)))):
        raise ValueError("first")
    for k, m in enumerate(members):
        if m >= h.size:
            raise ValueError("not in the input")
        r, s, b, _ = O.node(h, int(m))
        if r + b > len(t) or s + b > len(q):
            raise ValueError("inside the block")
    for c in range(len(first) - 1):
        for k in range(int(first[c]), int(first[c + 1]) - 1):
            if not O.precedes(h, None, int(members[k]), int(members[k + 1]), O.MAX_OVERLAP):
                raise ValueError("overlaps")


def trim(t, q, sub, hsps, members, first, diag_pen=0, anti_pen=0, gap_costs=None):
    """-> (M.SEG trimmed HSPs, one per member entry; CHAIN chains; LINK links in entry order)."""
    h = np.asarray(hsps, dtype=M.SEG)
    validate(t, q, h, members, first)
    tab = G.validate(gap_costs) if gap_costs is not None else None
    out = h[np.asarray(members, dtype=np.int64)].copy() if len(members) else np.zeros(0, dtype=M.SEG)
    head, tail = [0] * out.size, [0] * out.size  # columns lost
    links, chains = [], np.zeros(len(first) - 1, dtype=CHAIN)
    for c in range(len(first) - 1):
        pen = trimmed = cut = 0
        for k in range(int(first[c]), int(first[c + 1]) - 1):
            j, i = int(members[k]), int(members[k + 1])
            o = O.overlap(h, j, i)
            gr, gq = O.trimmed_gaps(h, j, i)
            x = 0
            if o:
                rj, qj, bj, _ = O.node(h, j)
                ri, qi, _, _ = O.node(h, i)
                x = crossover(columns(t, q, sub, rj + bj - o, qj + bj - o, o), columns(t, q, sub, ri, qi, o))
                tail[k], head[k + 1] = o - x, x
                trimmed, cut = trimmed + 1, cut + o
            links.append((o, x, gr, gq))
            pen += O.link_penalty(h, j, i, diag_pen, anti_pen, tab)
        chains[c] = (-pen, trimmed, cut)
    for k in range(out.size):
        if head[k] or tail[k]:
            r, s, b, _ = O.node(out, k)
            r, s, b = r + head[k], s + head[k], b - head[k] - tail[k]
            assert b >= 1
            out[k] = (r, s, b - 1, sum(columns(t, q, sub, r, s, b)))
    for c in range(len(first) - 1):
        chains[c]["score"] += int(out["score"][int(first[c]):int(first[c + 1])].astype(np.int64).sum())
    return out, chains, np.array(links, dtype=LINK)
