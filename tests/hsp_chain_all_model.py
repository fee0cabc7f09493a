"""The contract of sa_chain_hsps_all (include/segalign_amd.h) in numpy: f and pred are hsp_chain_model.chain's, the
peeling is the sequential rule applied literally."""
import numpy as np

import hsp_chain_model as M

RECORD = np.dtype([("group", "<u4"), ("head", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"), ("score", "<i8"), ("joined", "<i4"),
                   ("pad", "<u4")])
MEMBER = np.dtype([("hsp_index", "<u4"), ("group", "<u4"), ("chain", "<u4"), ("pad", "<u4"), ("f", "<i8")])
NONE = 0xFFFFFFFF


def peel(f, pred, rank):
    """The sequential rule on input indices.  -> (head int64[n], [(head, score, joined or -1, walk from the head down), ...] in the
    order the chains are peeled)."""
    n = len(f)
    prio = sorted(range(n), key=lambda u: (-int(f[u]), int(rank[u])))
    used, head, chains = [False] * n, np.full(n, -1, dtype=np.int64), []
    for u in prio:
        if used[u]:
            continue
        v, walk = u, []
        while v >= 0 and not used[v]:
            used[v] = True
            head[v] = u
            walk.append(v)
            v = int(pred[v])
        chains.append((u, int(f[u]) - (int(f[v]) if v >= 0 else 0), v, walk))
    return head, chains


def chain_all(hsps, groups=None, diag_pen=0, anti_pen=0, max_gap=0, min_score=0, dp=None):
    """-> (f, pred in input order as hsp_chain_model.chain, RECORD chains, MEMBER members, uint32 chain_of in input order).
    dp: (f, pred) of hsp_chain_model.chain on the same input, where the caller has them already."""
    h = np.asarray(hsps, dtype=M.SEG)
    n = h.size
    g = np.zeros(n, dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    f, pred = dp if dp is not None else M.chain(h, g, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap)[:2]
    rank = np.zeros(n, dtype=np.int64)
    rank[M.rank_order(h, g)] = np.arange(n)
    _, peeled = peel(f, pred, rank)
    kept = sorted((c for c in peeled if c[1] >= min_score), key=lambda c: (int(g[c[0]]), -c[1], int(rank[c[0]])))
    chains, members, chain_of = np.zeros(len(kept), dtype=RECORD), [], np.full(n, NONE, dtype=np.uint32)
    for k, (u, score, s, walk) in enumerate(kept):
        chains[k] = (g[u], u, len(members), len(walk), score, s, 0)
        for v in reversed(walk):  # a predecessor has the lower rank: the reversed walk is in rank order
            members.append((v, g[v], k, 0, f[v]))
            chain_of[v] = k
    return f, pred, chains, np.array(members, dtype=MEMBER), chain_of
