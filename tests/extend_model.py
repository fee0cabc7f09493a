"""Plain Python restatement of the ungapped X-drop extension of one anchor, as stated at the head of segalign_amd/csrc/extend.hip
(src/seed_filter.cu:299-647 of the reference), for tests/extend_regimes.py: positions and scores with the entropy factor off.

Per side (right: k = 0, 1, ..; left: k = 1, 2, ..):

    stop at the first position outside either sequence
    score += M[r][q]
    stop if max(best, score) - score > xdrop
    if score > best: best = score, bestpos = k          (strict: the first position that attains the maximum wins)

record = (ref_loc - offL, query_loc - offL, posR + offL, bestR + bestL), kept iff bestR + bestL >= hspthresh.

A Side also says what the walk went through -- where it stopped and why, how many bases it scored, its deepest surviving dip and
where that dip first reached its depth -- so that a regime can show it is in the state it names.  Nothing here is vectorised or shared with the
oracle: tests/test_extend_regimes.py holds it to oracle.extend_hit, scalar and tiled, on every anchor."""
import numpy as np

SEG = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])


class Side:
    __slots__ = ("best", "pos", "examined", "stop", "edge", "dip", "dip_at", "last", "ties")

    def __repr__(self):
        return "Side(best=%d pos=%d examined=%d stop=%d edge=%s dip=%d@%d)" % (self.best, self.pos, self.examined, self.stop, self.edge,
                                                                                self.dip, self.dip_at)


def side(ref, qry, mat, ref_loc, query_loc, xdrop, left):
    """One side of one anchor.  ref, qry: code sequences (indexable, ints 0..7); mat: 64 scores, row = target code.
    best, pos      the side's best score and the offset k of its first occurrence (right: -1 if none, left: 0 if none)
    examined       bases scored, the one that drops included
    stop, edge     the k at which the walk ended: the base that dropped (edge False) or the first k outside a sequence (edge True)
    dip, dip_at    the largest max(best, score) - score among the bases the walk survived, and the first k that had it
    last           the running score after the last base the walk survived
    ties           the k, after pos, at which the score came back to exactly `best` (and so did not move pos)"""
    s = Side()
    s.best, s.pos, s.examined, s.dip, s.dip_at, s.last, s.ties = 0, (0 if left else -1), 0, 0, -1, 0, []
    nr, nq = len(ref), len(qry)
    score = 0
    k = 1 if left else 0
    while True:
        if left:
            if not (ref_loc >= k and query_loc >= k):
                s.stop, s.edge = k, True
                return s
            r, q = ref[ref_loc - k], qry[query_loc - k]
        else:
            if not (ref_loc + k < nr and query_loc + k < nq):
                s.stop, s.edge = k, True
                return s
            r, q = ref[ref_loc + k], qry[query_loc + k]
        score += mat[r * 8 + q]
        s.examined += 1
        d = max(s.best, score) - score
        if d > xdrop:
            s.stop, s.edge = k, False
            return s
        if score > s.best:
            s.best, s.pos, s.ties = score, k, []
        elif score == s.best and s.best > 0:
            s.ties.append(k)
        if d > s.dip:
            s.dip, s.dip_at = d, k
        s.last = score
        k += 1


class Ext:
    __slots__ = ("R", "L", "total", "rec", "passed", "examined")


def extend(ref, qry, mat, ref_loc, query_loc, xdrop, hspthresh):
    """Both sides of one anchor with the entropy factor off: .R, .L (Side), .total, .rec (4 ints), .passed, .examined."""
    e = Ext()
    e.R = side(ref, qry, mat, ref_loc, query_loc, xdrop, False)
    e.L = side(ref, qry, mat, ref_loc, query_loc, xdrop, True)
    e.total = e.R.best + e.L.best
    e.rec = (ref_loc - e.L.pos, query_loc - e.L.pos, e.R.pos + e.L.pos, e.total)
    e.passed = e.total >= hspthresh
    e.examined = e.R.examined + e.L.examined
    return e


def as_lists(ref, qry, mat):
    """the three inputs in the form side() indexes fastest"""
    return bytes(np.ascontiguousarray(ref, np.uint8)), bytes(np.ascontiguousarray(qry, np.uint8)), [int(x) for x in np.asarray(mat).ravel()]


def extend_all(ref, qry, mat, anchors, xdrop, hspthresh):
    """-> list of Ext, one per anchor (anchors: (n, 2) of ref_loc, query_loc)"""
    r, q, m = as_lists(ref, qry, mat)
    return [extend(r, q, m, int(a), int(b), xdrop, hspthresh) for a, b in np.asarray(anchors).reshape(-1, 2)]


def records(exts):
    """the passing records of a list of Ext as a SEG array, in anchor order"""
    keep = [e.rec for e in exts if e.passed]
    out = np.zeros(len(keep), dtype=SEG)
    for i, (a, b, l, s) in enumerate(keep):
        out[i] = (a & 0xFFFFFFFF, b & 0xFFFFFFFF, l & 0xFFFFFFFF, s)
    return out


def is_candidate(e, hspthresh, long_cap):
    """Does the byte-coded filter (extend_filter_kernel) hand this anchor to the exact kernel?  It walks a side in chunks of 8 bases and
    forwards the anchor when a side is still alive after long_cap bases -- the right side has then survived k = 0 .. long_cap - 1, the
    left side k = 1 .. long_cap --; an anchor whose sides both ended is a candidate iff its total passes."""
    cap = max(long_cap, 8)
    if e.R.stop >= cap:
        return True
    if e.L.stop - 1 >= cap:
        return True
    return e.total >= hspthresh


# ---- the chain shortcut (extend.hip 2b) on the anchors of ONE call that share a diagonal --------------------------------------
CHAIN_GAP_MAX, CHAIN_WALK_EXTRA, CHAIN_QSHIFT = 256, 96, 9


def chain_is_head(ref, qry, mat, c, pc, xdrop):
    """chain_is_run_head: does candidate c = (ref_loc, query_loc) start a run, given its sorted predecessor pc?  The bounded left walk is
    made in chunks of 8 bases from k = 1 while the chunk's first k <= gap + CHAIN_WALK_EXTRA, and looked at after every chunk."""
    if not (c[0] - c[1] == pc[0] - pc[1] and c[1] > pc[1]):
        return True
    g = c[1] - pc[1]
    if g > CHAIN_GAP_MAX:
        return True
    score, best, bpos = 0, 0, 0
    k0 = 1
    while k0 <= g + CHAIN_WALK_EXTRA:
        dropped = False
        for k in range(k0, k0 + 8):
            if dropped:
                break
            if not (c[0] >= k and c[1] >= k):
                dropped = True
                break
            score += mat[ref[c[0] - k] * 8 + qry[c[1] - k]]
            if max(best, score) - score > xdrop:
                dropped = True
                break
            if score > best:
                best, bpos = score, k
        if bpos > g:
            return False
        if dropped:
            break
        k0 += 8
    return True


def chain_records(ref, qry, mat, anchors, xdrop, hspthresh):
    """The records a call of these candidates leaves with the chain shortcut on, when they are alone in their buckets: candidates of one
    diagonal and one 512-base query window are sorted by position (exact duplicates in input order), each is tested against its
    predecessor, and every run is walked head by head.  anchors: every one a candidate (its total passes or a side is capped)."""
    r, q, m = as_lists(ref, qry, mat)
    groups = {}
    for i, (a, b) in enumerate(np.asarray(anchors).reshape(-1, 2).tolist()):
        groups.setdefault((a - b, b >> CHAIN_QSHIFT), []).append((b, i, a))
    out = []
    for key in groups:
        srt = [(a, b) for b, i, a in sorted(groups[key])]
        head = [True] + [chain_is_head(r, q, m, srt[j], srt[j - 1], xdrop) for j in range(1, len(srt))]
        j = 0
        while j < len(srt):           # j is a run head (flagged, or promoted)
            e = extend(r, q, m, srt[j][0], srt[j][1], xdrop, hspthresh)
            if e.passed:
                out.append(e.rec)
            right_end = srt[j][0] + e.R.pos
            n = j + 1
            while n < len(srt) and not head[n] and not srt[n][0] > right_end:
                n += 1
            j = n                       # a flagged head starts its own run; a member beyond the right end is promoted
    res = np.zeros(len(out), dtype=SEG)
    for i, (a, b, l, s) in enumerate(out):
        res[i] = (a & 0xFFFFFFFF, b & 0xFFFFFFFF, l & 0xFFFFFFFF, s)
    return res
