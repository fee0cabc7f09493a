"""A plain model of the two X-drop FILTER levels of a context-table call (extend.hip 1d and 1b; DESIGN.md 4.5a, 4.5'''), hit for hit.

Both levels are pure integer functions of one hit's bases, the class scores or the matrix, xdrop, hspthresh, seed_size, left_skip and
long_cap.  Written from the rules the kernels' comments and kernels.h (L2Rec, CtxRec) state, on plain code arrays: no phase copies,
no packed registers, no table of fields, no lanes.

LEVEL 1, the class filter.  x = (target 2-bit code) ^ (query 2-bit code) is the class of a base pair, cls[x] its score; a 2-bit code
is the code itself for ACGT and 0 for every code >= 4 and every position outside the block.
  right side   the 54 bases from the anchor on: t2[ref_loc + k] ^ q2[query_loc + k] of this strand
  left side    the 58 bases in front of lend = ref_loc - left_skip, in walking order: (3 - t2[lend - 1 - k]) ^ o2[lp + k], o2 the OTHER
               strand and lp = query_len - query_loc + left_skip (the reverse of a strand is the complement of the other strand:
               this is t ^ q wherever both bases are ACGT and inside their blocks)
  walk         per base: T += cls[x], best = max(best, T), N = T - best.  Right: T = 0, best = 0.  Left: behind the seed window, which
               is bounded and not walked: T = best = left_skip * max(cls, 0)
  alive        N >= -xdrop at EVERY FIELD END: after 6, 12 .. 54 bases; on the left also after the four-base tail (58)
  best         over the whole context, also behind a drop
  forward      r_alive or l_alive or bestR + bestL >= hspthresh; a hit outside the repeat masker's window is skipped: neither forwarded
               nor audited
  record       flags = r_alive | l_alive << 1, sent as 3 when 0; known = bestL if r_alive else bestR; state = {T : best - T} of the left
               walk -- of the right walk when flags == 1 under l2_right_state; hidx = the hit's index in call order

LEVEL 2, the packed walk on what level 1 forwards (or on every hit of the call: lookup mode 1, no context table).
  pair score   SM[t][q & 7]: t the 2-bit target code, 0 outside the block; q = 7 outside the block; row 0 is the maximum of the matrix rows
               0, 4 .. 7; entries are raised to -16383
  walk         two bases per step: {T1, T2} = sat16(T + s0), sat16(T + (s0 + s1)); best = max(best, T1, T2); T = T2
  drop test    best - T <= xdrop, asked after every 16 bases; a side that fails it ends with the best it has
  long_cap     asked after every 64 bases of a side that is still alive: walked + 10 >= long_cap forwards the hit
  start        flags 3: right from the anchor, then left from the anchor.  flags 1: right from the anchor -- under l2_right_state resumed at
               walked = 54 from `state` --, the left best is `known`.  flags 2: bestR = known, the left walk resumed at walked = 58 + left_skip
               from `state` = {T, best = T + D}
  candidate    forwarded, or bestR + bestL >= hspthresh"""
import numpy as np

import image_model as IM
import probe_model as PM
import table_model as TM

R_BASES, L_BASES = TM.CTX_R_BASES, TM.CTX_L_BASES
R_ENDS = tuple(range(5, R_BASES, 6))                    # k of the last base of every right field
L_ENDS = tuple(range(5, 54, 6)) + (L_BASES - 1,)        # nine fields and the four-base tail
L2REC = np.dtype([("ref_loc", "<u4"), ("query_loc", "<u4"), ("hidx", "<u4"), ("state", "<u4"), ("meta", "<u4")])
L2_NSUB = 256
I16_MIN, I16_MAX = -32768, 32767


class Params:
    def __init__(self, seed_size, xdrop, hspthresh, left_skip=None, long_cap=128, l2_right_state=0, rm_window=None):
        self.seed_size, self.xdrop, self.hspthresh = int(seed_size), int(xdrop), int(hspthresh)
        self.left_skip = self.seed_size if left_skip is None else int(left_skip)
        self.long_cap, self.l2_right_state, self.rm_window = int(long_cap) & ~7, int(l2_right_state), rm_window


# ---- the hits of a call, in call order --------------------------------------------------------------------------------------------------
class Sparse:
    """an array over all 4^k keys that is `default` outside a sorted key list: what Table needs of one, for key spaces too large to
    hold densely (14of22: 4^14 keys)"""

    def __init__(self, keys, vals, default=0):
        self.keys, self.vals, self.default = np.asarray(keys, dtype=np.int64), np.asarray(vals), default

    def __getitem__(self, k):
        k = np.asarray(k, dtype=np.int64)
        if not self.keys.size:
            return np.full(k.shape, self.default, dtype=self.vals.dtype)
        i = np.minimum(np.searchsorted(self.keys, k), self.keys.size - 1)
        return np.where(self.keys[i] == k, self.vals[i], self.default)

    def max(self):
        return self.vals.max() if self.vals.size else self.default


class SparseStart:
    """nbr_start over all keys: the run entries in front of key k"""

    def __init__(self, keys, run):
        self.keys = np.asarray(keys, dtype=np.int64)
        self.cum = np.concatenate([[0], np.cumsum(run)]).astype(np.uint64)

    def __getitem__(self, k):
        return self.cum[np.searchsorted(self.keys, np.asarray(k, dtype=np.int64), side="left")]


class Table:
    """probe_model.Table plus what turns a run entry into a target position.  Dense over the 4^k keys through table_model.neighbourhood
    up to weight 12; above that (or when asked) the same table from its rule on the keys that occur: the run of key k is bucket(k)
    followed by bucket(k ^ m) for the transition masks m in word order, runs in key order"""

    def __init__(self, target_codes, shape, step, transition=True, sparse=None):
        self.shape, self.transition = shape, bool(transition)
        keys, self.pos = TM.seed_entries(target_codes, shape, step)
        self.masks = np.array(shape.masks(transition), dtype=np.int64)
        self.words = int(self.masks.size)
        if sparse is None:
            sparse = shape.weight > 12
        if not sparse:
            self.bucket = np.bincount(keys, minlength=shape.nkeys).astype(np.int64)
            self.nbr_start, self.src = TM.neighbourhood(keys, shape, transition)
            self.run = np.diff(self.nbr_start.astype(np.int64))
            return
        u, c = np.unique(np.asarray(keys, dtype=np.int64), return_counts=True)
        first = np.concatenate([[0], np.cumsum(c)[:-1]]) if u.size else np.zeros(0, dtype=np.int64)
        self.bucket = Sparse(u, c.astype(np.int64))
        # one piece per (bucket, mask): it lies in the run of key u ^ m, behind the pieces of the masks in front of m
        rk = np.concatenate([u ^ m for m in self.masks]) if u.size else np.zeros(0, dtype=np.int64)
        j = np.repeat(np.arange(self.masks.size), u.size)
        order = np.lexsort((j, rk))
        ln, st = np.tile(c, self.masks.size)[order], np.tile(first, self.masks.size)[order]
        total = int(ln.sum())
        self.src = np.repeat(st, ln) + (np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln))
        ru, inv = np.unique(rk[order], return_inverse=True)
        run = np.bincount(inv, weights=ln, minlength=ru.size).astype(np.int64)
        self.run = Sparse(ru, run)
        self.nbr_start = SparseStart(ru, run)


def call_hits(table, query_codes, start, end):
    """(ref_loc, query_loc) of every hit of the call over query positions [start, end) of this strand, in call order: the records of
    probe_model.probe in order, the entries of a record's run in table order.  Hit g of the call is row g: its hidx."""
    qkeys = PM.position_keys(query_codes, table.shape)
    end = min(end, qkeys.size)
    if end <= start:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    out = PM.probe(table, qkeys, start, end, end - start, 1, 1 << 30, head_bits=False)
    rec, hits = out["records"], out["hits"]
    prefix = rec["prefix"].astype(np.int64)
    cnt = np.diff(prefix)
    g = np.arange(hits, dtype=np.int64)
    entry = np.repeat(rec["off"][:-1].astype(np.int64), cnt) + (g - np.repeat(prefix[:-1], cnt))
    s = table.shape.span
    return table.pos[table.src[entry]].astype(np.int64) + s, np.repeat(rec["qpos"][:-1].astype(np.int64), cnt) + s


# ---- level 1 ----------------------------------------------------------------------------------------------------------------------------
def class_strings(tc, qc, oc, ref_loc, query_loc, left_skip):
    """the class of every context base: (n, 54) right and (n, 58) left, walking order"""
    t2, q2, o2 = IM.two_bit(np.asarray(tc, np.uint8)), IM.two_bit(np.asarray(qc, np.uint8)), IM.two_bit(np.asarray(oc, np.uint8))
    ref_loc, query_loc = np.asarray(ref_loc, np.int64), np.asarray(query_loc, np.int64)
    kr, kl = np.arange(R_BASES, dtype=np.int64)[None, :], np.arange(L_BASES, dtype=np.int64)[None, :]
    xr = IM._at(t2, ref_loc[:, None] + kr, 0) ^ IM._at(q2, query_loc[:, None] + kr, 0)
    lend = ref_loc - left_skip
    lp = len(qc) - query_loc + left_skip
    xl = (3 - IM._at(t2, lend[:, None] - 1 - kl, 0)) ^ IM._at(o2, lp[:, None] + kl, 0)
    return xr, xl


def walk_one(classes, cls, t0, ends):
    """the stated per-base walk on one class string with plain ints -> (T, N, W, best, per-base N): W = the lowest N at a field end"""
    T, best, W, trace = t0, t0, 0, []
    for k, x in enumerate(classes):
        T += cls[int(x)]
        best = max(best, T)
        trace.append(T - best)
        if k in ends:
            W = min(W, T - best)
    return T, T - best, W, best, trace


def _walk(classes, cls, t0, ends, keep=None):
    """walk_one on every row at once -> (T, N, W, best) at the end of the context; keep: a list that receives (T, N) of every base"""
    s = np.asarray(cls, dtype=np.int64)[classes]
    T = t0 + np.cumsum(s, axis=1)
    best = np.maximum(np.maximum.accumulate(T, axis=1), t0)
    N = T - best
    W = np.minimum(N[:, list(ends)].min(axis=1), 0)
    if keep is not None:
        keep.append((T, N))
    return T[:, -1], N[:, -1], W, best[:, -1]


def seed_bound(cls, left_skip):
    return left_skip * max(max(cls), 0)


def level1(tc, qc, oc, ref_loc, query_loc, cls, P, block=1 << 16, detail=False):
    """every hit of a call through the class filter -> dict of per-hit arrays (fwd, skip, r_alive, l_alive, bestR, bestL, flags, known,
    state, and the walks' end states TR, NR, TL, NL); rows = call order"""
    ref_loc, query_loc = np.asarray(ref_loc, np.int64), np.asarray(query_loc, np.int64)
    n = ref_loc.size
    keys = ("TR", "NR", "WR", "bestR", "TL", "NL", "WL", "bestL")
    o = {k: np.zeros(n, dtype=np.int64) for k in keys}
    t0 = seed_bound(cls, P.left_skip)
    kr, kl = ([], []) if detail else (None, None)
    for lo in range(0, n, block):
        sl = slice(lo, min(lo + block, n))
        xr, xl = class_strings(tc, qc, oc, ref_loc[sl], query_loc[sl], P.left_skip)
        o["TR"][sl], o["NR"][sl], o["WR"][sl], o["bestR"][sl] = _walk(xr, cls, 0, R_ENDS, kr)
        o["TL"][sl], o["NL"][sl], o["WL"][sl], o["bestL"][sl] = _walk(xl, cls, t0, L_ENDS, kl)
    if detail and n:     # (tests) the walks base by base: T and N after every base of either context
        o["TR_all"], o["NR_all"] = (np.concatenate([a[i] for a in kr]) for i in (0, 1))
        o["TL_all"], o["NL_all"] = (np.concatenate([a[i] for a in kl]) for i in (0, 1))
    for k in keys:      # the kernel keeps T and N as int16: a regime that left the range would not be the one it states
        assert o[k].size == 0 or (o[k].min() >= I16_MIN and o[k].max() <= I16_MAX), k
    o["skip"] = np.zeros(n, dtype=bool)
    if P.rm_window is not None:
        o["skip"] = ~((ref_loc >= P.rm_window[0]) & (ref_loc <= P.rm_window[1]))
    o["r_alive"], o["l_alive"] = o["WR"] >= -P.xdrop, o["WL"] >= -P.xdrop
    o["fwd"] = ~o["skip"] & (o["r_alive"] | o["l_alive"] | (o["bestR"] + o["bestL"] >= P.hspthresh))
    fl = o["r_alive"].astype(np.int64) | (o["l_alive"].astype(np.int64) << 1)
    o["flags"] = np.where(fl == 0, 3, fl)
    o["known"] = np.where(o["r_alive"], o["bestL"], o["bestR"])
    right = (fl == 1) & bool(P.l2_right_state)
    T, N = np.where(right, o["TR"], o["TL"]), np.where(right, o["NR"], o["NL"])
    o["state"] = ((T & 0xFFFF) << 16) | ((-N) & 0xFFFF)
    o["ref_loc"], o["query_loc"] = ref_loc, query_loc
    return o


def forwards(o):
    """the hand-over records of a level-1 result, in call order (= sorted by hidx)"""
    idx = np.flatnonzero(o["fwd"])
    rec = np.zeros(idx.size, dtype=L2REC)
    rec["ref_loc"], rec["query_loc"], rec["hidx"] = o["ref_loc"][idx], o["query_loc"][idx], idx
    rec["state"] = o["state"][idx]
    rec["meta"] = o["known"][idx] | (o["flags"][idx] << 16)
    return rec


# ---- level 2 ----------------------------------------------------------------------------------------------------------------------------
def pair_matrix(sub_mat):
    """(4, 8): the exact pair score of a 2-bit target code and a query code"""
    m = np.asarray(sub_mat, dtype=np.int64).reshape(8, 8)
    sm = m[:4].copy()
    sm[0] = np.maximum(m[0], m[4:8].max(axis=0))
    return np.maximum(sm, -16383)


def _sat(v):
    return np.clip(v, I16_MIN, I16_MAX)


def packed_side(t2, q7, sm, ref_loc, query_loc, left, walked, T, best, P):
    """one side of every record at once: from `walked` bases behind the anchor with running score T and best score `best`
    -> (best at the end, forwarded by the long_cap rule, bases walked when the side ended)"""
    global SATURATED
    n = ref_loc.size
    walked, T, best = (np.array(np.broadcast_to(v, n), dtype=np.int64) for v in (walked, T, best))
    fwd = np.zeros(n, dtype=bool)
    live = np.arange(n)
    while live.size:
        for _ in range(4):                           # a window of 64 bases in four tests
            w = walked[live][:, None] + np.arange(16, dtype=np.int64)[None, :]
            rp = ref_loc[live][:, None] + (-(w + 1) if left else w)
            qp = query_loc[live][:, None] + (-(w + 1) if left else w)
            s = sm[IM._at(t2, rp, 0), IM._at(q7, qp, 7)]
            edge = (IM._at(q7, qp, 7) == 7).any(axis=1)      # the step meets the query's end or a record separator
            t, b = T[live], best[live]
            for j in range(0, 16, 2):
                t1, t2_ = _sat(t + s[:, j]), _sat(t + (s[:, j] + s[:, j + 1]))
                clamped = (t1 != t + s[:, j]) | (t2_ != t + (s[:, j] + s[:, j + 1]))
                SATURATED += int(np.count_nonzero(clamped & ~edge))
                b = np.maximum(b, np.maximum(t1, t2_))
                t = t2_
            T[live], best[live] = t, b
            walked[live] += 16
            live = live[b - t <= P.xdrop]            # the others have dropped: their best stands
            if not live.size:
                break
        capped = walked[live] + 10 >= P.long_cap
        fwd[live[capped]] = True
        live = live[~capped]
    return best, fwd, walked


SATURATED = 0      # pair steps of packed_side that left int16 and were clamped although their 16 bases hold no separator and lie inside
                   # the query block, since the module was loaded (behind the query's end every base scores against code 7)


def level2(tc, qc, sub_mat, rec, P, from_anchor=False):
    """the records `rec` (L2REC) through the packed walk -> dict of per-record arrays: cand, forward, bestR, bestL and endR, endL (the
    bases walked when the side ended; 0: not walked).  from_anchor: every record as flags 3 (the
    model of a call without context table, where every hit of the call is walked from its anchor)"""
    t2 = IM.two_bit(np.asarray(tc, np.uint8))
    q7 = np.asarray(qc, np.uint8) & 7
    sm = pair_matrix(sub_mat)
    n = rec.size
    ref_loc, query_loc = rec["ref_loc"].astype(np.int64), rec["query_loc"].astype(np.int64)
    flags = np.full(n, 3) if from_anchor else ((rec["meta"] >> 16) & 3).astype(np.int64)
    known = (rec["meta"] & 0xFFFF).astype(np.int64)
    sT = (rec["state"] >> 16).astype(np.int16).astype(np.int64)
    sB = (sT + (rec["state"] & 0xFFFF).astype(np.int64)).astype(np.int16).astype(np.int64)    # T + D, kept as int16
    bestR, bestL = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    forward = np.zeros(n, dtype=bool)
    endR, endL = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    skip = (ref_loc > len(tc)) | (query_loc > len(qc))
    if P.rm_window is not None:
        skip |= ~((ref_loc >= P.rm_window[0]) & (ref_loc <= P.rm_window[1]))
    # right side: flags 1 and 3 (flags 2: known)
    resume_r = (flags == 1) & bool(P.l2_right_state)
    bestR[flags == 2] = known[flags == 2]
    for sel, w0, t0, b0 in ((~skip & (flags != 2) & ~resume_r, 0, 0, 0), (~skip & resume_r, R_BASES, sT, sB)):
        i = np.flatnonzero(sel)
        if i.size:
            pick = (lambda v: v[i] if isinstance(v, np.ndarray) else v)
            bestR[i], forward[i], endR[i] = packed_side(t2, q7, sm, ref_loc[i], query_loc[i], False, w0, pick(t0), pick(b0), P)
    # left side: what is not forwarded yet; flags 1: known
    bestL[flags == 1] = known[flags == 1]
    open_l = ~skip & ~forward
    for sel, w0, t0, b0 in ((open_l & (flags == 3), 0, 0, 0), (open_l & (flags == 2), L_BASES + P.left_skip, sT, sB)):
        i = np.flatnonzero(sel)
        if i.size:
            pick = (lambda v: v[i] if isinstance(v, np.ndarray) else v)
            bestL[i], f, endL[i] = packed_side(t2, q7, sm, ref_loc[i], query_loc[i], True, w0, pick(t0), pick(b0), P)
            forward[i] |= f
    bestR[skip], bestL[skip] = 0, 0
    return dict(cand=forward | (bestR + bestL >= P.hspthresh), forward=forward, bestR=bestR, bestL=bestL, endR=endR, endL=endL, flags=flags)


def hits_as_records(ref_loc, query_loc):
    rec = np.zeros(len(ref_loc), dtype=L2REC)
    rec["ref_loc"], rec["query_loc"], rec["hidx"] = ref_loc, query_loc, np.arange(len(ref_loc))
    rec["meta"] = 3 << 16
    return rec


def alive_shares(cls, xdrop, lengths, n=1 << 20, seed=1):
    """the share of uniform random flanks (classes 0 .. 3 equally likely) on which the stated walk, from T = 0, is alive after `length`
    bases: never more than xdrop below its best at the end of a six-base field, or at the end of the walk"""
    x = np.random.default_rng(seed).integers(0, 4, (n, max(lengths)))
    s = np.asarray(cls, dtype=np.int64)[x]
    T = np.cumsum(s, axis=1)
    N = T - np.maximum(np.maximum.accumulate(T, axis=1), 0)
    out = {}
    for L in lengths:
        ends = sorted(set(range(5, L, 6)) | {L - 1})
        out[L] = float(np.mean(N[:, ends].min(axis=1) >= -xdrop))
    return out


# ---- a whole call -----------------------------------------------------------------------------------------------------------------------
class Verdicts:
    """what a call must report: .forwards (L2REC sorted by hidx; None without context table), .cand (the candidates' (ref_loc, query_loc)),
    .audit (the rejected hits' pairs, both levels), .num_hits"""


def pairs(ref_loc, query_loc):
    a = np.stack([np.asarray(ref_loc, np.int64), np.asarray(query_loc, np.int64)], axis=1)
    return a[np.lexsort((a[:, 1], a[:, 0]))] if a.size else a.reshape(0, 2)


def call(table, tc, qc, oc, sub_mat, start, end, P, ctx=True, detail=False):
    v = Verdicts()
    ref_loc, query_loc = call_hits(table, qc, start, end)
    v.num_hits = int(ref_loc.size)
    if ctx:
        cls = IM.class_scores(sub_mat, IM.presence(tc), IM.presence(qc))
        v.cls = cls
        v.l1 = level1(tc, qc, oc, ref_loc, query_loc, cls, P, detail=detail)
        v.forwards = forwards(v.l1)
        v.l2 = level2(tc, qc, sub_mat, v.forwards, P)
        cand = v.l2["cand"]
        rej1 = ~v.l1["fwd"] & ~v.l1["skip"]
        rej = np.concatenate([pairs(ref_loc[rej1], query_loc[rej1]), pairs(v.forwards["ref_loc"][~cand], v.forwards["query_loc"][~cand])])
        v.cand = pairs(v.forwards["ref_loc"][cand], v.forwards["query_loc"][cand])
    else:
        v.forwards = None
        v.l2 = level2(tc, qc, sub_mat, hits_as_records(ref_loc, query_loc), P, from_anchor=True)
        cand = v.l2["cand"]
        rej = pairs(ref_loc[~cand], query_loc[~cand])
        v.cand = pairs(ref_loc[cand], query_loc[cand])
    v.audit = pairs(rej[:, 0], rej[:, 1])
    return v
