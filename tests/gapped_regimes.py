"""Hand-built inputs that put the gapped kernels (gapped.hip) into regimes the sampled-HSP tests never reach, shared by
tests/test_gapped_regimes.py (CPU: each input is shown, on the serial checkers alone, to be in the regime it claims) and
tests/test_gpu_gapped_regimes.py (GPU: every field against the checkers on those inputs).

  A  every kernel instance K = 2, 4, 8, 17, 33 with sides longer than 64 K + 192 target bases: the window base moves, the X stream is
     refilled, the trace holds moved window bases; and paths on which i << j and i >> j.
  B  low-complexity inputs on which the live band grows to a tuned width and stays there while the window moves: the smallest
     max_band that does not cap is exactly 64 K - 1 (the candidate range may be as wide as the window) for K = 2, 4, 8, 17.
  C  single gap runs of 70, 130 and 300 bases: longer than one, two and four stages of the walk kernel.
  D  a unit matrix and cheap gaps: equal scores everywhere, so the tie rules decide best cells and paths.

What A does not reach: its live band is 91 to 165 cells wide at every K (min_uncapped_band gives 163 at K = 4, 8, 17 and 165 at K = 33:
5 of 64 lanes at K = 33), so A is the "window moves, streams refilled" half of the regime only.  The window-wide bands are B's; B also
runs continuation pieces and the greedy entry on them (b_pieces_params).

The contract's second band-cap rule -- the candidates of d span more than max_band + 1 values of i -- has no input here because it
cannot fire before the first rule does.  With L1 = [lo1, hi1], L2 = [lo2, hi2] the live ranges of d - 1 and d - 2, the candidates of d
are [min(lo1, lo2 + 1), max(hi1, hi2) + 1].  Taken from one range alone they span at most its width + 1 <= max_band + 1.  Taken from
both (say hi1 + 1 and lo2 + 1): L1 lies inside the candidates of d - 1, so hi1 <= max(hi2, hi3) + 1; if hi1 <= hi2 + 1 the span is at
most the width of L2 plus 1, otherwise hi1 <= hi3 + 1 and the span hi1 - lo2 + 1 is at most that of the candidates of d - 2, which hold
both hi3 + 1 and lo2; the mirrored case likewise.  So span(d) <= max(max_band + 1, span(d - 2)), spans start at 2, and clamping to
max_extent only shrinks them: while every live range is at most max_band wide the rule is unreachable (max_band >= 1).

All anchors are SEG_DTYPE rows with len = 0 on blocks of a few kbp; nothing here needs the seeding stage."""
import functools

import numpy as np

import gapped_model as G
import gapped_pieces_model as PM
import gapped_trace_model as T

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
AMP = np.frombuffer(b"&", dtype=np.uint8)


def cells_per_lane(max_band):
    """K of the kernel instance a band runs in (gapped_cells_per_lane of gapped.hip)."""
    return next(k for k in (2, 4, 8, 17, 33) if 64 * k >= max_band + 1)


def unit_sub():
    """+1 on the A C G T diagonal, -1 off it, every other entry as in gapped_model.SUB."""
    m = G.SUB.reshape(8, 8).copy()
    m[:4, :4] = np.where(np.eye(4, dtype=bool), 1, -1)
    return m.reshape(64)


UNIT = unit_sub()


def random_dna(n, seed):
    return _ACGT[np.random.default_rng(seed).integers(0, 4, size=n)]


def ascii_of(s):
    return np.frombuffer(s.encode(), dtype=np.uint8).copy()


def join(recs):
    parts = []
    for k, r in enumerate(recs):
        parts += ([AMP] if k else []) + [r]
    return np.concatenate(parts)


def offsets(recs):
    """Block offset of each record of join(recs)."""
    out, p = [], 0
    for r in recs:
        out.append(p)
        p += r.size + 1
    return out


def anchors(points):
    """SEG_DTYPE rows with len = 0 at (target, query) points; the scores shuffle the greedy priority order."""
    h = np.zeros(len(points), dtype=G.SEG_DTYPE)
    for k, (r, q) in enumerate(points):
        h[k] = (r, q, 0, 3000 + (k * 7919) % 5000)
    return h


def diverge(seq, seed, sub_rate, indel_every=0, max_indel=1, kinds="ID", jitter=True):
    """A diverged copy of seq and, per base of seq, its position in the copy (for a deleted base: where it would be).  Substitutions
    by a different base at sub_rate; every indel_every bases (jittered by half unless jitter is off) an insertion or a deletion, the
    kind drawn from `kinds`, of 1 .. max_indel bases (exactly max_indel when jitter is off)."""
    rng = np.random.default_rng(seed)
    n = seq.size
    idx = np.searchsorted(_ACGT, seq)
    sub = rng.random(n) < sub_rate
    new = _ACGT[(idx + rng.integers(1, 4, size=n)) % 4]
    base = np.where(sub, new, seq)
    out, pos, i, q = [], np.zeros(n, dtype=np.int64), 0, 0

    def gap():
        return int(rng.integers(indel_every // 2, indel_every * 3 // 2 + 1)) if jitter else indel_every
    nxt = gap() if indel_every else n + 1
    while i < n:
        if i == nxt:
            k = int(rng.integers(1, max_indel + 1)) if jitter else max_indel
            if kinds[int(rng.integers(0, len(kinds)))] == "I":
                out.append(_ACGT[rng.integers(0, 4, size=k)])
                q += k
            else:
                k = min(k, n - i)
                pos[i:i + k] = q
                i += k
            nxt = i + gap()
            continue
        e = min(n, nxt)
        out.append(base[i:e])
        pos[i:e] = q + np.arange(e - i)
        q += e - i
        i = e
    return np.concatenate(out), pos


class Block:
    """One target block and one query block (ascii), their codes and the matrix the engine is started with."""

    def __init__(self, target, query, sub=G.SUB):
        self.target, self.query, self.sub = target, query, sub
        self.tc, self.qc = PM.encode(target), PM.encode(query)


def sides(b, hsps, **kw):
    """[(best, best_i, best_j, cells, flags)] of the checker: left and right side of every anchor."""
    out = []
    for r, q, ln, _ in hsps.tolist():
        for d in (-1, +1):
            out.append(G.side(b.tc, b.qc, b.sub, r + ln // 2, q + ln // 2, d, **kw))
    return out


# ---- A: every instance with a moving window ---------------------------------------------------------------------------------------

A_BANDS = {2: 100, 4: 200, 8: 400, 17: 1024, 33: 2048}
A_LEN = 13_000  # each side of a middle anchor has 6500 bases: two full pieces and a short one at the widest instance


def a_extent(K):
    return max(64 * K + 600, 3000 if K == 33 else 0)


@functools.lru_cache(maxsize=None)
def block_a():
    """-> (Block, anchors).  Target: one record of 13 kbp.  Query: four copies of it in four records -- two diverged ones (5 % and 8 %
    substitutions, indels of 1-10 bases), one that gained 30 bases every 200 (i << j along the path) and one that lost 30 every 200
    (i >> j).  Two anchors per copy near the middle."""
    t = random_dna(A_LEN, 7001)
    copies = [diverge(t, 7002, 0.05, 300, 10), diverge(t, 7003, 0.08, 500, 10), diverge(t, 7004, 0.02, 200, 30, "I", jitter=False),
              diverge(t, 7005, 0.02, 200, 30, "D", jitter=False)]
    off = offsets([c for c, _ in copies])
    pts = []
    for k, (_, pos) in enumerate(copies):
        for p in (A_LEN // 2 - 190 + 60 * k, A_LEN // 2 + 115 + 45 * k):
            pts.append((p, off[k] + int(pos[p])))
    return Block(t, join([c for c, _ in copies])), anchors(pts)


def a_params(K):
    """HOXD70 defaults -- except ydrop at K = 2: under the default 9430 the live band of these sequences is wider than 100 and every
    side ends at the band cap after 49 bases (measured with the checker), so the narrowest instance gets ydrop 4000, under which no
    side caps and a 30-base gap (1300) still survives."""
    return dict(max_band=A_BANDS[K], max_extent=a_extent(K), **({"ydrop": 4000} if K == 2 else {}))


# ---- B: tight windows ---------------------------------------------------------------------------------------------------------------

B_LEN, B_EXTENT = 6000, 2500
# (gap_open, gap_extend, ydrop) under which the smallest max_band that does not cap is exactly the key, found by bisecting ydrop with
# the checker (tune_b below; `python tests/gapped_regimes.py` prints them again).  Record 0 is the homopolymer, record 1 the repeat.
B_TUNED = {
    ("homo", 127): (0, 30, 9422),
    ("homo", 255): (0, 10, 14006),
    ("homo", 511): (0, 5, 25664),
    ("homo", 1087): (0, 1, 50408),
    ("rep", 127): (0, 30, 1807),
    ("rep", 255): (0, 10, 3839),
    ("rep", 511): (0, 5, 10589),
    ("rep", 1087): (0, 1, 34864),
}
B_WIDE = {"homo": (0, 1, 80000), "rep": (0, 1, 80000)}  # bands 1723 and 1950 wide (min_uncapped_band), run at max_band 2048


@functools.lru_cache(maxsize=None)
def block_b():
    """-> (Block, {"homo": anchor, "rep": anchor}).  Record 0: A^6000 against itself (a band symmetric about the diagonal).  Record 1: a
    period-5 repeat with 5 % substitutions against another such copy (a band that is not).  One anchor in the middle of each."""
    homo = ascii_of("A" * B_LEN)
    tile = np.tile(ascii_of("ACGTT"), B_LEN // 5)
    x, _ = diverge(tile, 7101, 0.05)
    y, _ = diverge(tile, 7102, 0.05)
    b = Block(join([homo, x]), join([homo, y]))
    return b, {"homo": anchors([(B_LEN // 2, B_LEN // 2)]), "rep": anchors([(B_LEN + 1 + B_LEN // 2, B_LEN + 1 + B_LEN // 2)])}


def b_params(name, width):
    o, e, y = B_TUNED[(name, width)] if (name, width) in B_TUNED else B_WIDE[name]
    return dict(gap_open=o, gap_extend=e, ydrop=y, max_extent=B_EXTENT)


# Continuation pieces and greedy on window-wide bands: (record, width) -> max_extent.  Each piece is a fresh extension, so on the
# homopolymer every piece grows the same band again: exactly `width` wide (measured from the origin of piece 1), three pieces per side.
# On the repeat the band of a 1200-base piece is 385 wide: not tight, but wider than the window of the next smaller instance.
B_PIECES = {("homo", 127): 1200, ("homo", 255): 1200, ("homo", 511): 1200, ("homo", 1087): 1400, ("rep", 511): 1200}


def b_pieces_params(name, width):
    return dict(b_params(name, width), max_extent=B_PIECES[(name, width)], max_band=width)


def b_pieces_anchors(name):
    """The record's middle anchor and a second one of lower score that greedy finds covered: 100 bases up the diagonal on the
    homopolymer (its path is the diagonal), the same point again on the repeat (whose path leaves the diagonal)."""
    _, anc = block_b()
    r, q = int(anc[name][0]["ref_start"]), int(anc[name][0]["query_start"])
    step = 100 if name == "homo" else 0
    h = anchors([(r, q), (r + step, q + step)])
    h["score"] = (9000, 4000)
    return h


def capped(b, hsps, **kw):
    return any(s[4] & G.BAND_CAP for s in sides(b, hsps, **kw))


def min_uncapped_band(b, hsps, **kw):
    """The smallest max_band at which no side of the anchors ends at the band cap (2049: none)."""
    lo, hi = 1, 2049
    while lo < hi:
        mid = (lo + hi) // 2
        if mid <= 2048 and not capped(b, hsps, max_band=mid, **kw):
            hi = mid
        else:
            lo = mid + 1
    return lo


def tune_b(name, width, gap_open, gap_extend, y_lo=100, y_hi=200_000):
    """The smallest ydrop at which max_band = width - 1 caps, if max_band = width does not cap there; else None."""
    b, anc = block_b()
    kw = dict(gap_open=gap_open, gap_extend=gap_extend, max_extent=B_EXTENT)
    while y_lo < y_hi:
        mid = (y_lo + y_hi) // 2
        if capped(b, anc[name], max_band=width - 1, ydrop=mid, **kw):
            y_hi = mid
        else:
            y_lo = mid + 1
    return None if capped(b, anc[name], max_band=width, ydrop=y_lo, **kw) else y_lo


# ---- C: gap runs longer than a walk stage ------------------------------------------------------------------------------------------

C_PARAMS = dict(gap_open=400, gap_extend=5)
# K = 2: under C_PARAMS the band is wider than 100, and max_band = 100 is too narrow for a 130-base gap anyway; the 70-base records
# cross their gaps at the default penalties with ydrop 2900 (gap cost 2500) without reaching the cap
C_PARAMS_K2 = dict(gap_open=400, gap_extend=30, ydrop=2900, max_band=100)
C_K2_RECORDS = (0, 1, 6)
C_LENGTHS = (70, 130, 300)
C_FLANK, C_FAR = 450, 500
C_STAGE_FAR = 510  # far flank of the stage-boundary record, found by stage_far() below


def c_record(seed, left, right, far_right=C_FAR):
    """One record pair: far flank, left gap, flank, ANCHOR, flank, right gap, far flank.  left / right: (kind, length), kind "I" (the
    query has the extra bases) or "D" (the target has them).  -> (target record, query record, anchor offsets in them)."""
    rng = np.random.default_rng(seed)
    parts = [random_dna(n, seed * 10 + k) for k, n in enumerate((C_FAR, C_FLANK, C_FLANK, far_right))]
    qparts = [diverge(p, seed * 10 + 5 + k, 0.02)[0] for k, p in enumerate(parts)]
    extra = [_ACGT[rng.integers(0, 4, size=left[1])], _ACGT[rng.integers(0, 4, size=right[1])]]
    t = [parts[0]] + ([extra[0]] if left[0] == "D" else []) + parts[1:3] + ([extra[1]] if right[0] == "D" else []) + [parts[3]]
    q = [qparts[0]] + ([extra[0]] if left[0] == "I" else []) + qparts[1:3] + ([extra[1]] if right[0] == "I" else []) + [qparts[3]]
    at = C_FAR + (left[1] if left[0] == "D" else 0) + C_FLANK
    aq = C_FAR + (left[1] if left[0] == "I" else 0) + C_FLANK
    return np.concatenate(t), np.concatenate(q), at, aq


@functools.lru_cache(maxsize=None)
def block_c():
    """-> (Block, anchors, planted): one record per length and arrangement (I left / D right, D left / I right), then the record
    whose right-side I run begins at a stage boundary of the walk.  planted[k] = ((left kind, length), (right kind, length))."""
    recs, planted = [], []
    for n, ln in enumerate(C_LENGTHS):
        for m, (a, b) in enumerate((("I", "D"), ("D", "I"))):
            planted.append(((a, ln), (b, ln)))
            recs.append(c_record(7200 + 2 * n + m, *planted[-1]))
    planted.append((("D", 70), ("I", 70)))
    recs.append(c_record(7290, *planted[-1], far_right=C_STAGE_FAR))
    to, qo = offsets([r[0] for r in recs]), offsets([r[1] for r in recs])
    b = Block(join([r[0] for r in recs]), join([r[1] for r in recs]))
    return b, anchors([(to[k] + r[2], qo[k] + r[3]) for k, r in enumerate(recs)]), planted


def gap_runs(ops_walk, dstar):
    """[(kind, length, antidiagonal of the run's first cell in walk order)] of the I and D runs of one side's ops in walk order."""
    out, d = [], dstar
    for x in ops_walk.tolist():
        ln, op = x >> 2, x & 3
        if op != T.OP_M:
            out.append(("I" if op == T.OP_I else "D", ln, d))
        d -= 2 * ln if op == T.OP_M else ln
    return out


def stage_far():
    """The far-flank length >= 500 at which the right side's I run of the last record of C begins at a stage boundary."""
    for far in range(500, 600):
        t, q, at, aq = c_record(7290, ("D", 70), ("I", 70), far_right=far)
        res, ops, _ = T.side(PM.encode(t), PM.encode(q), G.SUB, at, aq, +1, **C_PARAMS)
        if any(k == "I" and ln == 70 and (res[1] + res[2] - d) % 64 == 0 for k, ln, d in gap_runs(ops, res[1] + res[2])):
            return far
    return None


# ---- D: ties ----------------------------------------------------------------------------------------------------------------------

D_EXTENT = 400
D_PREFIXES = (0, 1, 5, 30, 62, 63, 64, 65, 126, 127, 128, 129, 190, 255, 256, 300, 390)


@functools.lru_cache(maxsize=None)
def block_d():
    """-> (Block under the unit matrix, [(name, anchors, parameters)]).
    "mixed": random sequence and period-3 / period-7 repeats against copies with 10 % substitutions and 1-base indels about every 40,
    at gap_open 0 and 1, gap_extend 1, ydrop 12, default band and K = 2.
    "tiles": records reverse(P1 GA) | P2 GA against reverse(P1 AG) | P2 AG with the anchor at the bar and free gaps: on each side the
    maximum |P| + 1 is reached on one antidiagonal by two cells (one base of the transposition skipped, the other matched) and
    never again, so the best cell is decided by the smallest-i rule alone; |P| runs over lanes and, at K = 2, past the window."""
    trecs, qrecs, pts_mixed = [], [], []
    srcs = [random_dna(2400, 7301), np.tile(ascii_of("ACG"), 400), np.tile(ascii_of("ACGTTGA"), 200)]
    for k, s in enumerate(srcs):
        x, _ = diverge(s, 7310 + k, 0.05) if k else (s, None)
        y, pos = diverge(x, 7320 + k, 0.10, 40, 1)
        trecs.append(x)
        qrecs.append(y)
        pts_mixed.append([(p, int(pos[p])) for p in np.linspace(450, x.size - 450, 4).astype(int)])
    n_mixed = len(trecs)
    rng = np.random.default_rng(7330)
    pairs = list(zip(D_PREFIXES, D_PREFIXES[::-1]))
    for p1, p2 in pairs:
        P1, P2 = _ACGT[rng.integers(0, 4, size=p1)], _ACGT[rng.integers(0, 4, size=p2)]
        trecs.append(np.concatenate([ascii_of("AG"), P1[::-1], P2, ascii_of("GA")]))
        qrecs.append(np.concatenate([ascii_of("GA"), P1[::-1], P2, ascii_of("AG")]))
    to, qo = offsets(trecs), offsets(qrecs)
    b = Block(join(trecs), join(qrecs), UNIT)
    mixed = anchors([(to[k] + r, qo[k] + q) for k in range(n_mixed) for r, q in pts_mixed[k]])
    tiles = anchors([(to[n_mixed + k] + 2 + p1, qo[n_mixed + k] + 2 + p1) for k, (p1, _) in enumerate(pairs)])
    sets = []
    for o in (0, 1):
        for band in (0, 100):
            sets.append(("mixed", mixed, dict(gap_open=o, gap_extend=1, ydrop=12, max_extent=D_EXTENT, max_band=band)))
    for band in (0, 100):
        sets.append(("tiles", tiles, dict(gap_open=0, gap_extend=0, ydrop=12, max_extent=D_EXTENT, max_band=band)))
    return b, sets


def variant_changes(b, hsps, variant, **kw):
    """(sides whose best cell differs, sides whose path differs, sides) between the path checker and its mutated build `variant`."""
    cell = path = n = 0
    kw = dict(kw, max_extent=kw.get("max_extent") or G.DEFAULT_EXTENT, max_band=kw.get("max_band") or G.DEFAULT_BAND)
    for r, q, ln, _ in hsps.tolist():
        for d in (-1, +1):
            res0, ops0, _ = T.side(b.tc, b.qc, b.sub, r + ln // 2, q + ln // 2, d, **kw)
            res1, ops1, _ = T.side(b.tc, b.qc, b.sub, r + ln // 2, q + ln // 2, d, variant=variant, **kw)
            n += 1
            cell += res0[1:3] != res1[1:3]
            path += not np.array_equal(ops0, ops1)
    return cell, path, n


if __name__ == "__main__":  # re-derive the tuned constants
    for name in ("homo", "rep"):
        for width, tries in ((127, ((0, 30), (0, 29), (0, 31), (0, 28))), (255, ((0, 10), (0, 11), (0, 9), (0, 12))),
                             (511, ((0, 5), (0, 4), (0, 6))), (1087, ((0, 1), (0, 2)))):
            for o, e in tries:
                y = tune_b(name, width, o, e)
                if y is not None:
                    print('    ("%s", %d): (%d, %d, %d),' % (name, width, o, e, y))
                    break
            else:
                print("no parameters found for", name, width)
    print("C_STAGE_FAR =", stage_far())
