"""Hand-built inputs that put the cover index of sa_gapped_align_greedy (cover.hip and the greedy loop of api_gapped.hip)
into named regimes, shared by tests/test_gapped_cover_regimes.py (CPU: each input is shown, on the serial checkers alone, to be in the
regime it names) and tests/test_gpu_gapped_cover_regimes.py (GPU: the engine against the sequential rule on those inputs).

  ends     one alignment with I and D runs on both sides, and probe anchors at the first and last pair of a run, just before it, at its
           exclusive end, on the neighbouring diagonals and inside the gap runs: a segment covers [t_begin, t_end) of one diagonal.
  carry    sides of more than 128 runs, probes on a run of each 64-run chunk of cover_emit_kernel's walk and next to it; and sides of
           exactly 63, 64 and 65 runs.
  nesting  two accepted paths that join the same diagonal, so index entries share a key and nest: the running maximum answers
           "covered" where the last entry's own t_end would not.
  merge    four alignments accepted in four batches whose segments interleave with, and repeat keys of, the resident index.
  ladder   140 anchors of which each covers the next: returned, covered, returned, ... in a dependency chain over three 64-survivor
           rounds of cover_resolve_kernel; and its mirror image.
  fans     a survivor with 100 in-edges of which none, or exactly one, comes from an accepted survivor.
  thresh   alignments below gappedthresh: they cover nothing, and "covered" takes precedence over "below threshold".
  ties     equal scores: the lower input index wins, among duplicates and among distinct anchors on each other's paths.
  gapanc   an anchor whose side begins with a gap run, so that the anchor point is no M pair of its own path: only the unit segment at
           the anchor covers its duplicate.

The index model (segments, Index) restates cover.hip's data structure in Python: per accepted record one segment (diag, t_begin, t_end)
per M run of the left ops, one per M run of the right ops (the two sides are emitted separately, so runs that meet at the anchor are not
merged) and one unit segment at the anchor.  That is what trace_emit and cover_select_kernel count with continuation pieces off: every
run of a traced side gets a slot, the M runs a key, cover_work appends the unit segment per eligible survivor, and cover_select_kernel
keeps the keyed slots of the accepted ones; CoverIndex::merge adds that number to cover_segments.  So cover_segments equals
segment_count() below.  Index.covered is the running-maximum rule; Index.covered_own_end is the deliberately wrong rule "the last entry
with key <= the point, by its own t_end", used only to show that an input tells the two apart.

All rows have len > 0 of both parities, so the anchor start + len // 2 differs from the start."""
import functools

import numpy as np

import gapped_greedy_model as GR
import gapped_model as G
import gapped_regimes as R
import gapped_trace_model as T

_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGT&")] = list(b"TGCA&")


def revcomp(seq):
    """The ascii reverse complement: uploaded as the query, its reverse strand is seq."""
    return _COMP[seq[::-1]].copy()


def rows(points, scores):
    """SEG_DTYPE rows whose anchors (start + len // 2) are the points; lengths 18 .. 24, both parities."""
    h = np.zeros(len(points), dtype=G.SEG_DTYPE)
    for k, ((r, q), s) in enumerate(zip(points, scores)):
        ln = 18 + (5 * k) % 7
        ln = min(ln, 2 * min(r, q))
        h[k] = (r - ln // 2, q - ln // 2, ln, s)
    return h


class Regime:
    """One input: block, HSP rows, the call's parameters (gappedthresh among them) and what the construction wants to remember."""

    def __init__(self, block, hsps, kw, **meta):
        self.block, self.hsps, self.kw, self.meta = block, hsps, dict(kw), meta
        self._want = None

    @property
    def thresh(self):
        return self.kw.get("gappedthresh", 3000)

    def checker_kw(self):
        return {k: v for k, v in self.kw.items() if k != "gappedthresh"}

    def raw(self):
        """Every HSP's own record and path (the checker's sa_gapped_align raw mode)."""
        if self._want is None:
            b = self.block
            recs, paths = T.align(b.tc, b.qc, b.sub, self.hsps, **self.checker_kw())
            self._want = (recs, paths, GR.greedy(self.hsps, recs, paths, self.thresh))
        return self._want[:2]

    def want(self):
        """-> (records, paths, stats with "state") of the sequential rule."""
        self.raw()
        return self._want[2]

    def cover_of(self, k):
        recs, paths = self.raw()
        return GR.cover_set(recs[k], np.concatenate(paths[k][:2]), GR.anchor(self.hsps[k]))

    def anchors(self):
        return [GR.anchor(x) for x in self.hsps]


# ---- the index model ------------------------------------------------------------------------------------------------------------------

def m_runs(t, q, ops):
    """[(t_begin, q_begin, length)] of the M runs of ops walked from (t, q), and the end point."""
    out = []
    for x in ops.tolist():
        ln, op = x >> 2, x & 3
        if op == T.OP_M:
            out.append((t, q, ln))
            t += ln
            q += ln
        elif op == T.OP_I:
            q += ln
        else:
            t += ln
    return out, (t, q)


def segments(rec, path, a):
    """[(t - q, t_begin, t_end)] of one accepted record: the M runs of its left ops, of its right ops, and the unit segment at a."""
    lo, ro, _ = path
    left, mid = m_runs(int(rec["ref_start"]), int(rec["query_start"]), lo)
    right, end = m_runs(mid[0], mid[1], ro)
    assert mid == a and end == (int(rec["ref_end"]), int(rec["query_end"]))
    return [(t - q, t, t + ln) for t, q, ln in left + right] + [(a[0] - a[1], a[0], a[0] + 1)]


def accepted_segments(reg, members=None):
    """The segments of the accepted HSPs (or of those in `members`), unsorted."""
    recs, paths = reg.raw()
    state = reg.want()[2]["state"]
    out = []
    for k in (range(reg.hsps.size) if members is None else members):
        if state[k] == 1:
            out += segments(recs[k], paths[k], GR.anchor(reg.hsps[k]))
    return out


def segment_count(reg):
    """cover_segments of a call with continuation pieces off."""
    return len(accepted_segments(reg))


class Index:
    """Accepted segments sorted by (diagonal, t_begin).  Entries of equal key have no defined order in the engine (the order of an
    atomic compaction, kept by a stable sort; across batches resident entries come first), so the wrong rule is asked with the order
    that suits it least."""

    def __init__(self, segs):
        self.e = sorted(segs)

    def keys(self):
        return [(d, tb) for d, tb, _ in self.e]

    def _upto(self, pt):
        d, t = pt[0] - pt[1], pt[0]
        return [x for x in self.e if (x[0], x[1]) <= (d, t)], d, t

    def covered(self, pt):
        """The running maximum of t_end over the point's diagonal up to the last entry with key <= the point."""
        le, d, t = self._upto(pt)
        return bool(le) and le[-1][0] == d and max(x[2] for x in le if x[0] == d) > t

    def covered_own_end(self, pt):
        """WRONG on purpose: the own t_end of the last entry with key <= the point -- of equal keys the one with the smallest t_end."""
        le, d, t = self._upto(pt)
        if not le or le[-1][0] != d:
            return False
        return min(x[2] for x in le if x[:2] == le[-1][:2]) > t


def batches(reg, B):
    """HSP indices per priority batch of size B."""
    pi = GR.priority(reg.hsps)
    return [pi[k:k + B] for k in range(0, len(pi), B)]


def genome_runs(reg, k):
    """[(side, walk index, op, length, t, q)] of HSP k's path in genome order.  Walk order runs from the far end to the origin on both
    sides: the left ops are in walk order, the right ops reversed."""
    recs, paths = reg.raw()
    lo, ro, _ = paths[k]
    t, q = int(recs[k]["ref_start"]), int(recs[k]["query_start"])
    out = []
    for side, ops in (("L", lo), ("R", ro)):
        for n, x in enumerate(ops.tolist()):
            ln, op = x >> 2, x & 3
            out.append((side, n if side == "L" else ops.size - 1 - n, op, ln, t, q))
            t += ln if op != T.OP_I else 0
            q += ln if op != T.OP_D else 0
    return out


# ---- ends: exclusive run end, neighbouring points, gap interiors ----------------------------------------------------------------------

ENDS_KW = dict(max_extent=700)


def _run_probes(runs, n, tag):
    """Probes around M run n of `runs` (genome order): name -> point."""
    side, _, op, ln, t, q = runs[n]
    assert op == T.OP_M and ln >= 4
    p = {"first": (t, q), "last": (t + ln - 1, q + ln - 1), "before": (t - 1, q - 1), "end": (t + ln, q + ln),
         "first_up": (t, q + 1), "first_down": (t, q - 1), "last_up": (t + ln - 1, q + ln), "last_down": (t + ln - 1, q + ln - 2),
         "end_up": (t + ln, q + ln + 1), "end_down": (t + ln, q + ln - 1)}
    return {"%s_%s" % (tag, k): v for k, v in p.items()}


def _gap_probe(runs, n):
    """A point strictly inside the rectangle a gap run of three bases spans, on a diagonal strictly between those of the M runs on
    either side of it, and none of the run probes."""
    _, _, op, ln, t, q = runs[n]
    assert op != T.OP_M and ln >= 3
    return (t - 1, q + 1) if op == T.OP_I else (t + 1, q)


@functools.lru_cache(maxsize=None)
def ends(part):
    """A 5 kbp target against a copy with 1 % substitutions and a 3-base insertion or deletion every 150 bases; the main anchor in the
    middle, max_extent 700.  part "runs": probes around an M run between an I and a D run, on the left and on the right side.
    part "path": probes around the path's first and last pair; the two points past the path's ends come first among them, since their
    own alignments run along the main path beyond its extent, where any other probe's alignment would cover them.  (The parts are two
    calls because those two alignments pass over the left side's runs in the other direction and place a gap run elsewhere.)
    meta["probes"]: name -> (HSP index, in the main alignment's cover set?)."""
    t = R.random_dna(5000, 7401)
    q, pos = R.diverge(t, 7402, 0.01, 150, 3, "ID", jitter=False)
    b = R.Block(t, q)
    main = (2500, int(pos[2500]))
    one = Regime(b, rows([main], [9000]), ENDS_KW)
    runs = genome_runs(one, 0)
    cover = one.cover_of(0)
    pts = {}
    for side in ("LR" if part == "runs" else ""):
        idx = [n for n, r in enumerate(runs) if r[0] == side]
        # an M run between an I run and a D run, away from the anchor and the far end
        mid = [n for n in idx[1:-1] if runs[n][2] == T.OP_M and {runs[n - 1][2], runs[n + 1][2]} == {T.OP_I, T.OP_D}
               and runs[n - 1][0] == runs[n + 1][0] == side]
        n = mid[len(mid) // 2]
        pts.update(_run_probes(runs, n, side))
        for g in (n - 1, n + 1):
            pts["%s_in_%s" % (side, "I" if runs[g][2] == T.OP_I else "D")] = _gap_probe(runs, g)
    first = next(n for n, r in enumerate(runs) if r[2] == T.OP_M)
    last = max(n for n, r in enumerate(runs) if r[2] == T.OP_M)
    f, e = _run_probes(runs, first, "path"), _run_probes(runs, last, "path")
    if part == "path":
        for k in ("first", "before", "first_up", "first_down"):
            pts["path_" + k] = f["path_" + k]
        for k in ("last", "end", "last_up", "last_down", "end_up", "end_down"):
            pts["path_" + k] = e["path_" + k]
    assert len(set(pts.values())) == len(pts)
    names = sorted(pts, key=lambda n: (n not in ("path_before", "path_end"), n))
    h = rows([main] + [pts[n] for n in names], [9000] + [8000 - 7 * k for k in range(len(names))])
    probes = {n: (1 + k, pts[n] in cover) for k, n in enumerate(names)}
    return Regime(b, h, ENDS_KW, probes=probes, runs=runs)


# ---- carry: more than 128 runs a side ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def carry_block(gap=False):
    """gap: the anchor at a deleted target base, so that the right side begins with a D run and has an even number of runs."""
    t = R.random_dna(7000, 7411)
    q, pos = R.diverge(t, 7412, 0.0, 12, 1, "ID", jitter=False)
    x = 3500
    while gap and not (pos[x] == pos[x + 1] and pos[x - 1] < pos[x]):
        x += 1
    return R.Block(t, q), (x, int(pos[x]))


@functools.lru_cache(maxsize=None)
def carry(max_extent=1100, chunks=(0, 1, 2), gap=False):
    """A copy with a 1-base insertion or deletion every 12 bases (default matrix): about 180 runs a side at max_extent 1100.  Per side
    and per 64-run chunk of the walk order a probe on the first pair of an M run (covered) and one on the diagonal point before it (in
    the gap run: not covered).  On each side the probes nearest the anchor come first in priority: a probe's own alignment passes over
    the runs between it and the main anchor in the other direction, where a 1-base gap may sit one base off, and must not cover a
    probe there.
    meta["probes"]: (side, chunk, walk index, covered?) -> HSP index."""
    b, main = carry_block(gap)
    kw = dict(max_extent=max_extent)
    one = Regime(b, rows([main], [9000]), kw)
    runs = genome_runs(one, 0)
    cover = one.cover_of(0)
    pts, tags = [], []
    for side in "LR":
        mine = [r for r in runs if r[0] == side]
        for c in sorted(chunks, reverse=True):  # nearest the anchor first, see the docstring
            # an M run in the middle of the chunk (or of what the side has of it) with a gap run before it in the genome
            cand = [r for r in mine if r[1] // 64 == c and r[2] == T.OP_M and (r[4] - 1, r[5] - 1) not in cover and r[3] >= 2]
            if not cand:
                continue
            r = sorted(cand, key=lambda x: x[1])[len(cand) // 2]
            pts += [(r[4], r[5]), (r[4] - 1, r[5] - 1)]
            tags += [(side, c, r[1], True), (side, c, r[1], False)]
    h = rows([main] + pts, [9000] + [8000 - 11 * k for k in range(len(pts))])
    return Regime(b, h, kw, probes={tag: 1 + k for k, tag in enumerate(tags)}, runs=runs,
                  n_runs={s: sum(r[0] == s for r in runs) for s in "LR"})


@functools.lru_cache(maxsize=None)
def carry_edge_extents():
    """{n: (gap, max_extent)} at which the right side of carry_block(gap)'s anchor has exactly n = 63, 64, 65 runs.  A side ends with
    an M run at its best cell, so an even count needs the gap anchor."""
    out = {}
    for gap in (False, True):
        b, main = carry_block(gap)
        for ext in range(330, 480):
            one = Regime(b, rows([main], [9000]), dict(max_extent=ext))
            n = sum(r[0] == "R" for r in genome_runs(one, 0))
            if n in (63, 64, 65):
                out.setdefault(n, (gap, ext))
    return out


# ---- nesting ----------------------------------------------------------------------------------------------------------------------------

NEST_KW = dict(max_extent=1000)


@functools.lru_cache(maxsize=None)
def identity_block():
    t = R.random_dna(12000, 1)
    return R.Block(t, t)


@functools.lru_cache(maxsize=None)
def nesting():
    """Identical sequences.  HSP 0 at (3500, 3500); HSP 1 at (3500, 3497), three off the main diagonal and of lower priority: not covered,
    and its path joins the main diagonal on both sides (997 M, 3 D | 3 I, 997 M), so the index holds the keys (main, 2500) and
    (main, 3500) twice, with different ends, and the unit segment (main, 3500, 3501) besides.  The probes on the main diagonal follow
    in priority, and one point next to HSP 1's anchor.  meta["probes"]: HSP indices."""
    b = identity_block()
    pts = [(3500, 3500), (3500, 3497)] + [(t, t) for t in (2499, 2500, 3496, 3497, 3498, 3499, 3501, 3503, 3800, 4496, 4497, 4499, 4500)]
    pts += [(3499, 3497)]
    h = rows(pts, [9000, 8000] + [7000 - 13 * k for k in range(len(pts) - 2)])
    return Regime(b, h, NEST_KW, probes=list(range(2, len(pts))))


# ---- merge: ties and interleaving across batches ----------------------------------------------------------------------------------------

MERGE_KW = dict(max_extent=1000)


@functools.lru_cache(maxsize=None)
def merge():
    """A 9 kbp target against a copy with a 2-base insertion or deletion every 400 bases.  Four anchors on the common path at
    max_extent 1000, in the priority order 2900, 5100, 4000 and 700, with an anchor that the one before it covers between them in
    priority, so that they are accepted in four batches at batch sizes 1 and 2.  Where two extents overlap both paths hold the runs
    that begin at a planted indel: the same key twice, the shorter run of the two being the one cut by its alignment's extent.  So the
    alignment at 4000 brings a longer run than the resident one of 2900 and a shorter one than the resident one of 5100.  The keys of
    5100 sort before the resident ones, those of 4000 between them and some of 700 (on the block's first diagonal) after them.  The
    probes, at and next to both ends of every run of the four, follow.  meta: mains, probes (HSP indices)."""
    t = R.random_dna(9000, 7421)
    q, pos = R.diverge(t, 7423, 0.0, 400, 2, "ID", jitter=False)
    b = R.Block(t, q)

    def on(x):
        return (x, int(pos[x]))
    mains = [on(2900), on(5100), on(4000), on(700)]
    fill = [on(2910), on(5110), on(4010)]  # covered by the main before them
    base = Regime(b, rows(mains, [9000, 8000, 7000, 6500]), MERGE_KW)
    ix = [Index(segments(base.raw()[0][k], base.raw()[1][k], mains[k])) for k in range(4)]
    probes = []
    for k in range(4):  # both ends of every run of every main, inside and outside
        for d, tb, te in ix[k].e:
            probes += [(tb - 1, tb - 1 - d), (tb, tb - d), (te - 1, te - 1 - d), (te, te - d)]
    probes = sorted(p for p in set(probes) - set(mains) - set(fill) if 1 <= p[0] < t.size and 1 <= p[1] < q.size)
    pts = [mains[0], fill[0], mains[1], fill[1], mains[2], fill[2], mains[3]] + probes
    h = rows(pts, [9000, 8900, 8000, 7900, 7000, 6900, 6500] + [6000 - 7 * k for k in range(len(probes))])
    return Regime(b, h, MERGE_KW, mains=(0, 2, 4, 6), probes=list(range(7, len(pts))))


# ---- ladder -----------------------------------------------------------------------------------------------------------------------------

LADDER_KW = dict(max_extent=100)
LADDER_N = 140


@functools.lru_cache(maxsize=None)
def ladder(mirror=False):
    """Identical sequences, max_extent 100: an anchor every 60 bases, scores descending to the right (mirror: to the left).  Each
    accepted anchor covers 100 bases either way, so it covers the next anchor and not the one after."""
    b = identity_block()
    pts = [(2000 + 60 * k, 2000 + 60 * k) for k in range(LADDER_N)]
    scores = [9000 - k for k in range(LADDER_N)]
    if mirror:
        scores = scores[::-1]
    return Regime(b, rows(pts, scores), LADDER_KW)


# ---- fans -------------------------------------------------------------------------------------------------------------------------------

FAN_N = 100


@functools.lru_cache(maxsize=None)
def fan(accepted_rank=None):
    """Identical sequences, max_extent 100.  The top anchor at 3000 covers [2900, 3100).  FAN_N owners at 3030 .. 3089, all covered by
    it, and all with 3125 on their paths.  The last anchor, at 3125 and of the lowest priority, is off the top anchor's path: it has
    FAN_N in-edges from eligible survivors, none from an accepted one, and is returned.  accepted_rank = 0, 1, 2: one more owner at
    3110, off the top anchor's path and so accepted, with the highest, a middle or the lowest priority among the owners: the last
    anchor is covered.  meta: top, owners, extra, last (HSP indices)."""
    b = identity_block()
    pts = [(3000, 3000)] + [(3030 + k % 60, 3030 + k % 60) for k in range(FAN_N)] + [(3125, 3125)]
    scores = [9000] + [8000 - 10 * k for k in range(FAN_N)] + [1000]
    extra = None
    if accepted_rank is not None:
        pts.append((3110, 3110))
        scores.append((8005, 8005 - 10 * (FAN_N // 2), 8005 - 10 * FAN_N)[accepted_rank])
        extra = len(pts) - 1
    return Regime(b, rows(pts, scores), LADDER_KW, top=0, owners=list(range(1, FAN_N + 1)), last=FAN_N + 1, extra=extra)


# ---- thresh -----------------------------------------------------------------------------------------------------------------------------

THRESH_KW = dict(max_extent=100, gappedthresh=15000)
THRESH_REC = 600


@functools.lru_cache(maxsize=None)
def thresh():
    """Four identical records of 600 bases.  An alignment in the middle of a record spans 200 bases and scores about 19 000; one
    anchored 20 bases from the record's start spans 120 and scores about 11 000; gappedthresh 15 000 lies between.
      record 0: strong anchor at 100, weak anchor at 20 on its path, next in priority (the same batch at batch size 2)
      record 1: strong anchor at 100, weak anchor at 20 on its path, five places later (a later batch at batch size 2)
      record 2: weak anchor at 20, then a strong anchor at 110 that lies on the weak alignment's path only
      record 3: two duplicate weak anchors at 20
    meta: the HSP indices by role."""
    rec = [R.random_dna(THRESH_REC, 7431 + k) for k in range(4)]
    off = R.offsets(rec)
    b = R.Block(R.join(rec), R.join(rec))
    at = lambda r, x: (off[r] + x, off[r] + x)  # noqa: E731
    pts = [at(0, 100), at(0, 20), at(1, 100), at(2, 20), at(2, 110), at(3, 20), at(3, 20), at(1, 20)]
    scores = [9000, 8900, 8800, 8700, 8600, 8500, 8400, 8300]
    return Regime(b, rows(pts, scores), THRESH_KW, strong=(0, 2), on_path=(1, 7), weak_first=3, strong_after=4, dup=(5, 6))


# ---- ties -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ties(seed=0):
    """Identical sequences, max_extent 100, every score equal within a group.  Three groups of duplicate rows (5, 9 and 2 copies) and
    three pairs of distinct anchors 30 bases apart, each on the other's path; the rows are then shuffled.  meta["groups"]: lists of
    HSP indices after the shuffle."""
    b = identity_block()
    pts, scores, groups = [], [], []
    for g, (x, n) in enumerate(((1000, 5), (1500, 9), (2000, 2))):
        groups.append(list(range(len(pts), len(pts) + n)))
        pts += [(x, x)] * n
        scores += [5000 + g] * n
    for g, x in enumerate((3000, 3500, 4000)):
        groups.append([len(pts), len(pts) + 1])
        pts += [(x, x), (x + 30, x + 30)]
        scores += [6000 + g] * 2
    h = rows(pts, scores)
    for grp in groups[:3]:  # duplicates are the same row
        h[grp] = h[grp[0]]
    perm = np.random.default_rng(7441 + seed).permutation(h.size)
    inv = np.argsort(perm)
    return Regime(b, h[perm], LADDER_KW, groups=[[int(inv[k]) for k in grp] for grp in groups])


# ---- gapanc: the anchor point that is no M pair ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gapanc():
    """The target holds one base more than the query, at the anchor: T = X c Y against Q = X Y, anchor (|X|, |X|), with c different
    from Y's first base.  The right side begins with a D run over c (any path that pairs c pays a mismatch and still needs the gap), so
    (|X|, |X|) is no M pair.  Two duplicate rows there."""
    x, y = R.random_dna(1500, 7451), R.random_dna(1500, 7452)
    c = R.ascii_of("ACGT"[(b"ACGT".index(bytes(y[:1])) + 1) % 4])
    b = R.Block(np.concatenate([x, c, y]), np.concatenate([x, y]))
    h = rows([(1500, 1500)] * 2, [5000, 5000])
    h[1] = h[0]
    return Regime(b, h, dict(max_extent=400))
