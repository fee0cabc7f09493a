"""Hand-built target / query pairs that put the ungapped extension stage (segalign_amd/csrc/extend.hip: the byte-coded X-drop filter in
its fast and exact forms, the packed int16 filter, the 512-bases-per-step exact kernel, the chain shortcut) on its window, lane, drop,
tie, cap and sequence-end edges, with the anchors placed by construction.  Shared by tests/test_extend_regimes.py (CPU: the model of
tests/extend_model.py equals the oracle on every anchor, and every regime is in the state it names) and
tests/test_gpu_extend_regimes.py (GPU: sa_extend_hits against the model).

A regime is a list of scores in WALKING order (`pattern`): the pair writes, for every score, two codes that score it under the pair's
matrix, to the right of the anchor (right side: item i is offset k = i) or mirrored to its left (left side: item i is offset k = i + 1),
and fills the space between regimes with target A against query C, which mismatches on every diagonal.  `facts` are the claims of the
construction -- ("R" | "L", attribute of extend_model.Side) or "total" -> value -- and the CPU test reads them off the model.

Five pairs: W (simple matrix: runs, dips, ties, sequence ends), F (simple matrix: thresholds, caps, the fast form's chunk edge, codes
above 3, entropy islands, chain runs), H (HOXD70: a selection of all of these), B (anchors whose BOTH walks meet a real sequence end) and C
(the islands again, seedable, for the class filter).  SETS lists the parameter sets the GPU test runs."""
import functools

import numpy as np

import extend_model as M

A, C, G, T, L, N, X, E = range(8)
ASCII = np.frombuffer(b"ACGTaNR&", dtype=np.uint8)   # one letter per code (common/seed_filter_interface.cu:18-47)
FILL = 16                                            # filler bases between regimes: a walk at xdrop <= 1000 drops inside them
LIMS = (0, 1, 7, 8, 9, 511, 512, 513)                # bases left to a sequence end
CAPS = (128, 64, 8)                                  # option long_cap
CHAIN_GAP_MAX, CHAIN_WALK_EXTRA = M.CHAIN_GAP_MAX, M.CHAIN_WALK_EXTRA


def simple_matrix(match=100):
    """+match / -100 on ACGT, with one small step: G against T scores -1 (so that a dip of xdrop + 1 and a total of hspthresh - 1 can
    be written down); masked and N -1000, other IUPAC -100, the separator far below the int16 range of the packed filter"""
    m = np.full((8, 8), -1000, dtype=np.int32)
    m[:4, :4] = -100
    for i in range(4):
        m[i, i] = match
    m[G, T] = m[T, G] = -1
    m[X, :] = m[:, X] = -100
    m[E, :] = m[:, E] = -20000
    return m.ravel().copy()


class Regime:
    def __init__(self, name, anchors, facts, single=True):
        self.name, self.anchors, self.facts, self.single = name, [tuple(a) for a in anchors], facts, single

    def __repr__(self):
        return "Regime(%s %s)" % (self.name, self.anchors[:3])


class Pair:
    """target and query code lists under construction, two cursors (the diagonal of the next regime is tcur - qcur)"""

    def __init__(self, name, mat, xdrop, hspthresh):
        self.name, self.mat, self.xdrop, self.hspthresh = name, np.asarray(mat, dtype=np.int32), xdrop, hspthresh
        self.t, self.q, self.regs, self.chain_cases = [], [], [], []
        self.by_score = {}
        for r in range(4):
            for q in range(4):
                self.by_score.setdefault(int(self.mat[r * 8 + q]), []).append((r, q))
        self._lcg = 12345

    def _pick(self, item):
        if isinstance(item, tuple):
            return item
        opts = self.by_score[item]
        self._lcg = (self._lcg * 1103515245 + 12345) & 0x7FFFFFFF
        return opts[(self._lcg >> 16) % len(opts)]

    def fill(self, n=FILL):
        self.t += [A] * n
        self.q += [C] * n

    def align_q(self, rem, mod=512):
        """filler until the query cursor is at rem modulo mod (chain buckets are windows of 512 query positions)"""
        self.fill((rem - len(self.q)) % mod)

    def add(self, name, patR=(), patL=(), facts=None, extra=(), single=True):
        """mirror(patL) + patR on the current diagonal, the anchor between them; extra: further anchors as offsets from the anchor.
        -> the anchor"""
        for item in reversed(list(patL)):
            r, q = self._pick(item)
            self.t.append(r)
            self.q.append(q)
        a = (len(self.t), len(self.q))
        for item in patR:
            r, q = self._pick(item)
            self.t.append(r)
            self.q.append(q)
        self.fill()
        self.regs.append(Regime(name, [a] + [(a[0] + d, a[1] + d) for d in extra], facts or {}, single))
        return a

    def done(self):
        self.ref = np.array(self.t, dtype=np.uint8)
        self.qry = np.array(self.q, dtype=np.uint8)
        assert self.ref.size <= 65536 and self.qry.size <= 65536, (self.name, self.ref.size, self.qry.size)
        return self

    # ---- what the tests read ----
    def anchors(self):
        return np.array([a for g in self.regs for a in g.anchors], dtype=np.uint32).reshape(-1, 2)

    def singles(self):
        """the regimes whose anchor is also sent in a call of its own"""
        return [g for g in self.regs if g.single]

    def bulk(self):
        """every anchor of the pair, and next to each two more (one and two bases further along its diagonal): anchors of mixed walk
        lengths in construction order"""
        a = self.anchors().astype(np.int64)
        more = [a]
        for d in (1, 2):
            b = a + d
            more.append(b[(b[:, 0] <= self.ref.size) & (b[:, 1] <= self.qry.size)])
        return np.concatenate(more).astype(np.uint32)

    def target_ascii(self):
        return ASCII[self.ref]

    def query_ascii(self, rev=False, oracle=None):
        """the query block to send; rev: the block whose reverse-complement strand is self.qry"""
        return ASCII[oracle.rev_comp_codes(self.qry)] if rev else ASCII[self.qry]


# ---- patterns (walking order; P = a match, the negatives by their scores) ------------------------------------------------------
class Kit:
    """the scores a pair's patterns are written in"""

    def __init__(self, hoxd, xdrop):
        self.hoxd, self.xdrop = hoxd, xdrop
        if hoxd:
            assert xdrop == 910
            self.P = 100
            self.dip_exact = [-125, -125, -123, -123, -114, -114] + [-31] * 6          # 910
            self.dip_over = [-125, -123, -31, -31, -31] + [-114] * 5                    # 911: only its last base drops
            self.recover = 12
            self.tie_down, self.tie_up = [-125] * 4, [100] * 5                          # back to exactly the earlier best
        else:
            assert xdrop == 1000
            self.P = 100
            self.dip_exact = [-100] * 10
            self.dip_over = [-100] * 10 + [-1]
            self.recover = 12
            self.tie_down, self.tie_up = [-100], [100]

    def run(self, n):
        if not self.hoxd:
            return [100] * n
        return [100 if (i * 7 + i // 3) % 3 else 91 for i in range(n)]


def shift_of(side):
    return 1 if side == "L" else 0


def pat_dip(kit, side, kb, over):
    """first island, a dip whose bottom is at offset kb -- of exactly xdrop, or of xdrop + 1 (over) --, a second island that would
    carry the best past the first"""
    neg = kit.dip_over if over else kit.dip_exact
    a = kb - shift_of(side) - len(neg) + 1
    assert a >= 1
    one, two = kit.run(a), [kit.P] * kit.recover
    pat = one + neg + two
    if over:
        facts = {(side, "stop"): kb, (side, "edge"): False, (side, "pos"): a - 1 + shift_of(side), (side, "best"): sum(one)}
    else:
        facts = {(side, "dip"): kit.xdrop, (side, "dip_at"): kb, (side, "pos"): kb + kit.recover,
                 (side, "best"): sum(one) - kit.xdrop + sum(two)}
    return pat, facts


def pat_tie(kit, side, p1, twin):
    """an island whose best is at offset p1, a dip, a second island that brings the score back to exactly that best (the earlier
    position is reported) or, twin, one match further (the later one is)"""
    a = p1 - shift_of(side) + 1
    assert a >= 1
    one = kit.run(a)
    pat = one + kit.tie_down + kit.tie_up + ([kit.P] if twin else [])
    p2 = p1 + len(kit.tie_down) + len(kit.tie_up)
    if twin:
        facts = {(side, "pos"): p2 + 1, (side, "best"): sum(one) + kit.P, (side, "ties"): []}
    else:
        facts = {(side, "pos"): p1, (side, "best"): sum(one), (side, "ties"): [p2]}
    return pat, facts


def merged(*fs):
    out = {}
    for f in fs:
        out.update(f)
    return out


# ---- families shared by the pairs ----------------------------------------------------------------------------------------------
def add_runs(p, kit, lengths, inner):
    """match runs: the anchor at the start has its right best at n - 1, the anchor behind the end its left best at n, the anchors at
    `inner` offsets both"""
    for n in lengths:
        ins = [a for a in inner if 0 < a < n]
        s = p.add("run%d right" % n, patR=kit.run(n), facts={("R", "pos"): n - 1, ("L", "pos"): 0, ("L", "best"): 0})
        p.regs.append(Regime("run%d left" % n, [(s[0] + n, s[1] + n)], {("L", "pos"): n, ("R", "pos"): -1, ("R", "best"): 0}))
        for a in ins:
            p.regs.append(Regime("run%d both@%d" % (n, a), [(s[0] + a, s[1] + a)], {("L", "pos"): a, ("R", "pos"): n - 1 - a}))


def add_dips(p, kit, bottoms, both):
    for kb in bottoms:
        for over in (False, True):
            for side in "RL":
                pat, facts = pat_dip(kit, side, kb, over)
                p.add("dip%s@%d %s" % ("+1" if over else "", kb, side), facts=facts, **{"pat" + side: pat})
    for kl, kr, over_l, over_r in both:
        pl, fl = pat_dip(kit, "L", kl, over_l)
        pr, fr = pat_dip(kit, "R", kr, over_r)
        p.add("dip L@%d%s R@%d%s" % (kl, "+1" * over_l, kr, "+1" * over_r), patR=pr, patL=pl, facts=merged(fl, fr))


def add_ties(p, kit, firsts, both):
    for p1 in firsts:
        for twin in (False, True):
            for side in "RL":
                if p1 - shift_of(side) + 1 < 1:
                    continue
                pat, facts = pat_tie(kit, side, p1, twin)
                p.add("tie%s@%d %s" % (" twin" if twin else "", p1, side), facts=facts, **{"pat" + side: pat})
    for pl1, pr1, twin in both:
        pl, fl = pat_tie(kit, "L", pl1, twin)
        pr, fr = pat_tie(kit, "R", pr1, twin)
        p.add("tie%s L@%d R@%d" % (" twin" if twin else "", pl1, pr1), patR=pr, patL=pl, facts=merged(fl, fr))


def add_separator_ends(p, kit, both):
    """a walk still at its best when it meets a separator (code E, in the target) lim bases on"""
    sep = (E, C)
    for lim in LIMS:
        run = kit.run(lim)
        p.add("E right lim%d" % lim, patR=run + [sep], facts={("R", "stop"): lim, ("R", "edge"): False, ("R", "pos"): lim - 1,
                                                               ("R", "last"): sum(run), ("R", "best"): sum(run)})
        p.add("E left lim%d" % lim, patL=run + [sep], facts={("L", "stop"): lim + 1, ("L", "edge"): False, ("L", "pos"): lim,
                                                              ("L", "last"): sum(run), ("L", "best"): sum(run)})
    for ll, lr in both:
        p.add("E both %d|%d" % (ll, lr), patL=kit.run(ll) + [sep], patR=kit.run(lr) + [sep],
              facts={("L", "stop"): ll + 1, ("L", "pos"): ll, ("R", "stop"): lr, ("R", "pos"): lr - 1, ("L", "edge"): False, ("R", "edge"): False})


def end_facts(side, lim, best=None):
    f = {(side, "stop"): lim + shift_of(side), (side, "edge"): True, (side, "pos"): lim - 1 + shift_of(side)}
    if best is not None:
        f[(side, "best")] = f[(side, "last")] = best
    return f


def gt_letters(n, seed):
    """n letters of G and T (they mismatch the filler's target A and its query C under the simple matrix)"""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.choice([G, T], size=n)]


# ---- pair W: windows, lanes, ties and sequence ends under the simple matrix ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_w():
    p, kit = Pair("W", simple_matrix(), 1000, 3000), Kit(False, 1000)
    top = max(LIMS)
    # -- the block start: the first 513 bases of both sequences are one run.  (lim, lim) ends at the start of both; (r, lim) on a copy
    #    of the run's first lim bases further down the TARGET ends at the query start with the target longer; (lim, q) the other way round
    pre = gt_letters(top, 1)
    p.t += pre
    p.q += pre
    p.fill()
    for lim in LIMS:
        p.regs.append(Regime("start both ends lim%d" % lim, [(lim, lim)], merged(end_facts("L", lim, 100 * lim), {("R", "pos"): top - 1 - lim})))
    for lim in LIMS:      # target copies and query copies side by side: they meet on no diagonal an anchor uses
        t0, q0 = len(p.t), len(p.q)
        p.t += pre[:lim]
        p.q += pre[:lim]
        p.regs.append(Regime("start query ends lim%d" % lim, [(t0 + lim, lim)], merged(end_facts("L", lim, 100 * lim), {("R", "best"): 0})))
        p.regs.append(Regime("start target ends lim%d" % lim, [(lim, q0 + lim)], merged(end_facts("L", lim, 100 * lim), {("R", "best"): 0})))
        p.fill()
    # -- the body
    add_runs(p, kit, (6, 7, 8, 9, 510, 511, 512, 513, 514, 1023, 1024, 1025, 1535, 1536), inner=(7, 8, 9, 511, 512, 513, 1024))
    add_dips(p, kit, (14, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 66, 511, 512, 513),
             both=[(16, 15, o, o2) for o, o2 in ((0, 0), (1, 1), (0, 1))] + [(24, 24, 0, 1), (25, 23, 1, 0), (33, 32, 0, 0), (65, 64, 1, 1),
                   (512, 511, 0, 0), (512, 511, 1, 1), (513, 512, 0, 0), (513, 512, 1, 1), (511, 513, 0, 1)])
    add_ties(p, kit, (1, 2, 6, 7, 126, 127, 254, 255, 510, 511), both=[(7, 6, False), (7, 6, True), (127, 126, False), (127, 126, True),
                                                                         (511, 510, False), (511, 510, True)])
    # (maxima ten lanes apart, and three maxima in a row)
    for side in "RL":
        one = kit.run(100 - shift_of(side))
        p.add("tie far %s" % side, facts={(side, "pos"): 99, (side, "ties"): [119]}, **{"pat" + side: one + [-100] * 10 + [100] * 10})
        p.add("tie thrice %s" % side, facts={(side, "pos"): 99, (side, "ties"): [101, 103, 521]},
              **{"pat" + side: one + [-100, 100] * 2 + [-100] * 9 + [100, -100] * 200 + [100] * 9})
    add_separator_ends(p, kit, both=[(0, 1), (1, 0), (0, 0), (7, 9), (8, 8), (9, 7), (511, 513), (512, 512), (513, 511)])
    # -- the block end, mirrored: the last 513 bases of both are one run
    suf = gt_letters(top, 2)
    t_regs, q_regs = [], []
    for lim in LIMS:
        t0, q0 = len(p.t), len(p.q)
        p.t += suf[top - lim:]
        p.q += suf[top - lim:]
        t_regs.append((lim, t0))
        q_regs.append((lim, q0))
        p.fill()
    p.t += suf
    p.q += suf
    nt, nq = len(p.t), len(p.q)
    for lim, t0 in t_regs:
        p.regs.append(Regime("end query ends lim%d" % lim, [(t0, nq - lim)], merged(end_facts("R", lim, 100 * lim), {("L", "best"): 0})))
    for lim, q0 in q_regs:
        p.regs.append(Regime("end target ends lim%d" % lim, [(nt - lim, q0)], merged(end_facts("R", lim, 100 * lim), {("L", "best"): 0})))
    for lim in LIMS:
        p.regs.append(Regime("end both ends lim%d" % lim, [(nt - lim, nq - lim)], merged(end_facts("R", lim, 100 * lim), {("L", "pos"): top - lim})))
    return p.done()


# ---- pair B: both walks of an anchor meet a real sequence end ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_b():
    """The target starts and the query ends with the same one-letter run (G), so on every diagonal between them the left walk of
    (l, query_len - r) is still at its best when it meets the TARGET start after l bases, and the right walk when it meets the QUERY end
    after r bases; the query start and the target end share a run of T the same way: (ref_len - r, l).  Every (l, r) of LIMS x LIMS, so
    that the two ends fall on either side of lane and window edges independently.  (One letter: a run that ends at the start of one
    sequence and at the end of the other is compared on a different diagonal for every l + r.)"""
    p = Pair("B", simple_matrix(), 1000, 3000)
    n = 2 * max(LIMS)
    p.t += [G] * n + [A] * 2 * FILL + [T] * n
    p.q += [T] * n + [C] * 2 * FILL + [G] * n
    nt, nq = len(p.t), len(p.q)
    for l in LIMS:
        for r in LIMS:
            facts = merged(end_facts("L", l, 100 * l), end_facts("R", r, 100 * r), {"total": 100 * (l + r)})
            p.regs.append(Regime("target start %d | query end %d" % (l, r), [(l, nq - r)], facts))
            p.regs.append(Regime("query start %d | target end %d" % (l, r), [(nt - r, l)], dict(facts)))
    return p.done()


# ---- pair F: the filter forms, their switches, the caps, the thresholds and the chain shortcut --------------------------------------
def alive(n):
    """n bases that keep a side alive at a best of 100 (or 0 for n = 0), then a separator, which drops it at once"""
    return [100, -100] * (n // 2) + [(E, C)]


def make_total(total):
    """a run of matches with as many one-point steps inside as it takes to reach `total`; the best is at its end"""
    n = -(-total // 100)
    steps = 100 * n - total
    assert n > 2 * steps + 2
    pat = [100] * n
    for i in range(steps):
        pat.insert(2 + 2 * i, -1)
    return pat


@functools.lru_cache(maxsize=None)
def pair_f():
    p, kit = Pair("F", simple_matrix(), 1000, 3000), Kit(False, 1000)
    h = 3000
    p.fill()
    # -- totals of hspthresh - 1 and hspthresh: all on one side, split evenly
    for tot in (h - 1, h):
        p.add("total %d right" % tot, patR=make_total(tot), facts={"total": tot, ("L", "best"): 0})
        p.add("total %d left" % tot, patL=make_total(tot), facts={"total": tot, ("R", "best"): 0})
        p.add("total %d split" % tot, patL=make_total(h // 2), patR=make_total(tot - h // 2), facts={"total": tot, ("L", "best"): h // 2})
    # -- long_cap: a side alive after exactly cap - 8, cap, cap + 8 bases, then dropped; the total at hspthresh - 1 and hspthresh comes
    #    from the other side
    for n in sorted({c + d for c in CAPS for d in (-8, 0, 8)}):
        for tot in (h - 1, h):
            mine = 100 if n else 0
            p.add("alive %d right total %d" % (n, tot), patR=alive(n), patL=make_total(tot - mine),
                  facts={("R", "stop"): n, ("R", "edge"): False, ("R", "best"): mine, "total": tot})
            p.add("alive %d left total %d" % (n, tot), patL=alive(n), patR=make_total(tot - mine),
                  facts={("L", "stop"): n + 1, ("L", "edge"): False, ("L", "best"): mine, "total": tot})
    #    ... and the same sides between two separators, with nothing else alive: a candidate iff n >= long_cap, whatever the cap
    for n in sorted({c + d for c in CAPS for d in (-8, 0, 8)}):
        p.add("lone %d right" % n, patR=alive(n), patL=[(E, C)], facts={("R", "stop"): n, ("L", "stop"): 1, "total": 100 if n else 0})
        p.add("lone %d left" % n, patL=alive(n), patR=[(E, C)], facts={("L", "stop"): n + 1, ("R", "stop"): 0, "total": 100 if n else 0})
    # -- a perfect run of at least long_cap bases (at max(M) = 127 the packed filter's int16 score is near its top when the cap fires)
    p.add("perfect 128 right", patR=[100] * 128, facts={("R", "pos"): 127})
    p.add("perfect 136 left", patL=[100] * 136, facts={("L", "pos"): 136})
    p.add("perfect 200 both", patL=[100] * 200, patR=[100] * 200, facts={("L", "pos"): 200, ("R", "pos"): 199})
    # -- the fast form (xdrop == 7 * max(M) = 700): 8m + 1 matches, seven mismatches (a dip of exactly 700), then the drop by a one-point
    #    step on the FIRST base of a chunk, then seven matches: the walk has ended, the side's best must not rise.  The other side supplies
    #    hspthresh - 1 - this side's best: were the seven matches counted, the total would pass.  (At xdrop 1000 the walk goes on.)
    #    The same with a dip of 601 for xdrop 600, where the exact form runs and a filter in the fast form would count the seven matches.
    for m8 in (8, 16, 64, 120):
        for side, other in (("R", "L"), ("L", "R")):
            for mism in (7, 6):
                one = m8 + 8 - mism           # the step is item m8 + 8: the first base of a chunk on either side
                pat = [100] * one + [-100] * mism + [-1] + [100] * 7 + [-100] * 12
                assert pat.index(-1) % 8 == 0
                rest = make_total(h - 1 - 100 * one) if 100 * one < h - 1 - 300 else []
                best = 100 * one if mism == 7 else 100 * one + 99      # (at the pair's own xdrop of 1000 the walk goes on to the seven matches)
                p.add("chunk edge drop %d after %d %s" % (mism * 100 + 1, one, side), facts={(side, "best"): best},
                      **{"pat" + side: pat, "pat" + other: rest})
    # -- masked, N and other IUPAC codes in the TARGET inside an island that is at the threshold (the packed form stores them as code 0)
    for code, name in ((L, "masked"), (N, "N"), (X, "iupac")):
        cost = -int(p.mat[code * 8 + A])
        for tot in (h - 1, h):
            for side in "RL":
                pat = [100] * 15 + [(code, A)] + make_total(tot - 1500 + cost)
                facts = {"total": tot}
                if cost == 1000:      # a dip of exactly xdrop on one base
                    facts.update({(side, "dip"): cost, (side, "dip_at"): 15 + shift_of(side)})
                p.add("%s in island total %d %s" % (name, tot, side), facts=facts, **{"pat" + side: pat})
    # -- entropy islands for hspthresh 3099 with the entropy factor on (oracle.extend_hit is the reference there): a one-letter island
    #    at 3 * hspthresh (inside the band: a factor near 0) and one point above it (outside: kept), a balanced island at hspthresh
    def one_letter(total):
        n = -(-total // 100)
        pat = [(C, C)] * n
        for i in range(100 * n - total):
            pat.insert(5 + 3 * i, (G, T))
        return pat
    p.entropy = {}
    p.entropy["band"] = p.add("one letter 9297", patR=one_letter(9297)[:50], patL=one_letter(9297)[50:], facts={"total": 9297})
    p.entropy["above"] = p.add("one letter 9298", patR=one_letter(9298)[:50], patL=one_letter(9298)[50:], facts={"total": 9298})
    bal = [(i % 4, i % 4) for i in range(31)]
    bal.insert(12, (G, T))
    p.entropy["balanced"] = p.add("balanced 3099", patR=bal[:16], patL=bal[16:], facts={"total": 3099})
    # -- the chain shortcut.  Every case is also sent as a call of its own (chain_cases), where the records it leaves are known exactly
    def case(name, anchors):
        p.chain_cases.append((name, np.array(anchors, dtype=np.uint32).reshape(-1, 2)))
    # b at a's best right end (covered, one record) and one past it (extended on its own)
    for name, db in (("at right end", 37), ("past right end", 38)):
        p.align_q(20)
        p.add("chain b " + name, patL=[100] * 2, patR=[100] * 38, extra=(db,), single=False)
        case("b " + name, p.regs[-1].anchors)
    # anchor gaps of 256 and 257 inside one island
    for g in (CHAIN_GAP_MAX, CHAIN_GAP_MAX + 1):
        p.align_q(10)
        p.add("chain gap %d" % g, patL=[100] * 5, patR=[100] * 300, extra=(g,), single=False)
        case("gap %d" % g, p.regs[-1].anchors)
    # b's new left best at offset gap + 96 (found by the bounded walk) and gap + 97 (not found); gap = 16 = the island between a and b, so
    # that b's best lies AT a until then
    for kn in (16 + CHAIN_WALK_EXTRA, 16 + CHAIN_WALK_EXTRA + 1):
        neg, climb = ([-100] * 9 + [-1], 10) if kn % 2 == 0 else ([-100] * 10, 11)
        stall = kn - 16 - len(neg) - climb
        assert stall % 2 == 0
        pat = [100] * 16 + neg + [100, -100] * (stall // 2) + [100] * climb + [100] * 3
        p.align_q(200)
        p.add("chain walk extra new best@%d" % kn, patL=pat, patR=[100] * 15, extra=(-16,), single=False, facts={("L", "pos"): kn + 3})
        case("new best at gap + %d" % (kn - 16), p.regs[-1].anchors)
    # strictness of (L): b's left walk comes back to exactly its best at a position before a and ends there; a's own goes further
    p.align_q(100)
    p.add("chain strict", patL=[100] * 40 + [-100] * 3 + [100] * 3 + [-100] * 11, patR=[100] * 5, extra=(-43,), single=False,
          facts={("L", "pos"): 40, ("L", "ties"): [46]})
    case("strict", p.regs[-1].anchors)
    # b's best exactly AT a (offset gap, not beyond it): a run head
    p.align_q(100)
    p.add("chain best at a", patL=[100] * 30 + [-100] * 11, patR=[100] * 5, extra=(-30,), single=False, facts={("L", "pos"): 30})
    case("best at a", p.regs[-1].anchors)
    # runs of 130 anchors on consecutive positions whose first member beyond the head's right end is number 63, 64, 65 of the run (the
    # exact kernel looks at 64 members at a time); behind the head's island a plateau that ties its best and never exceeds it, so that
    # every later member is promoted in turn
    for e in (63, 64, 65):
        p.align_q(100)
        p.add("chain run beyond@%d" % e, patL=[100] * 3, patR=[100] * e + [-100, 100] * 40, extra=tuple(range(1, 130)), single=False,
              facts={("R", "pos"): e - 1})
        case("run beyond@%d" % e, p.regs[-1].anchors)
    # two anchors one base apart at query positions 511 and 512: two windows, two buckets
    p.align_q(511 - 20)
    p.add("chain windows", patL=[100] * 20, patR=[100] * 20, extra=(1,), single=False)
    assert p.regs[-1].anchors[0][1] % 512 == 511
    case("windows 511|512", p.regs[-1].anchors)
    # exact duplicates of one anchor
    p.align_q(50)
    d = p.add("chain duplicates", patL=[100] * 20, patR=[100] * 20, single=False)
    case("duplicates", [d, d, d])
    p.fill()
    return p.done()



# ---- pair H: HOXD70 at xdrop 910, hspthresh 3000 -------------------------------------------------------------------------------------
def hoxd_total(total):
    """matches of 100 (C, G) and 91 (A, T), one transition (-31) inside where it takes one: 3000 = 30 x 100; 2999 = 3 x 100 + 30 x 91 - 31"""
    best = None
    for j in range(0, 6):
        for a in range(0, 60):
            rest = total + 31 * j - 91 * a
            if rest >= 0 and rest % 100 == 0 and (best is None or a + j + rest // 100 < len(best)):
                pat = [100] * (rest // 100) + [91] * a
                for i in range(j):
                    pat.insert(4 + 2 * i, -31)
                best = pat
    assert best is not None, total
    return best


@functools.lru_cache(maxsize=None)
def pair_h(oracle_mat):
    mat = np.array(oracle_mat, dtype=np.int32)
    p, kit = Pair("H", mat, 910, 3000), Kit(True, 910)
    top = max(LIMS)
    pre = [int(x) for x in np.random.default_rng(3).integers(0, 4, top)]
    p.t += pre
    p.q += pre
    p.fill()
    for lim in LIMS:
        p.regs.append(Regime("start both ends lim%d" % lim, [(lim, lim)], end_facts("L", lim)))
    add_runs(p, kit, (7, 8, 9, 511, 512, 513, 514, 1024, 1025), inner=(8, 512, 513))
    add_dips(p, kit, (15, 16, 17, 23, 24, 25, 63, 64, 65, 511, 512, 513),
             both=[(16, 15, 0, 1), (25, 24, 1, 0), (512, 511, 0, 0), (513, 512, 1, 1)])
    add_ties(p, kit, (3, 4, 123, 124, 507, 508), both=[(124, 123, False), (508, 507, False), (508, 507, True)])
    add_separator_ends(p, kit, both=[(0, 0), (8, 8), (512, 511)])
    h = 3000
    for tot in (h - 1, h):
        p.add("total %d right" % tot, patR=hoxd_total(tot), facts={"total": tot})
        p.add("total %d left" % tot, patL=hoxd_total(tot), facts={"total": tot})
        p.add("total %d split" % tot, patL=hoxd_total(1500), patR=hoxd_total(tot - 1500), facts={"total": tot})
    for code, name in ((L, "masked"), (N, "N"), (X, "iupac")):
        cost = -int(mat[code * 8 + C])
        for tot in (h - 1, h):
            for side in "RL":
                if cost > 910:      # the walk ends on it: the island before it carries the total
                    pat = hoxd_total(tot) + [(code, C)] + [100] * 20
                    facts = {"total": tot, (side, "stop"): len(pat) - 21 + shift_of(side)}
                else:
                    pat = [100] * 15 + [(code, C)] + hoxd_total(tot - 1500 + cost)
                    facts = {"total": tot}
                p.add("%s in island total %d %s" % (name, tot, side), facts=facts, **{"pat" + side: pat})
    suf = [int(x) for x in np.random.default_rng(4).integers(0, 4, top)]
    p.t += suf
    p.q += suf
    nt, nq = len(p.t), len(p.q)
    for lim in LIMS:
        p.regs.append(Regime("end both ends lim%d" % lim, [(nt - lim, nq - lim)], end_facts("R", lim)))
    return p.done()


# ---- pair C: the near-threshold, dip and tie islands again, with runs long enough to seed, for the table-direct calls (class filter) ----
@functools.lru_cache(maxsize=None)
def pair_c(oracle_mat):
    """Every seed hit inside an island is an anchor, so a drop behind a run of n >= 19 + j bases lies at every offset up to j from some
    anchor: the runs are sized so that the drops fall on the ends of the class filter's six-base fields (right offsets 5 + 6i, left
    offsets 25 + 6i behind the 19-base seed window) and of its four-base tail (left offset 77), and one base before and after them.
    Regime.facts: "kept" -- the island's record is in the call's output (total == hspthresh) or no record starts in it (hspthresh - 1)."""
    mat = np.array(oracle_mat, dtype=np.int32)
    p, kit = Pair("C", mat, 910, 3000), Kit(True, 910)
    p.fill(40)

    def island(name, pat, kept, at=19):
        s = p.add(name, patR=pat, facts={"kept": kept, "span": None})
        g = p.regs[-1]
        g.anchors = [(s[0] + at, s[1] + at)]
        g.facts["span"] = (s[0], len(pat))
    h = 3000
    for rep in range(3):
        island("total %d #%d" % (h, rep), hoxd_total(h), True)
        island("total %d #%d" % (h - 1, rep), hoxd_total(h - 1), False)
    # two islands that pass only together, through a dip of exactly xdrop; with a dip of xdrop + 1 neither passes
    for t1 in range(2000, 2700, 100):
        one, two = hoxd_total(t1), hoxd_total(h + 910 - t1)
        island("through dip %d" % t1, one + kit.dip_exact + two, True)
        island("before dip+1 %d" % t1, one + kit.dip_over + two, False)
        island("through dip %d mirrored" % t1, two + kit.dip_exact[::-1] + one, True, at=len(two) + 12 + 19)
        island("before dip+1 %d mirrored" % t1, two + kit.dip_over[::-1] + one, False, at=len(two) + 10 + 19)
    # long runs on both sides of the dips: the drop at every offset the contexts reach, the far field ends and the tail included
    for neg in (kit.dip_exact, kit.dip_over, kit.dip_exact[::-1], kit.dip_over[::-1]):
        island("long dip", kit.run(100) + list(neg) + kit.run(100), True)
        del p.regs[-1].facts["kept"]
    for twin in (False, True):
        island("tie", kit.run(100) + kit.tie_down + kit.tie_up + ([100] if twin else []) + kit.tie_down + kit.run(100)[::-1], True)
        del p.regs[-1].facts["kept"]
    p.fill(40)
    return p.done()


# ---- parameter sets ----------------------------------------------------------------------------------------------------------------
class Set:
    """pair + matrix + thresholds + options.  modes: filter_mode() expected under the default options and under no_packed_filter
    (3 packed, 1 byte-coded fast, 0 byte-coded exact)"""

    def __init__(self, name, pair, mat=None, xdrop=None, hspthresh=None, noentropy=True, rev=False, options=None, modes=(3, 1), chain_exact=False):
        self.name, self.pair_fn, self.mat_fn, self.noentropy, self.rev = name, pair, mat, noentropy, rev
        self._xdrop, self._hspthresh, self.options, self.modes, self.chain_exact = xdrop, hspthresh, dict(options or {}), modes, chain_exact

    def resolve(self, oracle):
        self.pair = pair_h(tuple(int(x) for x in oracle.build_sub_mat(910))) if self.pair_fn == "H" else {"W": pair_w, "F": pair_f, "B": pair_b}[self.pair_fn]()
        self.xdrop = self.pair.xdrop if self._xdrop is None else self._xdrop
        self.hspthresh = self.pair.hspthresh if self._hspthresh is None else self._hspthresh
        self.mat = self.pair.mat if self.mat_fn is None else np.asarray(self.mat_fn(oracle), dtype=np.int32)
        self.long_cap = int(self.options.get("long_cap", 128))
        return self

    def __repr__(self):
        return "Set(%s)" % self.name


SETS = [
    Set("W", "W"),
    Set("W rev", "W", rev=True),
    Set("F", "F", chain_exact=True),
    Set("H hoxd70", "H"),
    Set("B both ends", "B"),
    Set("B both ends rev", "B", rev=True),
    Set("B both ends xdrop 0", "B", xdrop=0, modes=(3, 0)),
    # the fast form and its switch (7 * max(M) = 700), and xdrop 0
    Set("F xdrop 700", "F", xdrop=700, modes=(3, 1)),
    Set("F xdrop 699", "F", xdrop=699, modes=(3, 0)),
    Set("F xdrop 600", "F", xdrop=600, modes=(3, 0)),
    Set("F xdrop 0", "F", xdrop=0, modes=(3, 0)),
    # the packed form's switches, each with its neighbour on the other side
    Set("F xdrop 16383", "F", xdrop=16383, modes=(3, 1)),
    Set("F xdrop 16384", "F", xdrop=16384, modes=(1, 1)),
    Set("F max 127", "F", mat=lambda o: simple_matrix(127), modes=(3, 1)),
    Set("F max 128", "F", mat=lambda o: simple_matrix(128), modes=(1, 1)),
    Set("H separator below int16, xdrop 5000", "H", mat=lambda o: o.build_sub_mat(5000), xdrop=5000, modes=(3, 1)),
    # long_cap
    Set("F long_cap 64", "F", options={"long_cap": 64}),
    Set("F long_cap 8", "F", options={"long_cap": 8}),
    Set("F max 127 long_cap 64", "F", mat=lambda o: simple_matrix(127), options={"long_cap": 64}),
    # crowded chain buckets, and buckets above the sort's capacity (left unsorted)
    Set("F chain_buckets 64", "F", options={"chain_buckets": 64}),
    Set("F chain_group_max 64", "F", options={"chain_group_max": 64}, chain_exact=True),
]
# entropy on: the oracle is the reference
ENTROPY_SETS = [
    Set("F entropy 3099", "F", hspthresh=3099, noentropy=False),
    Set("H entropy", "H", noentropy=False),
    Set("W entropy", "W", noentropy=False),
]

OPTION_SETS = [("default", {}), ("no chain", {"no_chain": 1}), ("byte-coded", {"no_packed_filter": 1}), ("exact filter", {"no_fast_filter": 1}),
               ("byte-coded no chain", {"no_packed_filter": 1, "no_chain": 1})]

QUEUE_SIZES = (1, 63, 64, 65, 64 * 4 * 3 + 1)
QUEUE_OPTIONS = [{"max_waves": 4, "no_packed_filter": 1, "fin_batch": fb} for fb in (1, 48, 64)] + \
                [{"packed_waves": 8, "fin_batch": fb} for fb in (1, 48, 64)]
