"""Hand-built inputs for the two X-drop filter levels (extend.hip 1d, 1b), held to tests/filter_model.py by tests/test_filter_model.py
(CPU: every world is in the regimes it names, shown from the model) and tests/test_gpu_filter_verdicts.py (GPU: every verdict of every
call equals the model).

A WORLD is one target block and one query block made of ISLANDS -- stretches the two blocks share, long enough to seed -- between filler
that mismatches on every diagonal (target A against query C under HOXD70, A against G under the simple matrix, where the class of A / C
also holds G / T = -1).  Every seed window inside an island is a hit of the call, so a feature behind a clean run lies at EVERY offset
from some anchor: a dip whose bottom falls on the end of a six-base field from one anchor lies one base before and behind it from the
neighbouring ones, and each strand sees it from its own side.  What a world was built for is written down as CLAIMS: predicates on the
model's per-hit results, each of which must hold for at least one hit of the named call."""
import functools

import numpy as np

import filter_model as F
import image_model as IM
import table_model as TM
from extend_regimes import hoxd_total, simple_matrix
from helpers import SHAPE_12OF19

A, C, G, T, L, N, X, E = range(8)
ASCII = np.frombuffer(b"ACGTaNR&", dtype=np.uint8)
FILL = 16


class Builder:
    """target and query code lists; an island goes to both, at the two cursors"""

    def __init__(self, hoxd):
        self.hoxd, self.t, self.q = hoxd, [], []
        self.fill_pair = (A, C) if hoxd else (A, G)      # (A against T would seed on the minus strand: poly-A against poly-A)
        # class of a score under the matrix: a pattern item is a class score, or an explicit (target, query) pair
        self.cls_of = {100: 0, -114: 1, -31: 2, -123: 3} if hoxd else {100: 0, -1: 1, -100: 3}
        self._lcg = 4711

    def _rand4(self):
        self._lcg = (self._lcg * 1103515245 + 12345) & 0x7FFFFFFF
        return (self._lcg >> 16) & 3

    def pair(self, item):
        if isinstance(item, tuple):
            return item
        r = self._rand4()
        if not self.hoxd and item == -1:
            r = (G, T)[r & 1]
        return r, r ^ self.cls_of[item]

    def codes(self, pattern):
        p = [self.pair(i) for i in pattern]
        return [a for a, _ in p], [b for _, b in p]

    def fill(self, n=FILL, t=True, q=True):
        if t:
            self.t += [self.fill_pair[0]] * n
        if q:
            self.q += [self.fill_pair[1]] * n

    def island(self, pattern, fill=FILL):
        tc, qc = self.codes(pattern)
        self.t += tc
        self.q += qc
        self.fill(fill)

    def split(self, pattern):
        """an island whose two halves are placed on their own (block starts and ends)"""
        return self.codes(pattern)


class World:
    def __init__(self, name, b, mat, xdrop, hspthresh, shape=SHAPE_12OF19, big=False):
        self.name, self.mat, self.xdrop, self.hspthresh = name, np.asarray(mat, dtype=np.int32), xdrop, hspthresh
        self.shape_text, self.S = shape, TM.Shape(shape)
        if isinstance(b, Builder):
            self.target, self.query = ASCII[np.array(b.t, dtype=np.uint8)], ASCII[np.array(b.q, dtype=np.uint8)]
        else:
            self.target, self.query = (np.ascontiguousarray(x, dtype=np.uint8) for x in b)
        self.big, self.sparse = big, None
        assert big or (self.target.size < 65536 and self.query.size < 65536), name
        self.tc, self.qc = IM.codes(self.target), IM.codes(self.query)
        self.qrc = IM.rev_comp(self.qc)
        self._cache = {}

    def __repr__(self):
        return "<world %s>" % self.name

    def flipped(self):
        """the same world with the query block reverse-complemented: its MINUS strand is this world's plus strand"""
        if "flipped" not in self._cache:
            q = ASCII[IM.rev_comp(self.qc)]
            assert np.array_equal(IM.codes(q), self.qrc), self.name       # (one letter per code)
            self._cache["flipped"] = World(self.name + " flipped", (self.target, q), self.mat, self.xdrop, self.hspthresh, self.shape_text, self.big)
            self._cache["flipped"]._cache["table"] = self.table
        return self._cache["flipped"]

    @property
    def table(self):
        if "table" not in self._cache:
            self._cache["table"] = F.Table(self.tc, self.S, 1, True, sparse=self.sparse)
            # (a larger bucket keeps its arrival order in the device's table: the call order of its hits would not be the model's)
            assert self._cache["table"].bucket.max() <= TM.SORT_MAX, self.name
        return self._cache["table"]

    @property
    def end(self):
        """one past the last query position whose seed window lies inside the block"""
        return max(self.query.size - self.S.span + 1, 0)

    def strand(self, rev):
        return (self.qrc, self.qc) if rev else (self.qc, self.qrc)

    def params(self, **kw):
        opt = dict(left_skip=self.S.span if kw.pop("ctx_skip_seed", 1) else 0)
        opt.update(kw)
        return F.Params(self.S.span, kw.pop("xdrop", self.xdrop), self.hspthresh, **{k: v for k, v in opt.items() if k != "xdrop"})

    def verdicts(self, rev, start=0, end=None, ctx=True, detail=False, **kw):
        """the model of one call (cached): kw = the options that are model inputs (ctx_skip_seed, l2_right_state, long_cap, xdrop,
        rm_window)"""
        end = self.end if end is None else end
        key = (rev, start, end, ctx, detail, tuple(sorted(kw.items())))
        if key not in self._cache:
            own, other = self.strand(rev)
            self._cache[key] = F.call(self.table, self.tc, own, other, self.mat, start, end, self.params(**kw), ctx=ctx, detail=detail)
        return self._cache[key]

    def hits_before(self, rev):
        """exclusive count of the strand's hits in front of every query position (and behind the last)"""
        key = ("ex", rev)
        if key not in self._cache:
            keys = F.PM.position_keys(self.strand(rev)[0], self.S)
            cnt = np.where(keys >= 0, self.table.run[np.maximum(keys, 0)], 0)
            self._cache[key] = np.concatenate([[0], np.cumsum(cnt)])
        return self._cache[key]

    def range_with(self, rev, n):
        """a range of query positions [s, e) whose call has exactly n hits (two pointers over the positions' hit counts), or None"""
        ex = self.hits_before(rev)
        i = 0
        for j in range(1, ex.size):
            while ex[j] - ex[i] > n:
                i += 1
            if ex[j] - ex[i] == n and n > 0:
                return i, j
        return None


# ---- patterns ---------------------------------------------------------------------------------------------------------------------------
def kit(hoxd):
    """the dips in CLASS scores: exactly xdrop deep, and one more"""
    if hoxd:      # classes 100 / -114 / -31 / -123, xdrop 910
        return dict(xdrop=910, exact=[-123] + [-114] * 5 + [-31] * 7, over=[-114] * 5 + [-31] * 11)
    return dict(xdrop=1000, exact=[-100] * 10, over=[-100] * 10 + [-1])   # classes 100 / -1 / -100 / -100, xdrop 1000


def class_total(hoxd, total):
    """a clean run of 26 matches, then single class mismatches with a match between them: the class scores add up to `total`, no prefix
    from either end dips by more than one mismatch"""
    if not hoxd:
        q, r = divmod(total, 100)
        neg = [-1] * ((100 - r) % 100)
        n_match = q + (1 if r else 0)
    else:
        best = None
        for b in range(13):
            for c in range(13):
                for d in range(13):
                    rest = total + 31 * b + 114 * c + 123 * d
                    if rest % 100 == 0 and (best is None or b + c + d < len(best[1])):
                        best = (rest // 100, [-31] * b + [-114] * c + [-123] * d)
        n_match, neg = best
    assert n_match >= 26 + len(neg) + 1, (total, n_match, len(neg))
    pat = [100] * 26
    for v in neg:
        pat += [100, v]
    return pat + [100] * (n_match - 26 - len(neg))


def run(n):
    return [100] * n


def main_world(name, hoxd, mat, xdrop=None, extra=(), shape=SHAPE_12OF19):
    """runs, dips, thresholds, block starts and ends: the walks of level 1 and the windows of level 2"""
    k = kit(hoxd)
    b = Builder(hoxd)
    h = 3000
    far = 100                                     # island bases at a block edge: anchors up to 81 bases from it
    # block starts: island a at the target's start, island c at the query's
    at, aq = b.split(run(far))
    ct, cq = b.split(run(far))
    dt, dq = b.split(run(far))
    et, eq = b.split(run(far))
    b.t += at
    b.fill(t=True, q=False)
    b.q += cq
    b.fill(t=False, q=True)
    b.q += aq
    b.fill(t=False, q=True)
    b.t += ct
    b.fill(t=True, q=False)
    for n in (19, 20, 24, 25, 26, 30, 31, 60, 140, 260):         # homology of every length: flags 1, 2, 3, long_cap 64 .. 192
        b.island(run(n))
    for dip in (k["exact"], k["over"]):                              # drops of xdrop and xdrop + 1 at every offset, both directions
        b.island(run(90) + dip + run(90))
        b.island(run(90) + dip[::-1] + run(90))
        b.island(run(40) + dip + run(25) + dip + run(40))          # a best behind a drop
    # a left side that is still alive at the end of its context at a modest score, a few matches just behind the context, then filler:
    # level 2 resumes at 58 + left_skip bases and its verdict hangs on the total -- resumed 19 bases early it scores the zigzag twice
    mm = -114 if hoxd else -100
    for r in range(1, 11):                                            # (the right side's best: the total crosses hspthresh along r)
        for far in ([100, mm] * 10, [100, 100, mm] * 7):              # scored twice, the far end of the context costs, or pays
            for behind in (6, 11):
                walk = [100, mm] * 19 + far[:20]                      # the 58 context bases in walking order, from the seed leftwards
                b.island(run(behind) + walk[::-1] + run(len(shape) + r))
    # (the best of a side is taken over its whole context, also behind a drop: an island that is to stand alone has 64 filler bases
    #  on either side)
    b.fill(64 - FILL)
    for tot in (h - 1, h, h + 1) if hoxd else (h - 1, h):            # both sides dropped, the class bound at the threshold
        b.island(class_total(hoxd, tot), fill=64)
        b.island(class_total(hoxd, tot)[::-1], fill=64)
    if hoxd:                                                        # exact pair totals at the threshold under a class bound above it
        for tot in (h - 1, h):
            b.island([(c, c) if s > 0 else s for s, c in zip(hoxd_total(tot), _letters(hoxd_total(tot)))], fill=64)
    for item in extra:
        b.island(item, fill=64)
    # block ends: island d at the target's end, island e at the query's
    b.q += dq
    b.fill(t=False, q=True)
    b.t += et
    b.fill(t=True, q=False)
    b.t += dt
    b.q += eq
    return World(name, b, mat, k["xdrop"] if xdrop is None else xdrop, h, shape=shape)


def _letters(scores):
    """the letter of every match of an exact HOXD70 pattern: 100 = C / G, 91 = A / T"""
    out, i = [], 0
    for s in scores:
        i += 1
        out.append(((C, G)[i & 1] if s == 100 else (A, T)[i & 1]) if s > 0 else None)
    return out


def codes_world(name, mat):
    """N, soft-masked and IUPAC letters inside either context, in the target and in the query: the presence masks raise the class scores"""
    b = Builder(True)
    b.fill()
    for code in (L, N, X):
        for side in (0, 1):
            for at in (3, 30, 70):
                pat = run(100)
                r = b._rand4()
                pat[at if side == 0 else 99 - at] = (code, r) if side == 0 else (r, code)
                b.island(pat)
    b.island(run(40))
    return World(name, b, mat, 910, 3000)


def field1_world(name, mat):
    """xdrop 351 = 123 + 2 x 114: six bases can drop -- the first field of either side.  352 = 4 x 31 + 2 x 114"""
    b = Builder(True)
    b.fill()
    for dip in ([-123, -114, -114], [-31] * 4 + [-114] * 2, [-123, -123, -114]):   # 351, 352, and 360 in three bases: deeper INSIDE a field
        for lead in range(0, 4):                                    # the dip's bottom on the last base of field 1, and around it
            b.island(run(30) + run(lead) + dip + run(60))             # (60: the filler behind it lies outside the context)
            b.island(run(60) + dip[::-1] + run(lead) + run(30))
    return World(name, b, mat, 351, 3000)


def repeat_world(name, mat, copies=140):
    """one query position with more than 128 hits (a key with `copies` target positions), records of one hit in rows of 64 and more
    (islands of unique sequence), records that start on every lane"""
    b = Builder(True)
    unit_t, unit_q = b.split(run(19))
    b.fill()
    for _ in range(copies):
        b.t += unit_t
        b.fill(5, t=True, q=False)
    b.fill(t=True, q=False)
    b.q += unit_q
    b.fill(t=False, q=True)
    for n in (19 + 63, 19 + 64, 19 + 200):                          # 64, 65 and 201 consecutive one-hit records
        b.island(run(n))
    return World(name, b, mat, 910, 3000)


def stage_world(name, mat):
    """the class filter's stage at its capacity of 95 records: 33 islands of one seed window each (one hit, rejected: 1900 + what the
    neighbours add stays below hspthresh), then one island of 95 seed windows, every one forwarded -- the first buffer of the call's one
    wave ends with 31 records staged (below the flush mark of 32), the second adds 64"""
    b = Builder(True)
    b.fill(20)
    for _ in range(33):
        b.island(run(19), fill=20)
    b.fill(44)                                  # (the long island outside the last short one's right context)
    b.island(run(19 + 94), fill=20)
    return World(name, b, mat, 910, 3000)


def stage_peaks(fwd, n_hits, wave_chunks=None):
    """records in a wave's stage after every buffer's append, before its flush: per wave (a list of chunk ranges [c_lo, c_hi); default one
    wave over the whole call) the stage takes a buffer's forwards, and once 32 or more are pending flushes up to 64 of them"""
    peaks = []
    for c_lo, c_hi in (wave_chunks or [(0, (n_hits + 4095) // 4096)]):
        n = 0
        for b in range(c_lo * 64, min(c_hi * 64, (n_hits + 63) // 64)):
            f = int(np.count_nonzero(fwd[64 * b:64 * b + 64]))
            peaks.append((n, f))
            n += f
            if n >= 32:
                n -= min(n, 64)
    return peaks


SHAPE_14OF22 = "TTT0T0TT00TT00T0T0TTTT"      # src/main.cpp:164-167, as tests/test_gpu_edge_cases.py runs it


def self_world(name, mat, n=3000, seed=11):
    """a block against itself: nearly every hit is forwarded, whole buffers of 64 forwards"""
    rng = np.random.default_rng(seed)
    s = ASCII[rng.integers(0, 4, n).astype(np.uint8)]
    return World(name, (s, s.copy()), mat, 910, 3000)


@functools.lru_cache(maxsize=None)
def worlds(hoxd_mat):
    hm = np.array(hoxd_mat, dtype=np.int32)
    sm = simple_matrix()
    # simple matrix: the class of A / C also holds G / T = -1, so an A / C pair (-100) costs the class bound 1: 31 matches with one of
    # them total 3000 exactly, with a G / T pair as well 2999, under class bounds of 3099 and 3098
    s_extra = [run(26) + [100, (A, C), 100, 100, 100, 100], run(26) + [100, (A, C), 100, (G, T), 100, 100, 100]]
    w = [main_world("H", True, hm), main_world("S", False, sm, extra=s_extra), codes_world("codes", hm), field1_world("field1", hm),
         repeat_world("repeat", hm), self_world("self", hm), synth_world("synth", hm), stage_world("stage", hm),
         main_world("H22", True, hm, shape=SHAPE_14OF22)]
    return {x.name: x for x in w}


def synth_world(name, mat, n=60000, big=False, **kw):
    """a diverged pair with soft-masked runs, N runs, indels and record separators (segalign_amd.synth)"""
    from segalign_amd import synth
    opt = dict(sub_rate=0.10, mask_frac=0.2, records=2, indel_every=120, n_runs=2)
    opt.update(kw)
    t, q = synth.make_pair(n, 81, 82, **opt)
    return World(name, (t, q), mat, 910, 3000, big=big)


STREAM_SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
