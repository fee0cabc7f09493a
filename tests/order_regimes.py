"""Hand-built inputs that put the ordering stage (dedup.hip: the per-segment LDS chain, the one-workgroup unique kernel, the tiled unique
kernels, the strip kernel, and the host step that closes the LDS chain's gaps) at its tile, capacity and segment edges.  Shared by
tests/test_order_regimes.py (CPU: every input is shown, on tests/order_model.py's intermediates, to be in the regime it names) and
tests/test_gpu_order_regimes.py (GPU: sa_order_hsps_segs against the model on those inputs).

Building block (line): records of ONE diagonal, written down in the order the first sort gives them, then shuffled.  The ops

  B   a base record (x, len 50), x advancing by 100: pairwise disjoint, always kept
  C   (b + 10, len 20), b the last base: contained in its sorted predecessor, dropped
  D   an exact copy of its predecessor: dropped by either predicate
  T   its predecessor with the score lowered by 7: a twin.  Kept by the rm chain's first (exact) unique, dropped by containment
  b1 b2   after a base at i - 2: (b + 10, len 20) and (b + 10, len 60).  b1 is inside the base and dropped; b2 CONTAINS b1 and reaches
          past the base, so it is dropped on account of its input neighbour b1 alone -- a unique that compared with the last KEPT
          record (the base) would keep it
  c1 c2   after a base at i - 2: (b + 10, len 5) and (b + 20, len 20).  c1 is dropped; c2 lies inside the base but apart from c1, so
          it is kept -- the non-transitive corner: a compare-with-last-kept unique would drop it

Every Regime carries `facts`, the claims of its construction, as positions in the model's stage lists."""
import functools

import numpy as np

import order_model as M

SEG = M.SEG
DIAG = 5            # the line's diagonal: query_start = ref_start - 5
TOTAL = 131072      # records per call the LDS chain accepts
SEG_CAP = 2048      # records per segment the LDS chain accepts
TILE = 8192         # records per pass of unique_kernel and per tile of the tiled kernels (1024 threads x 8)
THREAD, WAVE = 8, 512


class Regime:
    def __init__(self, name, recs, seg=None, nsegs=1, lds=True, rm_too=False, **facts):
        self.name, self.recs, self.nsegs = name, np.ascontiguousarray(recs, dtype=SEG), int(nsegs)
        self.seg = np.zeros(self.recs.size, dtype=np.uint32) if seg is None else np.ascontiguousarray(seg, dtype=np.uint32)
        self.lds, self.rm_too, self.facts = lds, rm_too, facts
        self._model = {}

    def model(self, rm=False):
        if rm not in self._model:
            self._model[rm] = M.order(self.recs, self.seg, self.nsegs, rm)
        return self._model[rm]

    def stages(self, rm=False):
        return M.global_stages(self.recs, self.seg, self.nsegs, rm)

    def __repr__(self):
        return "Regime(%s, n=%d, nsegs=%d)" % (self.name, self.recs.size, self.nsegs)


def line(n, ops=None, x0=1000, score=3000):
    """n records of the diagonal in first-sort order; ops: {index: op}, B elsewhere.  -> records"""
    ops = ops or {}
    out = np.zeros(n, dtype=SEG)
    x, b = x0, None
    for i in range(n):
        op = ops.get(i, "B")
        if op == "B":
            b = x
            rec = (x, x - DIAG, 50, score + (i * 37) % 11)
            x += 100
        elif op in ("C", "b1"):
            rec = (b + 10, b + 10 - DIAG, 20, score)
        elif op == "b2":
            rec = (b + 10, b + 10 - DIAG, 60, score)
        elif op == "c1":
            rec = (b + 10, b + 10 - DIAG, 5, score)
        elif op == "c2":
            rec = (b + 20, b + 20 - DIAG, 20, score)
        elif op == "D":
            rec = tuple(out[i - 1])
        elif op == "T":
            p = out[i - 1]
            rec = (p["ref_start"], p["query_start"], p["len"], int(p["score"]) - 7)
        else:
            raise ValueError(op)
        out[i] = rec
    return out


def shuffled(recs, seed, seg=None):
    p = np.random.default_rng(seed).permutation(recs.size)
    return (recs[p], seg[p]) if seg is not None else recs[p]


# ---- sizes of the LDS chain ---------------------------------------------------------------------------------------------------------------
LDS_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048)


@functools.lru_cache(maxsize=None)
def size_distinct(m):
    """m2 = m: the second network runs at the same P as the first, with no pad entries when m is a power of two"""
    srt = line(m)
    return Regime("distinct-%d" % m, shuffled(srt, m), sorted0=srt, m=m, m2=m)


@functools.lru_cache(maxsize=None)
def size_tower(m):
    """A0 contains A1 contains A2 ...: every record but the first is dropped, m2 = 1"""
    k = np.arange(m)
    srt = np.zeros(m, dtype=SEG)
    srt["ref_start"], srt["len"], srt["score"] = 5000 + k, 2 * (SEG_CAP + 8 - k), 3000 + k % 7
    srt["query_start"] = srt["ref_start"] - DIAG
    return Regime("tower-%d" % m, shuffled(srt, 100 + m), sorted0=srt, m=m, m2=1)


@functools.lru_cache(maxsize=None)
def size_across(m, m2):
    """m > 1024 records of which m2 in {1023, 1024, 1025} are kept: the second sort runs at another (or just the same) P than the first"""
    drops = m - m2
    assert 0 < drops <= 2 * (m // 3)
    srt = line(m, {3 * (k // 2) + 1 + k % 2: "C" for k in range(drops)})     # B C C B C C ...: the second C repeats the first
    return Regime("across-%d-%d" % (m, m2), shuffled(srt, 7 * m + m2), sorted0=srt, m=m, m2=m2)


# ---- tile edges of the LDS unique ---------------------------------------------------------------------------------------------------------
LDS_THREADS = (64, 192, 1024)


@functools.lru_cache(maxsize=None)
def lds_tile_edge(T, kind):
    """Workgroup size T: the unique loop's tiles begin at sorted indices T and 2T.  kind: "drop" (C at the edge, its predecessor kept),
    "chain" (b1 at T - 1, b2 at T) or "corner" (c1 at T - 1, c2 at T); at least T / 4 drops in every earlier tile, so its in-place
    compaction has moved slots before the edge record reads its neighbour."""
    n = min(SEG_CAP, 2 * T + 40)
    edges = [e for e in (T, 2 * T) if e + 2 <= n]
    ops = {}
    for e in edges:
        if kind == "drop":
            ops[e] = "C"
        elif kind == "chain":
            ops[e - 1], ops[e] = "b1", "b2"
        else:
            ops[e - 1], ops[e] = "c1", "c2"
        for k in range(T // 4 + 1):      # drops in the tile before the edge, well clear of it
            ops[e - T + 2 * k + 3] = "C"
    srt = line(n, ops)
    return Regime("lds-edge-%d-%s" % (T, kind), shuffled(srt, T + len(kind)), sorted0=srt, threads=T, edges=edges, kind=kind,
                  drops=[i for i, o in ops.items() if o in ("C", "b1", "b2", "c1")], keeps=[i for i, o in ops.items() if o == "c2"])


# ---- edges of the library unique kernels --------------------------------------------------------------------------------------------------
LIB_SIZES = (8191, 8192, 8193, 16385, 32768, 32769, 40960, 40961)


def _edges(n, first=(THREAD, 2 * THREAD)):
    e = [x for x in first + (WAVE + THREAD, WAVE, 2 * WAVE, TILE + THREAD, TILE + WAVE, TILE, 2 * TILE, 3 * TILE, 4 * TILE, 5 * TILE) if x < n]
    return sorted(e)


@functools.lru_cache(maxsize=None)
def lib_edges(n, variant):
    """Plain chain, n records in one segment: at multiples of 8 (a thread's first record), 512 (a wave's) and 8192 (a pass's or tile's)
    alternately a drop (C) and a corner keep (c1 c2), `variant` choosing which edges get which."""
    ops, drops, keeps = {}, [], []
    for k, e in enumerate(_edges(n)):
        if (k + variant) % 2 == 0:
            ops[e] = "C"
            drops.append(e)
        else:
            ops[e - 1], ops[e] = "c1", "c2"
            drops.append(e - 1)
            keeps.append(e)
    srt = line(n, ops)
    return Regime("lib-edges-%d-%d" % (n, variant), shuffled(srt, n + variant), lds=False, sorted0=srt, drops=drops, keeps=keeps, n=n)


@functools.lru_cache(maxsize=None)
def lib_edges_rm(n, variant):
    """The rm chain, n records in one segment.  First list (exact unique): at the edges alternately a copy D (dropped) and a twin T (kept).
    Second list, what the first pass kept: at ITS edges alternately a containment drop C and a corner keep c2.  Twins are containment
    drops of the second list wherever they land."""
    e1 = _edges(n, tuple(THREAD * k for k in range(1, 7)))      # (three copies among the first six: the two lists' edges stay apart)
    d1 = {e for k, e in enumerate(e1) if (k + variant) % 2 == 0}
    t1 = {e for k, e in enumerate(e1) if (k + variant) % 2 == 1}
    ops2 = {}
    for k, e in enumerate(_edges(n - len(d1) - 2, (9 * THREAD, 10 * THREAD))):
        if (k + variant) % 2 == 0:
            ops2[e] = "C"
        else:
            ops2[e - 1], ops2[e] = "c1", "c2"
    ops, j, drops1, keeps1, drops2, keeps2 = {}, 0, [], [], [], []
    for i in range(n):
        if i in d1:
            ops[i] = "D"
            drops1.append(i)
            continue
        if i in t1:
            ops[i] = "T"
            keeps1.append(i)
            drops2.append(j)
        else:
            op = ops2.get(j, "B")
            if op != "B":
                assert (i - 1) not in d1 and (i - 1) not in t1 and (i + 1) not in d1 and (i + 1) not in t1, (n, variant, i, j)
                ops[i] = op
                (keeps2 if op == "c2" else drops2).append(j)
        j += 1
    first = line(n, ops)
    return Regime("lib-edges-rm-%d-%d" % (n, variant), shuffled(first, 3 * n + variant), lds=False, rm_too=True, sorted0_rm=first,
                  drops1=drops1, keeps1=keeps1, drops2=drops2, keeps2=keeps2, n=n, n1=n - len(drops1))


# ---- segments, path 0 ---------------------------------------------------------------------------------------------------------------------
SEG_COUNTS = (1, 2, 8, 511, 512)


@functools.lru_cache(maxsize=None)
def seg_mix(nsegs):
    """Segments of different sizes with drops in each, ids interleaved.  From 8 segments on, segments 0, nsegs // 2 and nsegs - 1 are empty.
    Neighbouring used segments share one identical record, and a pair that would merge (base + C) is split between them."""
    empty = {0, nsegs // 2, nsegs - 1} if nsegs >= 8 else set()
    used = [g for g in range(nsegs) if g not in empty]
    big = nsegs <= 8
    parts, segs, want_counts = [], [], np.zeros(nsegs, dtype=np.uint32)
    for k, g in enumerate(used):
        n = (40 + 397 * k) if big else 1 + (g * 7) % 5
        ops = {i: "C" for i in range(1, n, 3)}
        own = line(n, ops, x0=1000 + 13 * g)
        extra = []
        if k + 1 < len(used):          # shared with the next used segment, and the base of a split pair
            extra += [(9_000_000 + 100 * k, 9_000_000 + 100 * k - DIAG, 50, 2500), (8_000_000 + 100 * k, 8_000_000 + 100 * k - DIAG, 50, 2400)]
        if k > 0:                      # the shared record again, and the contained half of the split pair
            extra += [(9_000_000 + 100 * (k - 1), 9_000_000 + 100 * (k - 1) - DIAG, 50, 2500),
                      (8_000_000 + 100 * (k - 1) + 10, 8_000_000 + 100 * (k - 1) + 10 - DIAG, 20, 2400)]
        r = np.concatenate([own, np.array(extra, dtype=SEG)]) if extra else own
        parts.append(r)
        segs.append(np.full(r.size, g, dtype=np.uint32))
        want_counts[g] = r.size - len(ops)
    recs, seg = shuffled(np.concatenate(parts), 50 + nsegs, np.concatenate(segs))
    return Regime("seg-mix-%d" % nsegs, recs, seg, nsegs, empty=sorted(empty), counts=want_counts, used=used)


@functools.lru_cache(maxsize=None)
def seg_last_only():
    """512 segments of which only segment 511 holds records: its slot offset is the sum of 511 empty counts"""
    srt = line(300, {i: "C" for i in range(1, 300, 4)})
    return Regime("seg-last-only", shuffled(srt, 511), np.full(300, 511, dtype=np.uint32), 512,
                  counts=np.array([0] * 511 + [300 - 75], dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def seg_full():
    """64 segments x 2048 distinct records = 131072: the call's total limit with every segment at capacity"""
    one = line(SEG_CAP)
    recs = np.tile(one, 64)
    recs["score"] += np.repeat(np.arange(64, dtype=np.int32), SEG_CAP)     # (the segments differ)
    seg = np.repeat(np.arange(64, dtype=np.uint32), SEG_CAP)
    recs, seg = shuffled(recs, 64, seg)
    return Regime("seg-full", recs, seg, 64, counts=np.full(64, SEG_CAP, dtype=np.uint32))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refusal(kind):
    """-> Regime with facts seg_max, count_on_device ("both" or True) and refused"""
    if kind in ("cap100-100", "cap100-101"):
        m = int(kind[-3:])
        srt = line(m, {1: "C", 50: "C"})
        return Regime(kind, shuffled(srt, m), seg_max=100, refused=m > 100, on_device="both")
    if kind in ("default-2048", "default-2049"):
        m = int(kind[-4:])
        srt = line(m, {1: "C", 2047: "C"})
        return Regime(kind, shuffled(srt, m), seg_max=0, refused=m > SEG_CAP, on_device="both")
    if kind == "one-oversized":       # segment 2 of 5 holds 2049 records, the others a few dozen
        parts = [line(30 + g, {1: "C"}, x0=1000 + g) if g != 2 else line(SEG_CAP + 1, {5: "C"}) for g in range(5)]
        seg = np.concatenate([np.full(p.size, g, dtype=np.uint32) for g, p in enumerate(parts)])
        recs, seg = shuffled(np.concatenate(parts), 5, seg)
        return Regime(kind, recs, seg, 5, seg_max=0, refused=True, on_device="both")
    if kind == "total-131073":        # 65 segments, none above capacity: only the device-side count refuses
        n = TOTAL + 1
        one = line(n)
        seg = (np.arange(n) % 65).astype(np.uint32)
        recs, seg = shuffled(one, 65, seg)
        return Regime(kind, recs, seg, 65, seg_max=0, refused=True, on_device=True)
    raise ValueError(kind)


REFUSALS = ("cap100-100", "cap100-101", "default-2048", "default-2049", "one-oversized", "total-131073")


# ---- segments, path 1 ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lib_seg_breaks(n):
    """Path 1, plain and rm: one line cut into segments exactly at a thread edge (8), a wave edge (512), a tile edge (8192) and, where n
    allows, 32768; the first record of each later segment is a C of the last record of the segment before it, so only the segment test
    of the unique predicate keeps it."""
    cuts = [c for c in (THREAD, WAVE, TILE, 4 * TILE) if c + 1 < n]
    srt = line(n, {c: "C" for c in cuts})
    seg = np.searchsorted(np.array(cuts), np.arange(n), side="right").astype(np.uint32)
    recs, sg = shuffled(srt, n, seg)
    return Regime("lib-seg-breaks-%d" % n, recs, sg, len(cuts) + 1, lds=False, rm_too=True, cuts=cuts, sorted0=srt, sorted_seg=seg)


@functools.lru_cache(maxsize=None)
def lib_strip_stride():
    """600000 distinct records in 3 interleaved segments: more kept records than the strip kernel's 2048 x 256 threads"""
    n = 600_000
    k = np.arange(n, dtype=np.int64)
    recs = np.zeros(n, dtype=SEG)
    recs["ref_start"], recs["len"], recs["score"] = 1000 + 100 * k, 50, 3000 + k % 13
    recs["query_start"] = recs["ref_start"] - DIAG - (k % 4)       # four diagonals
    seg = (k % 3).astype(np.uint32)
    recs, seg = shuffled(recs, 600, seg)
    return Regime("lib-strip-stride", recs, seg, 3, lds=False, rm_too=True, kept=n)


# ---- magnitudes ---------------------------------------------------------------------------------------------------------------------------
MAGNITUDES = ("ends", "diagonals", "lens", "scores")


@functools.lru_cache(maxsize=None)
def magnitudes(kind):
    """One segment, a few hundred to a few thousand records drawn from small pools, so that ties, twins and containments abound."""
    rng = np.random.default_rng({"ends": 1, "diagonals": 2, "lens": 3, "scores": 4}[kind])
    n = 1500
    top = 1 << 32
    if kind == "ends":         # ref_start + len on both sides of 2^32
        r = top - 1 - rng.integers(0, 160, n)
        ln = rng.choice([0, 10, 40, 80, 159, 160, 161, 300], n) + rng.integers(0, 2, n)
        q = r - rng.choice([3, 4], n)
        sc = 3000 + 10 * rng.integers(0, 4, n)
    elif kind == "diagonals":  # query_start > ref_start; diagonals 0 and 2^32 - 1 next to each other in the first sort
        r = 500 + rng.integers(0, 120, n)
        q = r + rng.choice([0, 1], n)
        ln = rng.choice([5, 17, 40, 41, 80], n)
        sc = 3000 + 10 * rng.integers(0, 4, n)
    elif kind == "lens":       # len 0 and 2^32 - 1
        r = 700 + rng.integers(0, 60, n)
        q = r - rng.choice([0, 2], n)
        ln = rng.choice([0, 0, 1, 30, 61, top - 1, top - 1, top - 2], n)
        sc = 3000 + 10 * rng.integers(0, 3, n)
    else:                      # score ties across INT32_MIN, -1, 0 and INT32_MAX; twins that differ in score only
        r = 900 + 10 * rng.integers(0, 12, n)
        q = r - rng.choice([1, 2], n)
        ln = rng.choice([20, 40], n)
        sc = rng.choice([-(1 << 31), -(1 << 31) + 1, -1, 0, 1, (1 << 31) - 2, (1 << 31) - 1], n)
    recs = np.zeros(n, dtype=SEG)
    recs["ref_start"], recs["query_start"], recs["len"], recs["score"] = r, q, ln, sc
    return Regime("magnitudes-" + kind, recs, rm_too=True, kind=kind)


def all_regimes(big=True):
    """Every designed set (the CPU model test walks them all)."""
    out = []
    for m in LDS_SIZES:
        out += [size_distinct(m), size_tower(m)]
        if m > 1024:
            out += [size_across(m, m2) for m2 in (1025, 1024, 1023) if m2 < m]
    out += [lds_tile_edge(T, kind) for T in LDS_THREADS for kind in ("drop", "chain", "corner")]
    out += [lib_edges(n, v) for n in LIB_SIZES for v in (0, 1)] + [lib_edges_rm(n, v) for n in LIB_SIZES for v in (0, 1)]
    out += [seg_mix(k) for k in SEG_COUNTS] + [seg_last_only()]
    out += [refusal(k) for k in REFUSALS if big or k != "total-131073"]
    out += [lib_seg_breaks(n) for n in (9000, 40961)]
    out += [magnitudes(k) for k in MAGNITUDES]
    if big:
        out += [seg_full(), lib_strip_stride()]
    return out
