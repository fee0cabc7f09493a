"""Hand-built calls that put the front of a table-direct call -- probe_kernel, probe_partials_kernel, probe_compact_kernel with
call_clear_kernel, probe_plan_kernel (probe.hip), driven by td_front (front.hip) -- on its edges (DESIGN.md 4.4').  Shared by
tests/test_probe_regimes.py (CPU: every call is in the regime it names, tests/probe_model.py equals the oracle where the oracle can
speak) and tests/test_gpu_probe_regimes.py (GPU: what sa_probe_call returns against the model, array by array).

TARGETS are built as tests/table_regimes.py builds them: non-overlapping windows (step = span + 1), the members of every bucket dealt
round-robin.  Every key that gets a bucket has all its fields in {A, C} or is a transition neighbour of such a key (one field in
{G, T}), so the runs of different {A, C} keys share no bucket: the run of each, and the pieces it is made of, are chosen freely.

QUERIES come in two forms, joined freely:
  * windows: `span` bases and one N, over and over -- only the window starts are valid positions, each with a key of its own;
  * stretches: a periodic text over {A, C} -- every position is valid, the positions share the few keys of the period, and one long
    run gives hundreds of hits per position for a few hundred target entries.

The values below restate constants of probe.hip / front.hip / kernels.h; the regime a call claims ties it to them."""
import functools

import numpy as np

import probe_model as PM
import table_model as M
import table_regimes as R

PR_TILE = 1024               # positions per workgroup of probe_kernel / probe_compact_kernel (256 threads x 4)
HB_LDS_WORDS = 4096          # head-bit words a workgroup of the compaction gathers in LDS
PP_TILE = 1024               # workgroup sums per workgroup of probe_partials_kernel
TD_CHUNK_HITS = PM.TD_CHUNK_HITS
HEAD_WORDS_MIN = 1 << 16     # td_front: the head-bit map of a slot starts at max(4 n + 64, 2^16) words
MAX_CHUNKS = 256             # SA_MAX_CHUNKS

SHAPE_W9, SHAPE_12OF19 = R.SHAPE_W9, R.SHAPE_12OF19
SHAPE_W9_SHORT = "TTTTT0TTTT"     # weight 9 in ten bases: a run of 8200 entries is 8200 windows of 11 bases, 90 kb of target
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def ac_key(shape, i):
    """the i-th key whose fields are all A or C (bit b of i: field b is a C)"""
    S = shape if isinstance(shape, M.Shape) else M.Shape(shape)
    return int("".join("01"[(i >> b) & 1] for b in range(S.weight)), 4)


def unit_keys(shape, unit):
    """the keys of the positions of a stretch of period `unit`, in the order of the phase"""
    S = M.Shape(shape)
    text = (unit * (S.span // len(unit) + 3))[:S.span + len(unit) - 1]
    return PM.position_keys(M.encode(np.frombuffer(text.encode(), dtype=np.uint8)), S).tolist()


class World:
    """a target, its seed shape and the options of the engine: what InitializeProcessor .. GenerateSeedPosTable get"""

    def __init__(self, name, shape, runs, transition=True, options=None, seed=1):
        """runs: {key: pieces}; pieces = entries of the key's own bucket, or the list of the entries of every piece of its run"""
        self.name, self.shape_text, self.S = name, shape, M.Shape(shape)
        self.transition, self.options = bool(transition), dict(options or {})
        masks = self.S.masks(True)
        sizes = {}
        for k, pieces in runs.items():
            pieces = [pieces] if isinstance(pieces, int) else list(pieces)
            assert len(pieces) <= len(masks)
            for m, n in zip(masks, pieces):
                if n:
                    assert (k ^ m) not in sizes, "two runs share a bucket"
                    sizes[k ^ m] = n
        self.target, self.step = R.windows(shape, R.spread(sorted(sizes.items())), seed=seed)
        self.runs = dict(runs)

    @classmethod
    def from_text(cls, name, shape, target, step, transition=True, options=None):
        """a world around a target that is given, not built"""
        w = cls.__new__(cls)
        w.name, w.shape_text, w.S = name, shape, M.Shape(shape)
        w.transition, w.options = bool(transition), dict(options or {})
        w.target, w.step, w.runs = np.ascontiguousarray(target, dtype=np.uint8), int(step), {}
        return w

    def __repr__(self):
        return "<world %s>" % self.name

    @functools.cached_property
    def codes(self):
        return M.encode(self.target)

    @functools.cached_property
    def table(self):
        return PM.Table(self.codes, self.S, self.step, self.transition)

    def variant(self, name, transition=None, options=None):
        w = World.__new__(World)
        w.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("table",)})
        w.name = name
        if transition is not None:
            w.transition = bool(transition)
        if options is not None:
            w.options = dict(options)
        return w


def rev_comp_codes(codes):
    """the minus strand of encoded sequence: reversed, A <-> T and C <-> G, every other code as it is"""
    c = np.asarray(codes, dtype=np.uint8)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)


_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMPLEMENT[_a] = _b


class TextQuery:
    """a query given as text: the target as its own query (the repeat masker's case), or the reverse complement of a built query, whose
    minus strand then holds that query's positions"""

    def __init__(self, S, text, marks=None):
        self.S, self.text, self.marks = S, np.ascontiguousarray(text, dtype=np.uint8), dict(marks or {})
        self.size = self.text.size

    def codes(self, rev=False):
        c = M.encode(self.text)
        return rev_comp_codes(c) if rev else c

    def keys(self, rev=False):
        cache = self.__dict__.setdefault("_keys", {})
        if rev not in cache:
            cache[rev] = PM.position_keys(self.codes(rev), self.S)
        return cache[rev]


def reverse_complement(query):
    return TextQuery(query.S, _COMPLEMENT[query.text[::-1]], query.marks)


class Query(TextQuery):
    """ASCII text put together from windows, stretches and filler"""

    def __init__(self, shape, seed=7):
        self.S = M.Shape(shape)
        self.shape_text = shape
        self.parts, self.size, self.seed = [], 0, seed
        self.marks = {}

    def _add(self, a):
        a = np.asarray(a, dtype=np.uint8)
        self.parts.append(a)
        self.size += a.size
        self.__dict__.pop("text", None)
        return self

    def mark(self, name):
        self.marks[name] = self.size
        return self

    def windows(self, keys):
        """one window per key (-1: a window with an N at its first care position), each followed by one N: position of window i =
        where the part starts + i (span + 1)"""
        keys = np.asarray(keys, dtype=np.int64)
        if keys.size == 0:
            return self
        self.seed += 1
        t, step = R.windows(self.shape_text, keys, seed=self.seed)
        t = np.concatenate([t[step:], [ord("N")]])
        t[self.S.span::step] = ord("N")
        assert t.size == step * keys.size
        return self._add(t)

    def stretch(self, unit, npos):
        """npos valid positions of period `unit` (span - 1 positions whose window runs into the N behind them follow)"""
        n = npos + self.S.span - 1
        text = (unit * (n // len(unit) + 1))[:n] + "N"
        return self._add(np.frombuffer(text.encode(), dtype=np.uint8))

    def fill(self, n, letter="N"):
        return self._add(np.full(n, ord(letter), dtype=np.uint8))

    def fill_to(self, pos, letter="N"):
        assert pos >= self.size, (pos, self.size)
        return self.fill(pos - self.size, letter)

    def put(self, pos, letter):
        """overwrite one base"""
        self.text[pos] = ord(letter)
        self.__dict__.pop("_keys", None)
        return self

    @functools.cached_property
    def text(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=np.uint8)


class Call:
    """one sa_probe_call: [start, end) of a strand of a query under a chunk size and a MAX_HITS (0: the engine's own)"""

    def __init__(self, name, world, query, start, end, chunk=250000, rev=False, buffer=0, max_hits=0, rm=False, claims=None):
        self.name, self.world, self.query = name, world, query
        self.start, self.end, self.chunk = int(start), int(end), int(chunk)
        self.rev, self.buffer, self.max_hits, self.rm = bool(rev), int(buffer), int(max_hits), bool(rm)
        self.claims = dict(claims or {})

    def __repr__(self):
        return "<call %s>" % self.name

    @property
    def clipped_end(self):
        """a seed window must lie inside the query"""
        return min(self.end, max(self.query.size - self.world.S.span + 1, 0))

    @property
    def num_chunks(self):
        """from the unclipped end, as the chunked entry counts them"""
        return (self.end - self.start + self.chunk - 1) // self.chunk if self.end > self.start else 0

    @property
    def grid_chunk(self):
        return self.chunk if self.num_chunks > 1 else self.clipped_end - self.start

    def model(self, max_hits=None):
        mh = int(max_hits if max_hits is not None else (self.max_hits or DEFAULT_MAX_HITS))
        cache = self.__dict__.setdefault("_model", {})
        if mh not in cache:
            cache.clear()
            cache[mh] = PM.probe(self.world.table, self.query.keys(self.rev), self.start, self.clipped_end, self.grid_chunk, self.num_chunks, mh,
                                 rm=self.rm, head_bits=not self.world.options.get("no_ctx"))
        return cache[mh]

    def facts(self, max_hits=None):
        """what the regimes are named after, from the model alone"""
        m = self.model(max_hits)
        n = self.clipped_end - self.start
        skew = self.start & 3
        cnt = m["t_cnt"].astype(np.int64)
        grid = np.zeros((n + skew + PR_TILE - 1) // PR_TILE * PR_TILE, dtype=np.int64)    # element e of the grid = position e - skew
        grid[skew:skew + n] = cnt
        tiles = grid.reshape(-1, PR_TILE)
        tile_hits = tiles.sum(axis=1)
        base = np.concatenate([[0], np.cumsum(tile_hits)])[:-1]
        words = np.where(tile_hits > 0, ((base + tile_hits - 1) >> 5) - (base >> 5) + 1, 0)
        pl = m["plans"]
        return {"n": n, "skew": skew, "len_mod4": n & 3, "K": self.num_chunks, "hits": m["hits"], "records": m["num_records"],
                "valid": int(m["bounds"]["valid"][-1]), "tiles": int(tiles.shape[0]), "tile_hits": tile_hits.tolist(),
                "tile_nonempty": (tiles > 0).sum(axis=1).tolist(), "tile_words": words.tolist(), "tile_base": base.tolist(),
                "n_iter": pl["n_iter"].tolist(), "chunk_hits": pl["num_hits"].tolist(), "ret": m["ret"],
                "head_words": ((m["hits"] + 63) >> 6) * 2 + 16, "max_run": int(cnt.max()) if n else 0}


# ---- the oracle's side of a call (the CPU tests, and the GPU tests that tie a plan to what a real call returns) ------------------------------
_oracle_tables = {}


def oracle_side(oracle, call):
    """(target codes, index, positions sorted per bucket, query ASCII of the strand, query codes of the strand)"""
    w = call.world
    if id(w.target) not in _oracle_tables:
        assert oracle.generate_shape_pos(w.S.text) == w.S.weight
        index, pos = oracle.generate_seed_pos_table(w.target.tobytes(), 0, w.target.size, w.step, w.S.span, w.S.weight)
        _oracle_tables[id(w.target)] = (oracle.encode(w.target.tobytes()), index, M.canonical(index, pos))
    ref, index, pos = _oracle_tables[id(w.target)]
    assert oracle.generate_shape_pos(w.S.text) == w.S.weight
    text = call.query.text
    fw, rc = oracle.encode_rev_comp(text.tobytes())
    assert np.array_equal(call.query.codes(False), fw) and np.array_equal(call.query.codes(True), rc)
    # (the mirrored text, not the reference's host RevComp: that one shifts the strand when the query holds IUPAC letters, hazard H14, and
    #  the device-seeded entries see the mirrored block)
    ascii_ = reverse_complement(call.query).text if call.rev else text
    assert np.array_equal(oracle.encode(ascii_.tobytes()), rc if call.rev else fw)
    return ref, index, pos, ascii_, (rc if call.rev else fw)


DEFAULT_MAX_HITS = 1 << 30   # (the CPU tests' stand-in for the engine's own MAX_HITS: no call here comes near either)


# ---- the worlds ------------------------------------------------------------------------------------------------------------------------
# stretch units and the run each of their keys gets
UNITS = {"A": 128, "C": 600, "AC": 1, "AAAAC": 31, "ACCCC": 32, "AAAC": 33, "ACCC": 100, "AACC": 0}
# keys for windows: name -> pieces of the run (own bucket first, then the transition words in emission order)
WINDOW_RUNS = {
    "w1": [1], "w2": [2], "w3": [3], "w31": [31], "w95": [95], "w0": [],
    "first": [5],                                  # only the position's first word bears hits
    "seventh": [0, 0, 0, 0, 0, 0, 4],              # only its seventh
    "last": None,                                  # only its last (filled in per shape)
    "every": None,                                 # 1, 2, 3 ... hits in its words
    "own_empty": [0, 3, 0, 2],                     # own bucket empty, two neighbours' not
    "first_last": None,                            # the first and the last word
}


@functools.lru_cache(maxsize=None)
def window_keys(shape):
    """name -> key, {A, C} keys that no stretch uses"""
    S = M.Shape(shape)
    used = {k for u in UNITS for k in unit_keys(shape, u)}
    out, i = {}, 5
    for name in WINDOW_RUNS:
        while ac_key(S, i) in used:
            i += 7
        out[name] = ac_key(S, i)
        used.add(out[name])
    return out


def pieces_of(shape, name):
    nw = len(M.Shape(shape).masks(True))
    p = WINDOW_RUNS[name]
    if name == "last":
        p = [0] * (nw - 1) + [6]
    elif name == "every":
        p = list(range(1, nw + 1))
    elif name == "first_last":
        p = [2] + [0] * (nw - 2) + [3]
    return p


@functools.lru_cache(maxsize=None)
def world(shape=SHAPE_W9, big=0):
    """the stretch runs and the window runs in one target; big: the C stretch's run instead of 600"""
    runs = {}
    for u, n in UNITS.items():
        if big and u != "C":          # (the big run fills the target: only what its call needs beside it)
            continue
        n = big if big else n
        for k in unit_keys(shape, u):
            assert k not in runs or runs[k] == n, "two stretch units share a key"
            runs[k] = n
    wk = window_keys(shape)
    for name in WINDOW_RUNS:
        if not big or name in ("w1", "w3", "w95"):
            runs[wk[name]] = pieces_of(shape, name)
    return World("%s%s" % ({SHAPE_12OF19: "12of19", SHAPE_W9: "w9"}.get(shape, shape), ", C run %d" % big if big else ""), shape, runs, seed=3)


def run_of(shape, name):
    return sum(pieces_of(shape, name))


def W(shape, *names):
    wk = window_keys(shape)
    return [(-1 if n is None else wk[n]) for n in names]


# ---- lookup and grid ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_query(shape=SHAPE_W9):
    """~6000 positions of everything: windows with every kind of run, stretches of every unit, invalid windows, empty runs"""
    q = Query(shape, seed=11)
    q.windows(W(shape, "w1", "w2", None, "w3", "w0", "w31", "every", None, None, "w95", "own_empty", "first", "seventh", "last", "first_last"))
    q.mark("A").stretch("A", 300)
    q.windows(W(shape, "w0", "w1"))
    q.mark("AC").stretch("AC", 150).mark("AAAAC").stretch("AAAAC", 140).mark("ACCCC").stretch("ACCCC", 130)
    q.windows(W(shape, None, None, "w2", "every"))
    q.mark("AAAC").stretch("AAAC", 260).mark("ACCC").stretch("ACCC", 250).mark("AACC").stretch("AACC", 90)
    q.mark("C").stretch("C", 40)
    q.mark("dense").stretch("AC", 2300)
    q.windows(W(shape, *(["w1", "w3", None, "w0", "every", "w31"] * 30)))
    q.mark("tail").stretch("ACCCC", 40)
    return q


@functools.lru_cache(maxsize=None)
def rc_mixed_query(shape=SHAPE_W9):
    """the reverse complement of the mixed query: its minus strand is the mixed query"""
    return reverse_complement(mixed_query(shape))


def grid_calls(shape=SHAPE_W9):
    """start & 3 crossed with (end - start) & 3; the sizes around the four positions of a thread and the tile, at skew 0 and 3"""
    w, q = world(shape), mixed_query(shape)
    calls = []
    base = q.marks["A"] - 24 & ~3
    for s in range(4):
        for l in range(4):
            calls.append(Call("start & 3 = %d, length & 3 = %d" % (s, l), w, q, base + s, base + s + 1300 + l, claims={"skew": s, "len_mod4": l}))
    d = q.marks["dense"] + 40 & ~3
    for skew in (0, 3):
        for n in (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049):
            calls.append(Call("n = %d at skew %d" % (n, skew), w, q, d + skew, d + skew + n, claims={"skew": skew, "n": n}))
    return calls


@functools.lru_cache(maxsize=None)
def letters_query(shape=SHAPE_W9):
    """valid windows next to windows that an N, a lower-case letter, '&' or an IUPAC letter at their first or last base makes invalid"""
    q = Query(shape, seed=21)
    q.stretch("A", 400)
    # (each letter invalidates the windows that hold it: those that start up to span - 1 bases in front of it, and the one that starts on it)
    for i, letter in enumerate("Nn&aRtY"):
        q.put(40 + 45 * i, letter)
    return q


def lookup_calls(shape=SHAPE_W9):
    w, q, lq = world(shape), mixed_query(shape), letters_query(shape)
    rq = rc_mixed_query(shape)
    S = w.S
    last = q.size - S.span              # the last window that fits the block
    calls = [
        Call("the last position is the last window that fits the block", w, q, last - 700, last + 1, claims={"n": 701}),
        Call("a range that the entry clips", w, q, last - 700, last + 500, claims={"n": 701}),
        Call("a range that the entry clips to one chunk of several", w, q, last - 700, last + 2500, chunk=1000, claims={"n": 701, "K": 4}),
        Call("windows invalid by N, lower case, & and IUPAC at their first and last base", w, lq, 0, lq.size, claims={}),
        Call("valid positions whose run is empty", w, q, q.marks["AACC"], q.marks["AACC"] + 90, claims={"valid": 90, "hits": 0, "ret": 90 * w.table.words}),
        Call("no valid position", w, q, q.marks["A"] + 300, q.marks["A"] + 300 + S.span - 1, claims={"valid": 0, "hits": 0, "ret": 0}),
        Call("reverse strand", w, rq, 1001, 3500, rev=True, claims={"skew": 1, "same_as_plus_of": "mixed"}),
        Call("reverse strand, the whole query", w, rq, 0, rq.size, rev=True, claims={"same_as_plus_of": "mixed"}),
        Call("reverse strand, the range that the entry clips", w, rq, last - 699, last + 77, rev=True, claims={"skew": (last - 699) & 3, "n": 700}),
        Call("query buffer 1", w, q, 4, q.size - 100, buffer=1, claims={"skew": 0}),
    ]
    return calls


# ---- tiles and the sums ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiles_query(shape=SHAPE_W9):
    q = Query(shape, seed=31)
    # tile 0: non-empty positions at elements 1022 and 1023, tile 1 from element 1024 on: a stretch across the border
    q.windows(W(shape, "w1", "w2", "w3")).fill_to(1022).stretch("AAAAC", 4)            # positions 1022 .. 1025
    q.fill_to(2 * PR_TILE + 10).windows(W(shape, "w1"))                                   # tile 2: one position
    q.fill_to(4 * PR_TILE - 6).windows(W(shape, "every"))                                 # tile 3 has one; tile 4 is ...
    q.fill_to(5 * PR_TILE).mark("full").stretch("A", PR_TILE)                             # ... tile 5: all 1024 positions non-empty
    q.windows(W(shape, "w2", "w95"))
    return q


def tile_calls(shape=SHAPE_W9):
    w, q = world(shape), tiles_query(shape)
    full = q.marks["full"]
    return [
        Call("non-empty positions at 1023 | 1024 of a tile", w, q, 0, 3 * PR_TILE, claims={"tile_nonempty": [5, 2, 1]}),
        Call("non-empty positions at 1023 | 1024 of a tile, skew 2", w, q, 2, 3 * PR_TILE, claims={"skew": 2, "tile_nonempty": [4, 2, 1]}),
        Call("a tile with no non-empty position between two that have some", w, q, 2 * PR_TILE, full + PR_TILE + 40,
             claims={"tile_nonempty": [1, 1, 0, PR_TILE, 2]}),
        Call("a tile in which all 1024 positions are non-empty", w, q, full, full + PR_TILE, claims={"tile_nonempty": [PR_TILE], "records": PR_TILE}),
        Call("a tile in which all 1024 positions are non-empty, skew 1", w, q, full + 1, full + 2 * PR_TILE, claims={"skew": 1, "tile_nonempty": [PR_TILE - 1, 2]}),
    ]


@functools.lru_cache(maxsize=None)
def long_query(far_mod4, shape=SHAPE_W9):
    """2.1 M positions of N between a group of windows and one far window: probe_partials_kernel's second and third workgroup.  The far
    window starts at a position that is far_mod4 modulo four, so that a call of n positions that ends on it starts on the grid"""
    q = Query(shape, seed=41)
    q.windows(W(shape, "w1", "every", "w95", "w3")).mark("gap")
    q.fill_to(2 * PP_TILE * PR_TILE + 600 + far_mod4).mark("far").windows(W(shape, "every"))
    q.fill(40)
    return q


def sums_calls(shape=SHAPE_W9):
    w = world(shape)
    calls = []
    for blocks in (PP_TILE, PP_TILE + 1, 2 * PP_TILE + 1):
        n = (blocks - 1) * PR_TILE + (1 if blocks > PP_TILE else PR_TILE)
        q = long_query((n - 1) & 3, shape)
        end = q.marks["far"] + 1         # the far window is the last position of the call: its hits are the last tile's
        assert (end - n) & 3 == 0
        calls.append(Call("%d workgroups, all hits in the first tile" % blocks, w, q, 0, n, claims={"tiles": blocks, "hits_in": "first", "skew": 0}))
        calls.append(Call("%d workgroups, all hits in the last tile" % blocks, w, q, end - n, end, claims={"tiles": blocks, "hits_in": "last", "skew": 0}))
    return calls


# ---- head bits --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def headbit_query(shift, shape=SHAPE_W9):
    """tile 0: ordinary windows whose hits end `shift` hits past a multiple of 32; tile 1: 1024 positions of 128 hits = 131072 hits, which
    span exactly 4096 head-bit words when they start on a word (LDS) and 4097 when they start one hit later (atomics); tile 2: ordinary"""
    q = Query(shape, seed=51)
    names = ["w31", "w1"] + (["w1"] if shift else []) + ["w95", "w1"]           # 128 hits, or 129
    q.windows(W(shape, *names)).fill_to(PR_TILE).stretch("A", PR_TILE).windows(W(shape, "w3", "every", "w2"))
    return q


@functools.lru_cache(maxsize=None)
def words_query(shape=SHAPE_W9):
    """tiles that share head-bit words: 0: 40 hits; 1: wholly inside word 1 (hits 40 .. 50), shared with both neighbours; 2: ends mid-word;
    3: no hit; 4: starts in the word tile 2 ended in"""
    q = Query(shape, seed=52)
    q.windows(W(shape, "w31", "w3", "w3", "w3"))                       # tile 0: hits 0 .. 39
    q.fill_to(PR_TILE + 5).windows(W(shape, "w3", "w2", "w3", "w2"))   # tile 1: hits 40 .. 49, all in word 1
    q.fill_to(2 * PR_TILE + 9).windows(W(shape, "w3", "w95", "w1"))    # tile 2: hits 50 .. 148: words 1 .. 4, ends mid-word
    q.fill_to(4 * PR_TILE + 3).windows(W(shape, "w2", "w31", "w95"))   # tile 4: starts at hit 149 in word 4
    q.fill(30)
    return q


@functools.lru_cache(maxsize=None)
def runs_query(dense, shape=SHAPE_W9):
    """stretches of 1, 31, 32, 33 and 100 hits per position -- the four positions of a thread in one word, in four different words and
    across skipped words -- one tile each; dense: 600-hit positions in every tile as well (more than 4096 words: the atomic path)"""
    q = Query(shape, seed=53)
    for t, unit in enumerate(("AC", "AAAAC", "ACCCC", "AAAC", "ACCC")):
        q.fill_to(t * PR_TILE)
        if dense:
            q.stretch("C", 260)
        q.stretch(unit, 700 if not dense else 600)
    return q


def headbit_calls(shape=SHAPE_W9):
    w = world(shape)
    calls = []
    for shift, words in ((0, HB_LDS_WORDS), (1, HB_LDS_WORDS + 1)):
        q = headbit_query(shift, shape)
        calls.append(Call("a tile whose hits span %d words (%s)" % (words, "LDS" if not shift else "atomics"), w, q, 0, q.size,
                          claims={"tile_words_1": words, "tile_base_1": 128 + shift}))
    wq = words_query(shape)
    calls.append(Call("tiles inside and across shared words, a zero-hit tile between two that share one", w, wq, 0, wq.size,
                      claims={"tile_hits": [40, 10, 99, 0, 128], "tile_words": [2, 1, 4, 0, 5]}))
    for dense in (False, True):
        q = runs_query(dense, shape)
        calls.append(Call("runs of 1, 31, 32, 33 and 100 hits on the %s path" % ("atomic" if dense else "LDS"), w, q, 0, q.size,
                          claims={"dense": dense}))
        calls.append(Call("runs of 1, 31, 32, 33 and 100 hits on the %s path, skew 3" % ("atomic" if dense else "LDS"), w, q, 3, q.size,
                          claims={"dense": dense, "skew": 3}))
    return calls


@functools.lru_cache(maxsize=None)
def regrow_query(shape=SHAPE_W9):
    """3600 positions of 600 hits: 2 160 000 hits, more than the 32 x 65536 the initial map of a slot holds"""
    return Query(shape, seed=54).windows(W(shape, "w1", "w3")).stretch("C", 3600).windows(W(shape, "w2"))


@functools.lru_cache(maxsize=None)
def poison_query(shape=SHAPE_W9):
    """what the GPU tests probe in a call's slot before the call itself: 2300 positions of 600 hits and a few windows, so that every
    buffer of the slot holds the records, head bits, td_chunk entries, bounds and plans of another call (every position from 0 on bears hits)"""
    return Query(shape, seed=55).stretch("C", 2300).windows(W(shape, "w95", "w1", "w31", "every"))


def regrow_calls(shape=SHAPE_W9):
    w, q = world(shape), regrow_query(shape)
    small = mixed_query(shape)
    return [Call("more hits than the initial head-bit map holds", w, q, 0, q.size, claims={}),
            Call("a small call behind the large one", w, small, 0, 200, buffer=1, claims={})]


# ---- td_chunk ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunk_mark_query(extra, shape=SHAPE_W9):
    """31 positions of 128 hits (3968) and windows of 95 + 31 + `extra` hits, then a window of 95: its first hit is hit 4094 + extra"""
    q = Query(shape, seed=61 + extra)
    q.stretch("A", 31).windows(W(shape, "w95", "w31", {1: "w1", 2: "w2", 3: "w3"}[extra], "w95", "w2", "every"))
    return q


@functools.lru_cache(maxsize=None)
def total_query(extra, shape=SHAPE_W9):
    q = Query(shape, seed=65)
    q.stretch("A", 32)
    if extra:
        q.windows(W(shape, "w1"))
    return q


def td_chunk_calls(shape=SHAPE_W9):
    w = world(shape)
    calls = []
    for extra in (1, 2, 3):
        q = chunk_mark_query(extra, shape)
        first = 3968 + 126 + extra
        calls.append(Call("a run whose first hit is hit %d (the run in front ends at hit %d)" % (first, first - 1), w, q, 0, q.size,
                          claims={"first_hit": first}))
    for extra in (0, 1):
        q = total_query(extra, shape)
        calls.append(Call("%d hits in all" % (4096 + extra), w, q, 0, q.size, claims={"hits": 4096 + extra}))
    if shape == SHAPE_W9:             # (once, on the shortest shape of weight 9: the run IS the target)
        short = SHAPE_W9_SHORT
        wb = world(short, big=8200)
        q = Query(short, seed=66).windows(W(short, "w95", "w3")).stretch("C", 3).windows(W(short, "w1"))
        calls.append(Call("runs of more than 8192 hits that hold two multiples of 4096", wb, q, 0, q.size, claims={"max_run": 8200, "hits": 3 * 8200 + 99}))
    return calls


# ---- chunks and bounds ------------------------------------------------------------------------------------------------------------------
def chunk_calls(shape=SHAPE_W9):
    w, q = world(shape), mixed_query(shape)
    d = q.marks["dense"] + 40 & ~3
    calls = []
    for chunk in (1, 2, 3, 5, 1023, 1024, 1025):
        for skew in (0, 1, 3):
            n = min(chunk * 7 + 2, chunk * MAX_CHUNKS) if chunk < 1000 else chunk * 2 + 7
            calls.append(Call("wga_chunk %d at skew %d" % (chunk, skew), w, q, d + skew, d + skew + n, chunk=chunk,
                              claims={"skew": skew, "K": -(-n // chunk)}))
    # boundaries on every element of a thread's four positions: chunk 5 moves them through all of them; chunk 3 puts two into one thread
    for k, skew in ((1, 0), (2, 0), (255, 2), (256, 0), (256, 3)):
        calls.append(Call("K = %d at skew %d" % (k, skew), w, q, d + skew, d + skew + 5 * k - (2 if k > 1 else 0), chunk=5, claims={"K": k, "skew": skew}))
    calls.append(Call("the bound that equals n", w, q, d, d + 40, chunk=5, claims={"K": 8}))
    # empty chunks first, last and in the middle: the positions behind a stretch hold no valid window, the N filler none either
    a = q.marks["A"]
    calls.append(Call("empty chunks first and in the middle", w, q, a - 8, q.marks["AC"] + 20, chunk=4, claims={"empty": ["first", "middle"]}))
    calls.append(Call("empty chunks last, a short last chunk", w, q, a + 280, a + 326, chunk=4, claims={"empty": ["last"], "K": 12}))
    calls.append(Call("chunks behind the clip are empty", w, q, q.size - w.S.span - 30, q.size + 40, chunk=10, claims={"K": -(-(w.S.span + 70) // 10), "n": 31}))
    return calls


# ---- plans ------------------------------------------------------------------------------------------------------------------------------
PLAN_CHUNK = 3      # windows per chunk of the plan query


@functools.lru_cache(maxsize=None)
def plan_query(shape=SHAPE_W9):
    """chunks of three windows (wga_chunk = 3 (span + 1)); the rows below are the chunks"""
    rows = [
        ("every", "w31", "w95"),              # 0  three non-empty positions
        ("w1", None, None),                   # 1  one position, one word: the first iteration is empty
        (None, None, None),                   # 2  no valid position
        ("w0", "w0", "w0"),                   # 3  valid positions, no hit
        ("w3", "first", None),                # 4  the last hit-bearing word is word 1 of its position
        ("w3", "seventh", "w0"),              # 5  ... word 7
        ("w3", "w2", "last"),                 # 6  ... the last word
        ("w31", "own_empty", "w0"),           # 7  the last non-empty position's own bucket is empty, a neighbour's is not
        ("first", "w3", "w2"),                # 8  a first word of 5 hits: MAX_HITS 5 and below is hazard H5
        ("every", "first_last", None),        # 9  greedy groups; word boundaries at known hits
        ("w95", "w95", None),                 # 10 two non-empty positions
        (None, "first_last", None),           # 11 one position, hits in its first and its last word
    ]
    q = Query(shape, seed=71)
    for r in rows:
        q.windows(W(shape, *r))
    q.rows = rows
    return q


@functools.lru_cache(maxsize=None)
def segs_query(shape=SHAPE_W9):
    """256 chunks of one window each: 255 of 5 hits in two words and one of 95"""
    q = Query(shape, seed=72)
    q.windows(W(shape, *(["first_last"] * 100 + ["w95"] + ["first_last"] * 155)))
    return q


def plan_calls(shape=SHAPE_W9):
    w, q = world(shape), plan_query(shape)
    S = w.S
    step = S.span + 1
    C = PLAN_CHUNK * step
    nw = w.table.words
    ev = nw * (nw + 1) // 2           # hits of "every"
    row = lambda r: (r * C, (r + 1) * C)
    calls = []

    def one(name, r, max_hits, **claims):
        a, b = row(r)
        calls.append(Call(name, w, q, a, b, chunk=C, max_hits=max_hits, claims=dict(claims, K=1)))

    h0 = ev + 31 + 95
    one("chunk hits of MAX_HITS - 1: everything before the last hit-bearing word, then that word", 0, h0 + 1, n_iter=[2], chunk_hits=[h0])
    one("chunk hits of MAX_HITS: greedy groups", 0, h0, n_iter=[3], chunk_hits=[h0])
    one("chunk hits of MAX_HITS + 1: greedy groups", 0, h0 - 1, n_iter=[3], chunk_hits=[h0])
    one("a chunk whose only hits are one word's: the first iteration is empty", 1, 0, n_iter=[2], upto0=0)
    one("the last hit-bearing word is word 1 of its position", 4, 0, n_iter=[2], upto0=3)
    one("the last hit-bearing word is word 7 of its position", 5, 0, n_iter=[2], upto0=3)
    one("the last hit-bearing word is the last word of its position", 6, 0, n_iter=[2], upto0=5)
    one("the last non-empty position's own bucket is empty while a neighbour's is not", 7, 0, n_iter=[2], upto0=31 + 3)
    one("a first word of exactly MAX_HITS hits (H5)", 8, 5, n_iter=[10 // 5 + 2], upto0=0)
    one("a first word of more than MAX_HITS hits (H5)", 8, 4, n_iter=[10 // 4 + 2], upto0=0)
    # row 9: the words of "every" end at hits 1, 3, 6, 10, 15, ...: a word boundary exactly on the limit, and one hit below it
    one("a word boundary exactly on the limit", 9, 15, n_iter=[(ev + 5) // 15 + 2], upto0=10)
    one("a word boundary one hit below the limit", 9, 16, n_iter=[(ev + 5) // 16 + 2], upto0=15)
    one("a chunk with two non-empty positions", 10, 0, n_iter=[2], upto0=95)
    one("a chunk with one non-empty position", 11, 0, n_iter=[2], upto0=2)
    h9 = ev + 5
    one("num_hits / MAX_HITS + 2 = 8: planned", 9, h9 // 6, n_iter=[8])
    one("num_hits / MAX_HITS + 2 = 9: refused", 9, h9 // 7, n_iter=[PM.OVERFLOW], ret=PM.REFUSED)
    calls.append(Call("every chunk of the plan query in one call, zero-iteration chunks between planned ones", w, q, 0, len(q.rows) * C, chunk=C,
                      max_hits=60, claims={"K": len(q.rows), "zero_iter_chunks": [2, 3]}))
    calls.append(Call("every chunk of the plan query in one call, below MAX_HITS", w, q, 0, len(q.rows) * C, chunk=C, max_hits=0,
                      claims={"K": len(q.rows), "zero_iter_chunks": [2, 3]}))
    calls.append(Call("every chunk of the plan query in one call, skew 2 and a short last chunk", w, q, 2, len(q.rows) * C - 20, chunk=C, max_hits=60,
                      claims={"K": len(q.rows), "skew": 2}))
    # a chunk with several thousand non-empty positions: both ends of the search over the records
    mq = mixed_query(shape)
    d = mq.marks["dense"]
    calls.append(Call("a chunk with several thousand non-empty positions in greedy groups", w, mq, d, d + 2300, max_hits=500,
                      claims={"K": 1, "records": 2300, "n_iter": [2300 // 500 + 2]}))
    calls.append(Call("a chunk with several thousand non-empty positions below MAX_HITS", w, mq, d - 200, d + 2300, max_hits=0, claims={"K": 1, "n_iter": [2]}))
    sq = segs_query(shape)
    calls.append(Call("256 chunks of two iterations each: 512 segments, accepted", w, sq, 0, 256 * step, chunk=step, max_hits=96,
                      claims={"K": 256, "segments": 512, "refused": False}))
    calls.append(Call("256 chunks, one of them at three iterations: 513 segments, refused", w, sq, 0, 256 * step, chunk=step, max_hits=95,
                      claims={"K": 256, "segments": 513, "refused": True, "ret": PM.REFUSED}))
    return calls


def wrap_calls(shape=SHAPE_W9):
    """MAX_HITS near 2^32, the target as its own query (so that the repeat masker's call can be made on the same positions):
    num_hits + MAX_HITS = 2^32 - 1 is planned; 2^32 is refused by a plain call and planned by the repeat masker's"""
    w = world(shape)
    tq = TextQuery(w.S, w.target)
    end = 4000                        # (some 150 000 hits: the oracle extends every one of them)
    h = Call("target as query", w, tq, 0, end).model()["hits"]
    calls = []
    for rm in (False, True):
        calls.append(Call("num_hits + MAX_HITS = 2^32 - 1, %s: planned" % ("repeat masker" if rm else "plain"), w, tq, 0, end, rm=rm,
                          max_hits=(1 << 32) - 1 - h, claims={"refused": False, "n_iter": [2]}))
        calls.append(Call("num_hits + MAX_HITS = 2^32, %s: %s" % ("repeat masker" if rm else "plain", "planned" if rm else "refused"), w, tq, 0, end,
                          rm=rm, max_hits=(1 << 32) - h, claims={"refused": not rm, "n_iter": [2 if rm else PM.OVERFLOW]}))
    return calls


# ---- other tables -----------------------------------------------------------------------------------------------------------------------
def notransition_calls(shape=SHAPE_W9):
    q = mixed_query(shape)
    out = []
    for name, opts in (("notransition", {}), ("notransition, alias table", {"no_ctx": 1})):
        w = world(shape).variant(name, transition=False, options=opts)
        out.append(Call("%s: one word per position" % name, w, q, 2, q.size, chunk=1000, claims={"words": 1}))
    return out


def no_ctx_calls(shape=SHAPE_W9):
    w = world(shape).variant("positions only", options={"no_ctx": 1})
    q = mixed_query(shape)
    hq = headbit_query(1, shape)
    pq = plan_query(shape)
    C = PLAN_CHUNK * (w.S.span + 1)
    return [Call("no_ctx: the mixed query in chunks", w, q, 1, q.size, chunk=1000, claims={"skew": 1}),
            Call("no_ctx: a tile of 131072 hits", w, hq, 0, hq.size, claims={}),
            Call("no_ctx: the plan query", w, pq, 0, len(pq.rows) * C, chunk=C, max_hits=60, claims={})]


# ---- ordinary sequence ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ordinary_calls(shape=SHAPE_W9, n=6000):
    """an ordinary step-1 target with N runs, soft-masked stretches, '&' and IUPAC letters, and a query that is a diverged copy of it with
    such letters of its own: plus and minus strand, one chunk and several, MAX_HITS above and below a chunk's hits"""
    t = R.ordinary_text(n, 301)
    w = World.from_text("ordinary %s" % ("12of19" if shape == SHAPE_12OF19 else "w9"), shape, t, 1)
    rng = np.random.default_rng(302)
    qt = R.ordinary_text(n, 303)
    keep = rng.random(n) < 0.6                  # 60 % of the query is the target's text, 3 % of that substituted
    qt[keep] = t[keep]
    sub = keep & (rng.random(n) < 0.03) & (qt < 97)
    qt[sub] = ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    q = TextQuery(w.S, qt)
    rq = reverse_complement(q)
    return [Call("ordinary, one chunk", w, q, 0, n, claims={}),
            Call("ordinary, chunks of 1000 from position 3", w, q, 3, n, chunk=1000, claims={"skew": 3}),
            Call("ordinary, chunks of 1000 under MAX_HITS 300", w, q, 0, n - 500, chunk=1000, max_hits=300, claims={}),
            Call("ordinary, minus strand", w, rq, 2, n, chunk=1500, rev=True, max_hits=2000, claims={"skew": 2}),
            Call("ordinary, the target against itself", w, TextQuery(w.S, t), 0, n, chunk=2000, max_hits=1500, claims={})]


GROUPS = {
    "grid": grid_calls, "lookup": lookup_calls, "tiles": tile_calls, "sums": sums_calls, "head bits": headbit_calls, "td_chunk": td_chunk_calls,
    "chunks": chunk_calls, "plans": plan_calls, "wrap plans": wrap_calls, "notransition": notransition_calls, "no_ctx": no_ctx_calls, "ordinary": ordinary_calls,
}
# a case or more of every group on 12of19 (13 words per position, 2^24 keys)
GROUPS_12OF19 = {
    "grid": lambda: [c for c in grid_calls(SHAPE_12OF19) if c.name in ("start & 3 = 3, length & 3 = 1", "n = 1025 at skew 3")],
    "lookup": lambda: lookup_calls(SHAPE_12OF19)[2:4],
    "tiles": lambda: tile_calls(SHAPE_12OF19)[2:3],
    "head bits": lambda: headbit_calls(SHAPE_12OF19)[1:3],
    "td_chunk": lambda: td_chunk_calls(SHAPE_12OF19)[1:2],
    "chunks": lambda: [c for c in chunk_calls(SHAPE_12OF19) if c.name in ("wga_chunk 3 at skew 1", "K = 256 at skew 3")],
    "plans": lambda: plan_calls(SHAPE_12OF19),
    "ordinary": lambda: ordinary_calls(SHAPE_12OF19)[2:4],
    "sums": lambda: sums_calls(SHAPE_12OF19)[2:4],
    "wrap plans": lambda: wrap_calls(SHAPE_12OF19),
    "notransition": lambda: notransition_calls(SHAPE_12OF19),
    "no_ctx": lambda: no_ctx_calls(SHAPE_12OF19)[:2],
}


@functools.lru_cache(maxsize=None)
def all_calls():
    out = {}
    for g, f in GROUPS.items():
        for c in f():
            key = "%s: %s" % (g, c.name)
            assert key not in out, key
            out[key] = c
    for g, f in GROUPS_12OF19.items():
        for c in f():
            key = "12of19 %s: %s" % (g, c.name)
            assert key not in out, key
            out[key] = c
    return out
