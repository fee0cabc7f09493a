"""GPU: the class filter's per-wave tiles (extend.hip 1d, one-copy form) -- the 64 position records and the 64 dwords of either strand's
unshifted 2-bit copy a wave keeps in LDS -- at the smallest shapes at which they can go wrong.  Every call is held, hit for hit and by
EXACT equality, to tests/filter_model.py (forwards field for field, audit list, num_candidates, sub-list counters) and to the oracle's
vector, through hold_call of tests/test_gpu_filter_verdicts.py; the model knows nothing of tiles, launch geometry or wave partition.

What a tile is, so that the worlds below can be read: a wave serves the position records of a 64-hit buffer from td_rec[base, base + 64)
and the query windows from dwords [base, base + 64) of a strand's copy (16 bases per dword, five dwords per window: a window may start
in the first WIN_SPAN = 60 dwords = 960 bases of a tile).  A buffer with a lane outside a tile loads the tile anew from its first lane
on; the other strand's window positions DESCEND along a call, so its new tile ends at the first lane's window.  A buffer whose windows
do not fit one tile even then reads them from memory.

Every world runs on the plus strand and, as its flipped twin, on the minus strand, under the default launch (one wave per 4096-hit
chunk, 1024 lanes per workgroup) and with one and three waves for the whole call in workgroups of 64 and 256 lanes."""
import numpy as np
import pytest

import filter_model as F
import filter_regimes as R
import test_gpu_filter_verdicts as V
from helpers import Case

pytestmark = pytest.mark.gpu

TILE_DWORDS, WIN_DWORDS = 64, 5
TILE_BASES = 16 * TILE_DWORDS                      # 1024
WIN_SPAN_BASES = 16 * (TILE_DWORDS - WIN_DWORDS + 1)   # 960: window starts a tile serves
ISLAND_STEPS = [WIN_SPAN_BASES - 16, WIN_SPAN_BASES, WIN_SPAN_BASES + 16, TILE_BASES - 16, TILE_BASES, TILE_BASES + 16]
CARE = [i for i, ch in enumerate(R.SHAPE_12OF19) if ch == "T"]
LAUNCHES = [{}, {"ctx_waves": 1, "ctx_threads": 64}, {"ctx_waves": 1, "ctx_threads": 256}, {"ctx_waves": 3, "ctx_threads": 64},
            {"ctx_waves": 3, "ctx_threads": 256}]
LAUNCH_IDS = ["default", "1 wave of 64", "1 wave of 256", "3 waves of 64", "3 waves of 256"]


class TileWorld(R.World):
    """a world of two ASCII blocks, with or without the transition neighbours"""

    def __init__(self, name, target, query, mat, transition=True):
        self.transition = transition
        super().__init__(name, (target, query), mat, 910, 3000, big=True)

    @property
    def table(self):
        if "table" not in self._cache:
            self._cache["table"] = F.Table(self.tc, self.S, 1, self.transition, sparse=None)
            assert self._cache["table"].bucket.max() <= R.TM.SORT_MAX, self.name      # (larger buckets keep their arrival order on the device)
        return self._cache["table"]

    def flipped(self):
        if "flipped" not in self._cache:
            f = TileWorld(self.name + " flipped", self.target, R.ASCII[R.IM.rev_comp(self.qc)], self.mat, self.transition)
            f._cache["table"] = self.table
            self._cache["flipped"] = f
        return self._cache["flipped"]


def dna(rng, n):
    return R.ASCII[rng.integers(0, 4, n).astype(np.uint8)]


def join(parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


GAP = np.frombuffer(b"NNN", dtype=np.uint8)        # no seed window crosses it


# ---- the worlds ---------------------------------------------------------------------------------------------------------------------------
def one_hit_world(mat):
    """the query is the random target itself, without transitions: one hit per position (20000 random 12-base keys among 4^12 collide
    a few times only), 64 positions per buffer -- the record tile is loaded anew for every buffer -- and every hit is forwarded"""
    t = dna(np.random.default_rng(101), 20000)
    return TileWorld("one hit per position", t, t.copy(), mat, transition=False)


def islands_world(mat):
    """unmasked islands of one to three positions between soft-masked runs: first runs of 1 to 5 kbp, among them runs that put the next
    position exactly ISLAND_STEPS bases behind the last one (the span of window starts a tile serves, a whole tile, and either -16 and
    +16 bases); then runs of 100 to 400 bases, where several islands share a tile.  A run is masked at every eighth base only: no seed
    window fits between two masked bases, but the flanks of a hit still match, so most hits are forwarded and a window taken from the
    wrong place shows as a missing forward.  The target holds the unmasked sequence six times, so a position has six hits and a buffer
    about ten positions: in the first part no tile holds a buffer (windows from memory, a new tile with every buffer), in the second a
    new tile does"""
    rng = np.random.default_rng(202)
    runs = [d - 19 for d in ISLAND_STEPS] + [int(x) for x in rng.integers(1000, 5001, 14)]
    rng.shuffle(runs)
    runs += [int(x) for x in rng.integers(100, 401, 60)]
    seq = dna(rng, sum(runs) + 21 * (len(runs) + 1) + 40)
    q = seq.copy()

    def mask(lo, hi, step=8):
        q[lo:hi:step] = np.frombuffer(bytes(q[lo:hi:step]).lower(), dtype=np.uint8)
    mask(0, 20, 1)
    at = 20
    for i, n in enumerate(runs):
        at += 19 + i % 3                                                  # an island of 1, 2 or 3 seed windows
        mask(at, at + n)                                                  # (last window in front of the run at - 19, first one behind it at + n)
        q[at + n - 1] = ord(chr(q[at + n - 1]).lower())
        at += n
    mask(at + 21, q.size, 1)
    assert q.size <= 65536
    return TileWorld("islands", join([x for _ in range(6) for x in (seq, GAP)]), q, mat)


def heavy_world(mat):
    """ONE query position heavier than a chunk: its seed word and its twelve transition neighbours occur 390 times each in the target
    (13 buckets of 390 <= 512 entries -- the size up to which the device's bucket order is the model's -- are one run of 5070 hits),
    with the don't-care bases of every copy drawn anew, between ordinary positions.  Chunk and wave cuts fall inside the run; with one
    wave for the call a single wave walks all of it"""
    rng = np.random.default_rng(303)
    unit = rng.integers(0, 4, 19).astype(np.uint8)
    parts = [GAP]                                                         # (target position 0 is never indexed)
    for v in range(13):
        for _ in range(390):
            u = rng.integers(0, 4, 19).astype(np.uint8)
            u[CARE] = unit[CARE]
            if v:
                u[CARE[v - 1]] ^= 2                                       # the transition at one care position
            parts += [R.ASCII[u], GAP]
    flank = dna(rng, 3000)
    t = join(parts + [flank])
    q = join([flank[:1500], R.ASCII[unit], flank[1500:]])
    return TileWorld("heavy position", t, q, mat)


def edge_world(mat, length):
    """every position of the query has a hit, the first and the last valid one of either strand included"""
    rng = np.random.default_rng(400 + length)
    t = dna(rng, 4000)
    return TileWorld("edges %d" % length, t, t[700:700 + length].copy(), mat)


def records_world(mat, first, rest):
    """without transitions: the query is a stretch S of 130 positions; the target holds `first` copies of all of S and rest - first more
    of S from position 64 on, so positions 0..63 have `first` hits and the others `rest`"""
    rng = np.random.default_rng(500 + first)
    s = dna(rng, 19 + 129)
    parts = [GAP] + [x for _ in range(first) for x in (s, GAP)] + [x for _ in range(rest - first) for x in (s[64:], GAP)]  # (target position 0 is never indexed)
    return TileWorld("records %d/%d" % (first, rest), join(parts), s.copy(), mat, transition=False)


WORLDS = {
    "one_hit": one_hit_world,
    "islands": islands_world,
    "heavy": heavy_world,
    "edges_0": lambda m: edge_world(m, 1600),          # query lengths = 0, 1 and 15 mod 16
    "edges_1": lambda m: edge_world(m, 1601),
    "edges_15": lambda m: edge_world(m, 1615),
    "records_64": lambda m: records_world(m, 64, 64),  # chunk 0 = positions 0..63 exactly: one record tile, no more
    "records_65": lambda m: records_world(m, 63, 64),  # chunk 0 = 64 positions of 63 hits and one of 64: the 65th record is one past the tile
}


@pytest.fixture(scope="module")
def tile_worlds(oracle):
    mat = np.array(oracle.build_sub_mat(910), dtype=np.int32)
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = WORLDS[name](mat)
        return cache[name]
    return get


@pytest.fixture
def E(engine):
    engine.ShutdownProcessor()
    engine.reset_option(None)
    try:
        yield engine
    finally:
        engine.ShutdownProcessor()
        engine.reset_option(None)


def open_world(E, oracle, w, options):
    E.set_option("audit_cap", V.AUDIT_CAP)
    E.set_option("fwd_keep", 1)
    for k, v in options.items():
        E.set_option(k, v)
    c = Case(w.target, w.query, shape=w.shape_text, transition=w.transition, chunk=max(w.query.size, 1 << 16), xdrop=w.xdrop,
             hspthresh=w.hspthresh, noentropy=True, sub_mat=w.mat)
    c.oracle_setup(oracle)
    assert np.array_equal(c.o_ref, w.tc) and np.array_equal(c.o_q, w.qc) and np.array_equal(c.o_qrc, w.qrc), w
    c.engine_setup(E)
    assert E.lookup_mode() == 2 and E.get_option("cls_one_copy") != 2, w
    return c


def both_strands(E, oracle, w, options, ranges=None):
    """the world's plus strand and its flipped twin's minus strand (the same hits seen from the other strand), and the other strand
    of either; ranges(world, rev) -> the calls [(start, end)], default the whole strand.  -> the verdicts of the calls with hits"""
    out = []
    for x, rev in ((w, False), (w.flipped(), True)):
        E.ShutdownProcessor()
        c = open_world(E, oracle, x, options)
        for r in (rev, not rev):
            for s, e in (ranges(x, r) if ranges else [(0, x.end)]):
                v, _ = V.hold_call(E, c, x, r, s, e, options)
                if r == rev:
                    out.append(v)
    return out


def records_per_chunk(w, rev):
    """position records every 4096-hit chunk of the whole-strand call touches"""
    ex = w.hits_before(rev)
    first = np.flatnonzero(np.diff(ex) > 0)                              # positions with hits
    start = ex[first]
    n = int(ex[-1])
    return [int(np.searchsorted(start, min(c + 4096, n) - 1, side="right") - np.searchsorted(start, c, side="right") + 1)
            for c in range(0, n, 4096)]


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", LAUNCHES, ids=LAUNCH_IDS)
def test_one_hit_per_position(oracle, E, tile_worlds, options):
    w = tile_worlds("one_hit")
    ex = w.hits_before(False)
    assert np.count_nonzero(np.diff(ex) == 1) > 0.99 * w.end and ex[-1] > 4 * 4096
    for v in both_strands(E, oracle, w, options):
        assert v.forwards.size > 0.99 * v.num_hits                      # (a copy: both sides of nearly every hit stay alive)


@pytest.mark.parametrize("options", LAUNCHES, ids=LAUNCH_IDS)
def test_positions_further_apart_than_a_window_tile(oracle, E, tile_worlds, options):
    w = tile_worlds("islands")
    for rev, x in ((False, w), (True, w.flipped())):
        pos = np.flatnonzero(np.diff(x.hits_before(rev)) > 0)
        gaps = np.diff(pos)
        assert all(np.any(gaps == d) for d in ISLAND_STEPS), (rev, gaps)
        assert np.count_nonzero(gaps > TILE_BASES) >= 14 and np.count_nonzero((gaps > 100) & (gaps < 450)) >= 50
    for v in both_strands(E, oracle, w, options):
        assert v.num_hits > 4 * 64 and v.forwards.size > v.num_hits // 4 and v.audit.shape[0] > 0


@pytest.mark.parametrize("options", LAUNCHES, ids=LAUNCH_IDS)
def test_one_position_heavier_than_a_chunk(oracle, E, tile_worlds, options):
    w = tile_worlds("heavy")
    per = np.diff(w.hits_before(False))
    p = int(np.argmax(per))
    assert per[p] >= 13 * 390 > 4096 and p == 1500 and per[p - 19] > 0 and per[p + 19] > 0  # (the windows that overlap the word have no hit)
    assert w.hits_before(False)[p] % 4096 + per[p] > 4096               # a chunk cut inside the run
    both_strands(E, oracle, w, options)


@pytest.mark.parametrize("options", LAUNCHES, ids=LAUNCH_IDS)
@pytest.mark.parametrize("name", ["edges_0", "edges_1", "edges_15"])
def test_block_edges(oracle, E, tile_worlds, name, options):
    """whole strands, a call that ends inside the strand's last tile, and the last positions alone"""
    w = tile_worlds(name)
    assert w.query.size % 16 == {"edges_0": 0, "edges_1": 1, "edges_15": 15}[name]
    for rev, x in ((False, w), (True, w.flipped())):
        per = np.diff(x.hits_before(rev))
        assert per[0] > 0 and per[x.end - 1] > 0                        # hits at the first and at the last valid position
    both_strands(E, oracle, w, options, ranges=lambda x, r: [(0, x.end), (0, x.end - 40), (x.end - 30, x.end), (0, 1)])


@pytest.mark.parametrize("options", LAUNCHES, ids=LAUNCH_IDS)
@pytest.mark.parametrize("name,records", [("records_64", 64), ("records_65", 65)])
def test_records_of_a_chunk_at_the_tile_boundary(oracle, E, tile_worlds, name, records, options):
    w = tile_worlds(name)
    assert records_per_chunk(w, False)[0] == records and w.hits_before(False)[-1] > 4096
    both_strands(E, oracle, w, options)
