"""GPU: the class filter's POSITION TILE (extend.hip 1d, one-copy form) -- the SLOTS = 32 slots a wave keeps in LDS, each with the
finished seven-dword query string of one query position, its anchor and the address of its record stream -- at the smallest shapes at
which it can go wrong.  Every call is held, hit for hit and by EXACT equality, to tests/filter_model.py (forwards field for field, audit
list, num_candidates, sub-list counters) and to the oracle's vector, through hold_call of tests/test_gpu_filter_verdicts.py and the
worlds of tests/test_gpu_cls_tiles.py; the model knows nothing of tiles, slots, launch geometry or wave partition.

What the tile is, so that the worlds below can be read: the slots hold td_rec[base, base + 32).  A 64-hit buffer with a lane whose
position record lies outside them builds them anew from its first lane's record on (lane l makes slot l, records past the last one
stay on it); the build takes its windows from the raw window tiles of test_gpu_cls_tiles.py, loads those anew from its first slot on
when a slot's windows lie outside them, and reads from memory the windows that do not fit even then.  A buffer that holds more than 32
positions makes its strings per lane.  A string is read when a buffer's records are requested, one buffer ahead of its scoring.

Every world runs on the plus strand and, as its flipped twin, on the minus strand, under the default launch (one wave per 4096-hit
chunk, 1024 lanes per workgroup) and with one and three waves for the whole call in workgroups of 64 and 256 lanes.  Every world
but the heavy one forwards most of its hits, so a string out of the wrong slot shows as a missing or an extra forward.  (The heavy
world is test_gpu_cls_tiles.py's: its target is longer than 64 kbp -- 4097 hits of one position are 4097 windows of 19 bases -- and
its copies cannot carry the query's flanks, which would be table buckets of 5070 entries, beyond the size up to which the device's
bucket order is the model's; there a wrong string shows in the fields of the forwards and in the audit list.)"""
import numpy as np
import pytest

import filter_regimes as R
import test_gpu_cls_tiles as T
import test_gpu_filter_verdicts as V

pytestmark = pytest.mark.gpu

SLOTS = 32


def counted_world(name, mat, counts, seed):
    """without transitions: the query is a random stretch of len(counts) positions, and position p has counts[p] hits: the target holds,
    for k = 1, 2, ..., every maximal run of positions with at least k hits once.  Layers one and two are nearly the whole stretch, so
    their hits have matching flanks and are forwarded"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    s = T.dna(rng, counts.size + 18)
    parts = [T.GAP]                                                       # (target position 0 is never indexed)
    for k in range(1, int(counts.max()) + 1):
        edge = np.diff(np.concatenate([[0], (counts >= k).astype(np.int8), [0]]))
        for lo, hi in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):   # positions [lo, hi)
            parts += [s[lo:hi + 18], T.GAP]
    return T.TileWorld(name, T.join(parts), s.copy(), mat, transition=False)


def slots_world(mat):
    """buffers of exactly 31, 32 and 33 positions (4 + 30 x 2, 32 x 2 and 1 + 1 + 31 x 2 hits: the last buffers the slots serve and the
    first one made per lane); three hits per position, where every other buffer builds the slots anew and starts in the middle of a
    position's run, so the slot of that position is built a second time; two hits per position behind an odd count, where every buffer
    cuts two runs and holds 33 positions; and positions of one to five hits at random.  Every cycle is padded to whole buffers; a
    dozen cycles make more than three chunks, and the stretch is long enough for the raw window tiles to be loaded anew inside a
    build several times, on the strand whose windows ascend and on the one whose windows descend"""
    rng = np.random.default_rng(707)
    counts = []
    for _ in range(13):
        cyc = [4] + [2] * 30 + [2] * 32 + [1, 1] + [2] * 31 + [3] * 64 + [3] + [2] * 94 + [1] + [int(x) for x in rng.integers(1, 6, 150)]
        pad = -sum(cyc) % 64
        counts += cyc + ([pad] if pad else [])
    w = counted_world("slots", mat, counts, 708)
    assert w.query.size <= 65536 and w.target.size <= 65536
    return w


def edges2_world(mat, length):
    """every position of the query has two hits, the first and the last valid one of either strand included: 32 positions per buffer"""
    rng = np.random.default_rng(800 + length)
    t = T.dna(rng, 4000)
    return T.TileWorld("edges2 %d" % length, T.join([T.GAP, t, T.GAP, t]), t[700:700 + length].copy(), mat)


WORLDS = {
    "slots": slots_world,
    "islands": T.islands_world,                        # slots whose windows no raw tile holds: the build reads them from memory
    "heavy": T.heavy_world,                            # one string for 5070 hits: chunk and wave cuts and rebuilds inside its run
    "edges2_0": lambda m: edges2_world(m, 1600),       # query lengths = 0, 1 and 15 mod 16
    "edges2_1": lambda m: edges2_world(m, 1601),
    "edges2_15": lambda m: edges2_world(m, 1615),
}


@pytest.fixture(scope="module")
def string_worlds(oracle):
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


def buffers(w, rev):
    """of the whole-strand call: (positions every 64-hit buffer holds, whether its first hit is the first of its position)"""
    ex = w.hits_before(rev)
    start = ex[np.flatnonzero(np.diff(ex) > 0)]                          # first hit of every position with hits
    n = int(ex[-1])
    b = np.arange(0, n, 64)
    lo = np.searchsorted(start, b, side="right")
    hi = np.searchsorted(start, np.minimum(b + 63, n - 1), side="right")
    return hi - lo + 1, np.isin(b, start)


def mostly_forwarded(verdicts):
    for v in verdicts:
        assert v.forwards.size > v.num_hits // 2, (v.forwards.size, v.num_hits)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", T.LAUNCHES, ids=T.LAUNCH_IDS)
def test_buffers_at_the_slot_count_and_rebuilds_inside_a_run(oracle, E, string_worlds, options):
    w = string_worlds("slots")
    for rev, x in ((False, w), (True, w.flipped())):
        per, at_start = buffers(x, rev)
        assert x.hits_before(rev)[-1] > 3 * 4096
        assert all(np.any(per == k) for k in (SLOTS - 1, SLOTS, SLOTS + 1)), (rev, np.unique(per))
        assert np.count_nonzero(~at_start & (per <= SLOTS - 8)) > 20      # three hits per position: served by slots, first lane inside a run
        assert np.count_nonzero(~at_start & (per == SLOTS + 1)) > 20      # two hits per position behind an odd count
        assert x.end > 4 * T.WIN_SPAN_BASES                               # the raw tiles are loaded anew along the call
    mostly_forwarded(T.both_strands(E, oracle, w, options))


@pytest.mark.parametrize("options", T.LAUNCHES, ids=T.LAUNCH_IDS)
def test_whole_window_context(oracle, E, string_worlds, options):
    """left_skip = 0: the other strand's window starts at another base, in the build and in the per-lane path"""
    w = string_worlds("slots")
    mostly_forwarded(T.both_strands(E, oracle, w, dict(options, ctx_skip_seed=0)))


@pytest.mark.parametrize("options", T.LAUNCHES, ids=T.LAUNCH_IDS)
def test_slots_with_windows_no_raw_tile_holds(oracle, E, string_worlds, options):
    w = string_worlds("islands")
    for rev, x in ((False, w), (True, w.flipped())):
        per, _ = buffers(x, rev)
        assert np.all(per < SLOTS) and np.median(per) >= 8                 # every buffer is served by slots, which span several islands
    for v in T.both_strands(E, oracle, w, options):
        assert v.forwards.size > v.num_hits // 4 and v.audit.shape[0] > 0


@pytest.mark.parametrize("options", T.LAUNCHES, ids=T.LAUNCH_IDS)
def test_one_string_for_more_than_a_chunk(oracle, E, string_worlds, options):
    w = string_worlds("heavy")
    ex = w.hits_before(False)
    per = np.diff(ex)
    p = int(np.argmax(per))
    assert per[p] >= 13 * 390 > 4096 and p == 1500 and ex[p] % 4096 + per[p] > 4096      # a chunk cut inside the run
    T.both_strands(E, oracle, w, options)


@pytest.mark.parametrize("options", T.LAUNCHES, ids=T.LAUNCH_IDS)
@pytest.mark.parametrize("name", ["edges2_0", "edges2_1", "edges2_15"])
def test_block_edges(oracle, E, string_worlds, name, options):
    """whole strands (the last build's records are clamped at the last one, the other strand's first window reaches the zero tail), a
    call that ends inside the strand's last tile, the last positions alone and the first one alone"""
    w = string_worlds(name)
    assert w.query.size % 16 == {"edges2_0": 0, "edges2_1": 1, "edges2_15": 15}[name]
    for rev, x in ((False, w), (True, w.flipped())):
        per = np.diff(x.hits_before(rev))
        assert per[0] >= 2 and per[x.end - 1] >= 2                        # hits at the first and at the last valid position
        assert np.median(buffers(x, rev)[0]) == SLOTS
    mostly_forwarded(T.both_strands(E, oracle, w, options, ranges=lambda x, r: [(0, x.end), (0, x.end - 40), (x.end - 30, x.end), (0, 1)]))
