"""Seed vectors for the drop-in entries (sa_seed_and_filter, sa_rm_seed_and_filter) and a plain model of the decision they take.

The entries replace a call by the table-direct call over [first, last + 1) when the host vector is exactly what the seeder emits for
those positions (front.hip dropin_td_front), and keep the reference-shaped path on the uploaded words otherwise.  `expected_fast` says
which, from that sentence alone.  The cases are edits of the seeder's own vector, each built so that ONE of the engine's checks has
to reject it, next to exact vectors (cut, short, beside a masked run) that must stay fast.  tests/test_dropin_cases.py shows without a
GPU that every case is in the regime it is named for and that a wrongly taken fast path would change the result;
tests/test_gpu_dropin_paths.py runs them.

No GPU here: everything comes from the oracle and numpy."""
import numpy as np

from helpers import Case, SHAPE_12OF19
from segalign_amd import synth

SHAPE_W8 = "T0T0TT00T0TTT"   # custom pattern, weight 8 (tests/test_gpu_edge_cases.py): 9 words per position with transitions
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
WINDOW = 4000                # query positions per window
BEFORE = (1500, 1000, 2000, 500, 2500, 3000)   # ... of which this many lie in front of the masked run the window is laid around
RUN = 40                     # bases of the masked run laid into the query for each strand
BLOCK = 256                # threads per block of seed_verify_kernel == seeds per block of expand_hits_kernel
POLY_A = (12000, 12300)      # the target's poly-A tract: one bucket of more than 256 positions (the heavy word)
SIZES = (1, 255, 256, 257)   # groups of the short exact vectors
EDGE_SIZES = (1, 255, 256, 257, 512, 513)   # words of the hand-built vectors for the reference-shaped path

# Families whose edit cannot be placed so that it changes the answer at every index.  They only permute words, so the call's hits
# stay the same multiset and num_hits stays; the records could change only through which iteration (each with a dedup scope of its
# own) meets which hit, and the words that trade places stand at the same query position (two transition words of a group) or at
# neighbouring ones (two adjacent groups), whose hits extend to the same HSPs.  They are run and held to the oracle like every other
# case, but the CPU file does not ask that their answer differs from the unedited vector's -- except for the one swap of two groups
# that can matter: the pair on either side of the masked run, under a max_hits that ends an iteration between them.  (Reversed and
# shuffled vectors, the other word permutations, are made to matter the same way and are not exempt.)
EXEMPT = ("swap_groups", "swap_transition_words")
ONLY_COUNT = ("drop_group", "first_lowered")
ONLY_VERIFY = ("duplicate_group", "swap_groups", "foreign_key", "altered_transition_word", "swap_transition_words", "onto_masked")
HOST = ("one_word_short", "reversed", "shuffled", "doubled")
EXACT = ("window", "head_cut", "tail_cut", "beside_masked", "short", "one_word_short_exact")


_pair = []


def make_pair(O):
    """~30 kbp: 5 % diverged query with an indel about every 300 bases (many HSPs per window), 5 kbp pieces of it inverted (HSPs on
    both strands), soft-masked runs and one N run in each sequence, and a poly-A tract in the target.  Per strand one more masked run
    of RUN bases goes into the query where that strand's seeds hit most densely, placed so that the seed positions right in front
    of it and right behind it hit the target with their own 12of19 key: the edits beside a masked run then fall on groups that
    matter to the result.  -> (target, query, {rev: first base of the run in that strand's coordinates})"""
    if _pair:
        return _pair[0]
    t, q = synth.make_pair(30000, 321, 322, sub_rate=0.05, mask_frac=0.1, n_runs=1, indel_every=300, invert_frac=0.5, invert_block=5000)
    t, q = t.copy(), q.copy()
    t[POLY_A[0]:POLY_A[1]] = ord("A")
    c = Case(t, q, transition=False, chunk=q.size).oracle_setup(O)
    idx = c.o_index.astype(np.int64)
    bucket = idx - np.concatenate([[0], idx[:-1]])
    span, runs = len(SHAPE_12OF19), {}
    for rev in (False, True):
        words = c.host_seeds(0, q.size - span + 1, rev)
        hit = np.zeros(q.size, dtype=np.int64)      # 1 where a seed stands whose key hits
        hit[(words & M32).astype(np.int64)] = bucket[(words >> S32).astype(np.int64)] > 0
        seed = np.zeros(q.size, dtype=bool)
        seed[(words & M32).astype(np.int64)] = True
        dens = np.convolve(hit, np.ones(WINDOW, dtype=np.int64), mode="valid")   # dens[lo]: hitting positions of [lo, lo + WINDOW)
        lo = int(np.argmax(dens))
        # (... and the run begins and ends with C or T: code bits other than those of a masked base, so the key that the low bits
        #  give at a position whose window reaches into the run is not the key of the unmasked sequence)
        strand = c.query_rc_ascii if rev else q
        m = next(m for m in range(lo + BEFORE[0], lo + WINDOW - 600)
                 if hit[m - span] and hit[m + RUN] and seed[m - 3 * span:m + RUN + 3 * span].all()
                 and chr(strand[m]) in "CT" and chr(strand[m + RUN - 1]) in "CT")
        runs[rev] = m
        a = q.size - m - RUN if rev else m
        q[a:a + RUN] |= 0x20
    _pair.append((t, q, runs))
    return _pair[0]


_ASCII = np.frombuffer(b"ACGTNNNN", dtype=np.uint8)


def expected_fast(O, vector, strand_codes, shape, transition):
    """Does `vector` equal the seeder's vector for the positions [first, last + 1) it spans?  (first / last: the positions of its
    first and last word.)  The seeder is the oracle's; the strand is given as codes (only 0..3 can stand in a seed window)."""
    v = np.ascontiguousarray(vector, dtype=np.uint64)
    if v.size == 0:
        return False
    first, last = int(v[0] & M32), int(v[-1] & M32)
    if last < first or last + len(shape) > strand_codes.size:
        return False   # no such range of seed windows in the block
    k = O.generate_shape_pos(shape)
    want = O.make_seeds(_ASCII[strand_codes & 7].tobytes(), 0, first, last + 1, len(shape), k, transition)
    return bool(np.array_equal(v, want))


class DropinCase:
    def __init__(self, family, tag, rev, vector, base, fast, max_hits=None):
        self.family, self.tag, self.rev, self.fast, self.max_hits = family, tag, bool(rev), bool(fast), max_hits
        self.vector = np.ascontiguousarray(vector, dtype=np.uint64).reshape(-1)
        self.base = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)   # the exact vector the edit was applied to

    @property
    def name(self):
        return "%s[%s]%s" % (self.family, self.tag, "-" if self.rev else "+")

    def __repr__(self):
        return self.name


class Config:
    """One (shape, transition) over the shared pair; rm: the target against itself (sa_rm_seed_and_filter)."""

    def __init__(self, O, name, shape=SHAPE_12OF19, transition=True, rm=False, strands=(False, True)):
        self.O, self.name, self.shape, self.transition, self.rm = O, name, shape, transition, rm
        t, q, _ = make_pair(O)
        self.case = Case(t, t if rm else q, shape=shape, transition=transition, chunk=30000).oracle_setup(O)
        c = self.case
        self.tbits = [s for s in range(c.kmer_size) if transition and O.is_transition_at_pos(s) == 1]
        self.per = 1 + len(self.tbits)
        self.care = [i for i, ch in enumerate(shape) if ch in "1T"]
        idx = c.o_index.astype(np.int64)
        self.bucket = idx - np.concatenate([[0], idx[:-1]])     # positions per key
        self.heavy_key = int(np.argmax(self.bucket))
        self.window, self.G, self.cases = {}, {}, []
        for rev in strands:
            self._strand(rev)

    # ---- the pieces -----------------------------------------------------------------------------------------------------------
    def codes(self, rev):
        return self.case.o_qrc if rev else self.case.o_q

    def host_seeds(self, lo, hi, rev):
        """the seeder's vector for [lo, hi) (the oracle keeps ONE current seed shape: set it first)"""
        self.O.generate_shape_pos(self.shape)
        return self.case.host_seeds(lo, hi, rev)

    def word_hits(self, words):
        return self.bucket[(np.asarray(words, dtype=np.uint64) >> S32).astype(np.int64)]

    def key_of_low_bits(self, rev, pos):
        """the key the low two bits of the codes give at `pos`, whether or not a seed may stand there (kmer_dev.h kmer_at)"""
        k = 0
        for i in self.care:
            k = (k << 2) + (int(self.codes(rev)[pos + i]) & 3)
        return k

    def group(self, key, pos):
        """the seeder's words for a position that holds `key` (src/seeder.cpp:57-74)"""
        return np.array([((key ^ m) << 32) + pos for m in [0] + [2 << (2 * s) for s in self.tbits]], dtype=np.uint64)

    def answer(self, vector, rev, max_hits=None):
        c = self.case
        mh = {} if max_hits is None else {"max_hits": max_hits}
        if not self.rm:
            return c.oracle_saf(vector, rev, **mh)
        return self.O.seed_and_filter(c.o_ref, self.codes(rev), c.o_index, c.o_pos, vector, c.sub_mat, seed_size=c.seed_size,
                                      xdrop=c.xdrop, hspthresh=c.hspthresh, noentropy=c.noentropy, rm=(rev, 0, c.target.size), **mh)

    def valid_positions(self, rev):
        bad = np.concatenate([[0], np.cumsum(self.codes(rev) >= 4)])
        return (bad[len(self.shape):] - bad[:-len(self.shape)]) == 0    # a seed window may start at p

    # ---- one strand's window and cases ----------------------------------------------------------------------------------------
    def _pick_window(self, rev):
        """WINDOW positions around a masked (or N) run, one of BEFORE of them in front of it: among the placements that leave 300
        seed positions on either side of the run and have hit-bearing groups right beside it, the one with the most hit-bearing
        positions.  -> (lo, hi, index of the group in front of the run)"""
        valid = self.valid_positions(rev)
        edge = np.diff(np.concatenate([[1], valid.astype(np.int8), [1]]))
        best = None
        runs = zip(np.flatnonzero(edge == -1), np.flatnonzero(edge == 1))
        for ga, gb, before in [(ga, gb, before) for (ga, gb) in runs for before in BEFORE]:
            lo, hi = int(ga) - before, int(ga) - before + WINDOW
            if lo < 0 or hi > valid.size or valid[lo:ga].sum() < 300 or valid[gb:hi].sum() < 300:
                continue
            H = self.word_hits(self.host_seeds(lo, hi, rev)).reshape(-1, self.per).sum(1)
            k = int(valid[lo:ga].sum()) - 1        # the group in front of the run
            if H[k] == 0 or H[k + 1] == 0:         # the edits beside the run fall on groups that bear hits
                continue
            bearing = int((H > 0).sum())
            if best is None or bearing > best[0]:
                best = (bearing, lo, hi, k)
        assert best is not None, "no masked run with room for a window"
        return best[1:]

    def _strand(self, rev):
        per = self.per
        lo, hi, run = self._pick_window(rev)      # run: the group in front of the masked run the window is laid around
        self.window[rev] = (lo, hi)
        G = self.G[rev] = self.host_seeds(lo, hi, rev).reshape(-1, per)
        ng = G.shape[0]
        pos = (G[:, 0] & M32).astype(np.int64)
        Hw = self.word_hits(G)
        H = Hw.sum(1)
        rng = np.random.default_rng(5 + int(rev))

        def add(family, tag, vector, base, fast=False, max_hits=None):
            self.cases.append(DropinCase(family, tag, rev, vector, base, fast, max_hits))

        def head_from(i, cond):
            """the exact vector G[a:], the first a at which cond(a + i) holds: the edit at index i then falls on a group that matters"""
            for a in range(0, ng - i - 300):
                if cond(a + i):
                    return a
            raise AssertionError("no placement for index %d" % i)

        def tail_to(cond):
            """the exact vector G[:b], the last b at which cond(b - 1) holds"""
            for b in range(ng, 300, -1):
                if cond(b - 1):
                    return b
            raise AssertionError("no placement for the last group")

        def other_key(not_hits):
            """the key of a position of the window whose bucket differs in size from `not_hits` (and holds something)"""
            for g in range(ng):
                if Hw[g, 0] != not_hits and Hw[g, 0] > 0:
                    return int(G[g, 0] >> S32)
            raise AssertionError("no foreign key")

        # ---- only the count can reject: every group is the seeder's, positions ascend, one position of the span is missing
        for i in (1, BLOCK - 1, BLOCK):
            a = head_from(i, lambda g: H[g] > 0)
            add("drop_group", i, np.delete(G[a:], i, axis=0), G[a:])
        b = tail_to(lambda g: H[g - 1] > 0)
        add("drop_group", "last-1", np.delete(G[:b], b - 2, axis=0), G[:b])
        # the first group's position lowered: the seeder's group of an earlier position in place of the first group of G[a + back:];
        # the span then holds `back` more positions than the vector has groups (hit-bearing ones: the call over the span differs)
        for back in (2, BLOCK):
            a = head_from(back, lambda g: H[g - back + 1:g + 1].sum() > 0 and H[g] != H[g - back])
            add("first_lowered", back, np.concatenate([G[a:a + 1], G[a + back + 1:]]), G[a + back:])

        # ---- only the verify kernel can reject: as many groups as [first, last] has positions, first and last untouched
        def dup(base, dst, src):
            v = base.copy()
            v[dst] = v[src]
            return v
        a = head_from(0, lambda g: H[g] != H[g + 1])
        add("duplicate_group", 0, dup(G[a:], 1, 0), G[a:])
        for i in (1, BLOCK - 1, BLOCK):     # (BLOCK - 1: the pair lies across two blocks of the verify kernel)
            a = head_from(i, lambda g: H[g] != H[g + 1])
            add("duplicate_group", i, dup(G[a:], i, i + 1), G[a:])
        b = tail_to(lambda g: H[g] != H[g - 1])
        add("duplicate_group", "last", dup(G[:b], b - 2, b - 1), G[:b])

        for i in (0, 1, BLOCK - 1, BLOCK, ng - 1):
            j = min(max(i, 1), ng - 3)
            v = G.copy()
            v[[j, j + 1]] = v[[j + 1, j]]
            add("swap_groups", i if i < ng - 1 else "last", v, G)
            # a group with the key (and the transition words) of another position: only the key test of its first word can object
            v = G.copy()
            donor = next(g for g in range(ng) if H[g] > 0 and H[g] != H[i])   # (its words hit another number of positions)
            v[i] = self.group(int(G[donor, 0] >> S32), int(pos[i]))
            add("foreign_key", i if i < ng - 1 else "last", v, G)
            if per > 1:
                w = 1 + (i % (per - 1)) if i < ng - 1 else per - 1    # (the last group: the call's very last word, which `last` is read from)
                v = G.copy()
                v[i, w] = np.uint64((other_key(Hw[i, w]) << 32) + int(pos[i]))
                add("altered_transition_word", i if i < ng - 1 else "last", v, G)
            if per > 2:
                v = G.copy()
                v[i, [1, per - 1]] = v[i, [per - 1, 1]]
                add("swap_transition_words", i if i < ng - 1 else "last", v, G)
        # the two groups on either side of the masked run trade places (they lie on different sides of at least one indel, so under
        # a max_hits that ends the first iteration with the group in front of the run the swap moves an HSP into another iteration)
        assert pos[run + 1] - pos[run] > 1 and 0 < run < ng - 2
        v = G.copy()
        v[[run, run + 1]] = v[[run + 1, run]]
        add("swap_groups", "across the run", v, G, max_hits=int(H[:run + 1].sum()) + 1)
        # a group moved onto the position without a seed next to it, with the key the low code bits give there
        for (g, step) in ((run, 1), (run + 1, -1)):
            for a in sorted({0, g - (BLOCK - 1)}):   # ... and once with that group at index BLOCK - 1
                v = G[a:].copy()
                p = int(pos[g]) + step
                v[g - a] = self.group(self.key_of_low_bits(rev, p), p)
                add("onto_masked", "%+d@%d" % (step, g - a), v, G[a:])

        # ---- the host's own checks
        if per > 1:
            b = tail_to(lambda g: Hw[g, per - 1] > 0)
            add("one_word_short", "window", G[:b].reshape(-1)[:-1], G[:b])
        else:
            add("one_word_short_exact", "window", G.reshape(-1)[:-1], G, fast=True)
        # (reversed and shuffled words are the same multiset of hits; with max_hits at a third of them the iterations, each with a
        #  dedup scope of its own, meet the window's HSPs in another order)
        third = max(int(H.sum()) // 3, 1)
        add("reversed", "window", G.reshape(-1)[::-1], G, max_hits=third)
        add("shuffled", "window", rng.permutation(G.reshape(-1)), G, max_hits=third)
        for n in (ng, BLOCK):
            add("doubled", n, np.concatenate([G[:n], G[:n]]), G[:n])

        # ---- exact vectors: they must stay on the fast path
        add("window", "all", G, G, fast=True)
        for k in (1, 2):
            add("head_cut", k, G[k:], G, fast=True)
            add("tail_cut", k, G[:-k], G, fast=True)
        k = run
        add("beside_masked", "ends", G[:k + 1], G, fast=True)
        add("beside_masked", "begins", G[k + 1:], G, fast=True)
        add("beside_masked", "across", G[k:k + 2], G, fast=True)
        for n in SIZES:
            add("short", n, G[:n], G, fast=True)                          # from the head of the window
            add("short", "%d across" % n, G[k + 2 - n:k + 2] if k + 2 >= n else G[:n], G, fast=True)   # ending right behind the run


# ---- hand-built vectors for the reference-shaped path (seed_lookup -> scan -> plan -> expand_hits) ------------------------------
class EdgeVector:
    def __init__(self, kind, n, at, rev, vector, max_hits):
        self.kind, self.n, self.at, self.rev, self.vector, self.max_hits = kind, n, at, bool(rev), vector, max_hits

    @property
    def name(self):
        return "%s n=%d at=%d max_hits=%s%s" % (self.kind, self.n, self.at, self.max_hits, "-" if self.rev else "+")


def edge_vectors(cfg):
    """Vectors of EDGE_SIZES words around the 256-seed block of expand_hits_kernel, made of words that hit nothing, words with exactly
    one hit and the heavy word (the poly-A bucket: more than 256 positions, more than one block's worth of lanes for one seed):
      lonely: one hit-bearing word among words that hit nothing (hazard H5 when it stands at index 0)
      heavy : the heavy word among words that hit nothing, max_hits below its bucket (it alone exceeds an iteration)
      full  : every word bears one hit, the heavy word among them; max_hits puts an iteration boundary between words 255 and 256
              (the hits of words 0..255, plus one), and -- second run -- lies below the heavy bucket
    the special word at index 0, 255, 256 and n - 1."""
    out = []
    for rev in (False, True):
        words = cfg.G[rev].reshape(-1)
        hits = cfg.word_hits(words)
        none, one = words[hits == 0], words[hits == 1]
        assert none.size >= max(EDGE_SIZES) and one.size >= max(EDGE_SIZES), (none.size, one.size)
        heavy = np.uint64((cfg.heavy_key << 32) + int(words[0] & M32))
        heavy_hits = int(cfg.bucket[cfg.heavy_key])
        for n in EDGE_SIZES:
            for at in sorted({0, BLOCK - 1, BLOCK, n - 1}):
                if at >= n:
                    continue
                v = none[:n].copy()
                v[at] = one[at]
                out.append(EdgeVector("lonely", n, at, rev, v, None))
                v = none[:n].copy()
                v[at] = heavy
                out.append(EdgeVector("heavy", n, at, rev, v, heavy_hits // 2))
                v = one[:n].copy()
                v[at] = heavy
                if n > BLOCK:
                    out.append(EdgeVector("full", n, at, rev, v, int(cfg.word_hits(v[:BLOCK]).sum()) + 1))
                out.append(EdgeVector("full", n, at, rev, v, heavy_hits * 3 // 4))
    return out


_configs = {}


def configs(O):
    """The configurations, built once per process: (name, Config) in a fixed order."""
    if not _configs:
        _configs["12of19"] = Config(O, "12of19")
        _configs["12of19 notransition"] = Config(O, "12of19 notransition", transition=False)
        _configs["weight 8"] = Config(O, "weight 8", shape=SHAPE_W8)
        _configs["repeat masker"] = Config(O, "repeat masker", rm=True, strands=(False,))
    return _configs
