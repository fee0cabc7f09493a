"""The blocks tests/test_gpu_sequence_images.py sends, and what each is for (DESIGN.md 4.1').  tests/test_image_model.py shows on the
CPU that every one of them is in the regime it names: the planted letters reach every place, the presence blocks hold their code where
they say, the large blocks wrap the loops they are meant to wrap."""
import numpy as np

# the smallest lengths at which an edge of a builder moves
LENGTHS = ([0, 1, 2, 3, 4, 5, 6, 7]                 # the rev-comp dword tail, 4-bit parity; 0: the packers alone run
           + [15, 16, 17, 31, 32, 33]               # the 16-byte vector body and the scalar tail
           + [127, 128, 129]                        # the physical size of a 2-bit phase copy steps from 384 to 512
           + [253, 254, 255, 256, 257]              # the 4-bit stride steps at 256
           + [379, 380, 381, 382, 383, 384, 385]    # the line edge of ref2 at base 384, the 2-bit stride step at 384
           + [767, 768, 769, 4099])
RM_LENGTHS = [5, 17, 385, 4099]
LONG_QUERY = 600_001            # wraps the grid-stride loops of the three packers (sixteen 2-bit copies)
LONG_TARGET = (1 << 23) + 70_001  # wraps the loops of the encoder, the row coder and the presence kernel
GRID_BLOCKS, BLOCK_THREADS = 2048, 256   # grid_for() of encode.hip: at most 256 * 8 workgroups of 256 threads

# what gets planted: soft-masked, N, the separator, other IUPAC letters, and byte values around the edges of the LUT
SPECIALS = [ord(ch) for ch in "acgtNn&RYKMSW"] + [0x00, 0x7F, 0x80, 0xFF]
_COMPLEMENT = np.full(256, ord("C"), dtype=np.uint8)
for _a, _b in ("AT", "CG", "GC", "TA"):
    _COMPLEMENT[ord(_a)] = ord(_b)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def places(n):
    """{position: name of the place} of a block of n bases: base 0, base n - 1, the four phases on either side of every base 384 m and of
    the boundary between the 16-byte body and the scalar tail"""
    out = {}
    bounds = [("line", 384 * m) for m in range(1, n // 384 + 2)] + [("tail", n - n % 16)]
    for kind, b in bounds:
        for o in range(-4, 4):
            if 0 <= b + o < n and b <= n:
                out.setdefault(b + o, "%s%+d" % (kind, o))
    if n:
        out[0] = "first"
        out[n - 1] = "last"
    return out


def block(n, variant, sparse=False, seed=None):
    """random A/C/G/T with SPECIALS planted at places(n), rotated by `variant`; sparse: only at every third place, so that the bases
    around an edge are mostly real ones (the 2-bit copies store every special as 0)"""
    rng = np.random.default_rng(1000 * n + variant if seed is None else seed)
    a = _ACGT[rng.integers(0, 4, n)].copy()
    for i, pos in enumerate(sorted(places(n))):
        if sparse and (i + variant) % 3:
            continue
        a[pos] = SPECIALS[(i + variant) % len(SPECIALS)]
    return a


def planted(n, variant, sparse=False):
    """[(place name, special)] of block(n, variant, sparse)"""
    pl = places(n)
    return [(pl[pos], SPECIALS[(i + variant) % len(SPECIALS)]) for i, pos in enumerate(sorted(pl)) if not (sparse and (i + variant) % 3)]


def poison(a, seed=7):
    """a LONGER block of complementary content: the complement under every A/C/G/T of `a`, C under everything else, and C/G/T (never
    code 0) behind it -- what a builder fails to overwrite then differs from what it should have written, in every image"""
    rng = np.random.default_rng(seed + a.size)
    n = max(2 * a.size + 300, a.size + 1500)
    out = np.frombuffer(b"CGT", dtype=np.uint8)[rng.integers(0, 3, n)].copy()
    out[:a.size] = _COMPLEMENT[a]
    return out


def blocks_of(n):
    """the four blocks of length n and where they go: two passes of (target, query buffer 0, query buffer 1)"""
    v = LENGTHS.index(n) if n in LENGTHS else n % 17
    return ((block(n, v, sparse=True), block(n, v), block(n, v + 5, sparse=True)),
            (block(n, v + 9), block(n, v + 11, sparse=True), block(n, v + 13)))


def uniform(n, ch):
    return np.full(n, ord(ch), dtype=np.uint8)


def lower_case(n):
    return np.frombuffer(b"acgt", dtype=np.uint8)[np.random.default_rng(n).integers(0, 4, n)].copy()


# ---- presence -----------------------------------------------------------------------------------------------------------
PRESENCE_LEN = 45          # a 32-byte vector body and a 13-byte tail
CODE_LETTER = {4: "g", 5: "N", 6: "R", 7: "&"}


def presence_blocks():
    """{name: (block, the one code >= 4 in it, its position)}: each of the codes 4..7 alone in the vector body, alone in the tail, only at
    base 0, only at base len - 1"""
    out = {}
    for code, ch in CODE_LETTER.items():
        for where, pos in (("body", 21), ("tail", 32 + code), ("first", 0), ("last", PRESENCE_LEN - 1)):
            a = _ACGT[np.random.default_rng(code).integers(0, 4, PRESENCE_LEN)].copy()
            a[pos] = ord(ch)
            out["code %d %s" % (code, where)] = (a, code, pos)
    return out


def plain(n, seed):
    return _ACGT[np.random.default_rng(seed).integers(0, 4, n)].copy()


# ---- the large blocks ---------------------------------------------------------------------------------------------------
def long_query():
    return block(LONG_QUERY, 3, sparse=True)


def long_target():
    """specials around every edge as everywhere; the only separator of the block lies in the vector body of the SECOND sweep of the
    grid-stride loops, the only N in the scalar tail"""
    a = block(LONG_TARGET, 6, sparse=True)
    a[a == ord("&")] = ord("R")
    a[(a == ord("N")) | (a == ord("n"))] = ord("Y")
    a[(1 << 23) + 4321] = ord("&")
    a[LONG_TARGET - 1] = ord("N")
    return a


# ---- why presence exists: one call whose HSP hangs on the N bit of the query's mask ---------------------------------------------------------
def n_matrix():
    """+40 / -100 on A/C/G/T; every pair with a soft-masked base or an N -- N against N too -- scores +120, above every A/C/G/T pair;
    other IUPAC letters -100, the separator -1000"""
    m = np.full((8, 8), 120, dtype=np.int32)
    m[:4, :4] = -100
    m[np.arange(4), np.arange(4)] = 40
    m[6, :] = m[:, 6] = -100
    m[7, :] = m[:, 7] = -1000
    return m.reshape(64)


class IslandCase:
    """A query of 335 bases (a 320-byte vector body and a 15-byte tail) on the diagonal 500 of a random target.  Every base mismatches the
    target but an island of 40 identical bases in front of the tail; the tail is thirteen N and two mismatches, and the target under it and
    behind it is a run of C.  The HSP of every seed hit inside the island is island + N run: 40 x 40 + 13 x 120 = 3160 >= hspthresh 3000.
    A mask without the N bit leaves the N pairs out of the class scores: the N run then counts as A against C, -100 a base, and no
    bound of a hit inside the island exceeds 1600."""
    N_LEN, TAIL, ISLAND, RUN, DIAG = 335, 15, 40, 13, 500
    XDROP, HSPTHRESH, SEED = 910, 3000, 19

    def __init__(self):
        rng = np.random.default_rng(24)
        t = rng.integers(0, 4, 2000).astype(np.uint8)
        body = self.N_LEN - self.TAIL
        t[self.DIAG + body:self.DIAG + body + 80] = 1                       # C under the tail and behind the block
        q = (t[self.DIAG:self.DIAG + self.N_LEN] + 1 + rng.integers(0, 3, self.N_LEN).astype(np.uint8)) & 3   # never the target's base
        self.island = (body - self.ISLAND, body)
        q[self.island[0]:self.island[1]] = t[self.DIAG + self.island[0]:self.DIAG + self.island[1]]
        q[body + self.RUN:] = 2                                             # G against C
        self.target = _ACGT[t].copy()
        self.query = _ACGT[q].copy()
        self.query[body:body + self.RUN] = ord("N")
        self.n_run = (body, body + self.RUN)
        self.hsp = (self.DIAG + self.island[0], self.island[0], self.ISLAND + self.RUN - 1, 40 * self.ISLAND + 120 * self.RUN)   # (len as the reference counts it)

    def anchors(self):
        """(target, query) anchors of the seed hits whose window lies inside the island: the base behind the window"""
        return [(self.DIAG + p + self.SEED, p + self.SEED) for p in range(self.island[0], self.island[1] - self.SEED + 1)]


def class_bound(t2, q2, cls, anchor_t, anchor_q, seed, xdrop, right_bases=54, left_bases=58):
    """The class filter's bound of a hit (extend.hip 1d) on 2-bit codes: the right side walks `right_bases` from the anchor in fields of
    six bases, the left side enters the context in front of the seed window with seed x the largest class score and walks `left_bases`
    (fields of six, then one of four); bases outside a block read 0.  -> (bestR + bestL, both sides dropped: more than xdrop below
    their best at a field end)"""
    def code(c, i):
        return int(c[i]) if 0 <= i < len(c) else 0

    def walk(start_t, start_q, step, n, T):
        best, lowest = T, 0
        for k in range(n):
            T += cls[code(t2, start_t + step * k) ^ code(q2, start_q + step * k)]
            best = max(best, T)
            if (k + 1) % 6 == 0 or k == n - 1:
                lowest = min(lowest, T - best)
        return best, lowest < -xdrop
    best_r, drop_r = walk(anchor_t, anchor_q, 1, right_bases, 0)
    best_l, drop_l = walk(anchor_t - seed - 1, anchor_q - seed - 1, -1, left_bases, seed * max(max(cls), 0))
    return best_r + best_l, drop_r and drop_l
