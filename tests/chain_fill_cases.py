"""The chains that tests/test_gpu_chain_fill.py runs through sa_fill_chains, and the regime each of them is there for, asserted on
what the model (chain_fill_model.fill) says.  tests/test_chain_fill_model.py asserts the same regimes on the CPU, on the codes this
file derives itself, so that a case that lost its regime shows before a GPU is involved.

One target and one query are built piece by piece: a member is a stretch the query copies from the target, a link is the space to the
next member, random on both sides but for what is planted there: copies of a piece of the link's target on a diagonal of its
rectangle, or the bases themselves where a test needs certain weights."""
import numpy as np

import chain_fill_model as F
import hsp_chain_model as M

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N = 700_000
SIZES = [1, 63, 64, 65, 127, 128, 129]  # dt + dq - 1
SMALL = dict(thresh=300, xdrop=200)  # four matches in a row: chance HSPs on most diagonals of a small rectangle
ONE = dict(thresh=90, xdrop=100)  # a single matching pair is an HSP
RANDOM_PARAMS = [dict(), dict(thresh=1500, xdrop=500, diag_pen=3, anti_pen=2, max_gap=250),
                 dict(thresh=2000, gap_costs="loose", anti_pen=1, min_fill=2500)]


def codes(a):
    """The plain codes of ASCII bases, as the engine holds them (A C G T = 0 .. 3, N = 5, & = 7)."""
    lut = np.full(256, 5, dtype=np.uint8)
    lut[list(b"ACGT")] = [0, 1, 2, 3]
    lut[ord("&")] = 7
    return lut[a]


def revcomp(a):
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return comp[a[::-1]]


class Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.t, self.q = ACGT[self.rng.integers(0, 4, N)], ACGT[self.rng.integers(0, 4, N)]
        self.rows, self.at = [], 1000

    def member(self, r, s, b):
        self.rows.append((r, s, b, 1000 + len(self.rows)))  # the input score is arbitrary: a member is returned as it came
        self.q[s:s + b] = self.t[r:r + b]
        return len(self.rows) - 1

    def chain(self, links, bases=20):
        """links[k] = (dt, dq, plants): plants are (i, j, n), the link's target bases i .. i + n copied to its query bases from j on,
        or (tseq, qseq[, i, j]) bytes written on both sides, at the rectangle's origin or at its bases i and j."""
        r = s = self.at
        out = [self.member(r, s, bases)]
        for dt, dq, plants in links:
            re, qe = r + bases, s + bases
            for p in plants:
                if len(p) == 3:
                    i, j, n = p
                    assert 0 <= i and i + n <= dt and 0 <= j and j + n <= dq
                    self.q[qe + j:qe + j + n] = self.t[re + i:re + i + n]
                else:
                    tseq, qseq = (np.frombuffer(x, dtype=np.uint8) for x in p[:2])
                    i, j = p[2:] if len(p) == 4 else (0, 0)
                    assert i + tseq.size <= dt and j + qseq.size <= dq
                    self.t[re + i:re + i + tseq.size], self.q[qe + j:qe + j + qseq.size] = tseq, qseq
            r, s = re + dt, qe + dq
            out.append(self.member(r, s, bases))
        self.at = max(r, s) + bases + 50
        assert self.at < N - 100
        return out


def random_links(rng, n):
    links = []
    for _ in range(n):
        dt, dq = int(rng.integers(0, 301)), int(rng.integers(0, 301))
        plants = []
        kind = int(rng.integers(0, 6))
        if min(dt, dq) >= 90 and kind >= 2:
            n1 = int(rng.integers(35, min(dt, dq) // 2))
            i, j = int(rng.integers(0, dt // 2 - n1 // 2 + 1)), int(rng.integers(0, dq // 2 - n1 // 2 + 1))
            plants.append((i, j, n1))
            if kind == 4:  # a second one behind the first: collinear
                n2 = int(rng.integers(20, min(dt - i - n1, dq - j - n1) + 1))
                plants.append((int(rng.integers(i + n1, dt - n2 + 1)), int(rng.integers(j + n1, dq - n2 + 1)), n2))
            if kind == 5 and dt - i - n1 >= 40 and j >= 0:  # a second one that crosses the first: later on the target, not on the query
                n2 = min(int(rng.integers(35, 80)), dt - i - n1, dq)
                plants.append((i + n1 + int(rng.integers(0, dt - i - n1 - n2 + 1)), int(rng.integers(0, max(1, min(j + n1, dq - n2)))), n2))
        links.append((dt, dq, plants))
    return links


def build_world():
    b = Builder(2025)
    rng = b.rng
    W = {}
    W["sizes"] = [b.chain([((D + 1) // 2, D + 1 - (D + 1) // 2, [(0, 0, min((D + 1) // 2, D + 1 - (D + 1) // 2))])]) for D in SIZES]
    W["sizes"] += [b.chain([(D, 1, [])]) for D in SIZES[1:]] + [b.chain([(1, D, [])]) for D in SIZES[1:]]
    W["tiny"] = [b.chain([(dt, dq, [(0, 0, 1)])]) for dt in (1, 2) for dq in (1, 2)] + [b.chain([(1, 300, [(0, 150, 1)])]),
                                                                                          b.chain([(300, 1, [(150, 0, 1)])])]
    W["past_stitch"] = [b.chain([(2049, 2049, [(700, 650, 60), (1300, 1400, 45)])])]
    W["skinny"] = [b.chain([(70, 5000, [(0, 2500, 34), (36, 4966, 34)])]), b.chain([(5000, 70, [(3000, 15, 50)])])]
    # the four edges, and on the main diagonal both corners: two segments on one diagonal
    W["edges"] = [b.chain([(200, 200, [(0, 60, 40), (70, 0, 40), (160, 110, 40), (110, 160, 40)])]), b.chain([(200, 200, [(0, 0, 40), (160, 160, 40)])])]
    # under ONE every matching pair is an HSP: the link's first and last diagonal (one cell each) and both sides of every 64-block
    W["diagonals"] = [b.chain([(100, 100, [(0, 99, 1), (99, 0, 1), (10, 46, 5), (30, 65, 5), (50, 22, 5), (70, 41, 5)])])]
    # weights by hand on the main diagonal (C/C 100, C/T -31, C/G -125): see hand_regimes
    W["hand"] = [b.chain([(4, 4, [(b"CCCC", b"CTTC")])]), b.chain([(11, 11, [(b"CCCCCCCCCCC", b"CCCCCGGGGCC")])])]
    # the target's separator inside a plant and right before one; the query's inside a plant and on one's last column
    W["separators"] = [b.chain([(120, 120, [(b"&", b"", 60, 0), (10, 10, 100), (b"", b"A", 0, 60)])]),
                       b.chain([(120, 120, [(10, 10, 100), (b"", b"&", 0, 61)])]),
                       b.chain([(120, 120, [(b"&", b""), (1, 1, 60)])]), b.chain([(120, 120, [(60, 60, 60), (b"", b"&", 0, 119)])])]
    W["homopolymer"] = [b.chain([(20, 20, [(b"A" * 20, b"A" * 20)])])]
    W["limits"] = [b.chain([(100, 60, [(5, 5, 50)])])]
    W["lengths"] = [b.chain([(int(rng.integers(0, 40)), int(rng.integers(0, 40)), []) for _ in range(n - 1)], bases=6) for n in (1, 2, 65, 300)]
    W["random"] = [[b.chain(random_links(rng, int(rng.integers(1, 30))), bases=int(rng.integers(1, 30))) for _ in range(25)] +
                   [b.chain([(0, 25, []), (30, 0, []), (0, 0, []), (120, 120, [(40, 50, 22)])])] for _ in range(6)]  # 22 bases: 2002 .. 2200
    W["crossing"] = [b.chain([(300, 300, [(20, 150, 60), (150, 20, 45)])])]
    W["collinear"] = [b.chain([(400, 400, [(10, 30, 50), (100, 110, 60), (250, 300, 70)])])]
    W["long_row"] = [b.chain([(30000, 1, [])])]  # 30 016 lanes; under ONE about 7 500 HSPs, one per matching cell
    return b.t, b.q, M.make(b.rows), W


def diag_index(link, h, re, qe):
    """e = d + dq - 1 of a found HSP of a link whose rectangle starts at (re, qe)."""
    return (int(h["ref_start"]) - re) - (int(h["query_start"]) - qe) + int(link["dq"]) - 1


def as_seg(found):
    """Found HSPs as hsp_chain_model.SEG records."""
    out = np.zeros(found.size, dtype=M.SEG)
    for f in M.SEG.names:
        out[f] = found[f]
    return out


def origin_of(hsps, chain, k=0):
    """(re, qe) of the link after member k of a chain."""
    r, s, n, _ = (int(v) for v in hsps[chain[k]])
    return r + n + 1, s + n + 1


def on_main(res, hsps, chain):
    """The found HSPs of a one-link chain's main diagonal as (i, len, score); res: the model's result on that chain alone."""
    re, qe = origin_of(hsps, chain)
    return [(int(h["ref_start"]) - re, int(h["len"]), int(h["score"])) for h in res[5] if int(h["ref_start"]) - re == int(h["query_start"]) - qe]


# ---- the regimes, each on what the model returned for the case's chains (res = F.fill's tuple) -------------------------------

def regime_sizes(res):
    links = res[4]
    assert sorted(set((links["dt"] + links["dq"] - 1).tolist())) == SIZES and np.all(links["flags"] == 0)
    assert (links["n_hsps"] > 0).sum() >= 12 and (links["n_hsps"] > 500).any() and links["n_hsps"][0] == 1  # under ONE


def regime_tiny(res):
    links = res[4]
    assert list(zip(links["dt"].tolist(), links["dq"].tolist())) == [(1, 1), (1, 2), (2, 1), (2, 2), (1, 300), (300, 1)]
    assert np.all(links["n_hsps"] >= 1) and np.all(links["n_fill"] >= 1) and links["n_hsps"][4] > 40 and links["n_hsps"][5] > 40


def regime_past_stitch(res):
    l = res[4][0]
    assert (l["dt"], l["dq"], l["cells"], l["n_hsps"], l["n_fill"]) == (2049, 2049, 2049 * 2049, 2, 2)


def regime_skinny(res, hsps, chains):
    links = res[4]
    assert links["n_hsps"].tolist() == [2, 1] and links["n_fill"].tolist() == [2, 1]
    re, qe = origin_of(hsps, chains[0])
    rel = [(int(h["ref_start"]) - re, int(h["query_start"]) - qe, int(h["len"]) + 1) for h in res[5][:2]]
    assert any(i == 0 for i, j, n in rel) and any(i + n == 70 and j + n == 5000 for i, j, n in rel)  # the first row; the far corner


def regime_edges(res, hsps, chains):
    found, links = res[5], res[4]
    assert links["n_hsps"].tolist() == [4, 2] and links["n_fill"].tolist() == [2, 2]
    re, qe = origin_of(hsps, chains[0])
    rel = [(int(h["ref_start"]) - re, int(h["query_start"]) - qe, int(h["len"]) + 1) for h in found[:4]]
    assert any(i == 0 for i, j, n in rel) and any(j == 0 for i, j, n in rel) and any(i + n == 200 for i, j, n in rel) and any(j + n == 200 for i, j, n in rel)
    re, qe = origin_of(hsps, chains[1])
    a, c = found[4], found[5]
    assert (int(a["ref_start"]), int(a["query_start"])) == (re, qe) and int(c["ref_start"]) + int(c["len"]) + 1 == re + 200
    assert int(c["ref_start"]) - int(c["query_start"]) == re - qe  # both corners, on one diagonal


def regime_diagonals(res, hsps, chains):
    re, qe = origin_of(hsps, chains[0])
    e = set(diag_index(res[4][0], h, re, qe) for h in res[5])
    assert {0, 63, 64, 127, 128, 198} <= e and res[4]["n_hsps"][0] > 1500
    per = np.bincount([diag_index(res[4][0], h, re, qe) for h in res[5]])
    assert per.max() >= 5  # several segments on one diagonal


def hand_regimes(fill_of, W, hsps):
    """The x-drop, zero and threshold boundaries on the main diagonals of W["hand"]; fill_of(chains, **params) -> a result as the
    model's (the caller holds it against the model)."""
    a, z = [W["hand"][0]], [W["hand"][1]]
    assert on_main(fill_of(a, thresh=100, xdrop=62), hsps, a[0]) == [(0, 3, 138)]  # b - s = 62 = xdrop: the scan goes on
    assert on_main(fill_of(a, thresh=100, xdrop=61), hsps, a[0]) == [(0, 0, 100), (3, 0, 100)]  # xdrop + 1: it ends
    assert on_main(fill_of(z, thresh=200, xdrop=500), hsps, z[0]) == [(0, 4, 500), (9, 1, 200)]  # s = 0 exactly after 5 x 100 - 4 x 125
    assert on_main(fill_of(z, thresh=201, xdrop=500), hsps, z[0]) == [(0, 4, 500)]  # 200 = thresh - 1


def regime_separators(res, t, q, hsps, chains):
    links, found = res[4], res[5]
    for c, axis in ((0, t), (1, q), (2, t), (3, q)):
        re, qe = origin_of(hsps, chains[c])
        lo = re if axis is t else qe
        assert (axis[lo:lo + 120] == 7).sum() == 1
    assert np.all(links["n_hsps"] >= 1)
    for h in found:
        r, s, n = int(h["ref_start"]), int(h["query_start"]), int(h["len"]) + 1
        assert not (t[r:r + n] == 7).any() and not (q[s:s + n] == 7).any()
    assert links["n_hsps"][0] == 2 and links["n_hsps"][1] == 2  # the separator inside the plant cuts it in two


def regime_lengths(res):
    assert np.diff(res[1].astype(np.int64)).tolist()[0] == 1 and res[4].size == 0 + 1 + 64 + 299
    assert (res[4]["n_hsps"] > 0).sum() > 20


def regime_random(res, k):
    links = res[4]
    swept = (links["cells"] > 0)
    assert 100 <= links.size <= 500, links.size
    assert (links["n_fill"] > 0).sum() >= 40 and (swept & (links["n_fill"] == 0)).sum() >= 20 and (~swept).sum() >= 1
    assert (links["n_fill"] > 1).sum() >= 3 and (links["n_hsps"] > links["n_fill"]).sum() >= 3
    if k == 2:
        assert ((links["n_hsps"] > 0) & (links["n_fill"] == 0)).sum() >= 1  # min_fill refuses a link's best chain
