"""Continuation pieces of the gapped stage (option gapped_pieces; include/segalign_amd.h) in plain Python over the
serial one-sided extension with traceback of tests/cpp/gapped_trace_check.c, which takes any origin: a side that ends at max_extent is
continued from its best cell by a fresh extension, piece after piece, and the pieces are joined into one record and one path.

Also here: the greedy rule of gapped_greedy_model with cover sets taken over the pieces, the .gapped / .maf text of the host, and the
deterministic inputs the CPU and GPU tests of the feature share (a small block pair, anchors found on the CPU, parameter sets)."""
import numpy as np

import gapped_greedy_model as GR
import gapped_model as G
import gapped_trace_model as T

EXTENT_CAP, BAND_CAP, CONTINUED = 1, 2, 4
SCORE_LIMIT = 1 << 29
# why a chain ended
STOP_ONE = "one piece"      # piece 0 did not ask for more (or P = 1)
STOP_P = "P reached"        # the last piece ended at max_extent, but it was piece P - 1
STOP_BAND = "band cap"      # a later piece ended at the band cap
STOP_STUCK = "no progress"  # a later piece ended at max_extent with its best cell at its origin
STOP_SCORE = "score limit"
STOP_END = "end"            # a later piece did not reach max_extent: a separator, the block's end or the y-drop


def side_chain(t, q, sub, ar, aq, direction, pieces=1, **kw):
    """One side under gapped_pieces = pieces.  -> (joined (best, i, j, cells, flags), [piece dicts], stop reason).  A piece dict holds
    its origin, its own result, its ops in walk order and its walk counts."""
    chain = []
    o_r, o_q = int(ar), int(aq)
    total = 0
    while True:
        res, ops, walk = T.side(t, q, sub, o_r, o_q, direction, **kw)
        best, bi, bj, cells, flags = res
        chain.append({"origin": (o_r, o_q), "res": res, "ops": ops, "walk": walk})
        total += best
        k = len(chain) - 1
        if flags & BAND_CAP:
            stop = STOP_BAND if k else STOP_ONE
        elif not (flags & EXTENT_CAP):
            stop = STOP_END if k else STOP_ONE
        elif (bi, bj) == (0, 0):
            stop = STOP_STUCK if k else STOP_ONE
        elif k + 1 >= pieces:
            stop = STOP_P if pieces > 1 else STOP_ONE
        elif total >= SCORE_LIMIT:
            stop = STOP_SCORE
        else:
            o_r += direction * bi
            o_q += direction * bj
            continue
        break
    last = chain[-1]["res"]
    joined = (sum(p["res"][0] for p in chain), sum(p["res"][1] for p in chain), sum(p["res"][2] for p in chain),
              min(sum(p["res"][3] for p in chain), 0xffffffff), last[4] | (CONTINUED if len(chain) > 1 else 0))
    return joined, chain, stop


def side_ops(chain, direction):
    """A side's ops in genome order: left side the last piece first, each in walk order; right side piece 0 first, each reversed.
    Runs are not merged where two pieces meet."""
    parts = [p["ops"] for p in reversed(chain)] if direction < 0 else [p["ops"][::-1] for p in chain]
    parts = [x for x in parts if x.size]
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)


def align(t, q, sub, hsps, pieces=1, gap_open=400, gap_extend=30, ydrop=9430, max_extent=0, max_band=0):
    """Raw records and per-record (left ops, right ops in genome order, counts) as gapped_trace_model.align gives them, under
    gapped_pieces = pieces; and per record the two sides' (joined, chain, stop)."""
    kw = dict(gap_open=gap_open, gap_extend=gap_extend, ydrop=ydrop, max_extent=max_extent or G.DEFAULT_EXTENT,
              max_band=max_band or G.DEFAULT_BAND)
    h = np.ascontiguousarray(hsps, dtype=G.SEG_DTYPE)
    recs = np.zeros(h.size, dtype=G.GAPPED_DTYPE)
    paths, sides = [], []
    for k, (rs, qs, ln, _) in enumerate(h.tolist()):
        ar, aq = rs + ln // 2, qs + ln // 2
        L = side_chain(t, q, sub, ar, aq, -1, pieces, **kw)
        R = side_chain(t, q, sub, ar, aq, +1, pieces, **kw)
        (lb, li, lj, lc, lf), (rb, ri, rj, rc, rf) = L[0], R[0]
        recs[k] = (ar - li, ar + ri, aq - lj, aq + rj, lb + rb, k, lf | rf, (lc + rc) & 0xffffffff)
        counts = {c: sum(p["walk"][c] for p in L[1] + R[1]) for c in ("matches", "mismatches", "gap_opens", "gap_bases")}
        paths.append((side_ops(L[1], -1), side_ops(R[1], +1), counts))
        sides.append((L, R))
    return recs, paths, sides


def cover_set_pieces(sides, a):
    """The cover set of one alignment stated over its pieces: the M pairs of every piece, each placed from that piece's own origin and
    best cell, plus the anchor point a."""
    pts = {a}
    for (_, chain, _), direction in zip(sides, (-1, +1)):
        for p in chain:
            (o_r, o_q), (_, bi, bj, _, _) = p["origin"], p["res"]
            # walk order runs from the piece's best cell to its origin
            i, j = o_r + direction * bi, o_q + direction * bj
            for x in p["ops"].tolist():
                ln, op = x >> 2, x & 3
                step = -direction  # towards the origin
                if op == T.OP_M:
                    for _ in range(ln):
                        # the pair consumed by a step: on the right side the base before the cell, on the left side the base at it
                        pts.add((i - 1, j - 1) if direction > 0 else (i, j))
                        i += step
                        j += step
                elif op == T.OP_I:
                    j += step * ln
                else:
                    i += step * ln
            assert (i, j) == (o_r, o_q)
    return pts


def greedy(t, q, sub, hsps, gappedthresh, pieces=1, **kw):
    """gapped_greedy_model.greedy over the joined records and paths: its cover_set walks a record's ops from (ref_start, query_start),
    which for joined sides is the M pairs of all pieces (test_gapped_pieces_checker holds it against cover_set_pieces)."""
    recs, paths, _ = align(t, q, sub, hsps, pieces, **kw)
    return GR.greedy(hsps, recs, paths, gappedthresh)


# ---- the host's files -------------------------------------------------------------------------------------------------------------

def encode(ascii_codes):
    """Plain codes of an unmasked A C G T block with '&' separators, as the engine holds them."""
    lut = np.full(256, 5, dtype=np.uint8)
    for k, c in enumerate(b"ACGT"):
        lut[c] = k
    lut[ord("&")] = 7
    return lut[np.ascontiguousarray(ascii_codes, dtype=np.uint8)]


def rc_codes(codes):
    out = codes[::-1].copy()
    m = out < 4
    out[m] = 3 - out[m]
    return out


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------

def block_pair():
    """Target: three records of 24, 40 and 56 kbp.  Queries 0 and 1: diverged copies (substitutions and indels) of the records, the
    middle record reverse-complemented in query 0 and the last one in query 1, so both strands carry long homologies; the second half
    of record 0 is unrelated sequence and record 2 has lost 150 bases in one place."""
    from segalign_amd import synth
    t_recs = [synth.random_dna(n, 900 + k) for k, n in enumerate((24_000, 40_000, 56_000))]
    qs = []
    for b, (rate, every, flip) in enumerate(((0.04, 300, 1), (0.07, 700, 2))):
        recs = [synth.mutate(r, 950 + 10 * b + k, rate, every) for k, r in enumerate(t_recs)]
        cut = recs[2].size * 3 // 5  # a 150-base deletion in record 2: a gap the band has to span
        recs[2] = np.concatenate([recs[2][:cut], recs[2][cut + 150:]])
        half = recs[0].size // 2  # record 0's homology ends in mid-record: unrelated sequence follows
        recs[0] = np.concatenate([recs[0][:half], synth.random_dna(recs[0].size - half, 990 + b)])
        recs[flip] = synth.reverse_complement(recs[flip])
        qs.append(synth.join_records(recs))
    return synth.join_records(t_recs), qs


def find_anchors(tc, qc, count, k=24, seed=1):
    """HSPs (SEG_DTYPE) at exact k-mer matches of two code arrays that are unique in both, `count` of them spread over the matches, with
    scores that shuffle the priority order."""
    def keys(c):
        ok = np.convolve((c < 4).astype(np.int64), np.ones(k, dtype=np.int64), "valid") == k
        key = np.zeros(c.size - k + 1, dtype=np.uint64)
        for x in range(k):
            key = key * np.uint64(4) + (c[x:x + key.size] & 3).astype(np.uint64)
        return key, ok
    kt, okt = keys(tc)
    kq, okq = keys(qc)
    ut, it, ct = np.unique(kt[okt], return_index=True, return_counts=True)
    uq, iq, cq = np.unique(kq[okq], return_index=True, return_counts=True)
    pt, pq = np.flatnonzero(okt)[it[ct == 1]], np.flatnonzero(okq)[iq[cq == 1]]
    _, xt, xq = np.intersect1d(ut[ct == 1], uq[cq == 1], return_indices=True)
    rp, qp = pt[xt], pq[xq]
    o = np.argsort(qp)
    rp, qp = rp[o], qp[o]
    pick = np.linspace(0, rp.size - 1, min(count, rp.size)).astype(np.int64)
    rng = np.random.default_rng(seed)
    h = np.zeros(pick.size, dtype=G.SEG_DTYPE)
    h["ref_start"], h["query_start"], h["len"] = rp[pick], qp[pick], k - 1
    h["score"] = rng.integers(3000, 9000, size=pick.size)
    return h


KEYS = [(0, False), (0, True), (1, False), (1, True)]
# parameter sets of the tests: chains of 2 to more than 10 pieces that end at P, at separators and at the block's ends; short pieces
# that run dry where a homology ends; a band that piece 0 fits and a later piece overflows
CHAIN = dict(max_extent=2000)
DRY = dict(max_extent=100)
BAND = dict(max_extent=1500, max_band=150, gap_extend=40)


def inputs(per_key=14):
    """-> (target ascii, [query ascii], target codes, {key: query strand codes}, {key: HSPs})."""
    t, qs = block_pair()
    tc = encode(t)
    codes, hsps = {}, {}
    for buf, rev in KEYS:
        qc = encode(qs[buf])
        codes[(buf, rev)] = rc_codes(qc) if rev else qc
        hsps[(buf, rev)] = find_anchors(tc, codes[(buf, rev)], per_key, seed=7 + 2 * buf + int(rev))
    return t, qs, tc, codes, hsps


def stop_reasons(sides):
    """{stop reason: count} and the longest chain over the sides of align()'s third result."""
    seen, longest = {}, 0
    for pair in sides:
        for _, chain, stop in pair:
            seen[stop] = seen.get(stop, 0) + 1
            longest = max(longest, len(chain))
    return seen, longest


def end_kind(t, q, rec, side):
    """What lies just beyond a record's far end on `side` (-1 left, +1 right): "separator", "block end" or "base"."""
    pt = int(rec["ref_end"]) if side > 0 else int(rec["ref_start"]) - 1
    pq = int(rec["query_end"]) if side > 0 else int(rec["query_start"]) - 1
    if pt < 0 or pt >= t.size or pq < 0 or pq >= q.size:
        return "block end"
    return "separator" if t[pt] == 7 or q[pq] == 7 else "base"
