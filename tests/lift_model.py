"""The model of sa_lift_intervals (include/segalign_amd.h), written from the header: the validation clauses, per interval
the clipped blocks of every chain of its group, touch and qualify, the image, the hit order, status and best chain, the hits under both
flags, the clipped block pairs and the counts; then the rendering of the two BED files segalign_host --gpu_lift writes.

Input: the chains as net_class_model takes them (first, block_start, block_end, oblock_start, oblock_end, ogroup / ostrand per chain or
None) with group per chain or None, and the intervals (iv_start, iv_end, iv_group or None).  Output: (records RECORD, hits HIT, blocks
BLOCK or None, stats dict).

It is brute force on purpose: per interval EVERY block of EVERY chain of the group is intersected with the interval (one int64 array
expression over all of them, then plain Python integers), the hull is the least start and the greatest end over ALL clipped other
blocks, and the candidate count is stated on the hulls directly.  No sorted chain list, no binary search and no prefix sum, so that it
shares no method with the device; the only ordering is that of an interval's touching chains by the contract's hit-order key."""
import numpy as np

RECORD = np.dtype([("status", "<u4"), ("n_touch", "<u4"), ("n_qualify", "<u4"), ("first_hit", "<u4"), ("chain", "<u4"), ("ogroup", "<u4"),
                   ("ostart", "<u4"), ("oend", "<u4"), ("mapped", "<u4"), ("first_block", "<u4"), ("n_blocks", "<u4"), ("strand", "u1"),
                   ("pad", "u1", (3,))])
HIT = np.dtype([("interval", "<u4"), ("chain", "<u4"), ("ostart", "<u4"), ("oend", "<u4"), ("mapped", "<u4"), ("first_block", "<u4"),
                ("n_blocks", "<u4"), ("out_block", "<u4")])
BLOCK = np.dtype([("start", "<u4"), ("end", "<u4"), ("ostart", "<u4"), ("oend", "<u4")])
RECORD_FIELDS = [k for k in RECORD.names if k != "pad"]
UNMAPPED, PARTIAL, MAPPED, DUPLICATED = 0, 1, 2, 3
NAMES = ("unmapped", "partial", "mapped", "duplicated")
REASONS = {UNMAPPED: "#Deleted", PARTIAL: "#Partially deleted", DUPLICATED: "#Duplicated"}
COUNTS = ("intervals", "chains", "blocks", "candidates", "touches", "n_status", "hits", "out_blocks")
NONE = 0xFFFFFFFF
LIMIT = 1 << 31


def _per(x, n):
    return [0] * n if x is None else [int(v) for v in x]


def validate(first, block_start, block_end, oblock_start, oblock_end, iv_start, iv_end, group=None, ogroup=None, ostrand=None,
             iv_group=None, min_match=(95, 100), flags=0):
    """The header's validation; ValueError names the clause."""
    first = [int(x) for x in first]
    bs, be = [int(x) for x in block_start], [int(x) for x in block_end]
    obs, obe = [int(x) for x in oblock_start], [int(x) for x in oblock_end]
    n = len(first) - 1
    if not 0 <= int(flags) <= 3:
        raise ValueError("flags")
    num, den = int(min_match[0]), int(min_match[1])
    if not 1 <= den <= 1 << 20:
        raise ValueError("den")
    if not 0 <= num <= den:
        raise ValueError("num")
    if len(iv_start) > 1 << 26:
        raise ValueError("intervals")
    if n > 1 << 22:
        raise ValueError("chains")
    if first[0] != 0 or any(b < a for a, b in zip(first, first[1:])) or first[-1] > 1 << 26:
        raise ValueError("first")
    if not len(bs) == len(be) == len(obs) == len(obe) or len(bs) < first[-1]:
        raise ValueError("block arrays")
    strand = _per(ostrand, n)
    if any(s not in (0, 1) for s in strand):
        raise ValueError("ostrand")
    if any(x is not None and len(x) != n for x in (group, ogroup, ostrand)):
        raise ValueError("per chain")
    for c in range(n):
        for k in range(first[c], first[c + 1]):
            if not bs[k] < be[k] < LIMIT:
                raise ValueError("block")
            if k > first[c] and be[k - 1] > bs[k]:
                raise ValueError("block order")
            if not obs[k] < obe[k] < LIMIT:
                raise ValueError("other block")
            if obe[k] - obs[k] != be[k] - bs[k]:
                raise ValueError("other block length")
            if k > first[c] and (obe[k] > obs[k - 1] if strand[c] else obe[k - 1] > obs[k]):
                raise ValueError("other block order")
    if len(iv_start) != len(iv_end) or (iv_group is not None and len(iv_group) != len(iv_start)):
        raise ValueError("per interval")
    for s, e in zip(iv_start, iv_end):
        if not int(s) < int(e):
            raise ValueError("interval")
        if int(e) >= LIMIT:
            raise ValueError("interval end")


def clip(k, s, e, bs, be, obs, obe, minus):
    """Block k cut to [s, e): -> (start, end, ostart, oend)."""
    dl, dr = max(bs[k], s) - bs[k], be[k] - min(be[k], e)
    return (max(bs[k], s), min(be[k], e)) + ((obs[k] + dr, obe[k] - dl) if minus else (obs[k] + dl, obe[k] - dr))


def lift(first, block_start, block_end, oblock_start, oblock_end, iv_start, iv_end, group=None, ogroup=None, ostrand=None, iv_group=None,
         min_match=(95, 100), multiple=False, blocks=False):
    """sa_lift_intervals.  -> (records, hits, blocks or None, stats)."""
    validate(first, block_start, block_end, oblock_start, oblock_end, iv_start, iv_end, group, ogroup, ostrand, iv_group, min_match,
             (1 if multiple else 0) | (2 if blocks else 0))
    first = [int(x) for x in first]
    n = len(first) - 1
    bs, be = [int(x) for x in block_start], [int(x) for x in block_end]
    obs, obe = [int(x) for x in oblock_start], [int(x) for x in oblock_end]
    grp, ogrp, strand = _per(group, n), _per(ogroup, n), _per(ostrand, n)
    num, den = int(min_match[0]), int(min_match[1])
    ivg = _per(iv_group, len(iv_start))
    # per group: every block of every chain of it (index, chain, start, end), and the hulls, an empty chain counting as (0, 0)
    by_group = {}
    for c in range(n):
        by_group.setdefault(grp[c], []).append(c)
    tab = {}
    for g, chains in by_group.items():
        ks = [k for c in chains for k in range(first[c], first[c + 1])]
        tab[g] = dict(k=np.array(ks, dtype=np.int64), s=np.array([bs[k] for k in ks], dtype=np.int64),
                      e=np.array([be[k] for k in ks], dtype=np.int64),
                      c=np.array([c for c in chains for _ in range(first[c], first[c + 1])], dtype=np.int64),
                      chain=np.array(chains, dtype=np.int64),
                      hs=np.array([bs[first[c]] if first[c + 1] > first[c] else 0 for c in chains], dtype=np.int64),
                      he=np.array([be[first[c + 1] - 1] if first[c + 1] > first[c] else 0 for c in chains], dtype=np.int64))
    rec = np.zeros(len(iv_start), dtype=RECORD)
    hits, out = [], []
    candidates = touches = 0
    for iv in range(len(iv_start)):
        s, e, t = int(iv_start[iv]), int(iv_end[iv]), tab.get(ivg[iv])
        touching = {}  # chain -> [first clipped block, last clipped block, mapped]
        if t is not None:
            ov = np.minimum(t["e"], e) - np.maximum(t["s"], s)
            for j in np.flatnonzero(ov > 0):
                x = touching.setdefault(int(t["c"][j]), [int(t["k"][j]), 0, 0])
                x[1] = int(t["k"][j])
                x[2] += int(ov[j])
            # what the device tests: in hit order from the first chain whose hull ends after s to the last whose hull starts before e
            m = t["hs"] < e
            f = m & (t["he"] > s)
            if f.any():
                h0 = int(t["hs"][f].min())
                c0 = int(t["chain"][f & (t["hs"] == h0)].min())
                candidates += int((m & ((t["hs"] > h0) | ((t["hs"] == h0) & (t["chain"] >= c0)))).sum())
        order = sorted(touching, key=lambda c: (bs[first[c]], c))
        images = {}
        for c in order:
            i, j, mapped = touching[c]
            cl = [clip(k, s, e, bs, be, obs, obe, strand[c]) for k in range(i, j + 1)]
            assert all(x[0] < x[1] for x in cl)  # the blocks between two clipped blocks are clipped blocks
            images[c] = (min(x[2] for x in cl), max(x[3] for x in cl), mapped, i, j - i + 1, cl)
        qual = [c for c in order if images[c][2] * den >= num * (e - s)]
        touches += len(order)
        status = UNMAPPED if not order else PARTIAL if not qual else MAPPED if len(qual) == 1 else DUPLICATED
        r = rec[iv]
        r["status"], r["n_touch"], r["n_qualify"], r["first_hit"], r["chain"] = status, len(order), len(qual), len(hits), NONE
        if order:
            best = max(order, key=lambda c: images[c][2])  # max returns the first of equal ones: the first in hit order
            im = images[best]
            r["chain"], r["ogroup"], r["ostart"], r["oend"], r["mapped"], r["first_block"], r["n_blocks"], r["strand"] = (
                best, ogrp[best], im[0], im[1], im[2], im[3], im[4], strand[best])
        for c in (qual if multiple else qual if status == MAPPED else []):
            im = images[c]
            hits.append((iv, c, im[0], im[1], im[2], im[3], im[4], len(out) if blocks else 0))
            if blocks:
                out += im[5]
    st = dict(intervals=len(iv_start), chains=n, blocks=first[-1], candidates=candidates, touches=touches,
              n_status=[int((rec["status"] == k).sum()) for k in range(4)], hits=len(hits), out_blocks=len(out))
    return rec, np.array(hits, dtype=HIT), (np.array(out, dtype=BLOCK) if blocks else None), st


def same(got, want):
    """Every field of every record, hit and block of (records, hits, blocks, ...) tuples."""
    assert got[0].size == want[0].size, (got[0].size, want[0].size)
    for k in RECORD_FIELDS:
        assert np.array_equal(got[0][k], want[0][k]), ("record", k, np.flatnonzero(got[0][k] != want[0][k])[:8], got[0][k][:8], want[0][k][:8])
    assert (got[0]["pad"] == 0).all()
    assert got[1].size == want[1].size, ("hits", got[1].size, want[1].size)
    for k in HIT.names:
        assert np.array_equal(got[1][k], want[1][k]), ("hit", k, np.flatnonzero(got[1][k] != want[1][k])[:8], got[1][k][:8], want[1][k][:8])
    assert (got[2] is None) == (want[2] is None)
    if want[2] is not None:
        assert got[2].size == want[2].size, ("blocks", got[2].size, want[2].size)
        for k in BLOCK.names:
            assert np.array_equal(got[2][k], want[2][k]), ("block", k, np.flatnonzero(got[2][k] != want[2][k])[:8])


def same_stats(got, want):
    for k in COUNTS:
        assert (list(got[k]) if k == "n_status" else int(got[k])) == want[k], (k, got[k], want[k])


# ---- the host's files ----
def parse_bed(text):
    """The lines of a BED file the host reads: -> [(line, name, start, end, rest)]; rest is what follows the third field, its tab
    included.  Empty lines and lines that start with # are skipped."""
    out = []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        f = line.split("\t", 3)
        out.append((line, f[0], int(f[1]), int(f[2]), "\t" + f[3] if len(f) > 3 else ""))
    return out


def render_bed(lines, records, names, starts, strand):
    """The two files of one .net.chains file.  lines: the parsed BED lines lifted through it, in input order; records: theirs;
    names[ogroup], starts[ogroup]: name of a query record and where it starts in the coordinates the chains were given in; strand: '+'
    or '-'.  -> (lifted text, unlifted text)."""
    lifted, unlifted = [], []
    for (line, _, _, _, rest), r in zip(lines, records):
        if int(r["status"]) == MAPPED:
            q = int(r["ogroup"])
            lifted.append("%s\t%d\t%d%s\t%s\n" % (names[q], int(r["ostart"]) - starts[q], int(r["oend"]) - starts[q], rest, strand))
        else:
            unlifted.append("%s\n%s\n" % (REASONS[int(r["status"])], line))
    return "".join(lifted), "".join(unlifted)
