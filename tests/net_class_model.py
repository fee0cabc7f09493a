"""The model of sa_net_classify (include/segalign_amd.h), written from the header in plain Python integers: the validation
clauses, the clipped other blocks, the hulls, the classes, the duplication by a per-base count, the filter with its subtree drop; then
net_select, a twin of net_other_blocks and the rendering of the file segalign_host --gpu_net_class writes.

Input: the CSR blocks of the netted axis (first, block_start, block_end), the same blocks on the other axis, the fills of net_model.net
on those blocks, ogroup / ostrand per chain or None, a filter dict or None.  Output: (classes CLASS, stats dict).

The duplication is brute force on purpose: one counter per covered base of an ogroup, no sort and no prefix sum, so that it
shares no method with the device.  sweep_dup() is the second way, the sorted-event sweep the device runs, stated on the host."""
import numpy as np

import net_model as NM

CLASS = np.dtype([("ostart", "<u4"), ("oend", "<u4"), ("oover", "<u4"), ("ofar", "<u4"), ("odup", "<u4"), ("ogroup", "<u4"),
                  ("type", "u1"), ("strand", "u1"), ("keep", "u1"), ("pad", "u1"), ("pad2", "<u4")])
FIELDS = ["ostart", "oend", "oover", "ofar", "odup", "ogroup", "type", "strand", "keep"]
TOP, SYN, INV, NONSYN = 0, 1, 2, 3
NAMES = ("top", "syn", "inv", "nonSyn")
THRESHOLDS = ("min_score", "min_top_score", "min_size", "min_ali", "max_far")
COUNTS = ("fills", "blocks", "events", "ogroups", "n_type", "kept", "dup_bases")
LIMIT = 1 << 31


def _per_chain(x, n):
    return [0] * n if x is None else [int(v) for v in x]


def validate(first, block_start, block_end, oblock_start, oblock_end, fills, ogroup=None, ostrand=None, filter=None):
    """The header's validation; ValueError names the clause."""
    first = [int(x) for x in first]
    bs, be = [int(x) for x in block_start], [int(x) for x in block_end]
    obs, obe = [int(x) for x in oblock_start], [int(x) for x in oblock_end]
    n = len(first) - 1
    if filter is not None:
        if set(filter) - set(THRESHOLDS):
            raise ValueError("filter names")
        if any(not 0 <= int(filter.get(k, 0)) <= LIMIT for k in ("min_size", "min_ali", "max_far")):
            raise ValueError("parameter")
        if any(not -(1 << 63) <= int(filter.get(k, 0)) < (1 << 63) for k in ("min_score", "min_top_score")):
            raise ValueError("parameter")
    if n > 1 << 22:
        raise ValueError("chains")
    if first[0] != 0 or any(b < a for a, b in zip(first, first[1:])) or first[-1] > 1 << 26:
        raise ValueError("first")
    if not len(bs) == len(be) == len(obs) == len(obe) or len(bs) < first[-1]:
        raise ValueError("block arrays")
    strand = _per_chain(ostrand, n)
    if any(s not in (0, 1) for s in strand):
        raise ValueError("ostrand")
    if ogroup is not None and len(ogroup) != n or ostrand is not None and len(ostrand) != n:
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
    if len(fills) >= LIMIT:
        raise ValueError("fills")
    total = 0
    for k, f in enumerate(fills):
        if int(f["start"]) >= int(f["end"]):
            raise ValueError("fill extent")
        c, fb, nb = int(f["chain"]), int(f["first_block"]), int(f["n_blocks"])
        if c >= n:
            raise ValueError("fill chain")
        if nb < 1 or fb < first[c] or fb + nb > first[c + 1]:
            raise ValueError("fill blocks")
        if be[fb] <= int(f["start"]) or bs[fb + nb - 1] >= int(f["end"]):
            raise ValueError("fill edge blocks")
        total += nb
        if total > 1 << 26:
            raise ValueError("clipped blocks")
        p = int(f["parent"])
        if p == -1:
            if int(f["depth"]) != 0:
                raise ValueError("fill depth")
            continue
        if p < 0 or p >= k:
            raise ValueError("fill parent")
        if int(f["depth"]) != int(fills[p]["depth"]) + 1:
            raise ValueError("fill depth")


PAGE = 1 << 12


def _pages(s, e):
    """[s, e) as (page, from, to) pieces of PAGE bases."""
    return [(p, max(s, p * PAGE) - p * PAGE, min(e, (p + 1) * PAGE) - p * PAGE) for p in range(s // PAGE, (e - 1) // PAGE + 1)]


def clipped_other(f, bs, be, obs, obe, strand):
    """[(ostart, oend)] of a fill's clipped other blocks, in block order."""
    out = []
    for k in range(int(f["first_block"]), int(f["first_block"]) + int(f["n_blocks"])):
        dl = max(int(bs[k]), int(f["start"])) - int(bs[k])
        dr = int(be[k]) - min(int(be[k]), int(f["end"]))
        out.append((int(obs[k]) + dr, int(obe[k]) - dl) if strand else (int(obs[k]) + dl, int(obe[k]) - dr))
    return out


def classify(first, block_start, block_end, oblock_start, oblock_end, fills, ogroup=None, ostrand=None, filter=None):
    """sa_net_classify.  -> (classes, stats)."""
    validate(first, block_start, block_end, oblock_start, oblock_end, fills, ogroup, ostrand, filter)
    n = len(first) - 1
    group, strand = _per_chain(ogroup, n), _per_chain(ostrand, n)
    cl = [clipped_other(f, block_start, block_end, oblock_start, oblock_end, strand[int(f["chain"])]) for f in fills]
    # duplication: one counter per base that any clipped other block covers, kept in pages so that far-apart blocks cost no memory
    depth = {}
    for f, blocks in zip(fills, cl):
        g = group[int(f["chain"])]
        for s, e in blocks:
            for page, a, b in _pages(s, e):
                depth.setdefault((g, page), np.zeros(PAGE, dtype=np.int32))[a:b] += 1
    out = np.zeros(len(fills), dtype=CLASS)
    P = {k: int((filter or {}).get(k, 0)) for k in THRESHOLDS}
    for k, (f, blocks) in enumerate(zip(fills, cl)):
        c = int(f["chain"])
        g = group[c]
        os_, oe = min(s for s, _ in blocks), max(e for _, e in blocks)
        typ, over, far = TOP, 0, 0
        p = int(f["parent"])
        if p >= 0:
            pc = int(fills[p]["chain"])
            if group[pc] != g:
                typ = NONSYN
            else:
                x = min(oe, int(out[p]["oend"])) - max(os_, int(out[p]["ostart"]))
                over, far = (x, 0) if x > 0 else (0, -x)
                typ = SYN if strand[pc] == strand[c] else INV
        odup = sum(int((depth[g, page][a:b] >= 2).sum()) for s, e in blocks for page, a, b in _pages(s, e))
        ok = True
        if filter is not None:
            ok = int(f["score"]) >= P["min_score"] and int(f["end"]) - int(f["start"]) >= P["min_size"] and int(f["ali"]) >= P["min_ali"]
            ok = ok and (int(f["score"]) >= P["min_top_score"] if typ == TOP else False if typ == NONSYN else far <= P["max_far"])
        keep = ok and (p < 0 or bool(out[p]["keep"]))
        out[k] = (os_, oe, over, far, odup, g, typ, strand[c], int(keep), 0, 0)
    st = dict(fills=len(fills), blocks=sum(len(b) for b in cl), events=2 * sum(len(b) for b in cl),
              ogroups=len({group[int(f["chain"])] for f in fills}), n_type=[int((out["type"] == t).sum()) for t in range(4)],
              kept=int(out["keep"].sum()), dup_bases=int(out["odup"].astype(np.int64).sum()))
    return out, st


def sweep_dup(first, block_start, block_end, oblock_start, oblock_end, fills, ogroup=None, ostrand=None):
    """The second way: per ogroup, sum over its bases of depth >= 2 of their depth, from one sweep over the sorted events (an end before
    a start at one coordinate).  -> {ogroup: bases weighted by depth}, which the odup of the group's fills must sum to."""
    n = len(first) - 1
    group, strand = _per_chain(ogroup, n), _per_chain(ostrand, n)
    events = []
    for f in fills:
        c = int(f["chain"])
        for s, e in clipped_other(f, block_start, block_end, oblock_start, oblock_end, strand[c]):
            events += [(group[c], s, 1), (group[c], e, 0)]
    events.sort()
    out, depth = {}, 0
    for i, (g, x, is_start) in enumerate(events):
        depth += 1 if is_start else -1
        out.setdefault(g, 0)
        if i + 1 < len(events) and events[i + 1][0] == g and depth >= 2:
            out[g] += depth * (events[i + 1][1] - x)
    assert depth == 0
    return out


def select(fills, keep):
    """net_select: the kept fills in order, parent remapped.  -> (fills', index)."""
    index = [k for k in range(len(fills)) if keep[k]]
    new = {old: k for k, old in enumerate(index)}
    out = np.array([fills[k] for k in index], dtype=NM.FILL_DTYPE)
    for k in range(out.size):
        if out[k]["parent"] >= 0:
            out[k]["parent"] = new[int(out[k]["parent"])]  # KeyError: keep is not closed under subtrees
    return out, np.array(index, dtype=np.uint32)


def other_blocks(hsps, members, first, axis="target", strand=None, size=None):
    """The twin of engine.net_other_blocks: every member's block on the other axis, flipped to size - coordinate for a strand-1 chain."""
    key = "query_start" if axis == "target" else "ref_start"
    first = [int(x) for x in first]
    s_out, e_out = [], []
    for c in range(len(first) - 1):
        for k in range(first[c], first[c + 1]):
            h = hsps[int(members[k])]
            s, e = int(h[key]), int(h[key]) + int(h["len"]) + 1
            if strand is not None and int(strand[c]):
                s, e = int(size[c]) - e, int(size[c]) - s
            s_out.append(s)
            e_out.append(e)
    return np.array(s_out, dtype=np.uint32), np.array(e_out, dtype=np.uint32)


def same(got, want):
    """Every field of every record."""
    assert got.size == want.size, (got.size, want.size)
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8], got[k][:8], want[k][:8])
    assert (got["pad"] == 0).all() and (got["pad2"] == 0).all()


def same_stats(got, want):
    for k in COUNTS:
        assert (list(got[k]) if k == "n_type" else int(got[k])) == want[k], (k, got[k], want[k])


def keep_closed(fills, classes):
    """keep is closed under subtrees: a kept fill's parent is kept."""
    return all(int(f["parent"]) < 0 or classes[int(f["parent"])]["keep"] for f, c in zip(fills, classes) if c["keep"])


# ---- the host's file ----
def render_class(net_text, classes, kept_only=False):
    """The .net.class file from the .net file's text: ` type=T qover=N qfar=N qdup=N` appended to every fill line, the k-th fill line
    taking record k.  kept_only (--gpu_net_syn): the lines of the dropped fills are left out, and a `net` line with no kept fill too."""
    out, k, pending = [], 0, None
    for line in net_text.splitlines():
        if line.startswith("net "):
            pending = line
            if not kept_only:
                out.append(line)
            continue
        c = classes[k]
        k += 1
        if kept_only and not c["keep"]:
            continue
        if kept_only and pending is not None:
            out.append(pending)
            pending = None
        out.append("%s type=%s qover=%d qfar=%d qdup=%d" % (line, NAMES[int(c["type"])], int(c["oover"]), int(c["ofar"]), int(c["odup"])))
    assert k == len(classes)
    return "".join(x + "\n" for x in out)
