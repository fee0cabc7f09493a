"""The model of sa_net_subset (include/segalign_amd.h), written from the header in plain Python integers: the validation
clauses, the clipped members, their scores, the runs and the sub-chain records; then the rendering of the two files segalign_host
--gpu_net_subset writes.

Input: the target codes t and the codes q of the query strand, the 64-entry matrix, HSPs (SEG), chains in CSR form (members, first), the
fills of net_model.net on net_blocks(hsps, members, first, axis).  Output: (out_hsps SEG, chains CHAIN, stats dict)."""
import bisect

import numpy as np

import hsp_chain_gap_model as GM

SEG = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])
CHAIN = np.dtype([("fill", "<u4"), ("chain", "<u4"), ("group", "<u4"), ("run", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"),
                  ("ref_start", "<u4"), ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"), ("score", "<i8"),
                  ("clipped", "<u4"), ("pad", "<u4")])
COUNTS = ("fills", "runs", "members", "cut_members", "bases_rescored", "splits")
MAX_PEN = 1 << 20
CODE = np.full(256, 6, dtype=np.uint8)  # the engine's plain codes: A C G T, soft-masked, N, other, separator
for _k, _c in enumerate(b"ACGT"):
    CODE[_c] = _k
CODE[list(b"acgt")] = 4
CODE[list(b"nN")] = 5
CODE[ord("&")] = 7


def encode(text):
    """ASCII bases -> plain codes."""
    return CODE[np.frombuffer(bytes(text), dtype=np.uint8)] if isinstance(text, (bytes, bytearray)) else CODE[np.asarray(text, dtype=np.uint8)]


def blocks(hsps, members, axis):
    """The block of every member on the axis: -> (start list, end list)."""
    key = "ref_start" if axis == "target" else "query_start"
    bs = [int(hsps[key][int(i)]) for i in members]
    return bs, [s + int(hsps["len"][int(i)]) + 1 for s, i in zip(bs, members)]


def clipped(f, bs, be):
    """[(start, end)] of a fill's clipped blocks."""
    k0 = int(f["first_block"])
    return [(max(bs[k], int(f["start"])), min(be[k], int(f["end"]))) for k in range(k0, k0 + int(f["n_blocks"]))]


def gap_of(child, cl):
    """The k with end_k <= child.start and child.end <= start_k+1 among the parent's clipped blocks cl, or None."""
    k = bisect.bisect_right([e for _, e in cl[:-1]], int(child["start"])) - 1  # the ends ascend: the last one at or before the start
    return k if k >= 0 and int(child["end"]) <= cl[k + 1][0] else None


def validate(t, q, hsps, members, first, fills, axis="target", diag_pen=0, anti_pen=0, gap_costs=None):
    """The header's validation; ValueError names the clause."""
    h = np.asarray(hsps, dtype=SEG)
    first = [int(x) for x in first]
    n_chains = len(first) - 1
    if axis not in ("target", "query"):
        raise ValueError("axis")
    if not (0 <= diag_pen <= MAX_PEN and 0 <= anti_pen <= MAX_PEN):
        raise ValueError("penalty")
    if gap_costs is not None:
        GM.validate(gap_costs)
    if first[0] != 0 or any(b < a for a, b in zip(first, first[1:])) or first[-1] != len(members) or first[-1] > 1 << 22:
        raise ValueError("first")
    for i in members:
        if int(i) >= h.size:
            raise ValueError("member index")
        x = h[int(i)]
        if int(x["ref_start"]) + int(x["len"]) + 1 > len(t) or int(x["query_start"]) + int(x["len"]) + 1 > len(q):
            raise ValueError("member outside the block")
    for c in range(n_chains):
        for k in range(first[c], first[c + 1] - 1):
            x, y = h[int(members[k])], h[int(members[k + 1])]
            n = int(x["len"]) + 1
            if int(x["ref_start"]) + n > int(y["ref_start"]) or int(x["query_start"]) + n > int(y["query_start"]):
                raise ValueError("collinear")
    bs, be = blocks(h, members, axis)
    total, cl_of = 0, {}
    for k, f in enumerate(fills):
        if int(f["start"]) >= int(f["end"]):
            raise ValueError("fill extent")
        c, fb, nb = int(f["chain"]), int(f["first_block"]), int(f["n_blocks"])
        if c >= n_chains:
            raise ValueError("fill chain")
        if nb < 1 or fb < first[c] or fb + nb > first[c + 1]:
            raise ValueError("fill blocks")
        if be[fb] <= int(f["start"]) or bs[fb + nb - 1] >= int(f["end"]):
            raise ValueError("fill edge blocks")
        total += nb
        if total > 1 << 26:
            raise ValueError("output members")
        p = int(f["parent"])
        if p == -1:
            continue
        if p < 0 or p >= k:
            raise ValueError("fill parent")
        if p not in cl_of:
            cl_of[p] = clipped(fills[p], bs, be)
        if gap_of(f, cl_of[p]) is None:
            raise ValueError("fill gap")


def penalty(x, y, diag_pen, anti_pen, table):
    """pen'(x, y) of two SEG records, x before y."""
    n = int(x["len"]) + 1
    rs_j, qs_j, rs_i, qs_i = int(x["ref_start"]), int(x["query_start"]), int(y["ref_start"]), int(y["query_start"])
    re_j, qe_j = rs_j + n, qs_j + n
    pen = diag_pen * abs((rs_i - qs_i) - (rs_j - qs_j)) + anti_pen * ((rs_i + qs_i) - (re_j + qe_j))
    if table is not None:
        pen += GM.gapcost(table, rs_i - re_j, qs_i - qe_j)
    return pen


def subset(t, q, sub, hsps, members, first, fills, axis="target", split=True, diag_pen=0, anti_pen=0, gap_costs=None):
    """sa_net_subset.  -> (out_hsps, chains, stats)."""
    validate(t, q, hsps, members, first, fills, axis, diag_pen, anti_pen, gap_costs)
    t, q = np.asarray(t, dtype=np.uint8), np.asarray(q, dtype=np.uint8)
    sub = np.asarray(sub, dtype=np.int64).reshape(64)
    h = np.asarray(hsps, dtype=SEG)
    table = None if gap_costs is None else GM.table(gap_costs)
    bs, be = blocks(h, members, axis)
    children = {}
    for k, f in enumerate(fills):
        if int(f["parent"]) >= 0:
            children.setdefault(int(f["parent"]), []).append(k)
    out, exact, recs = [], [], []
    st = dict.fromkeys(COUNTS, 0)
    for k, f in enumerate(fills):
        fb, nb = int(f["first_block"]), int(f["n_blocks"])
        cl = clipped(f, bs, be)
        ends = [e for _, e in cl[:-1]]
        cuts = {bisect.bisect_right(ends, int(fills[c]["start"])) - 1 for c in children.get(k, [])} if split else set()  # validate(): in a gap
        assert all(0 <= j < nb - 1 for j in cuts)
        base = len(out)
        sides = []
        for j, (s, e) in enumerate(cl):
            x = h[int(members[fb + j])]
            d = s - bs[fb + j]
            rs, qs, n = int(x["ref_start"]) + d, int(x["query_start"]) + d, e - s
            side = (1 if bs[fb + j] < s else 0) | (2 if be[fb + j] > e else 0)
            assert n >= 1 and (side == 0 or j in (0, nb - 1))
            score = int(x["score"])
            if side:
                score = int(sub[t[rs:rs + n].astype(np.int64) * 8 + q[qs:qs + n].astype(np.int64)].sum())
                st["cut_members"] += 1
                st["bases_rescored"] += n
            out.append((rs, qs, n - 1, max(-(1 << 31), min((1 << 31) - 1, score))))
            exact.append(score)
            sides.append(side)
        heads = [0] + [j + 1 for j in sorted(cuts)] + [nb]
        for r, (a, b) in enumerate(zip(heads, heads[1:])):
            mem = [np.array(out[base + j], dtype=SEG) for j in range(a, b)]
            score = sum(exact[base + a:base + b]) - sum(penalty(x, y, diag_pen, anti_pen, table) for x, y in zip(mem, mem[1:]))
            x, y = out[base + a], out[base + b - 1]
            recs.append((k, int(f["chain"]), int(f["group"]), r, base + a, b - a, x[0], y[0] + y[2] + 1, x[1], y[1] + y[2] + 1, score,
                         (sides[a] & 1) | (sides[b - 1] & 2), 0))
        st["splits"] += len(cuts)
    st.update(fills=len(fills), runs=len(recs), members=len(out))
    return np.array(out, dtype=SEG), np.array(recs, dtype=CHAIN), st


def csr(chains):
    """The sub-chains as a CSR over out_hsps: -> (members 0 .. m - 1, first)."""
    m = int(chains["first_member"][-1]) + int(chains["n_members"][-1]) if chains.size else 0
    return np.arange(m, dtype=np.uint32), np.concatenate([chains["first_member"], [m]]).astype(np.uint32)


def same(got_hsps, got_chains, want_hsps, want_chains):
    """Every field of every output HSP and sub-chain."""
    assert got_hsps.size == want_hsps.size and got_chains.size == want_chains.size, (got_hsps.size, want_hsps.size, got_chains.size, want_chains.size)
    for k in SEG.names:
        assert np.array_equal(got_hsps[k], want_hsps[k]), (k, np.flatnonzero(got_hsps[k] != want_hsps[k])[:8])
    for k in CHAIN.names:
        assert np.array_equal(got_chains[k], want_chains[k]), (k, np.flatnonzero(got_chains[k] != want_chains[k])[:8])


def hulls_disjoint(chains, axis="target"):
    """Consequence (a): the hulls of all sub-chains of a group are pairwise disjoint on the axis."""
    s, e = ("ref_start", "ref_end") if axis == "target" else ("query_start", "query_end")
    for g in np.unique(chains["group"]):
        mine = chains[chains["group"] == g]
        order = np.argsort(mine[s], kind="stable")
        if np.any(mine[e][order][:-1].astype(np.int64) > mine[s][order][1:].astype(np.int64)):
            return False
    return True


# ---- the host's files ----
SEG_LINE = "%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\n"


def _where(starts, x):
    return bisect.bisect_right(starts, x) - 1


def render_chains(out_hsps, chains, rev, t_names, t_starts, q_names, q_starts):
    """The .net.chains file: per sub-chain `#chain k fill=F run=R score=S tname tstart tend qname qstart qend strand` (1-based starts
    within the record, as the .segments lines), then its members as .segments lines.  Coordinates in: block coordinates."""
    lines, strand = [], "-" if rev else "+"
    for k, c in enumerate(chains):
        r0, r1, q0, q1 = int(c["ref_start"]), int(c["ref_end"]), int(c["query_start"]), int(c["query_end"])
        ri, qi = _where(t_starts, r0), _where(q_starts, q0)
        lines.append("#chain %d fill=%d run=%d score=%d %s %d %d %s %d %d %s\n" % (
            k, int(c["fill"]), int(c["run"]), int(c["score"]), t_names[ri], r0 + 1 - t_starts[ri], r1 - t_starts[ri], q_names[qi],
            q0 + 1 - q_starts[qi], q1 - q_starts[qi], strand))
        for x in out_hsps[int(c["first_member"]):int(c["first_member"]) + int(c["n_members"])]:
            a, b, n = int(x["ref_start"]), int(x["query_start"]), int(x["len"]) + 1
            ri, qi = _where(t_starts, a), _where(q_starts, b)
            lines.append(SEG_LINE % (t_names[ri], a + 1 - t_starts[ri], a + n - t_starts[ri], q_names[qi], b + 1 - q_starts[qi],
                                     b + n - q_starts[qi], strand, int(x["score"])))
    return "".join(lines)


def render_maf(records, texts, rev, t_names, t_starts, t_lens, q_names, q_starts, q_lens):
    """The .net.maf file in .stitched.maf's layout: records are stitch records, texts[k] the (target, query) alignment rows of record k."""
    out, strand = [], "-" if rev else "+"
    for r, (ta, qa) in zip(records, texts):
        r0, r1, q0, q1 = int(r["ref_start"]), int(r["ref_end"]), int(r["query_start"]), int(r["query_end"])
        ri, qi = _where(t_starts, r0), _where(q_starts, q0)
        out.append("a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n" % (
            int(r["score"]), t_names[ri], r0 - t_starts[ri], r1 - r0, t_lens[ri], ta, q_names[qi], q0 - q_starts[qi], q1 - q0, strand,
            q_lens[qi], qa))
    return "".join(out)
