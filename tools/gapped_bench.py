"""Gapped extension throughput: one forty-chunk call (10 Mbp of one query strand) through sa_seed_calls, then its HSPs through
sa_gapped_extend with the default parameters.  Prints one JSON line per workload: anchors, live cells, cells per anchor, flag
counts, kernel ms and giga-cells per second (cells / kernel time).  With --align the same HSPs also go through sa_gapped_align:
the line then adds its extension, trace-sweep and walk ms, the trace bytes and batches, and the ops returned.  With --greedy the same
HSPs go through sa_gapped_align in selection mode and through sa_gapped_align_greedy: the line then adds, for both, the anchors
extended, returned, covered, skipped and below threshold and the extension / trace / walk / cover ms.

With --pieces N the engine runs with option gapped_pieces = N (sides that end at max_extent are continued), with
--max-extent M the three entries get max_extent = M; the line then adds the sides continued, their further pieces and the rounds, the
records still extent-capped or continued and the summed alignment length of each entry.

With --chain [--chain-pen D,A] the HSPs (one group) first go through sa_chain_hsps: the line then adds n, groups, the
members kept, pair evaluations, tile steps, the chain kernel ms and pair evaluations per second, and the extension (with --align /
--greedy also the alignment / greedy) times on the chain's members beside those on all HSPs.  f and pred of every HSP and the members
are checked against the numpy model (tests/hsp_chain_model.py) once per run.

With --chain-costs loose|medium|FILE (with --chain) the same HSPs also go through sa_chain_hsps_costs under that gap-cost
table (FILE: axtChain's linearGap layout) on top of --chain-pen, in runs that alternate with the linear ones: the line then adds the
chain kernel ms and pair evaluations per second of the table runs beside the linear ones, every run's kernel ms, their ratio, and the
members and score under the table.  f, pred and the members are checked against tests/hsp_chain_gap_model.py once per run.

With --chain-overlap N (with --chain) the same HSPs also go through sa_chain_hsps_ovl under an allowance of N bases, on
top of --chain-pen and --chain-costs, in runs that alternate with the plain ones (the table's where one is given, the linear ones
otherwise): the line then adds the kernel ms of both, every run's, their ratio, and members and score with and without the allowance.
f, pred and the members are checked against tests/hsp_chain_overlap_model.py once per run.  The chain is then trimmed (sa_trim_chains):
the line adds trim ms (the least of the runs), the links trimmed, the members cut and the exact score, checked against
tests/chain_trim_model.py once per run.  The later stages (--chain-all, --stitch, --net ...) go on from the plain chains.

With --chain-all [--chain-min N] (which implies --chain) the HSPs also go through sa_chain_hsps_all: the line then adds
the chains before min_score, the chains, joined chains and members kept, the doubling rounds, peel ms beside the DP's kernel ms, and
the gapped times on the kept chains' members beside those on the best chain and on all HSPs.  The chains, members and chain_of are
checked against the numpy model (tests/hsp_chain_all_model.py) once per run, on the f and pred the --chain check computed.

With --fill [--fill-thresh N] (which implies --chain-all) the links of the kept chains go through sa_fill_chains under
--chain-pen: the line then adds the links by flag, the cells, count / emit / chain ms (the run with the least sweep time) and G cells/s
over both passes, the HSPs found, the fills and the links filled, and sa_stitch_chains's long links and records on the chains before
and after filling.  A prefix of the chains, links of at most 2^28 cells together, is checked against tests/chain_fill_model.py once
per run.

With --stitch [--stitch-max-link N] (which implies --chain-all) the kept chains go through sa_stitch_chains: the line then
adds the links by sweep instance, the broken links by reason, the cells, member / sweep / walk ms, giga-cells per second of the sweep, the
trace bytes and batches, and the target bases the stitched records span beside those the gapped alignments of the same members span.
Records, ops and links are checked against the model (tests/stitch_model.py) once per run.

With --net [--net-space N] [--net-fill N] (which implies --chain-all) the kept chains go through sa_net_chains on the target axis
(DESIGN.md 19): the line then adds the chains and blocks, fills, rounds, spaces searched, max depth, chains without a fill, prep ms and
net ms beside peel ms and the DP's kernel ms.  The fills are checked against the model (tests/net_model.py) once per run.

With --net-subset (which implies --net) the fills go through sa_net_subset with the split flag, under --chain-pen: the
line then adds fills, runs, members, cut members, bases rescored, the output bytes and subset ms beside net ms and peel ms.  Output HSPs
and sub-chains are checked against the model (tests/net_subset_model.py) once per run.

With --net-class [--net-class-filter S,T,Z,A,F] (which implies --net) the fills go through sa_net_classify with the query as the other
axis, once without a filter and once under the given thresholds (min_score, min_top_score, min_size, min_ali, max_far):
the line then adds the fills per class, clipped blocks, events, the sum of odup, the fills kept under the filter, the entry's own kernel
launches (the sort's come on top) and class ms, the least of the repeats, beside net ms and, with --net-subset, subset ms.  The records
and counts of both calls are checked against the model (tests/net_class_model.py) once per run.

With --lift[=N] (which implies --net-subset) N intervals (default 1 << 20) drawn from the target with a fixed seed, a third each points,
100-base and 10 000-base intervals, go through sa_lift_intervals with the query as the other axis, once through the
sub-chains of sa_net_subset and once through all chains: the line then adds per chain set the intervals per status, the candidates per
interval, the hits, and prep ms and lift ms, each the least of the repeats, beside net ms and subset ms, and the entry's own kernel
launches (the sort's and the running maximum's come on top).  The records, hits and blocks of a 4 096-interval sample through the
sub-chains, under both flags, are checked against the model (tests/lift_model.py) once per run.

  python tools/gapped_bench.py [--workloads standin,lumpy] [--repeat 3] [--align] [--greedy] [--batches 1024,2048,...]
                               [--pieces N] [--max-extent M] [--chain] [--chain-pen D,A] [--chain-costs T] [--chain-overlap N] [--fill] [--fill-thresh N] [--chain-all] [--chain-min N] [--stitch] [--stitch-max-link N]
                               [--net] [--net-space N] [--net-fill N] [--net-subset] [--net-class] [--net-class-filter S,T,Z,A,F] [--lift[=N]]
"""
import argparse
import functools
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # the engine's host: a hardware queue per slot

import numpy as np  # noqa: E402

from segalign_amd import engine as E  # noqa: E402
from segalign_amd import synth  # noqa: E402

SHAPE = "TTT0T00TT00T0T0TTTT"
# HOXD70 over A C G T and the engine's entries for L, N, X, E (what sa_initialize_processor gets for xdrop 910)
SUB = np.array([
    [91, -114, -31, -123, -1000, -1000, -100, -9100],
    [-114, 100, -125, -31, -1000, -1000, -100, -9100],
    [-31, -125, 100, -114, -1000, -1000, -100, -9100],
    [-123, -31, -114, 91, -1000, -1000, -100, -9100],
    [-1000] * 7 + [-9100],
    [-1000] * 7 + [-9100],
    [-100, -100, -100, -100, -1000, -1000, -100, -9100],
    [-9100] * 8], dtype=np.int32).reshape(64)


@functools.lru_cache(maxsize=None)
def workload(name):
    if name == "standin":  # the 100 Mbp stand-in of bench.py / BASELINE configs[1]
        return synth.make_pair(100_000_000, 3, 4, sub_rate=0.08, mask_frac=0.2, records=7, invert_frac=0.3, invert_block=100_000)
    if name == "lumpy":
        return synth.make_realistic(100_000_000)
    raise SystemExit("unknown workload %s" % name)


def with_stderr(f):
    """f() with file descriptor 2 captured: -> (result, what the library wrote to stderr)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            r = f()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return r, tmp.read().decode(errors="replace")


def greedy_edges(text):
    """(edges, largest pass, resolve passes) from the line option debug makes sa_gapped_align_greedy print."""
    m = re.search(r"GappedAlignGreedy: \d+ HSPs, \d+ priority batches, (\d+) resolve passes, (\d+) edges \(at most (\d+)", text)
    return (int(m.group(2)), int(m.group(3)), int(m.group(1))) if m else (None, None, None)


KW = {}  # max_extent for the three entries (--max-extent)


def pieces_line(text):
    """(sides continued, further pieces, rounds) summed over the lines option debug makes continue_sides print."""
    tot = [0, 0, 0]
    for m in re.finditer(r"GappedPieces: \d+ sides, (\d+) continued, (\d+) further pieces, (\d+) rounds", text):
        for k in range(3):
            tot[k] += int(m.group(k + 1))
    return tot


def span(recs):
    """Summed target length of records, and how many are still extent-capped / were continued."""
    return {"aligned_bases": int((recs["ref_end"].astype(np.int64) - recs["ref_start"]).sum()),
            "still_capped": int(np.count_nonzero(recs["flags"] & 1)), "continued": int(np.count_nonzero(recs["flags"] & 4))}


def greedy_fields(hsps, repeat, with_sel=True):
    """sa_gapped_align selection mode and sa_gapped_align_greedy on the same HSPs, the run with the least device time of each."""
    def best_of(f):
        best = None
        for _ in range(repeat):
            t0 = time.perf_counter()
            r = f()
            wall = (time.perf_counter() - t0) * 1e3
            st = r[3]
            total = st["kernel_ms"] + st["trace_ms"] + st["walk_ms"] + st.get("cover_ms", 0.0)
            if best is None or total < best[0]:
                best = (total, r, wall)
        return best
    g_total, (grecs, _, gops, gst), g_wall = best_of(lambda: E.GappedAlignGreedy(hsps, False, 0, **KW))
    _, err = with_stderr(lambda: E.GappedAlignGreedy(hsps, False, 0, **KW))  # option debug is on: the call prints its edge count
    n_edges, max_edges, passes = greedy_edges(err)
    n = int(hsps.size)
    sel = {}
    s_total = None
    if with_sel:
        s_total, (srecs, _, _, sst), s_wall = best_of(lambda: E.GappedAlign(hsps, False, 0, **KW))
        below = int(np.count_nonzero(E.GappedExtend(hsps, False, 0, raw=True, **KW)[0]["score"] < 3000))
        sel = {"sel_anchors": n, "sel_extended": int(sst["anchors"]), "sel_returned": int(srecs.size), "sel_below_thresh": below,
               "sel_extend_ms": round(sst["kernel_ms"], 3), "sel_trace_ms": round(sst["trace_ms"], 3), "sel_walk_ms": round(sst["walk_ms"], 3),
               "sel_kernel_ms": round(s_total, 3), "sel_call_ms": round(s_wall, 3), "sel_trace_bytes": int(sst["trace_bytes"]),
               "sel_trace_batches": int(sst["trace_batches"])}
    if with_sel:
        sel.update({"sel_" + k: v for k, v in span(srecs).items()})
    sel.update({"greedy_" + k: v for k, v in span(grecs).items()})
    gp = pieces_line(err)
    sel.update({"greedy_sides_continued": gp[0], "greedy_further_pieces": gp[1]})
    return {**sel, "greedy_anchors": n, "greedy_extended": int(gst["anchors"]), "greedy_returned": int(grecs.size),
            "greedy_covered": int(gst["covered"]), "greedy_skipped": int(gst["skipped"]), "greedy_below_thresh": int(gst["below_thresh"]),
            "greedy_extend_ms": round(gst["kernel_ms"], 3), "greedy_trace_ms": round(gst["trace_ms"], 3),
            "greedy_walk_ms": round(gst["walk_ms"], 3), "greedy_trace_bytes": int(gst["trace_bytes"]),
            "greedy_trace_batches": int(gst["trace_batches"]), "greedy_traced_not_returned": int(gst["anchors"]) - int(grecs.size),
            "edges": n_edges, "edges_max_pass": max_edges, "resolve_passes": passes, "greedy_cover_ms": round(gst["cover_ms"], 3), "greedy_kernel_ms": round(g_total, 3),
            "greedy_call_ms": round(g_wall, 3), "greedy_over_sel": round(g_total / s_total, 3) if s_total else None,
            "cover_share": round(gst["cover_ms"] / g_total, 4) if g_total > 0 else None, "priority_batches": int(gst["priority_batches"]),
            "greedy_batch": int(E.get_option("gapped_greedy_batch")), "cover_segments": int(gst["cover_segments"]),
            "trace_mb": int(E.get_option("gapped_trace_mb")), "greedy_ops": int(gops.size)}


def kept_fields(kept, repeat, align, greedy, prefix):
    """The gapped entries on the HSPs a chaining step kept."""
    kst = min((E.GappedExtend(kept, False, 0, **KW)[1] for _ in range(repeat)), key=lambda x: x["kernel_ms"])
    out = {prefix + "extend_ms": round(kst["kernel_ms"], 3), prefix + "cells": int(kst["cells"]), prefix + "alignments": int(kst["returned"])}
    if align:
        ast = min((E.GappedAlign(kept, False, 0, **KW)[3] for _ in range(repeat)), key=lambda x: x["kernel_ms"] + x["trace_ms"] + x["walk_ms"])
        out[prefix + "align_kernel_ms"] = round(ast["kernel_ms"] + ast["trace_ms"] + ast["walk_ms"], 3)
    if greedy:
        gst = min((E.GappedAlignGreedy(kept, False, 0, **KW)[3] for _ in range(repeat)),
                  key=lambda x: x["kernel_ms"] + x["trace_ms"] + x["walk_ms"] + x["cover_ms"])
        out[prefix + "greedy_kernel_ms"] = round(gst["kernel_ms"] + gst["trace_ms"] + gst["walk_ms"] + gst["cover_ms"], 3)
    return out


DIFF = False  # --diff: also read the alignments of --align and --stitch back (sa_diff_alignments)


def diff_fields(prefix, spans, ops, repeat, beside):
    """sa_diff_alignments on a producer's alignments, the run with the least count and emit time, checked against the
    model.  beside: the producer's own times of the same run, repeated here.  The bytes are what the two passes read of the sequences
    (two bytes per M column, one per gap column, each pass), over their time, as a fraction of the HBM rate."""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import diff_model as D
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.DiffAlignments(spans, ops, False, 0)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[2]["count_ms"] + r[2]["emit_ms"] < best[0][2]["count_ms"] + best[0][2]["emit_ms"]:
            best = (r, wall)
    (ev, sm, st), wall = best
    t0 = time.perf_counter()
    want = D.diff(E.copy_ref_codes(), E.copy_query_codes(0, False), spans, ops)
    model_s = time.perf_counter() - t0
    if not (np.array_equal(ev, want[0]) and np.array_equal(sm, want[1]) and np.array_equal(st["pairs"], want[2])):
        raise SystemExit("sa_diff_alignments differs from the model")
    m_cols = int(st["pairs"].sum())
    read = 2 * (2 * m_cols + (int(st["columns"]) - m_cols))
    ms = st["count_ms"] + st["emit_ms"]
    out = {"spans": int(st["spans"]), "ops": int(st["ops"]), "columns": int(st["columns"]), "work_items": int(st["work_items"]),
           "events": int(st["events"]), "matches": int(sm["matches"].astype(np.int64).sum()),
           "transitions": int(sm["transitions"].astype(np.int64).sum()), "transversions": int(sm["transversions"].astype(np.int64).sum()),
           "others": int(sm["others"].astype(np.int64).sum()), "prep_ms": round(st["prep_ms"], 3), "count_ms": round(st["count_ms"], 3),
           "emit_ms": round(st["emit_ms"], 3), "call_ms": round(wall, 3), "sequence_bytes_read": read,
           "fraction_of_hbm_rate": round(read / (ms * 1e-3) / HBM_BYTES_PER_S, 5) if ms > 0 else None, "model_checked": True,
           "model_s": round(model_s, 1)}
    out = {prefix + "diff_" + k: v for k, v in out.items()}
    out.update({prefix + "diff_beside_" + k: round(v, 3) for k, v in beside.items()})
    return out


HBM_BYTES_PER_S = 8e12  # MI355X: 8 TB/s


def stitch_fields(hsps, members, repeat, max_link):
    """sa_stitch_chains on the kept chains, the run with the least sweep time, checked against the model."""
    import stitch_model as S
    mem, first = E.chain_csr(members)
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.StitchChains(hsps, mem, first, False, 0, max_link=max_link, links=True)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[3]["sweep_ms"] < best[0][3]["sweep_ms"]:
            best = (r, wall)
    (recs, ops, links, st), wall = best
    t0 = time.perf_counter()
    want = S.stitch(E.copy_ref_codes(), E.copy_query_codes(0, False), SUB, hsps, mem, first, max_link=max_link)
    model_s = time.perf_counter() - t0
    if not (np.array_equal(recs, want[0].astype(recs.dtype)) and np.array_equal(ops, want[1]) and np.array_equal(links, want[2].astype(links.dtype))):
        raise SystemExit("sa_stitch_chains differs from the model")
    swept = links[(links["flags"] & E.STITCH_LONG) == 0]
    by_k = {str(k): int(np.count_nonzero([S.instance(int(d)) == k for d in swept["dt"]])) for k in S.INSTANCES}
    grecs = E.GappedExtend(hsps[np.sort(members["hsp_index"])], False, 0, **KW)[0]
    extra = diff_fields("stitch_", E.diff_spans(recs), ops, repeat, {"sweep_ms": st["sweep_ms"], "walk_ms": st["walk_ms"]}) if DIFF else {}
    return {**extra, "stitch_max_link": int(max_link or S.MAX_LINK), "stitch_chains": int(first.size - 1), "stitch_members": int(mem.size),
            "stitch_links": int(st["links"]), "stitch_swept": int(st["swept"]), "stitch_links_by_instance": by_k,
            "stitch_long": int(st["long_links"]), "stitch_dead": int(st["dead_links"]), "stitch_low": int(st["low_links"]),
            "stitch_records": int(st["records"]), "stitch_cells": int(st["cells"]), "stitch_member_ms": round(st["member_ms"], 3),
            "stitch_sweep_ms": round(st["sweep_ms"], 3), "stitch_walk_ms": round(st["walk_ms"], 3), "stitch_call_ms": round(wall, 3),
            "stitch_gcells_per_s": round(st["cells"] / (st["sweep_ms"] * 1e-3) / 1e9, 3) if st["sweep_ms"] > 0 else None,
            "stitch_trace_bytes": int(st["trace_bytes"]), "stitch_batches": int(st["batches"]), "stitch_ops": int(ops.size),
            "stitch_aligned_bases": int((recs["ref_end"].astype(np.int64) - recs["ref_start"]).sum()),
            "stitch_gap_bases": int(recs["gap_bases"].sum()), "kept_gapped_aligned_bases": span(grecs)["aligned_bases"],
            "kept_gapped_alignments": int(grecs.size), "stitch_model_checked": True, "stitch_model_s": round(model_s, 1)}


def fill_fields(hsps, members, repeat, pen, thresh):
    """sa_fill_chains on the kept chains, the run with the least count and emit time; sa_stitch_chains's long links and
    records on the chains before and after; a prefix of the chains (links of at most 2^28 cells together) checked against the model."""
    import chain_fill_model as F
    mem, first = E.chain_csr(members)
    kw = dict(thresh=thresh, diag_pen=pen[0], anti_pen=pen[1])
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.FillChains(hsps, mem, first, False, 0, links=True, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[5]["count_ms"] + r[5]["emit_ms"] < best[0][5]["count_ms"] + best[0][5]["emit_ms"]:
            best = (r, wall)
    (out, first_out, origin, ch, links, st), wall = best
    before = E.StitchChains(hsps, mem, first, False, 0)[2]
    after = E.StitchChains(out, np.arange(out.size, dtype=np.uint32), first_out, False, 0)[2]
    # the model on the first chains: as many as keep the scalar checker below 2^28 cells
    nl = np.maximum(np.diff(first.astype(np.int64)) - 1, 0)
    cells = np.concatenate([[0], np.cumsum(links["cells"].astype(np.int64))])[np.cumsum(nl)]  # the cells up to and including chain c
    k = min(max(1, int(np.searchsorted(cells, 1 << 28, side="right"))), first.size - 1)
    t0 = time.perf_counter()
    got = E.FillChains(hsps, mem[:first[k]], first[:k + 1], False, 0, links=True, found=True, **kw)
    want = F.fill(E.copy_ref_codes(), E.copy_query_codes(0, False), SUB, hsps, mem[:first[k]], first[:k + 1], **kw)
    model_s = time.perf_counter() - t0
    for g, w in zip(got[:6], want):
        if g.size != w.size or not all(np.array_equal(g[f], w[f]) for f in (w.dtype.names or ())) or (not w.dtype.names and not np.array_equal(g, w)):
            raise SystemExit("sa_fill_chains differs from the model")
    sweep_ms = st["count_ms"] + st["emit_ms"]
    return {"fill_thresh": int(thresh), "fill_links": int(st["links"]), "fill_swept": int(st["swept"]), "fill_long": int(st["long_links"]),
            "fill_large": int(st["large_links"]), "fill_crowded": int(st["crowded_links"]), "fill_cells": int(st["cells"]),
            "fill_hsps_found": int(st["hsps"]), "fill_fills": int(st["fills"]), "fill_links_filled": int(st["filled_links"]),
            "fill_bases": int(ch["fill_bases"].astype(np.int64).sum()), "fill_count_ms": round(st["count_ms"], 3), "fill_emit_ms": round(st["emit_ms"], 3),
            "fill_chain_ms": round(st["chain_ms"], 3), "fill_call_ms": round(wall, 3),
            "fill_gcells_per_s": round(2 * st["cells"] / (sweep_ms * 1e-3) / 1e9, 3) if sweep_ms > 0 else None,  # both passes sweep every cell
            "fill_stitch_long_before": int(before["long_links"]), "fill_stitch_records_before": int(before["records"]),
            "fill_stitch_long_after": int(after["long_links"]), "fill_stitch_records_after": int(after["records"]),
            "fill_model_checked": True, "fill_model_chains": int(k), "fill_model_links": int(want[4].size), "fill_model_s": round(model_s, 1)}


def subset_fields(hsps, mem, first, fills, repeat, pen, net_ms, peel_ms):
    """sa_net_subset on the fills of the net, the run with the least subset time, checked against the model."""
    import net_subset_model as NS
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        # the penalties must be the chains': chain_all_fields calls ChainHspsAll under pen without a gap-cost table, so none is given here;
        # should --chain-costs ever reach ChainHspsAll, the same table belongs here and in the model call below
        r = E.NetSubset(hsps, mem, first, fills, False, 0, axis="target", split=True, diag_pen=pen[0], anti_pen=pen[1])
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[2]["subset_ms"] < best[0][2]["subset_ms"]:
            best = (r, wall)
    (out, sub, st), wall = best
    t0 = time.perf_counter()
    want_h, want_c, want_st = NS.subset(E.copy_ref_codes(), E.copy_query_codes(0, False), SUB, hsps, mem, first, fills, diag_pen=pen[0],
                                        anti_pen=pen[1])
    model_s = time.perf_counter() - t0
    if not (np.array_equal(out, want_h.astype(out.dtype)) and np.array_equal(sub, want_c.astype(sub.dtype))
            and all(st[k] == want_st[k] for k in NS.COUNTS)):
        raise SystemExit("sa_net_subset differs from the model")
    return {"subset_fills": int(st["fills"]), "subset_runs": int(st["runs"]), "subset_members": int(st["members"]),
            "subset_cut_members": int(st["cut_members"]), "subset_bases_rescored": int(st["bases_rescored"]), "subset_splits": int(st["splits"]),
            "subset_out_bytes": int(out.nbytes + sub.nbytes), "subset_ms": round(st["subset_ms"], 3), "subset_net_ms": round(net_ms, 3),
            "subset_peel_ms": round(peel_ms, 3), "subset_call_ms": round(wall, 3),
            "subset_over_net": round(st["subset_ms"] / net_ms, 4) if net_ms > 0 else None, "subset_model_checked": True,
            "subset_model_s": round(model_s, 1)}


def class_fields(hsps, mem, first, bs, be, fills, repeat, thresholds, net_ms, subset_ms):
    """sa_net_classify on the fills of the net with the query as the other axis (one query record, one strand), without a filter (the
    run with the least class time) and under `thresholds`, both checked against the model."""
    import net_class_model as NC
    obs, obe = E.net_other_blocks(hsps, mem, first, axis="target")
    flt = dict(zip(NC.THRESHOLDS, thresholds))
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.NetClassify(first, bs, be, obs, obe, fills)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[1]["class_ms"] < best[0][1]["class_ms"]:
            best = (r, wall)
    (cls, st), wall = best
    fcls, fst = E.NetClassify(first, bs, be, obs, obe, fills, filter=flt)
    t0 = time.perf_counter()
    for got, got_st, want in ((cls, st, NC.classify(first, bs, be, obs, obe, fills)), (fcls, fst, NC.classify(first, bs, be, obs, obe, fills, filter=flt))):
        if not np.array_equal(got, want[0].astype(got.dtype)) or any((list(got_st[k]) if k == "n_type" else got_st[k]) != want[1][k] for k in NC.COUNTS):
            raise SystemExit("sa_net_classify differs from the model")
    model_s = time.perf_counter() - t0
    return {"class_fills": int(st["fills"]), **{"class_" + n: int(st["n_type"][k]) for k, n in enumerate(NC.NAMES)},
            "class_blocks": int(st["blocks"]), "class_events": int(st["events"]), "class_dup_bases": int(st["dup_bases"]),
            "class_filter": ",".join(str(int(x)) for x in thresholds), "class_kept": int(fst["kept"]),
            "class_launches": 18, "class_launches_filtered": 19,  # counts, emit, flags, segments, block_dup, classes (keep); four scans of three
            "class_ms": round(st["class_ms"], 3), "class_filtered_ms": round(fst["class_ms"], 3), "class_net_ms": round(net_ms, 3),
            "class_subset_ms": None if subset_ms is None else round(subset_ms, 3), "class_call_ms": round(wall, 3),
            "class_over_net": round(st["class_ms"] / net_ms, 4) if net_ms > 0 else None, "class_model_checked": True,
            "class_model_s": round(model_s, 1)}


def lift_fields(hsps, mem, first, bs, be, fills, repeat, n, pen, net_ms, subset_ms):
    """sa_lift_intervals on n intervals of the target (fixed seed; points, 100-base and 10 000-base intervals a third each), through the
    sub-chains of the net and through all chains, per chain set the least prep and lift time; a 4 096-interval sample through the
    sub-chains, under both flags, checked against the model."""
    import lift_model as LM
    out, sub, _ = E.NetSubset(hsps, mem, first, fills, False, 0, axis="target", split=True, diag_pen=pen[0], anti_pen=pen[1])
    smem, sfirst = E.subset_csr(sub)
    sets = {"sub": (sfirst,) + E.net_blocks(out, smem, sfirst, axis="target") + E.net_blocks(out, smem, sfirst, axis="query"),
            "all": (first, bs, be) + E.net_other_blocks(hsps, mem, first, axis="target")}
    rng = np.random.default_rng(2323)
    top = int(be.max()) if be.size else 1 << 20
    length = np.repeat(np.array([1, 100, 10_000], dtype=np.int64), (n + 2) // 3)[:n]
    start = (rng.random(n) * np.maximum(top - length, 1)).astype(np.int64)
    order = rng.permutation(n)
    start, end = start[order].astype(np.uint32), (start + length)[order].astype(np.uint32)
    res = {"lift_intervals": int(n), "lift_launches": 11, "lift_launches_blocks": 15,  # block_len, keys, gather, count, emit (blocks); two (three) scans of three
           "lift_net_ms": round(net_ms, 3), "lift_subset_ms": None if subset_ms is None else round(subset_ms, 3)}
    for name, c in sets.items():
        prep = lift = wall = None
        for _ in range(repeat):
            t0 = time.perf_counter()
            rec, hits, _, st = E.LiftIntervals(*c, start, end)
            w = (time.perf_counter() - t0) * 1e3
            prep = st["prep_ms"] if prep is None else min(prep, st["prep_ms"])
            lift = st["lift_ms"] if lift is None else min(lift, st["lift_ms"])
            wall = w if wall is None else min(wall, w)
        res.update({"lift_%s_chains" % name: int(st["chains"]), "lift_%s_blocks" % name: int(st["blocks"]),
                    **{"lift_%s_%s" % (name, s): int(st["n_status"][k]) for k, s in enumerate(LM.NAMES)},
                    "lift_%s_candidates_per_interval" % name: round(st["candidates"] / max(n, 1), 3),
                    "lift_%s_touches_per_interval" % name: round(st["touches"] / max(n, 1), 3), "lift_%s_hits" % name: int(st["hits"]),
                    "lift_%s_prep_ms" % name: round(prep, 3), "lift_%s_ms" % name: round(lift, 3), "lift_%s_call_ms" % name: round(wall, 3)})
    t0 = time.perf_counter()
    k = min(n, 4096)
    got = E.LiftIntervals(*sets["sub"], start[:k], end[:k], multiple=True, blocks=True)
    want = LM.lift(*sets["sub"], start[:k], end[:k], multiple=True, blocks=True)
    try:
        LM.same(got, want)
        LM.same_stats(got[3], want[3])
    except AssertionError as ex:
        raise SystemExit("sa_lift_intervals differs from the model: %s" % (ex,))
    res.update({"lift_model_checked": True, "lift_model_intervals": int(k), "lift_model_s": round(time.perf_counter() - t0, 1)})
    return res


def net_fields(hsps, chains, members, repeat, net, peel_ms, dp_ms, pen=(0, 0)):
    """sa_net_chains on the kept chains' target blocks, the run with the least net time, checked against the model; net[2]: also
    subset_fields on its fills; net[3]: also class_fields on them, under the thresholds net[4]; net[5]: also lift_fields on so many
    intervals."""
    import net_model as N
    mem, first = E.chain_csr(members)
    bs, be = E.net_blocks(hsps, mem, first, axis="target")
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.NetChains(first, bs, be, chains["score"], chains["group"], min_space=net[0], min_fill=net[1])
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[1]["net_ms"] < best[0][1]["net_ms"]:
            best = (r, wall)
    (fills, st), wall = best
    t0 = time.perf_counter()
    want, want_st = N.net(first, bs, be, chains["score"], chains["group"], min_space=net[0], min_fill=net[1])
    model_s = time.perf_counter() - t0
    if not np.array_equal(fills, want.astype(fills.dtype)) or any(st[k] != want_st[k] for k in ("fills", "filled", "max_depth")):
        raise SystemExit("sa_net_chains differs from the model")
    extra = subset_fields(hsps, mem, first, fills, repeat, pen, st["net_ms"], peel_ms) if len(net) > 2 and net[2] else {}
    if len(net) > 3 and net[3]:
        extra.update(class_fields(hsps, mem, first, bs, be, fills, repeat, net[4], st["net_ms"], extra.get("subset_ms")))
    if len(net) > 5 and net[5]:
        extra.update(lift_fields(hsps, mem, first, bs, be, fills, repeat, net[5], pen, st["net_ms"], extra.get("subset_ms")))
    return {**extra, "net_min_space": int(net[0]), "net_min_fill": int(net[1]), "net_chains": int(st["chains"]), "net_blocks": int(st["blocks"]),
            "net_fills": int(st["fills"]), "net_rounds": int(st["rounds"]), "net_spaces": int(st["spaces"]), "net_max_depth": int(st["max_depth"]),
            "net_chains_without_fill": int(st["chains"] - st["filled"]), "net_prep_ms": round(st["prep_ms"], 3), "net_ms": round(st["net_ms"], 3),
            "net_call_ms": round(wall, 3), "net_over_peel": round(st["net_ms"] / peel_ms, 4) if peel_ms > 0 else None,
            "net_over_dp": round(st["net_ms"] / dp_ms, 4) if dp_ms > 0 else None, "net_model_checked": True, "net_model_s": round(model_s, 1)}


def chain_all_fields(hsps, repeat, pen, min_score, dp, align, greedy, stitch=None, net=None, fill=None):
    """sa_chain_hsps_all on the HSPs as one group, checked against the numpy model on the DP values `dp` that chain_fields checked, and
    the gapped entries on the kept chains' members."""
    import hsp_chain_all_model as A
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.ChainHspsAll(hsps, None, diag_pen=pen[0], anti_pen=pen[1], min_score=min_score, nodes=True)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or r[4]["peel_ms"] < best[0][4]["peel_ms"]:
            best = (r, wall)
    (chains, members, nodes, chain_of, st), wall = best
    f, pred, want_c, want_m, want_of = A.chain_all(hsps, None, diag_pen=pen[0], anti_pen=pen[1], min_score=min_score, dp=dp)
    if not (np.array_equal(nodes["f"], f) and np.array_equal(nodes["pred"], pred) and np.array_equal(chains, want_c.astype(chains.dtype))
            and np.array_equal(members, want_m.astype(members.dtype)) and np.array_equal(chain_of, want_of)):
        raise SystemExit("sa_chain_hsps_all differs from the numpy model")
    out = {"all_min_score": int(min_score), "all_chains_before_min": int(st["chains_all"]), "all_chains": int(st["chains"]),
           "all_joined": int(st["joined"]), "all_members": int(st["members"]), "peel_rounds": int(st["peel_rounds"]),
           "peel_ms": round(st["peel_ms"], 3), "all_dp_kernel_ms": round(st["kernel_ms"], 3),
           "peel_over_dp": round(st["peel_ms"] / st["kernel_ms"], 4) if st["kernel_ms"] > 0 else None, "all_call_ms": round(wall, 3),
           "all_model_checked": True}
    out.update(kept_fields(hsps[np.sort(members["hsp_index"])], repeat, align, greedy, "all_kept_"))
    if stitch is not None:
        out.update(stitch_fields(hsps, members, repeat, stitch))
    if net is not None:
        out.update(net_fields(hsps, chains, members, repeat, net, st["peel_ms"], st["kernel_ms"], pen))
    if fill is not None:
        out.update(fill_fields(hsps, members, repeat, pen, fill))
    return out


def chain_costs_table(name):
    """--chain-costs: a preset's name or a linearGap file -> what engine.chain_gap_costs takes."""
    if name in ("loose", "medium"):
        return name
    with open(name) as f:
        return E.parse_linear_gap(f.read())


def chain_costs_fields(hsps, pen, costs, runs, linear_ms):
    """The runs of sa_chain_hsps_costs that chain_fields interleaved with the linear ones, checked against the model."""
    import hsp_chain_gap_model as GM
    members, nodes, st = min(runs, key=lambda r: r[2]["kernel_ms"])
    t0 = time.perf_counter()
    f, pred, want = GM.chain(hsps, None, diag_pen=pen[0], anti_pen=pen[1], gap_costs=chain_costs_table(costs))
    model_s = time.perf_counter() - t0
    if not (np.array_equal(nodes["f"], f) and np.array_equal(nodes["pred"], pred) and np.array_equal(members, want)):
        raise SystemExit("sa_chain_hsps_costs differs from the model")
    ms = st["kernel_ms"]
    return {"chain_costs": costs, "chain_costs_members": int(st["members"]), "chain_costs_score": int(members["f"][-1]) if members.size else None,
            "chain_costs_pair_evals": int(st["pair_evals"]), "chain_costs_kernel_ms": round(ms, 3),
            "chain_costs_gpairs_per_s": round(st["pair_evals"] / (ms * 1e-3) / 1e9, 3) if ms > 0 else None,
            "chain_costs_runs_ms": [round(r[2]["kernel_ms"], 3) for r in runs], "chain_linear_runs_ms": [round(x, 3) for x in linear_ms],
            "chain_costs_over_linear": round(ms / min(linear_ms), 3) if min(linear_ms) > 0 else None,
            "chain_costs_model_checked": True, "chain_costs_model_s": round(model_s, 1)}


def chain_overlap_fields(hsps, pen, costs, overlap, runs, plain_runs):
    """The runs of sa_chain_hsps_ovl that chain_fields interleaved with the plain ones (under the table where there is one), checked
    against the model."""
    import hsp_chain_overlap_model as OM
    members, nodes, st = min(runs, key=lambda r: r[2]["kernel_ms"])
    plain_m, _, plain_st = min(plain_runs, key=lambda r: r[2]["kernel_ms"])
    t0 = time.perf_counter()
    f, pred, want = OM.chain_rows(hsps, None, diag_pen=pen[0], anti_pen=pen[1], gap_costs=chain_costs_table(costs) if costs else None,
                                  max_overlap=overlap)
    model_s = time.perf_counter() - t0
    if not (np.array_equal(nodes["f"], f) and np.array_equal(nodes["pred"], pred) and np.array_equal(members, want)):
        raise SystemExit("sa_chain_hsps_ovl differs from the model")
    idx = members["hsp_index"]
    re, qe = hsps["ref_start"].astype(np.int64) + hsps["len"] + 1, hsps["query_start"].astype(np.int64) + hsps["len"] + 1
    o = np.maximum(0, np.maximum(re[idx[:-1]] - hsps["ref_start"][idx[1:]], qe[idx[:-1]] - hsps["query_start"][idx[1:]])) if idx.size > 1 else np.zeros(0)
    ms, plain_ms = st["kernel_ms"], plain_st["kernel_ms"]
    import chain_trim_model as TM
    mem, first = E.chain_csr(members)
    table = chain_costs_table(costs) if costs else None
    trims = [E.TrimChains(hsps, mem, first, False, 0, diag_pen=pen[0], anti_pen=pen[1], gap_costs=table, links=True) for _ in runs]
    t_out, t_ch, t_links, t_st = min(trims, key=lambda r: r[3]["kernel_ms"])
    w_out, w_ch, w_links = TM.trim(E.copy_ref_codes(), E.copy_query_codes(0, False), SUB, hsps, mem, first, diag_pen=pen[0], anti_pen=pen[1],
                                   gap_costs=table)
    if not (all(np.array_equal(t_out[k], w_out[k]) for k in w_out.dtype.names) and all(np.array_equal(t_ch[k], w_ch[k]) for k in w_ch.dtype.names)
            and all(np.array_equal(t_links[k], w_links[k]) for k in w_links.dtype.names)):
        raise SystemExit("sa_trim_chains differs from the model")
    trim = {"trim_ms": round(t_st["kernel_ms"], 3), "trim_runs_ms": [round(r[3]["kernel_ms"], 3) for r in trims],
            "trim_links": int(t_st["trimmed_links"]), "trim_cut_members": int(t_st["cut_members"]), "trim_bases_cut": int(t_st["bases_cut"]),
            "trim_exact_score": int(t_ch["score"][0]) if t_ch.size else None, "trim_model_checked": True}
    return {**trim, "chain_overlap": int(overlap), "chain_overlap_members": int(st["members"]), "chain_overlap_score": int(members["f"][-1]) if members.size else None,
            "chain_overlap_links_overlapping": int((o > 0).sum()), "chain_overlap_largest": int(o.max()) if o.size else 0,
            "chain_overlap_plain_members": int(plain_st["members"]), "chain_overlap_plain_score": int(plain_m["f"][-1]) if plain_m.size else None,
            "chain_overlap_kernel_ms": round(ms, 3), "chain_overlap_plain_kernel_ms": round(plain_ms, 3),
            "chain_overlap_runs_ms": [round(r[2]["kernel_ms"], 3) for r in runs], "chain_overlap_plain_runs_ms": [round(r[2]["kernel_ms"], 3) for r in plain_runs],
            "chain_overlap_median_ms": round(float(np.median([r[2]["kernel_ms"] for r in runs])), 3),
            "chain_overlap_plain_median_ms": round(float(np.median([r[2]["kernel_ms"] for r in plain_runs])), 3),
            "chain_overlap_over_plain": round(float(np.median([r[2]["kernel_ms"] for r in runs]) / np.median([r[2]["kernel_ms"] for r in plain_runs])), 3),
            "chain_overlap_model_checked": True, "chain_overlap_model_s": round(model_s, 1)}


def chain_fields(hsps, repeat, pen, align, greedy, all_min=None, stitch=None, net=None, costs=None, overlap=0, fill=None):
    """sa_chain_hsps on the HSPs as one group, checked against the numpy model, and the gapped entries on the chain's members; with
    all_min also chain_all_fields, with costs also chain_costs_fields (its runs alternate with the linear ones), with overlap also
    chain_overlap_fields (its runs alternate with the plain ones)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hsp_chain_model as M
    best, cost_runs, linear_ms, linear_runs, overlap_runs = None, [], [], [], []
    table = E.chain_gap_costs(chain_costs_table(costs)) if costs else None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = E.ChainHsps(hsps, None, diag_pen=pen[0], anti_pen=pen[1], nodes=True)
        wall = (time.perf_counter() - t0) * 1e3
        linear_ms.append(r[2]["kernel_ms"])
        linear_runs.append(r)
        if best is None or r[2]["kernel_ms"] < best[0][2]["kernel_ms"]:
            best = (r, wall)
        if table is not None:
            cost_runs.append(E.ChainHsps(hsps, None, diag_pen=pen[0], anti_pen=pen[1], nodes=True, gap_costs=table))
        if overlap:
            overlap_runs.append(E.ChainHsps(hsps, None, diag_pen=pen[0], anti_pen=pen[1], nodes=True, gap_costs=table, max_overlap=overlap))
    (members, nodes, st), wall = best
    t0 = time.perf_counter()
    f, pred, want = M.chain(hsps, None, diag_pen=pen[0], anti_pen=pen[1])
    model_s = time.perf_counter() - t0
    if not (np.array_equal(nodes["f"], f) and np.array_equal(nodes["pred"], pred) and np.array_equal(members, want)):
        raise SystemExit("sa_chain_hsps differs from the numpy model")
    kept = hsps[np.sort(members["hsp_index"])]
    out = {"chain_pen": list(pen), "chain_n": int(st["hsps"]), "chain_groups": int(st["groups"]), "chain_members": int(st["members"]),
           "chain_score": int(members["f"][-1]) if members.size else None, "chain_pair_evals": int(st["pair_evals"]),
           "chain_tile_steps": int(st["tile_steps"]), "chain_tile": int(E.get_option("chain_tile")), "chain_kernel_ms": round(st["kernel_ms"], 3),
           "chain_call_ms": round(wall, 3), "chain_gpairs_per_s": round(st["pair_evals"] / (st["kernel_ms"] * 1e-3) / 1e9, 3) if st["kernel_ms"] > 0 else None,
           "chain_model_checked": True, "chain_model_s": round(model_s, 1)}
    if costs:
        out.update(chain_costs_fields(hsps, pen, costs, cost_runs, linear_ms))
    if overlap:
        out.update(chain_overlap_fields(hsps, pen, costs, overlap, overlap_runs, cost_runs if costs else linear_runs))
    out.update(kept_fields(kept, repeat, align, greedy, "kept_"))
    if all_min is not None:
        out.update(chain_all_fields(hsps, repeat, pen, all_min, (f, pred), align, greedy, stitch, net, fill))
    return out


def run(name, repeat, align=False, greedy=False, with_sel=True, pieces=0, chain=None, chain_all_min=None, stitch=None, net=None, chain_costs=None,
        chain_overlap=0, fill=None):
    t, q = workload(name)
    if greedy or pieces:
        E.set_option("debug", 1)  # sa_gapped_align_greedy then prints its edge count, the continuation its pieces
    if pieces:
        E.set_option("gapped_pieces", pieces)
    E.InitializeInterface(1)
    E.GenerateShapePos(SHAPE)
    E.InitializeProcessor(True, 250_000, 19, SUB, 910, 3000, False)
    keep = E.SendRefWriteRequest(t, 0, t.size)
    E.GenerateSeedPosTable(keep, 0, t.size, 1, 19, 12)
    E.SendQueryWriteRequest(q, 0, q.size, 0)
    call = (0, min(40 * 250_000, q.size - 19), False)
    outs, _ = E.SeedCalls([call], buffer=0, threads=1)
    hsps = outs[0]
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        recs, st = E.GappedExtend(hsps, False, 0, **KW)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or st["kernel_ms"] < best[1]["kernel_ms"]:
            best = (recs, st, wall)
    recs, st, wall = best
    extra = {}
    if pieces:
        _, err = with_stderr(lambda: E.GappedExtend(hsps, False, 0, **KW))
        pc = pieces_line(err)
        extra = {"pieces": pieces, "max_extent": KW.get("max_extent", 65536), "sides_continued": pc[0], "further_pieces": pc[1],
                 "rounds": pc[2], "pieces_per_continued_side": round(1 + pc[1] / pc[0], 3) if pc[0] else None, **span(recs)}
    if align:
        best_a = None
        for _ in range(repeat):
            t0 = time.perf_counter()
            arecs, paths, ops, ast = E.GappedAlign(hsps, False, 0, **KW)
            awall = (time.perf_counter() - t0) * 1e3
            total = ast["kernel_ms"] + ast["trace_ms"] + ast["walk_ms"]
            if best_a is None or total < best_a[0]:
                best_a = (total, arecs, ops, ast, awall, paths)
        total, arecs, ops, ast, awall, paths = best_a
        if not np.array_equal(arecs, recs):
            raise SystemExit("sa_gapped_align returned other records than sa_gapped_extend")
        extra.update({"align_extend_ms": round(ast["kernel_ms"], 3), "align_trace_ms": round(ast["trace_ms"], 3),
                 "align_walk_ms": round(ast["walk_ms"], 3), "align_kernel_ms": round(total, 3), "align_call_ms": round(awall, 3),
                 "align_over_extend": round(total / st["kernel_ms"], 3) if st["kernel_ms"] > 0 else None,
                 "trace_bytes": int(ast["trace_bytes"]), "trace_batches": int(ast["trace_batches"]), "ops": int(ops.size)})
        if DIFF:
            extra.update(diff_fields("align_", E.diff_spans(arecs, paths), ops, repeat, {"trace_ms": ast["trace_ms"], "walk_ms": ast["walk_ms"]}))
    if greedy:
        extra.update(greedy_fields(hsps, repeat, with_sel))
    if chain is not None:
        extra.update(chain_fields(hsps, repeat, chain, align, greedy, chain_all_min, stitch, net, chain_costs, chain_overlap, fill))
    E.ShutdownProcessor()
    if greedy or pieces:
        E.reset_option("debug")
    if pieces:
        E.reset_option("gapped_pieces")
    return {"workload": name, "call": list(call), "anchors": int(st["anchors"]), "alignments": int(st["returned"]),
            "cells": int(st["cells"]), "cells_per_anchor": st["cells"] / max(st["anchors"], 1),
            "extent_capped": int(st["extent_capped"]), "band_capped": int(st["band_capped"]),
            "kernel_ms": round(st["kernel_ms"], 3), "call_ms": round(wall, 3),
            "gcells_per_s": round(st["cells"] / (st["kernel_ms"] * 1e-3) / 1e9, 3) if st["kernel_ms"] > 0 else None, **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="standin,lumpy")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--align", action="store_true", help="also time sa_gapped_align on the same HSPs")
    ap.add_argument("--greedy", action="store_true", help="also time sa_gapped_align (selection mode) and sa_gapped_align_greedy")
    ap.add_argument("--batches", default="", help="with --greedy: one line per gapped_greedy_batch value, greedy only (a sweep)")
    ap.add_argument("--pieces", type=int, default=0, help="engine option gapped_pieces (0: left at its default of 1)")
    ap.add_argument("--max-extent", type=int, default=0, help="max_extent of every entry (0: the default, 65536)")
    ap.add_argument("--chain", action="store_true", help="also chain the HSPs (sa_chain_hsps) and time the gapped entries on the chain's members")
    ap.add_argument("--chain-pen", default="0,0", help="with --chain: diag_pen,anti_pen")
    ap.add_argument("--chain-costs", default="", help="with --chain: also chain under this gap-cost table (loose, medium or a linearGap file)")
    ap.add_argument("--chain-overlap", type=int, default=0, help="with --chain: also chain under this overlap allowance (1 .. 4096 bases)")
    ap.add_argument("--chain-all", action="store_true", help="also peel the HSPs into all chains (sa_chain_hsps_all); implies --chain")
    ap.add_argument("--chain-min", type=int, default=0, help="with --chain-all: min_score")
    ap.add_argument("--stitch", action="store_true", help="also stitch the kept chains (sa_stitch_chains); implies --chain-all")
    ap.add_argument("--stitch-max-link", type=int, default=0, help="with --stitch: max_link (0: the default, 2048)")
    ap.add_argument("--net", action="store_true", help="also net the kept chains on the target axis (sa_net_chains); implies --chain-all")
    ap.add_argument("--net-space", type=int, default=1, help="with --net: min_space")
    ap.add_argument("--net-fill", type=int, default=1, help="with --net: min_fill")
    ap.add_argument("--net-subset", action="store_true", help="also cut the fills into sub-chains (sa_net_subset); implies --net")
    ap.add_argument("--net-class", action="store_true", help="also class the fills against their parents on the query (sa_net_classify); implies --net")
    ap.add_argument("--net-class-filter", default="3000,5000,30,25,100000",
                    help="with --net-class: min_score,min_top_score,min_size,min_ali,max_far of the filtered call")
    ap.add_argument("--lift", type=int, nargs="?", const=1 << 20, default=0, metavar="N",
                    help="also lift N intervals of the target through the sub-chains and through all chains (sa_lift_intervals); implies --net-subset")
    ap.add_argument("--fill", action="store_true", help="also fill the links of the kept chains (sa_fill_chains); implies --chain-all")
    ap.add_argument("--fill-thresh", type=int, default=3000, help="with --fill: thresh")
    ap.add_argument("--diff", action="store_true", help="with --align and/or --stitch: also read their alignments back (sa_diff_alignments)")
    a = ap.parse_args()
    if a.diff and not (a.align or a.stitch):
        ap.error("--diff needs --align or --stitch")
    global DIFF
    DIFF = a.diff
    if a.lift < 0 or a.lift > 1 << 26:
        ap.error("--lift takes 1 .. 1 << 26 intervals")
    a.net_subset = a.net_subset or a.lift > 0
    a.net = a.net or a.net_subset or a.net_class
    class_filter = tuple(int(x) for x in a.net_class_filter.split(","))
    if len(class_filter) != 5:
        ap.error("--net-class-filter takes five values")
    a.chain_all = a.chain_all or a.stitch or a.net or a.fill
    chain = tuple(int(x) for x in a.chain_pen.split(",")) if a.chain or a.chain_all else None
    if a.chain_costs and chain is None:
        ap.error("--chain-costs needs --chain")
    if not 0 <= a.chain_overlap <= 4096:
        ap.error("--chain-overlap takes 0 .. 4096 (0: off)")
    if a.chain_overlap and chain is None:
        ap.error("--chain-overlap needs --chain")
    if a.max_extent:
        KW["max_extent"] = a.max_extent
    for name in a.workloads.split(","):
        if not a.batches:
            print(json.dumps(run(name, a.repeat, a.align, a.greedy, pieces=a.pieces, chain=chain, chain_all_min=a.chain_min if a.chain_all else None,
                                 stitch=a.stitch_max_link if a.stitch else None, net=(a.net_space, a.net_fill, a.net_subset, a.net_class, class_filter, a.lift) if a.net else None,
                                 chain_costs=a.chain_costs or None, chain_overlap=a.chain_overlap, fill=a.fill_thresh if a.fill else None)),
                  flush=True)
            continue
        for b in a.batches.split(","):
            E.set_option("gapped_greedy_batch", int(b))
            print(json.dumps(run(name, a.repeat, a.align, True, with_sel=False, pieces=a.pieces)), flush=True)
        E.reset_option("gapped_greedy_batch")


if __name__ == "__main__":
    main()
