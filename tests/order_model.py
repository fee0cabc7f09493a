"""The ordering stage (dedup.hip) restated in plain numpy, per segment, with every intermediate exposed.

The plain chain is the reference's stable_sort(hspComp) -> unique_copy(hspEqual) -> stable_sort(hspCompLastz), src/seed_filter.cu:47-108
and :776-782; the rm chain is the repeat masker's stable_sort(hspComp) -> unique_copy(hspEqual) -> stable_sort(hspDiagComp) ->
unique_copy(hspDiagEqual) -> stable_sort(hspFinalComp), repeat_masker_src/seed_filter.cu:45-135 and :819-831.  A stable sort is a stable
np.lexsort over the comparator's keys; unique_copy on the device is a head flag on adjacent INPUT pairs (hazard H3): record i of the
sorted list is kept iff i == 0 or not pred(sorted[i - 1], sorted[i]), whether or not record i - 1 was kept itself.

All arithmetic is the reference's: segmentPair holds three uint32 and an int, so `ref_start - query_start` and `ref_start + len` wrap at
2^32 and scores compare signed.  Nothing here shares code with oracle/segalign_oracle.c (comparison functions + merge sort + a loop);
tests/test_order_model.py holds the two equal."""
import numpy as np

SEG = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])


def diag(r):
    """ref_start - query_start as the reference computes it: uint32, wrapping"""
    return ((r["ref_start"].astype(np.int64) - r["query_start"].astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)


def end(r):
    """ref_start + len as the reference computes it: uint32, wrapping"""
    return ((r["ref_start"].astype(np.int64) + r["len"].astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)


def _asc(a):
    return a.astype(np.int64)


def _desc(a):
    return -a.astype(np.int64)


# comparator -> its keys, most significant first (every comparator is a lexicographic strict order on them)
KEYS = {
    "hspComp":      lambda r: (_asc(diag(r)), _asc(r["ref_start"]), _asc(r["len"]), _desc(r["score"])),           # src :54-80
    "hspCompLastz": lambda r: (_asc(r["query_start"]), _asc(r["ref_start"]), _asc(r["len"]), _desc(r["score"])),  # src :82-108
    "rmHspComp":    lambda r: (_asc(r["query_start"]), _desc(r["len"]), _asc(r["ref_start"]), _desc(r["score"])), # rm :109-135
    "hspDiagComp":  lambda r: (_asc(diag(r)), _asc(r["ref_start"]), _asc(r["query_start"]), _desc(r["score"])),   # rm :52-78
    "hspFinalComp": lambda r: (_asc(r["query_start"]), _desc(r["score"]), _desc(r["ref_start"])),                 # rm :87-107
}


def stable_sort(recs, comp):
    keys = KEYS[comp](recs)
    return recs[np.lexsort(keys[::-1])] if recs.size else recs.copy()


def contained(x, y):
    """hspEqual, src :47-52 == hspDiagEqual, rm :45-50, elementwise: same diagonal and one interval inside the other"""
    return (diag(x) == diag(y)) & (((x["ref_start"] >= y["ref_start"]) & (end(x) <= end(y))) |
                                   ((y["ref_start"] >= x["ref_start"]) & (end(y) <= end(x))))


def same(x, y):
    """the repeat masker's hspEqual, rm :80-85, elementwise"""
    return ((x["ref_start"] == y["ref_start"]) & (x["query_start"] == y["query_start"]) & (x["len"] == y["len"]) &
            (x["score"] == y["score"]))


PRED = {"hspEqual": contained, "hspDiagEqual": contained, "rmHspEqual": same}


def head_flags(srt, pred):
    """keep mask of unique_copy on the device: the verdict of record i rests on its input neighbour i - 1 alone"""
    keep = np.ones(srt.size, dtype=bool)
    if srt.size > 1:
        keep[1:] = ~PRED[pred](srt[:-1], srt[1:])
    return keep


PLAIN = (("hspComp", "hspEqual"), ("hspCompLastz", None))
RM = (("rmHspComp", "rmHspEqual"), ("hspDiagComp", "hspDiagEqual"), ("hspFinalComp", None))


def chain(recs, rm=False):
    """One dedup scope.  -> {"stages": [{"comp", "pred", "sorted", "keep"}, ...], "final"}; the last stage has pred None, keep all."""
    cur = np.ascontiguousarray(recs, dtype=SEG)
    stages = []
    for comp, pred in (RM if rm else PLAIN):
        srt = stable_sort(cur, comp)
        keep = head_flags(srt, pred) if pred else np.ones(srt.size, dtype=bool)
        stages.append({"comp": comp, "pred": pred, "sorted": srt, "keep": keep})
        cur = srt[keep]
    return {"stages": stages, "final": cur}


def order(recs, seg=None, nsegs=1, rm=False):
    """Every segment's chain on its own records (in input order), results concatenated by segment as a call returns them.
    -> {"records", "seg", "counts", "segments": [chain(...) per segment]}"""
    recs = np.ascontiguousarray(recs, dtype=SEG)
    seg = np.zeros(recs.size, dtype=np.uint32) if seg is None else np.asarray(seg, dtype=np.uint32)
    assert seg.shape == recs.shape and (seg.size == 0 or int(seg.max()) < nsegs)
    per = [chain(recs[seg == g], rm) for g in range(nsegs)]
    counts = np.array([c["final"].size for c in per], dtype=np.uint32)
    return {"records": np.concatenate([c["final"] for c in per]) if per else np.zeros(0, dtype=SEG),
            "seg": np.repeat(np.arange(nsegs, dtype=np.uint32), counts), "counts": counts, "segments": per}


def global_stages(recs, seg, nsegs, rm=False):
    """The library chain's own view: ONE sorted list per stage with the segment as the major key, and its keep mask with the segment test
    (a record whose input neighbour lies in another segment is kept).  Equal to the per-segment stages laid end to end; the positions in
    these lists are the ones the unique kernels' thread, wave and tile edges refer to."""
    m = order(recs, seg, nsegs, rm)
    out = []
    for k in range(len(RM if rm else PLAIN)):
        out.append({"sorted": np.concatenate([c["stages"][k]["sorted"] for c in m["segments"]]),
                    "keep": np.concatenate([c["stages"][k]["keep"] for c in m["segments"]]),
                    "seg": np.repeat(np.arange(nsegs, dtype=np.uint32), [c["stages"][k]["sorted"].size for c in m["segments"]])})
    return out
