"""The contract of sa_diff_alignments (include/segalign_amd.h) by plain column expansion: every span's op entries are
expanded into one op per column, every column gets its bases, class and kind, and the events are the maximal runs of one kind.

ref, qry: the resident codes (uint8; the low three bits are the code: A 0, C 1, G 2, T 3, soft-masked 4, N 5, X 6, separator 7)."""
import numpy as np

OP_M, OP_I, OP_D = 0, 1, 2
SUB, OTHER, INS, DEL, NONE = 0, 1, 2, 3, 4
MATCH, TS, TV, CLS_OTHER = 0, 1, 2, 3
NO_CODE = 8
DEFAULT_CHUNK = 4096

SPAN_DTYPE = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("op_offset", "<u8"), ("n_ops", "<u4"), ("pad", "<u4")])
EVENT_DTYPE = np.dtype([("span", "<u4"), ("ref_pos", "<u4"), ("query_pos", "<u4"), ("len", "<u4"), ("column", "<u4"), ("kind", "u1"),
                        ("tcode", "u1"), ("qcode", "u1"), ("pad", "u1")])
SUMMARY_DTYPE = np.dtype([("first_event", "<u8"), ("n_events", "<u4"), ("columns", "<u4"), ("matches", "<u4"), ("transitions", "<u4"),
                          ("transversions", "<u4"), ("others", "<u4"), ("ins_runs", "<u4"), ("ins_bases", "<u4"), ("del_runs", "<u4"),
                          ("del_bases", "<u4")])


def op(run, code):
    return (int(run) << 2) | int(code)


def make_spans(rows):
    """rows: (ref_start, query_start, op_offset, n_ops)."""
    sp = np.zeros(len(rows), dtype=SPAN_DTYPE)
    for k, r in enumerate(rows):
        sp[k]["ref_start"], sp[k]["query_start"], sp[k]["op_offset"], sp[k]["n_ops"] = r
    return sp


def pack(alignments):
    """alignments: (ref_start, query_start, [(run, code), ...]) -> (spans, ops), the op ranges behind each other."""
    rows, ops = [], []
    for rs, qs, runs in alignments:
        rows.append((rs, qs, len(ops), len(runs)))
        ops += [op(r, c) for r, c in runs]
    return make_spans(rows), np.array(ops, dtype=np.uint32)


def classes(x, y):
    """The class of every pair of codes."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    c = np.where((x ^ y) == 2, TS, TV)
    c = np.where(x == y, MATCH, c)
    return np.where((x >= 4) | (y >= 4), CLS_OTHER, c)


def columns(ref, qry, span, ops):
    """One span column by column: -> (op, ref base index, query base index, tcode, qcode, kind); tcode / qcode are NO_CODE on a side the
    column does not consume, and the base index there is that of the next base."""
    o = np.asarray(ops[int(span["op_offset"]):int(span["op_offset"]) + int(span["n_ops"])], dtype=np.int64)
    col = np.repeat(o & 3, o >> 2)
    ts, qs = (col != OP_I).astype(np.int64), (col != OP_D).astype(np.int64)
    r = int(span["ref_start"]) + np.cumsum(ts) - ts
    q = int(span["query_start"]) + np.cumsum(qs) - qs
    tc, qc = np.full(col.size, NO_CODE, dtype=np.int64), np.full(col.size, NO_CODE, dtype=np.int64)
    tc[ts == 1] = ref[r[ts == 1]] & 7
    qc[qs == 1] = qry[q[qs == 1]] & 7
    kind = np.where(col == OP_I, INS, DEL)
    m = col == OP_M
    cls = classes(tc[m], qc[m])
    kind[m] = np.where(cls == MATCH, NONE, np.where(cls == CLS_OTHER, OTHER, SUB))
    return col, r, q, tc, qc, kind


def diff(ref, qry, spans, ops, per_base=False):
    """-> (events, summaries, pairs): what sa_diff_alignments returns without SA_DIFF_NO_EVENTS, pairs as 64 counts."""
    ref, qry = np.asarray(ref), np.asarray(qry)
    events, sums = [], np.zeros(len(spans), dtype=SUMMARY_DTYPE)
    pairs = np.zeros(64, dtype=np.uint64)
    for k, sp in enumerate(spans):
        col, r, q, tc, qc, kind = columns(ref, qry, sp, ops)
        s = sums[k]
        s["first_event"] = len(events)
        s["columns"] = col.size
        if col.size:
            m = col == OP_M
            cls = classes(tc[m], qc[m])
            pairs += np.bincount(tc[m] * 8 + qc[m], minlength=64).astype(np.uint64)[:64]
            s["matches"], s["transitions"] = int((cls == MATCH).sum()), int((cls == TS).sum())
            s["transversions"], s["others"] = int((cls == TV).sum()), int((cls == CLS_OTHER).sum())
            s["ins_bases"], s["del_bases"] = int((col == OP_I).sum()), int((col == OP_D).sum())
            first = np.ones(col.size, dtype=bool)  # the first column of a run of one kind
            first[1:] = kind[1:] != kind[:-1]
            runs = np.flatnonzero(first)
            s["ins_runs"], s["del_runs"] = int((kind[runs] == INS).sum()), int((kind[runs] == DEL).sum())
            if per_base:
                first |= kind == SUB
                runs = np.flatnonzero(first)
            ends = np.append(runs[1:], col.size)
            for a, e in zip(runs.tolist(), ends.tolist()):
                if kind[a] != NONE:
                    events.append((k, r[a], q[a], e - a, a, kind[a], tc[a], qc[a], 0))
        s["n_events"] = len(events) - int(s["first_event"])
    return np.array(events, dtype=EVENT_DTYPE), sums, pairs


def work_items(spans, ops, chunk=0):
    """The work items of a call: an M entry of run L is ceil(L / chunk) of them, a gap entry one."""
    c = chunk or DEFAULT_CHUNK
    n = 0
    for sp in spans:
        o = np.asarray(ops[int(sp["op_offset"]):int(sp["op_offset"]) + int(sp["n_ops"])], dtype=np.int64)
        n += int(np.where((o & 3) == OP_M, ((o >> 2) + c - 1) // c, 1).sum())
    return n


KIND_NAME = ("sub", "other", "ins", "del")
CODE = np.full(256, 6, dtype=np.uint8)  # the engine's codes of sequence letters
for _k, _c in enumerate(b"ACGT"):
    CODE[_c] = _k
CODE[list(b"acgt")] = 4
CODE[list(b"nN")] = 5
CODE[ord("&")] = 7


def maf_blocks(text):
    """The blocks of a MAF file without header as segalign_host writes it: -> [(tname, tstart, ttext, qname, strand, qstart, qtext)]."""
    out, rows = [], []
    for line in text.splitlines():
        if line.startswith("s "):
            rows.append(line.split())
        if len(rows) == 2:
            (_, tn, ts, _, _, _, tt), (_, qn, qs, _, st, _, qt) = rows
            out.append((tn, int(ts), tt, qn, st, int(qs), qt))
            rows = []
    return out


def render_maf(text, per_base=False):
    """The .diff file segalign_host --gpu_diff writes beside a .maf file, from the MAF text alone: every block's two
    rows give its bases and its ops, and the model gives its events."""
    out = []
    for k, (tn, ts, tt, qn, st, qs, qt) in enumerate(maf_blocks(text)):
        assert len(tt) == len(qt)
        col = np.array([OP_I if a == "-" else OP_D if b == "-" else OP_M for a, b in zip(tt, qt)], dtype=np.int64)
        cut = np.flatnonzero(np.concatenate([[True], col[1:] != col[:-1]])) if col.size else np.zeros(0, dtype=np.int64)
        runs = [(int(e - a), int(col[a])) for a, e in zip(cut, np.append(cut[1:], col.size))]
        tb, qb = tt.replace("-", ""), qt.replace("-", "")
        spans, ops = pack([(0, 0, runs)])
        ev, sm, _ = diff(CODE[np.frombuffer(tb.encode(), dtype=np.uint8)], CODE[np.frombuffer(qb.encode(), dtype=np.uint8)], spans, ops, per_base)
        s = sm[0]
        out.append("#a %d %s %d %s %s %d columns=%d matches=%d transitions=%d transversions=%d others=%d ins=%d/%d del=%d/%d events=%d identity=%d/%d\n"
                   % (k, tn, ts, qn, st, qs, s["columns"], s["matches"], s["transitions"], s["transversions"], s["others"], s["ins_runs"],
                      s["ins_bases"], s["del_runs"], s["del_bases"], s["n_events"], s["matches"], s["columns"]))
        for e in ev:
            out.append("%s\t%s\t%d\t%s\t%s\t%d\t%d\t%s\t%s\n" % (KIND_NAME[e["kind"]], tn, ts + e["ref_pos"], qn, st, qs + e["query_pos"], e["len"],
                                                               "-" if e["kind"] == INS else tb[e["ref_pos"]], "-" if e["kind"] == DEL else qb[e["query_pos"]]))
    return "".join(out)
