"""The link checker (tests/cpp/stitch_check.c) through ctypes, and sa_stitch_chains's records, ops and links assembled from it in
numpy: the contract of include/segalign_amd.h / DESIGN.md 17, restated.

The C file is compiled with the system C compiler into a temporary directory the first time it is needed."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "stitch_check.c")
SEG_DTYPE = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])
RECORD_DTYPE = np.dtype([("chain", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"), ("flags", "<u4"), ("ref_start", "<u4"),
                         ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"), ("score", "<i8"), ("op_offset", "<u8"),
                         ("n_ops", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"), ("gap_opens", "<u4"), ("gap_bases", "<u4"),
                         ("pad", "<u4")])
LINK_DTYPE = np.dtype([("chain", "<u4"), ("member", "<u4"), ("dt", "<u4"), ("dq", "<u4"), ("score", "<i4"), ("flags", "<u4"),
                       ("cells", "<u8")])
OP_M, OP_I, OP_D = 0, 1, 2
LONG, DEAD, LOW = 1, 2, 4
NEVER = -(1 << 31)
MAX_LINK = 2048
RUN_MAX = (1 << 30) - 1
INSTANCES = (2, 4, 8, 17, 33)

_lib = None


class Link(C.Structure):
    _fields_ = [("score", C.c_int32), ("dead", C.c_int32), ("n_ops", C.c_uint32), ("matches", C.c_uint32), ("mismatches", C.c_uint32),
                ("gap_opens", C.c_uint32), ("gap_bases", C.c_uint32), ("rescore", C.c_int32), ("err", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        d = tempfile.mkdtemp(prefix="stitch_check_")
        so = os.path.join(d, "libstitch_check.so")
        subprocess.check_call([cc, "-O2", "-std=c99", "-Wall", "-shared", "-fPIC", SRC, "-o", so])
        L = C.CDLL(so)
        L.sc_align.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(Link)]
        L.sc_align.restype = None
        _lib = L
    return _lib


def link(x, y, sub, gap_open=400, gap_extend=30):
    """One link on the target codes x and query codes y: -> (dict of the checker's result, ops in genome order)."""
    x, y = np.ascontiguousarray(x, dtype=np.uint8), np.ascontiguousarray(y, dtype=np.uint8)
    m = np.ascontiguousarray(sub, dtype=np.int32)
    assert m.size == 64
    ops = np.zeros(x.size + y.size + 1, dtype=np.uint32)
    r = Link()
    lib().sc_align(x.ctypes.data, x.size, y.ctypes.data, y.size, m.ctypes.data, int(gap_open), int(gap_extend), ops.ctypes.data, C.byref(r))
    res = {k: getattr(r, k) for k, _ in Link._fields_}
    assert res["err"] == 0, res
    if not res["dead"]:
        assert res["rescore"] == res["score"], res
    return res, ops[:r.n_ops].copy()


def instance(dt):
    """K of the sweep instance a link of dt target bases runs on: the smallest with 64 K >= dt + 1."""
    return next(k for k in INSTANCES if 64 * k >= dt + 1)


def make(rows):
    """[(ref_start, query_start, len, score), ...] -> SEG_DTYPE."""
    return np.array([tuple(r) for r in rows], dtype=SEG_DTYPE)


def csr(chains):
    """[[hsp index, ...], ...] -> (members, first)."""
    members = np.array([i for c in chains for i in c], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.uint32)
    return members, first


def _merge(runs, ln, op):
    if ln == 0:
        return
    if runs and runs[-1][1] == op:
        runs[-1][0] += ln
    else:
        runs.append([ln, op])


def stitch(t, q, sub, hsps, members, first, gap_open=400, gap_extend=30, max_link=0, min_link_score=None):
    """sa_stitch_chains on the target codes t and the query strand's codes q: -> (records, ops, links, counts)."""
    t, q = np.asarray(t, dtype=np.uint8), np.asarray(q, dtype=np.uint8)
    sub = np.asarray(sub, dtype=np.int64).reshape(64)
    h = np.asarray(hsps, dtype=SEG_DTYPE)
    max_link = max_link or MAX_LINK
    floor = NEVER if min_link_score is None else min_link_score
    assert max_link <= MAX_LINK
    recs, ops, links = [], [], []
    cache = {}
    for c in range(len(first) - 1):
        mem = [h[int(i)] for i in members[int(first[c]):int(first[c + 1])]]
        rs = [int(m["ref_start"]) for m in mem]
        qs = [int(m["query_start"]) for m in mem]
        n = [int(m["len"]) + 1 for m in mem]
        for a, b, k in zip(rs, qs, n):
            assert a + k <= t.size and b + k <= q.size, "a member outside the block"
        p = 0
        while p < len(mem):
            rec = dict(chain=c, first_member=p, n_members=0, flags=0, ref_start=rs[p], query_start=qs[p], score=0, matches=0, mismatches=0)
            runs = []
            while True:
                a, b = t[rs[p]:rs[p] + n[p]].astype(np.int64), q[qs[p]:qs[p] + n[p]].astype(np.int64)
                rec["score"] += int(sub[a * 8 + b].sum())
                eq = int(np.count_nonzero((a == b) & (a < 4)))
                rec["matches"] += eq
                rec["mismatches"] += n[p] - eq
                rec["n_members"] += 1
                rec["ref_end"], rec["query_end"] = rs[p] + n[p], qs[p] + n[p]
                _merge(runs, n[p], OP_M)
                if p + 1 == len(mem):
                    break
                re_, qe_ = rs[p] + n[p], qs[p] + n[p]
                dt, dq = rs[p + 1] - re_, qs[p + 1] - qe_
                assert dt >= 0 and dq >= 0, "members that are not collinear"
                lk = dict(chain=c, member=p, dt=dt, dq=dq, score=0, flags=0, cells=0)
                lops = None
                if dt > max_link or dq > max_link:
                    lk["flags"] = LONG
                else:
                    lk["cells"] = (dt + 1) * (dq + 1)
                    key = (re_, qe_, dt, dq)
                    if key not in cache:
                        cache[key] = link(t[re_:re_ + dt], q[qe_:qe_ + dq], sub, gap_open, gap_extend)
                    res, lops = cache[key]
                    if res["dead"]:
                        lk["flags"], lk["score"] = DEAD, NEVER
                    else:
                        lk["score"] = res["score"]
                        if res["score"] < floor:
                            lk["flags"] = LOW
                links.append(lk)
                if lk["flags"]:
                    rec["flags"] = lk["flags"]
                    break
                rec["score"] += res["score"]
                rec["matches"] += res["matches"]
                rec["mismatches"] += res["mismatches"]
                for o in lops.tolist():
                    _merge(runs, o >> 2, o & 3)
                p += 1
            p += 1
            rec["op_offset"] = len(ops)
            rec["gap_opens"] = sum(1 for ln, op in runs if op != OP_M)
            rec["gap_bases"] = sum(ln for ln, op in runs if op != OP_M)
            for ln, op in runs:
                while ln:
                    piece = min(ln, RUN_MAX)
                    ops.append(piece << 2 | op)
                    ln -= piece
            rec["n_ops"] = len(ops) - rec["op_offset"]
            recs.append(rec)
    R = np.zeros(len(recs), dtype=RECORD_DTYPE)
    for k, r in enumerate(recs):
        for f, v in r.items():
            R[k][f] = v
    Lk = np.zeros(len(links), dtype=LINK_DTYPE)
    for k, r in enumerate(links):
        for f, v in r.items():
            Lk[k][f] = v
    counts = dict(links=len(links), swept=int(np.count_nonzero(Lk["flags"] != LONG)), long_links=int(np.count_nonzero(Lk["flags"] == LONG)),
                  dead_links=int(np.count_nonzero(Lk["flags"] == DEAD)), low_links=int(np.count_nonzero(Lk["flags"] == LOW)),
                  cells=int(Lk["cells"].sum()), records=len(recs))
    return R, np.array(ops, dtype=np.uint32), Lk, counts


def record_ops(recs, ops, k):
    o = int(recs[k]["op_offset"])
    return ops[o:o + int(recs[k]["n_ops"])]


def consumed(ops):
    """(target bases, query bases) the runs consume."""
    ln, op = (ops >> 2).astype(np.int64), ops & 3
    return int(ln[op != OP_I].sum()), int(ln[op != OP_D].sum())


def rescore(t, q, sub, r0, q0, ops, gap_open, gap_extend):
    """Score of a run list in genome order from target r0, query q0: sub over the M pairs minus O + k E per gap run (runs that a cut
    at RUN_MAX split count once)."""
    sub = np.asarray(sub, dtype=np.int64).reshape(64)
    s, i, j, prev = 0, r0, q0, -1
    for x in ops.tolist():
        ln, op = x >> 2, x & 3
        if op == OP_M:
            a, b = t[i:i + ln].astype(np.int64), q[j:j + ln].astype(np.int64)
            s += int(sub[a * 8 + b].sum())
            i += ln
            j += ln
        else:
            s -= (gap_open if op != prev else 0) + ln * gap_extend
            if op == OP_I:
                j += ln
            else:
                i += ln
        prev = op
    return s


def check_invariants(t, q, sub, recs, ops, gap_open=400, gap_extend=30):
    """What the contract promises of every record, whoever computed it."""
    total = 0
    for k in range(recs.size):
        r = recs[k]
        assert int(r["op_offset"]) == total
        total += int(r["n_ops"])
        o = record_ops(recs, ops, k)
        ln, op = o >> 2, o & 3
        assert np.all(ln > 0) and np.all(op <= 2)
        same = np.flatnonzero(op[1:] == op[:-1])
        assert np.all(ln[same] == RUN_MAX), "equal neighbours anywhere but at a cut"
        assert consumed(o) == (int(r["ref_end"]) - int(r["ref_start"]), int(r["query_end"]) - int(r["query_start"]))
        assert rescore(t, q, sub, int(r["ref_start"]), int(r["query_start"]), o, gap_open, gap_extend) == int(r["score"])
    assert total == ops.size
