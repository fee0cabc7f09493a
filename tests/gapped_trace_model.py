"""The path checker (tests/cpp/gapped_trace_check.c) through ctypes, records and paths of sa_gapped_align built from it, the path
invariants, and a MAF model.

The C file is compiled with the system C compiler into a temporary directory the first time it is needed."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import gapped_model as G

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "gapped_trace_check.c")
PATH_DTYPE = np.dtype([("op_offset", "<u8"), ("n_left", "<u4"), ("n_right", "<u4"), ("matches", "<u4"), ("mismatches", "<u4"),
                       ("gap_opens", "<u4"), ("gap_bases", "<u4")])
OP_M, OP_I, OP_D = 0, 1, 2

_libs = {}


class SideResult(C.Structure):
    _fields_ = [("best", C.c_int32), ("best_i", C.c_int32), ("best_j", C.c_int32), ("cells", C.c_uint32), ("flags", C.c_uint32)]


class Walk(C.Structure):
    _fields_ = [("n_ops", C.c_uint32), ("matches", C.c_uint32), ("mismatches", C.c_uint32), ("gap_opens", C.c_uint32),
                ("gap_bases", C.c_uint32), ("score", C.c_int32), ("err", C.c_int32)]


def lib(variant=0):
    """The checker; variant != 0: the deliberately wrong build GT_VARIANT = variant (see the C file), for tie-sensitivity checks only."""
    if variant not in _libs:
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        d = tempfile.mkdtemp(prefix="gapped_trace_check_")
        so = os.path.join(d, "libgapped_trace_check.so")
        subprocess.check_call([cc, "-O2", "-std=c99", "-Wall", "-shared", "-fPIC", "-DGT_VARIANT=%d" % variant, SRC, "-o", so])
        L = C.CDLL(so)
        L.gt_side.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SideResult), C.c_void_p, C.POINTER(Walk)]
        _libs[variant] = L
    return _libs[variant]


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def side(t, q, sub, ar, aq, direction, gap_open=400, gap_extend=30, ydrop=9430, max_extent=G.DEFAULT_EXTENT, max_band=G.DEFAULT_BAND,
         variant=0):
    """One side: -> ((best, best_i, best_j, cells, flags), ops in walk order (uint32 array), walk dict)."""
    t, q = _u8(t), _u8(q)
    m = np.ascontiguousarray(sub, dtype=np.int32)
    r, w = SideResult(), Walk()
    ops = np.zeros(2 * max_extent + 2, dtype=np.uint32)
    lib(variant).gt_side(t.ctypes.data, t.size, q.ctypes.data, q.size, m.ctypes.data, int(ar), int(aq), int(direction), gap_open, gap_extend,
                         ydrop, max_extent, max_band, C.byref(r), ops.ctypes.data, C.byref(w))
    walk = {k: getattr(w, k) for k, _ in Walk._fields_}
    assert walk["err"] == 0, walk
    return (r.best, r.best_i, r.best_j, r.cells, r.flags), ops[:w.n_ops].copy(), walk


def align(t, q, sub, hsps, gap_open=400, gap_extend=30, ydrop=9430, max_extent=0, max_band=0):
    """Raw records (as gapped_model.extend) and, per record, (left ops, right ops in genome order, path counts)."""
    kw = dict(gap_open=gap_open, gap_extend=gap_extend, ydrop=ydrop, max_extent=max_extent or G.DEFAULT_EXTENT,
              max_band=max_band or G.DEFAULT_BAND)
    h = np.ascontiguousarray(hsps, dtype=G.SEG_DTYPE)
    recs = np.zeros(h.size, dtype=G.GAPPED_DTYPE)
    paths = []
    for k, (rs, qs, ln, _) in enumerate(h.tolist()):
        ar, aq = rs + ln // 2, qs + ln // 2
        (lb, li, lj, lc, lf), lops, lw = side(t, q, sub, ar, aq, -1, **kw)
        (rb, ri, rj, rc, rf), rops, rw = side(t, q, sub, ar, aq, +1, **kw)
        recs[k] = (ar - li, ar + ri, aq - lj, aq + rj, lb + rb, k, lf | rf, lc + rc)
        counts = {c: lw[c] + rw[c] for c in ("matches", "mismatches", "gap_opens", "gap_bases")}
        paths.append((lops, rops[::-1].copy(), counts))
    return recs, paths


def select(raw, paths, gappedthresh):
    """Selection mode: the records of gapped_model.select and their paths (each record's is that of its hsp_index)."""
    sel = G.select(raw, gappedthresh)
    return sel, [paths[int(r["hsp_index"])] for r in sel]


def pack(paths):
    """Paths as sa_gapped_align returns them: (PATH_DTYPE array, concatenated ops)."""
    pa = np.zeros(len(paths), dtype=PATH_DTYPE)
    ops, off = [], 0
    for k, (lo, ro, c) in enumerate(paths):
        pa[k] = (off, lo.size, ro.size, c["matches"], c["mismatches"], c["gap_opens"], c["gap_bases"])
        ops += [lo, ro]
        off += lo.size + ro.size
    return pa, (np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, dtype=np.uint32))


def record_ops(paths, ops, k):
    """(left ops, right ops) of record k from sa_gapped_align's outputs."""
    p = paths[k]
    o = int(p["op_offset"])
    nl, nr = int(p["n_left"]), int(p["n_right"])
    return ops[o:o + nl], ops[o + nl:o + nl + nr]


def consumed(ops):
    """(target bases, query bases) the runs consume."""
    ln, op = ops >> 2, ops & 3
    return int(ln[op != OP_I].sum()), int(ln[op != OP_D].sum())


def canonical(ops):
    ln, op = ops >> 2, ops & 3
    return bool(np.all(ln > 0) and np.all(op <= 2) and np.all(op[1:] != op[:-1]))


def rescore(t, q, sub, r0, q0, ops, gap_open, gap_extend):
    """Score of a run list in genome order starting at target r0, query q0 (codes), and (matches, mismatches)."""
    s, i, j, mt, mm = 0, r0, q0, 0, 0
    for x in ops.tolist():
        ln, op = x >> 2, x & 3
        if op == OP_M:
            a, b = t[i:i + ln].astype(np.int64), q[j:j + ln].astype(np.int64)
            s += int(sub[a * 8 + b].sum())
            eq = int(np.count_nonzero((a == b) & (a < 4)))
            mt += eq
            mm += ln - eq
            i += ln
            j += ln
        else:
            s -= gap_open + ln * gap_extend
            if op == OP_I:
                j += ln
            else:
                i += ln
    return s, mt, mm


def maf_texts(tseq, qseq, r0, q0, ops):
    """The two text rows of an alignment: target and query characters with '-' in the gaps."""
    a, b, i, j = [], [], r0, q0
    for x in ops.tolist():
        ln, op = x >> 2, x & 3
        if op == OP_M:
            a.append(tseq[i:i + ln]); b.append(qseq[j:j + ln]); i += ln; j += ln
        elif op == OP_I:
            a.append("-" * ln); b.append(qseq[j:j + ln]); j += ln
        else:
            a.append(tseq[i:i + ln]); b.append("-" * ln); i += ln
    return "".join(a), "".join(b)
