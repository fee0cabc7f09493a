"""The contract of sa_fill_chains (include/segalign_amd.h): the scan checker (tests/cpp/fill_check.c) through ctypes, a
direct Python restatement of the scan for small rectangles, the choice of a link's fill by hsp_chain_gap_model.chain (which is
hsp_chain_model.chain without a table), and the assembly of the filled chains.  t and q are the codes of the resident target block and
query strand.  Written from the header, not from the kernel.

The C file is compiled with the system C compiler into a temporary directory the first time it is needed."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import hsp_chain_gap_model as G
import hsp_chain_model as M
import hsp_chain_overlap_model as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "fill_check.c")
CHAIN = np.dtype([("score", "<i8"), ("fills", "<u4"), ("fill_bases", "<u4")])
LINK = np.dtype([("dt", "<u4"), ("dq", "<u4"), ("flags", "<u4"), ("n_hsps", "<u4"), ("n_fill", "<u4"), ("pad", "<u4"), ("cells", "<u8")])
HSP = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4"), ("link", "<u4"), ("pad", "<u4")])
FC_HSP = np.dtype([("i", "<u4"), ("j", "<u4"), ("len", "<u4"), ("score", "<i4")])
LONG, LARGE, CROWDED = 1, 2, 4
NONE = 0xFFFFFFFF
DEFAULTS = dict(thresh=3000, xdrop=910, max_side=32768, max_cells=1 << 30, max_link_hsps=65536)
SEP = 7

_lib = None


def lib():
    global _lib
    if _lib is None:
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        d = tempfile.mkdtemp(prefix="fill_check_")
        so = os.path.join(d, "libfill_check.so")
        subprocess.check_call([cc, "-O2", "-std=c99", "-Wall", "-shared", "-fPIC", SRC, "-o", so])
        L = C.CDLL(so)
        L.fc_scan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64]
        L.fc_scan.restype = C.c_uint64
        _lib = L
    return _lib


def scan(x, y, sub, thresh, xdrop):
    """The checker on the target codes x and query codes y of one rectangle: -> FC_HSP records in the contract's order."""
    x, y = np.ascontiguousarray(x, dtype=np.uint8), np.ascontiguousarray(y, dtype=np.uint8)
    m = np.ascontiguousarray(sub, dtype=np.int32)
    assert m.size == 64
    cap = 1024
    while True:
        out = np.zeros(cap, dtype=FC_HSP)
        n = int(lib().fc_scan(x.ctypes.data, x.size, y.ctypes.data, y.size, m.ctypes.data, thresh, xdrop, out.ctypes.data, cap))
        if n <= cap:
            return out[:n].copy()
        cap = n


def scan_py(x, y, sub, thresh, xdrop):
    """The scan of the header, clause by clause, in Python integers: -> [(i, j, len, score)] in the contract's order."""
    m = [int(v) for v in np.asarray(sub).reshape(64)]
    dt, dq = len(x), len(y)
    found = []
    for d in range(-(dq - 1), dt):
        i0, j0 = max(d, 0), max(-d, 0)
        n = min(dt - i0, dq - j0)
        s = b = start = bend = 0

        def flush():
            if b >= thresh:
                found.append((i0 + start, j0 + start, bend - start, b))

        for k in range(n):
            a, c = int(x[i0 + k]) & 7, int(y[j0 + k]) & 7
            if a == SEP or c == SEP:  # clause 1
                flush()
                s = b = 0
                continue
            if s == 0 and b == 0:  # 2
                start = k
            s += m[a * 8 + c]  # 3
            if s > b:  # 4
                b, bend = s, k
            if s <= 0 or b - s > xdrop:  # 5
                flush()
                s = b = 0
        flush()  # 6
    return found


def validate(t, q, sub, hsps, members, first, max_side):
    """The contract's checks; ValueError names the clause that fails."""
    h = np.asarray(hsps, dtype=M.SEG)
    if len(first) - 1 > 1 << 22 or (len(first) > 1 and (first[0] != 0 or any(first[c + 1] < first[c] for c in range(len(first) - 1)))):
        raise ValueError("first")
    big = max(abs(int(v)) for v in np.asarray(sub).reshape(8, 8)[:7, :7].ravel())
    if max_side > 1 << 20 or max_side * big >= 1 << 31:
        raise ValueError("headroom")
    for m in members:
        if m >= h.size:
            raise ValueError("not in the input")
        r, s, b, _ = O.node(h, int(m))
        if r + b > len(t) or s + b > len(q):
            raise ValueError("inside the block")
    for c in range(len(first) - 1):
        for k in range(int(first[c]), int(first[c + 1]) - 1):
            if not M.precedes(h, None, int(members[k]), int(members[k + 1])):
                raise ValueError("overlaps")


def fill(t, q, sub, hsps, members, first, thresh=3000, xdrop=910, diag_pen=0, anti_pen=0, max_gap=0, gap_costs=None, min_fill=0, max_side=0,
         max_cells=0, max_link_hsps=0):
    """-> (M.SEG entries of the filled chains, uint32 first_out, uint32 origin, CHAIN chains, LINK links, HSP found HSPs)."""
    h = np.asarray(hsps, dtype=M.SEG)
    max_side, max_cells = max_side or DEFAULTS["max_side"], max_cells or DEFAULTS["max_cells"]
    max_link_hsps = max_link_hsps or DEFAULTS["max_link_hsps"]
    if thresh < 1 or xdrop < 0 or max_cells > 1 << 36 or max_link_hsps > 1 << 22:
        raise ValueError("parameters")
    validate(t, q, sub, h, members, first, max_side)
    tab = G.validate(gap_costs) if gap_costs is not None else None
    out, origin, first_out, links, found = [], [], [0], [], []
    chains = np.zeros(len(first) - 1, dtype=CHAIN)
    for c in range(len(first) - 1):
        fills = bases = 0
        for k in range(int(first[c]), int(first[c + 1])):
            out.append(tuple(h[int(members[k])]))
            origin.append(int(members[k]))
            if k + 1 == int(first[c + 1]):
                break
            rj, qj, bj, _ = O.node(h, int(members[k]))
            ri, qi, _, _ = O.node(h, int(members[k + 1]))
            re, qe = rj + bj, qj + bj
            dt, dq = ri - re, qi - qe
            flags = n_hsps = n_fill = cells = 0
            if dt and dq:
                if dt > max_side or dq > max_side:
                    flags = LONG
                elif dt * dq > max_cells:
                    flags = LARGE
                else:
                    cells = dt * dq
                    got = scan(t[re:ri], q[qe:qi], sub, thresh, xdrop)
                    n_hsps = got.size
                    if n_hsps > max_link_hsps:
                        flags = CROWDED
                    elif n_hsps:
                        cand = np.zeros(n_hsps, dtype=M.SEG)
                        cand["ref_start"], cand["query_start"] = got["i"] + re, got["j"] + qe
                        cand["len"], cand["score"] = got["len"], got["score"]
                        for x in cand:
                            found.append(tuple(x) + (len(links), 0))
                        _, _, mem = G.chain(cand, None, diag_pen=diag_pen, anti_pen=anti_pen, max_gap=max_gap, min_score=min_fill,
                                            gap_costs=gap_costs)
                        n_fill = mem.size
                        for i in mem["hsp_index"]:
                            out.append(tuple(cand[int(i)]))
                            origin.append(NONE)
                            fills, bases = fills + 1, bases + int(cand["len"][int(i)]) + 1
            links.append((dt, dq, flags, n_hsps, n_fill, 0, cells))
        first_out.append(len(out))
        chains[c]["fills"], chains[c]["fill_bases"] = fills, bases
    res = np.array(out, dtype=M.SEG) if out else np.zeros(0, dtype=M.SEG)
    for c in range(len(first) - 1):
        a, b = first_out[c], first_out[c + 1]
        pen = sum(O.link_penalty(res, k, k + 1, diag_pen, anti_pen, tab) for k in range(a, b - 1))
        chains[c]["score"] = int(res["score"][a:b].astype(np.int64).sum()) - pen
    return (res, np.array(first_out, dtype=np.uint32), np.array(origin, dtype=np.uint32), chains,
            np.array(links, dtype=LINK) if links else np.zeros(0, dtype=LINK), np.array(found, dtype=HSP) if found else np.zeros(0, dtype=HSP))
