"""The gapped-extension checker (tests/cpp/gapped_check.c) through ctypes, and the selection rules of sa_gapped_extend in Python.

The C file is compiled with the system C compiler into a temporary directory the first time it is needed."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "gapped_check.c")
GAPPED_DTYPE = np.dtype([("ref_start", "<u4"), ("ref_end", "<u4"), ("query_start", "<u4"), ("query_end", "<u4"), ("score", "<i4"),
                         ("hsp_index", "<u4"), ("flags", "<u4"), ("cells", "<u4")])
SEG_DTYPE = np.dtype([("ref_start", "<u4"), ("query_start", "<u4"), ("len", "<u4"), ("score", "<i4")])
EXTENT_CAP, BAND_CAP = 1, 2
DEFAULT_EXTENT, DEFAULT_BAND = 65536, 1024
# the engine's default matrix (HOXD70 over A C G T; L = soft-masked, N, X, E = separator), as sa_initialize_processor gets it
SUB = np.array([
    [91, -114, -31, -123, -1000, -1000, -100, -9100],
    [-114, 100, -125, -31, -1000, -1000, -100, -9100],
    [-31, -125, 100, -114, -1000, -1000, -100, -9100],
    [-123, -31, -114, 91, -1000, -1000, -100, -9100],
    [-1000] * 7 + [-9100],
    [-1000] * 7 + [-9100],
    [-100, -100, -100, -100, -1000, -1000, -100, -9100],
    [-9100] * 8], dtype=np.int32).reshape(64)

_lib = None


class SideResult(C.Structure):
    _fields_ = [("best", C.c_int32), ("best_i", C.c_int32), ("best_j", C.c_int32), ("cells", C.c_uint32), ("flags", C.c_uint32)]


def lib():
    global _lib
    if _lib is None:
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        d = tempfile.mkdtemp(prefix="gapped_check_")
        so = os.path.join(d, "libgapped_check.so")
        subprocess.check_call([cc, "-O2", "-std=c99", "-Wall", "-shared", "-fPIC", SRC, "-o", so])
        L = C.CDLL(so)
        L.gc_side.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SideResult)]
        L.gc_extend.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def side(t, q, sub, ar, aq, direction, gap_open=400, gap_extend=30, ydrop=9430, max_extent=DEFAULT_EXTENT, max_band=DEFAULT_BAND):
    """One one-sided extension: -> (best, best_i, best_j, cells, flags)."""
    t, q = _u8(t), _u8(q)
    m = np.ascontiguousarray(sub, dtype=np.int32)
    r = SideResult()
    lib().gc_side(t.ctypes.data, t.size, q.ctypes.data, q.size, m.ctypes.data, int(ar), int(aq), int(direction), gap_open, gap_extend,
                  ydrop, max_extent, max_band, C.byref(r))
    return r.best, r.best_i, r.best_j, r.cells, r.flags


def extend(t, q, sub, hsps, gap_open=400, gap_extend=30, ydrop=9430, max_extent=0, max_band=0):
    """Raw records (one per HSP, input order) exactly as sa_gapped_extend(raw=1) must return them."""
    t, q = _u8(t), _u8(q)
    m = np.ascontiguousarray(sub, dtype=np.int32)
    h = np.ascontiguousarray(hsps, dtype=SEG_DTYPE)
    out = np.zeros(h.size, dtype=GAPPED_DTYPE)
    if h.size:
        lib().gc_extend(t.ctypes.data, t.size, q.ctypes.data, q.size, m.ctypes.data, h.ctypes.data, h.size, gap_open, gap_extend, ydrop,
                        max_extent or DEFAULT_EXTENT, max_band or DEFAULT_BAND, out.ctypes.data)
    return out


def select(raw, gappedthresh):
    """Selection mode: threshold, one record per identical extent (highest score, then lowest index), output order."""
    kept = [r for r in raw.tolist() if r[4] >= gappedthresh]
    best = {}
    for r in kept:
        key = (r[0], r[1], r[2], r[3])
        if key not in best or (r[4], -r[5]) > (best[key][4], -best[key][5]):
            best[key] = r
    rows = sorted(best.values(), key=lambda r: (r[2], r[0], r[3], r[1], -r[4], r[5]))
    return np.array(rows, dtype=GAPPED_DTYPE) if rows else np.zeros(0, dtype=GAPPED_DTYPE)
