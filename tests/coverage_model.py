"""numpy model of the repeat masker's post-processing (repeat_masker_src/seeder.cpp:153-188: uint8 coverage counters, runs of positions
with count >= M), independent of the oracle's loop and of the device's scans: a difference array, one cumsum, `& 0xFF`, run boundaries
by the diff of the covered mask.  Shared by tests/test_oracle_rm_coverage.py and tests/test_coverage_regimes.py (CPU: the oracle is held
to it) and tests/test_gpu_coverage_regimes.py (GPU: sa_rm_coverage_intervals is held to it).

The rules:
  * `len` is bases - 1: an HSP counts query_start .. query_start + len - 1; len == 0 counts nothing;
  * an HSP that runs past the block is CLIPPED to it (the reference indexes out of bounds there; the clipping is the project's rule,
    oracle/segalign_oracle.c): query_start < block_len counts [query_start, min(query_start + len, block_len)), a start at or past
    block_len counts nothing;
  * the counters are uint8: the depth compared with M is the true depth mod 256;
  * a run is written when the first uncovered position behind it is seen, and there is no flush after the loop: a run that covers the
    block's last position is never written (M == 0: the whole block is such a run)."""
import numpy as np


def clipped(hsps, block_len):
    """-> (start, end) int64 arrays of the half-open position ranges the HSPs count, the ones that count nothing left out"""
    s = np.asarray(hsps["query_start"], dtype=np.int64)
    n = np.asarray(hsps["len"], dtype=np.int64)
    keep = (n > 0) & (s < block_len)
    s = s[keep]
    return s, np.minimum(s + n[keep], block_len)


def true_depth(hsps, block_len):
    """the number of HSPs that count each position of the block, not reduced mod 256 (int64[block_len])"""
    s, e = clipped(hsps, block_len)
    d = np.bincount(s, minlength=block_len + 1) - np.bincount(e, minlength=block_len + 1)
    return np.cumsum(d)[:block_len]


def runs_of(depth, M):
    """[(query_start, len)] of the runs with (depth mod 256) >= M that a following uncovered position closes"""
    cov = ((depth & 0xFF) >= M).astype(np.int8)
    step = np.diff(cov, prepend=np.int8(0))
    starts = np.flatnonzero(step == 1)
    ends = np.flatnonzero(step == -1)  # the first uncovered position behind a run; the open last run has none (:168-186)
    return [(int(a), int(b - a)) for a, b in zip(starts[:ends.size], ends)]


def numpy_model(hsps, block_len, M):
    return runs_of(true_depth(hsps, block_len), M)
