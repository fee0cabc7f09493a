#!/usr/bin/env python3
"""kernel_ms (sa_chain_stats: rank, DP and finish kernels) of engine.ChainHsps on synthetic HSPs that overlap the way HSPs on the two
sides of an indel do: pieces of 20 .. 60 bases whose starts lie about 30 apart on two close diagonals, one group, shuffled.  Per size
and cost table the plain DP and, unless --plain-only, the DP under --max-overlap run alternating --repeat + 1 times on the same HSPs
(the first of each is a warm-up); one JSON document with the sorted times, the medians' ratio, and members, score and pairs of each.

--tree DIR takes the package (and its built library) from another checkout of this repository, for an A/B of the plain entries
across two trees: run the tool once per tree, alternating, as separate processes (profiles/r26_chain_overlap/commands.txt).  That
other checkout is the caller's to make; no test and nothing else in the repository needs one."""
import argparse
import json
import os
import sys

import numpy as np


def hsps(E, n, rng):
    k = np.arange(n)
    q = 1000 + k * 30 + rng.integers(0, 30, n)
    h = np.zeros(n, dtype=E.SEG_DTYPE)
    h["query_start"] = q
    h["ref_start"] = q + 20000 + rng.integers(0, 2, n) * 7 + rng.integers(0, 3, n)
    h["len"] = rng.integers(19, 60, n)
    h["score"] = rng.integers(300, 4000, n)
    return h[rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=None)
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-overlap", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from segalign_amd import engine as E
    E.InitializeInterface(1)
    rng = np.random.default_rng(1)
    out = {"tree": a.tree or "this tree"}
    for n in (int(x) for x in a.sizes.split(",")):
        h = hsps(E, n, rng)
        for costs in (None, "loose"):
            runs = [("plain", {})] + ([] if a.plain_only else [("overlap", {"max_overlap": a.max_overlap})])
            ms, res = {name: [] for name, _ in runs}, {}
            for rep in range(a.repeat + 1):
                for name, kw in runs:
                    m, st = E.ChainHsps(h, None, gap_costs=costs, **kw)
                    if rep:
                        ms[name].append(round(st["kernel_ms"], 3))
                    res[name] = {"members": int(m.size), "score": int(m["f"][-1]), "pairs": int(st["pair_evals"])}
            row = {name: dict(res[name], ms=sorted(ms[name]), median_ms=float(np.median(ms[name]))) for name, _ in runs}
            if not a.plain_only:
                row["overlap_over_plain"] = round(row["overlap"]["median_ms"] / row["plain"]["median_ms"], 4)
            out["n=%d costs=%s" % (n, costs)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
