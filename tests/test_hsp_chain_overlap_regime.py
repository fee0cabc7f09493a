"""CPU: the overlap chaining model on the project's own host input, the `pair` of tests/test_gpu_host_chain.py (7 % substitutions, an
indel every 500 bases; the .segments files are the oracle's).  Without an allowance the best chains keep 37 of the plus file's 106
HSPs and 8 of the minus file's 55, because most neighbours across an indel share a few bases; with the host's default
allowance of 64 they must keep strictly more, through at least one overlapping link in each file."""
import numpy as np

import hsp_chain_model as M
import hsp_chain_overlap_model as O
from host_model import expected_outputs
from test_gpu_host_chain import file_hsps, pair  # noqa: F401  (pair: the fixture)

PLAIN = {"plus": 37, "minus": 8}  # members of the best chains today


def test_the_allowance_lengthens_the_best_chains_of_the_host_input(oracle, pair):
    _, _, _, t_recs, q_recs, R, Q = pair
    files, _ = expected_outputs(oracle, [(n, s.tobytes()) for n, s in t_recs], [(n, s.tobytes()) for n, s in q_recs], chunk=20000)
    seen = set()
    for f in sorted(x for x in files if x.endswith(".segments")):
        strand = "minus" if ".minus." in f else "plus"
        h, g = file_hsps(files[f], strand == "minus", R, Q)
        plain = M.chain(h, g)[2]
        assert plain.size == PLAIN[strand], (f, plain.size)
        f0, p0, m0 = O.chain(h, g, max_overlap=0)
        assert np.array_equal(m0, plain)
        _, _, members = O.chain(h, g, max_overlap=64)
        links = [(int(members["hsp_index"][k - 1]), int(members["hsp_index"][k])) for k in range(1, members.size)
                 if members["group"][k] == members["group"][k - 1]]
        overlapping = [O.overlap(h, j, i) for j, i in links if O.overlap(h, j, i) > 0]
        assert members.size > PLAIN[strand] and len(overlapping) >= 1, (f, members.size, len(overlapping))
        assert all(O.precedes(h, g, j, i, 64) for j, i in links) and max(overlapping) <= 64
        for grp in np.unique(plain["group"]):  # a chain without overlaps stays valid at the same value: no group's chain scores less
            assert members["f"][members["group"] == grp][-1] >= plain["f"][plain["group"] == grp][-1]
        seen.add(strand)
    assert seen == {"plus", "minus"}
