"""GPU: sa_fill_chains (include/segalign_amd.h) against the model of tests/chain_fill_model.py: every field of every
entry, chain, link and found HSP, each regime asserted with the model first (tests/chain_fill_cases.py holds the cases and their
regimes; tests/test_chain_fill_model.py asserts the same regimes without a GPU)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import chain_fill_cases as K
import chain_fill_model as F
import hsp_chain_model as M
import stitch_model as S
from gapped_model import SUB
from helpers import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class World:
    pass


@pytest.fixture(scope="module")
def world(engine):
    E = engine
    w = World()
    w.E = E
    w.t, w.q, w.hsps, w.chains = K.build_world()
    Case(w.t, w.q, chunk=250_000, sub_mat=SUB).engine_setup(E, num_gpu=1)
    E.SendQueryWriteRequest(K.revcomp(w.q), 0, w.q.size, 1)
    w.ref = E.copy_ref_codes()
    w.codes = {(buf, rev): E.copy_query_codes(buf, rev) for buf in (0, 1) for rev in (False, True)}
    assert np.array_equal(w.ref, K.codes(w.t)) and np.array_equal(w.codes[(0, False)], K.codes(w.q))
    assert np.array_equal(w.codes[(0, False)], w.codes[(1, True)])
    w.models = {}
    yield w
    E.ShutdownProcessor()


def model(w, chains, rev=False, buf=0, **kw):
    """The model's result, computed once per case and parameter set and left unchanged."""
    key = (tuple(tuple(c) for c in chains), rev, buf, tuple(sorted(kw.items())))
    if key not in w.models:
        members, first = S.csr(chains)
        w.models[key] = F.fill(w.ref, w.codes[(buf, rev)], SUB, w.hsps, members, first, **kw)
    return w.models[key]


def same(got, want):
    assert len(got) == len(want)
    for g, m in zip(got, want):
        assert g.size == m.size, (g.size, m.size)
        if m.dtype.names:
            for f in m.dtype.names:
                assert np.array_equal(g[f], m[f]), (f, np.flatnonzero(g[f] != m[f])[:8])
        else:
            assert np.array_equal(g, m), np.flatnonzero(g != m)[:8]


def run(w, chains, rev=False, buf=0, **kw):
    """One engine call held against the model, field for field.  -> the model's result, the engine's stats."""
    want = model(w, chains, rev, buf, **kw)
    members, first = S.csr(chains)
    got = w.E.FillChains(w.hsps, members, first, rev, buf, links=True, found=True, **kw)
    same(got[:6], want)
    st, links = got[6], want[4]
    assert (st["links"], st["swept"], st["cells"]) == (links.size, int((links["cells"] > 0).sum()), int(links["cells"].sum()))
    assert [st["long_links"], st["large_links"], st["crowded_links"]] == [int(((links["flags"] & b) != 0).sum()) for b in (1, 2, 4)]
    assert (st["hsps"], st["fills"], st["filled_links"]) == (want[5].size, int(links["n_fill"].sum()), int((links["n_fill"] > 0).sum()))
    only = w.E.FillChains(w.hsps, members, first, rev, buf, **kw)  # without the links and the found HSPs
    assert len(only) == 5
    same(only[:4], want[:4])
    return want, st


def test_every_block_count_of_diagonals(world):
    K.regime_sizes(run(world, world.chains["sizes"], **K.ONE)[0])


def test_the_smallest_rectangles_one_row_and_one_column(world):
    K.regime_tiny(run(world, world.chains["tiny"], **K.ONE)[0])


def test_a_link_past_the_stitch_limit_and_skinny_links(world):
    w = world
    K.regime_past_stitch(run(w, w.chains["past_stitch"])[0])
    K.regime_skinny(run(w, w.chains["skinny"])[0], w.hsps, w.chains["skinny"])


def test_the_four_edges_both_corners_and_two_segments_on_a_diagonal(world):
    w = world
    K.regime_edges(run(w, w.chains["edges"])[0], w.hsps, w.chains["edges"])


def test_the_first_and_last_diagonal_of_a_block_and_of_the_link(world):
    w = world
    K.regime_diagonals(run(w, w.chains["diagonals"], **K.ONE)[0], w.hsps, w.chains["diagonals"])


def test_the_xdrop_zero_and_threshold_boundaries(world):
    w = world
    K.hand_regimes(lambda chains, **kw: run(w, chains, **kw)[0], w.chains, w.hsps)


def test_a_separator_in_either_range(world):
    w = world
    K.regime_separators(run(w, w.chains["separators"])[0], w.ref, w.codes[(0, False)], w.hsps, w.chains["separators"])


def test_the_three_limits_at_and_below_the_value(world):
    w = world
    lim, homo = w.chains["limits"], w.chains["homopolymer"]
    assert run(w, lim, max_side=100)[0][4]["flags"].tolist() == [0] and run(w, lim, max_side=99)[0][4]["flags"].tolist() == [F.LONG]
    assert run(w, lim, max_cells=6000)[0][4]["flags"].tolist() == [0] and run(w, lim, max_cells=5999)[0][4]["flags"].tolist() == [F.LARGE]
    assert run(w, homo, thresh=91, max_link_hsps=39)[0][4][["flags", "n_hsps", "n_fill"]].tolist() == [(0, 39, 1)]
    res, st = run(w, homo, thresh=91, max_link_hsps=38)
    assert res[4][["flags", "n_hsps", "n_fill"]].tolist() == [(F.CROWDED, 39, 0)] and st["crowded_links"] == 1 and st["hsps"] == 0
    # a crowded link beside others in one batch: only it is dropped
    mixed, _ = run(w, w.chains["tiny"][:2] + homo + w.chains["tiny"][2:4] + w.chains["edges"], thresh=91, max_link_hsps=38)
    assert mixed[4]["flags"].tolist() == [0, 0, F.CROWDED, 0, 0, F.CROWDED, F.CROWDED] and 2 <= mixed[5].size <= 10


def test_min_fill_and_the_choice_among_crossing_and_collinear_fills(world):
    w = world
    res, _ = run(w, w.chains["collinear"] + w.chains["crossing"], diag_pen=1, anti_pen=1)
    assert res[4]["n_hsps"].tolist() == [3, 2] and res[4]["n_fill"].tolist() == [3, 1]
    score = int(run(w, w.chains["limits"])[0][5]["score"][0])
    assert run(w, w.chains["limits"], min_fill=score)[0][4]["n_fill"].tolist() == [1]
    assert run(w, w.chains["limits"], min_fill=score + 1)[0][4]["n_fill"].tolist() == [0]


def test_the_other_strand_and_the_second_buffer(world):
    w = world
    chains = w.chains["random"][0][:10] + w.chains["edges"]
    want, _ = run(w, chains)
    got, _ = run(w, chains, rev=True, buf=1)  # buffer 1 holds the reverse complement: its minus strand is buffer 0's plus strand
    same(got, want)
    assert want[4]["n_fill"].sum() > 10
    # the same coordinates on a strand the chains were not made for: nothing is found
    none, st = run(w, chains, rev=True, buf=0)
    assert none[5].size == 0 and st["fills"] == 0 and st["swept"] == want[4]["cells"].astype(bool).sum() and np.array_equal(none[1], S.csr(chains)[1])


def test_chains_of_1_2_65_and_300_members(world):
    res, _ = run(world, world.chains["lengths"], **K.SMALL)
    K.regime_lengths(res)
    assert [len(c) for c in world.chains["lengths"]] == [1, 2, 65, 300]


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("s", range(6))
def test_random_links_under_every_parameter_set(world, s, k):
    res, _ = run(world, world.chains["random"][s], **K.RANDOM_PARAMS[k])
    K.regime_random(res, k)


def test_eight_concurrent_callers(world):
    w = world
    sets = [(w.chains["random"][k % 6], K.RANDOM_PARAMS[k % 3]) for k in range(8)]
    want = [model(w, c, **kw) for c, kw in sets]
    got, errors = [None] * 8, []

    def call(k):
        try:
            members, first = S.csr(sets[k][0])
            got[k] = w.E.FillChains(w.hsps, members, first, False, 0, links=True, found=True, **sets[k][1])
        except Exception as e:  # noqa: BLE001 -- reported below, in the test's thread
            errors.append(e)

    threads = [threading.Thread(target=call, args=(k,)) for k in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(8):
        same(got[k][:6], want[k])


def test_more_lanes_than_a_batch_and_more_hsps_than_an_emit_group(world):
    """The same chain 150 times (an HSP may be a member of several chains): the sweep takes two batches of at most 1 << 22 lanes, the
    emit two groups of at most 1 << 20 HSPs.  The model runs on one copy; the expected output is that, repeated."""
    w = world
    one = model(w, w.chains["long_row"], **K.ONE)
    copies = 150
    n1, lanes = one[5].size, (30000 + 63) // 64 * 64
    assert copies * lanes > 1 << 22 and copies * n1 > 1 << 20 and one[4]["n_fill"].tolist() == [1] and one[0].size == 3
    members, first = S.csr(w.chains["long_row"] * copies)
    got = w.E.FillChains(w.hsps, members, first, False, 0, links=True, found=True, **K.ONE)
    found = np.tile(one[5], copies)
    found["link"] = np.repeat(np.arange(copies, dtype=np.uint32), n1)
    want = (np.tile(one[0], copies), (np.arange(copies + 1) * 3).astype(np.uint32), np.tile(one[2], copies), np.tile(one[3], copies),
            np.tile(one[4], copies), found)
    same(got[:6], want)
    assert got[6]["hsps"] == copies * n1 and got[6]["fills"] == copies


def test_empty_inputs(world):
    w = world
    none = np.zeros(0, dtype=np.uint32)
    out, first_out, origin, ch, links, found, st = w.E.FillChains(w.hsps, none, np.zeros(1, dtype=np.uint32), False, 0, links=True, found=True)
    assert out.size == origin.size == ch.size == links.size == found.size == 0 and first_out.tolist() == [0] and st["links"] == 0
    res, st = run(w, [[], [w.chains["edges"][0][0]], []])
    assert res[1].tolist() == [0, 0, 1, 1] and st["links"] == 0 and res[0].size == 1
    res, _ = run(w, [[], []])
    assert res[1].tolist() == [0, 0, 0] and res[0].size == 0 and res[3].size == 2


def test_the_filled_chains_stitch_and_net_as_they_are(world):
    w = world
    E = w.E
    chains = w.chains["random"][1][:12] + w.chains["past_stitch"] + w.chains["edges"] + w.chains["collinear"]
    members0, first0 = S.csr(chains)
    res, _ = run(w, chains)
    out, first = res[0], res[1]
    assert out.size > members0.size + 15
    members = np.arange(out.size, dtype=np.uint32)
    recs, ops, slinks, cnt = S.stitch(w.ref, w.codes[(0, False)], SUB, out, members, first)
    g_recs, g_ops, g_links, st = E.StitchChains(out, members, first, False, 0, links=True)
    assert g_recs.size == recs.size and all(np.array_equal(g_recs[f], recs[f]) for f in S.RECORD_DTYPE.names) and np.array_equal(g_ops, ops)
    for r in g_recs:  # the ops re-score
        o = g_ops[int(r["op_offset"]):int(r["op_offset"]) + int(r["n_ops"])]
        assert S.rescore(w.ref, w.codes[(0, False)], SUB, int(r["ref_start"]), int(r["query_start"]), o, 400, 30) == int(r["score"])
    # the link past the stitch limit cut its chain in two; filled, it is one record
    plain = E.StitchChains(w.hsps, members0, first0, False, 0)[0]
    assert (plain["flags"] & S.LONG).sum() > (g_recs["flags"] & S.LONG).sum() and plain.size > g_recs.size
    bs, be = E.net_blocks(out, members, first)
    fills, _ = E.NetChains(first, bs, be, res[3]["score"])
    assert fills.size >= len(chains)
    sub_h, sub_c, _ = E.NetSubset(out, members, first, fills, False, 0)
    assert sub_h.size == out.size and sub_c.size == len(chains)  # the chains do not overlap: every one is a top-level fill, whole


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import chain_fill_cases as K
import stitch_model as S
from gapped_model import SUB
from helpers import Case
from segalign_amd import engine as E
t, q, hsps, chains = K.build_world()
what = %r
sub = SUB.copy()
if what == "headroom":
    sub[0] = 4000
Case(t, q, chunk=250_000, sub_mat=sub).engine_setup(E, num_gpu=1)
h = hsps.copy()
c = chains["collinear"][0]
members, first = S.csr([c])
if what == "overlap":
    h[c[1]]["ref_start"] = h[c[0]]["ref_start"] + 10
    h[c[1]]["query_start"] = h[c[0]]["query_start"] + 10
if what == "outside":
    h[c[1]]["ref_start"] = t.size - 5
E.FillChains(h, members, first, False, 0, max_side=(1 << 20) if what == "headroom" else 0, thresh=0 if what == "thresh" else 3000)
print("returned")
"""


@pytest.mark.parametrize("what,message", [("overlap", b"sa_trim_chains first"), ("outside", b"inside the block"), ("headroom", b"int32 headroom"),
                                          ("thresh", b"thresh")])
def test_what_is_refused_ends_the_process_with_a_message(what, message):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), what)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"returned" not in r.stdout, (r.returncode, r.stderr[-300:])
    assert message in r.stderr and b"FillChains" in r.stderr, r.stderr[-300:]
