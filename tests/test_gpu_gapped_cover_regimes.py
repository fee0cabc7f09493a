"""GPU: sa_gapped_align_greedy on the hand-built inputs of tests/gapped_cover_regimes.py -- exclusive run ends and their neighbours, sides
of more than two 64-run emit chunks, nested index entries, merges that repeat and interleave keys, a dependency chain over three resolve
rounds, survivors with a hundred in-edges, alignments below the threshold, priority ties, both strands and both query buffers -- held to
the sequential rule over the serial path checker: records, paths and ops exactly, the accounting, the returned HSPs and the number of
index segments.  tests/test_gapped_cover_regimes.py shows on the CPU that each input is in the regime it names."""
import numpy as np
import pytest

import gapped_cover_regimes as CR
import gapped_regimes as R
from helpers import Case
from test_gpu_gapped_greedy import debug_line, same

pytestmark = pytest.mark.gpu

_up = {"key": None, "opts": ()}


def use(E, key, block, rev=False, buf=0, **opts):
    """The engine started on `block` under `opts`, the block's query as strand `rev` of buffer `buf`; restarted only when any of these
    changes.  For the reverse strand the query's reverse complement is uploaded; for buffer 1 buffer 0 gets a query of another length."""
    full = (key, rev, buf, tuple(sorted(opts.items())))
    if _up["key"] == full:
        return
    down(E)
    for k, v in opts.items():
        E.set_option(k, v)
    _up.update(key=full, opts=tuple(opts))
    q = CR.revcomp(block.query) if rev else block.query
    other = R.random_dna(block.query.size // 2 + 101, 7499)
    Case(block.target, other if buf else q, chunk=100_000, sub_mat=block.sub).engine_setup(E, num_gpu=1)
    if buf:
        E.SendQueryWriteRequest(q, 0, q.size, buf)
    assert np.array_equal(E.copy_ref_codes(), block.tc) and np.array_equal(E.copy_query_codes(buf, rev), block.qc)


def down(E):
    if _up["key"] is not None:
        E.ShutdownProcessor()
        for k in _up["opts"]:
            E.lib().sa_reset_option(k.encode())
        _up.update(key=None, opts=())


@pytest.fixture(scope="module", autouse=True)
def shutdown(engine):
    yield
    down(engine)


def check(E, reg, rev=False, buf=0):
    """One call against the sequential rule; -> its stats."""
    got = E.GappedAlignGreedy(reg.hsps, rev, buf, **reg.kw)
    sel, sel_paths, want = reg.want()
    same(got, sel, sel_paths)
    st, n = got[3], reg.hsps.size
    assert (st["returned"], st["covered"], st["below_thresh"]) == (want["returned"], want["covered"], want["below_thresh"])
    assert st["returned"] + st["covered"] + st["below_thresh"] == n
    assert sorted(got[0]["hsp_index"].tolist()) == np.nonzero(want["state"] == 1)[0].tolist()  # the per-HSP state
    assert st["skipped"] <= st["covered"] and st["anchors"] == n - st["skipped"]
    assert st["cover_segments"] == CR.segment_count(reg)
    return st


# ---- the identity block, default options ------------------------------------------------------------------------------------------------

def test_nesting_in_one_batch(engine):
    """The in-batch edges path: the probes are decided by the edges of the two accepted alignments."""
    use(engine, "identity", CR.identity_block())
    st = check(engine, CR.nesting())
    assert st["priority_batches"] == 1 and st["skipped"] == 0


@pytest.mark.parametrize("mirror", [False, True])
def test_ladder_in_one_resolve_launch(engine, mirror):
    use(engine, "identity", CR.identity_block())
    st = check(engine, CR.ladder(mirror))
    assert st["priority_batches"] == 1 and (st["returned"], st["covered"]) == (70, 70)


@pytest.mark.parametrize("rank", [None, 0, 1, 2])
def test_fan_of_in_edges(engine, rank):
    use(engine, "identity", CR.identity_block())
    reg = CR.fan(rank)
    got = engine.GappedAlignGreedy(reg.hsps, False, 0, **reg.kw)
    check(engine, reg)
    assert (reg.meta["last"] in got[0]["hsp_index"].tolist()) == (rank is None)


@pytest.mark.parametrize("seed", [0, 1])
def test_priority_ties(engine, seed):
    use(engine, "identity", CR.identity_block())
    reg = CR.ties(seed)
    check(engine, reg)
    got = engine.GappedAlignGreedy(reg.hsps, False, 0, **reg.kw)
    assert sorted(got[0]["hsp_index"].tolist()) == sorted(min(g) for g in reg.meta["groups"])


# ---- the identity block, options that need a restart ----------------------------------------------------------------------------------

def test_nesting_probes_in_later_batches(engine):
    """The index query path after a merge: both accepted alignments are batch 0, every probe is asked of the merged index."""
    use(engine, "identity", CR.identity_block(), gapped_greedy_batch=2)
    reg = CR.nesting()
    st = check(engine, reg)
    assert st["priority_batches"] == reg.hsps.size // 2 and st["skipped"] == st["covered"] > 0


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_ladder_in_batches(engine, B, mirror):
    use(engine, "identity", CR.identity_block(), gapped_greedy_batch=B)
    reg = CR.ladder(mirror)
    st = check(engine, reg)
    assert st["priority_batches"] == -(-reg.hsps.size // B)
    if B == 1:
        assert st["skipped"] == st["covered"]


@pytest.mark.parametrize("mirror", [False, True])
def test_ladder_passes_split_inside_the_chain(engine, capfd, mirror):
    """139 edges, each from one anchor to the next, in passes of at most 10."""
    use(engine, "identity", CR.identity_block(), gapped_greedy_edges=10, debug=1)
    capfd.readouterr()
    check(engine, CR.ladder(mirror))
    batches, passes, edges = debug_line(capfd.readouterr().err)
    assert batches == 1 and passes > batches and passes >= 10 and edges > 0


# ---- ends, carry, merge, thresh, gapanc: their own blocks -------------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["runs", "path"])
def test_run_ends_neighbours_and_gap_interiors(engine, part):
    reg = CR.ends(part)
    use(engine, "ends", reg.block)
    check(engine, reg)


def test_emit_chunk_carry(engine):
    reg = CR.carry()
    use(engine, "carry", reg.block)
    check(engine, reg)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_emit_side_of_one_chunk_more_or_less(engine, n):
    gap, ext = CR.carry_edge_extents()[n]
    reg = CR.carry(ext, (0, 1), gap)
    use(engine, "carry", reg.block)
    check(engine, reg)


def test_anchor_point_that_is_no_m_pair(engine):
    reg = CR.gapanc()
    use(engine, "gapanc", reg.block)
    st = check(engine, reg)
    assert (st["returned"], st["covered"]) == (1, 1)


def test_below_threshold(engine):
    reg = CR.thresh()
    use(engine, "thresh", reg.block)
    st = check(engine, reg)
    assert st["below_thresh"] == 3 and st["covered"] == 2


def test_below_threshold_across_batches(engine):
    reg = CR.thresh()
    use(engine, "thresh", reg.block, gapped_greedy_batch=2)
    st = check(engine, reg)
    assert st["below_thresh"] == 3 and st["covered"] == 2 and st["skipped"] == 1


@pytest.mark.parametrize("B", [None, 1, 2])
def test_merge_ties_and_interleaving(engine, B):
    reg = CR.merge()
    use(engine, "merge", reg.block, **({} if B is None else {"gapped_greedy_batch": B}))
    st = check(engine, reg)
    assert st["priority_batches"] == (1 if B is None else -(-reg.hsps.size // B))


# ---- strand and buffer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rev,buf", [(True, 0), (False, 1)], ids=["minus", "buffer1"])
def test_other_strand_and_other_buffer(engine, rev, buf):
    use(engine, "identity", CR.identity_block(), rev, buf)
    check(engine, CR.nesting(), rev, buf)
    check(engine, CR.ladder(), rev, buf)
    check(engine, CR.ladder(True), rev, buf)
    for part in ("runs", "path"):
        reg = CR.ends(part)
        use(engine, "ends", reg.block, rev, buf)
        check(engine, reg, rev, buf)
