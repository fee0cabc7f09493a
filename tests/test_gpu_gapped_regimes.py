"""GPU: the gapped kernels on the hand-built inputs of tests/gapped_regimes.py -- every band instance with a moving window and
refilled streams, bands exactly as wide as the window, gap runs longer than a walk stage, and scores full of ties -- every field
against the serial checkers.  tests/test_gapped_regimes.py shows on the CPU that each input is in the regime it claims."""
import numpy as np
import pytest

import gapped_greedy_model as GR
import gapped_model as G
import gapped_pieces_model as PM
import gapped_regimes as R
import gapped_trace_model as T
from helpers import Case
from test_gpu_gapped import check_raw
from test_gpu_gapped_align import check_align

pytestmark = pytest.mark.gpu

_up = {"key": None, "opts": ()}


def use(E, key, block, **opts):
    """The engine started on `block` (its matrix included) under `opts`; restarted only when either changes."""
    if _up["key"] == (key, tuple(sorted(opts.items()))):
        return
    down(E)
    for k, v in opts.items():
        E.set_option(k, v)
    _up.update(key=(key, tuple(sorted(opts.items()))), opts=tuple(opts))
    Case(block.target, block.query, chunk=100_000, sub_mat=block.sub).engine_setup(E, num_gpu=1)
    assert np.array_equal(E.copy_ref_codes(), block.tc) and np.array_equal(E.copy_query_codes(0, False), block.qc)


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


def both(E, b, h, **kw):
    """sa_gapped_extend and sa_gapped_align, raw, against both checkers."""
    check_raw(E, b.tc, b.qc, h, False, 0, sub=b.sub, **kw)
    return check_align(E, b.tc, b.qc, h, False, 0, sub=b.sub, **kw)


# ---- A ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", sorted(R.A_BANDS))
def test_a_every_instance_with_a_moving_window(engine, K):
    E = engine
    b, h = R.block_a()
    use(E, "A", b)
    kw = R.a_params(K)
    recs, *_ = both(E, b, h, **kw)
    assert np.all(recs["flags"] & G.EXTENT_CAP) and not np.any(recs["flags"] & G.BAND_CAP)
    got = E.GappedAlignGreedy(h, False, 0, **kw)
    sel, sel_paths, want = GR.from_checker(b.tc, b.qc, b.sub, h, 3000, **kw)
    wp, wops = T.pack(sel_paths)
    assert np.array_equal(got[0], sel) and np.array_equal(got[1], wp) and np.array_equal(got[2], wops)
    assert (got[3]["returned"], got[3]["covered"], got[3]["below_thresh"]) == (want["returned"], want["covered"], want["below_thresh"])


@pytest.mark.parametrize("K", sorted(R.A_BANDS))
def test_a_continuation_pieces_in_every_instance(engine, K):
    E = engine
    b, h = R.block_a()
    use(E, "A", b, gapped_pieces=3)
    kw = R.a_params(K)
    want, wpaths, _ = PM.align(b.tc, b.qc, b.sub, h, 3, **kw)
    ext, _ = E.GappedExtend(h, False, 0, raw=True, **kw)
    assert np.array_equal(ext, want), (ext[:3], want[:3])
    recs, paths, ops, _ = E.GappedAlign(h, False, 0, raw=True, **kw)
    wp, wops = T.pack(wpaths)
    assert np.array_equal(recs, want) and np.array_equal(paths, wp) and np.array_equal(ops, wops)
    assert np.all(recs["flags"] & PM.CONTINUED)


# ---- B ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,width", sorted(R.B_TUNED))
def test_b_band_exactly_as_wide_as_the_window(engine, name, width):
    """max_band = 64 K - 2 caps (on the checker's antidiagonal: cells agree), 64 K - 1 does not and the candidate range fills the
    window, 64 K is the next instance and gives the same records and paths."""
    E = engine
    b, anc = R.block_b()
    use(E, "B", b)
    kw = R.b_params(name, width)
    recs, *_ = both(E, b, anc[name], max_band=width - 1, **kw)
    assert recs[0]["flags"] & G.BAND_CAP
    tight = both(E, b, anc[name], max_band=width, **kw)
    assert not tight[0][0]["flags"] & G.BAND_CAP and tight[0][0]["flags"] & G.EXTENT_CAP
    nxt = both(E, b, anc[name], max_band=width + 1, **kw)
    for x, y in zip(tight[:3], nxt[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name,width", sorted(R.B_PIECES))
def test_b_continuation_pieces_and_greedy_on_a_wide_band(engine, name, width):
    """gapped_sides_kernel, the trace of later pieces and the greedy entry on bands as wide as the window (homopolymer) or wider than
    the next smaller instance's (repeat)."""
    E = engine
    b, _ = R.block_b()
    use(E, "B", b, gapped_pieces=3)
    kw = R.b_pieces_params(name, width)
    h = R.b_pieces_anchors(name)
    want, wpaths, _ = PM.align(b.tc, b.qc, b.sub, h, 3, **kw)
    ext, _ = E.GappedExtend(h, False, 0, raw=True, **kw)
    assert np.array_equal(ext, want), (ext, want)
    recs, paths, ops, _ = E.GappedAlign(h, False, 0, raw=True, **kw)
    wp, wops = T.pack(wpaths)
    assert np.array_equal(recs, want) and np.array_equal(paths, wp) and np.array_equal(ops, wops)
    assert np.all(recs["flags"] & PM.CONTINUED) and not np.any(recs["flags"] & G.BAND_CAP)
    got = E.GappedAlignGreedy(h, False, 0, **kw)
    sel, sel_paths, gw = PM.greedy(b.tc, b.qc, b.sub, h, 3000, 3, **kw)
    sp, sops = T.pack(sel_paths)
    assert np.array_equal(got[0], sel) and np.array_equal(got[1], sp) and np.array_equal(got[2], sops)
    assert (got[3]["returned"], got[3]["covered"]) == (gw["returned"], gw["covered"]) == (1, 1)


@pytest.mark.parametrize("name", sorted(R.B_WIDE))
def test_b_widest_instance_with_a_wide_band(engine, name):
    E = engine
    b, anc = R.block_b()
    use(E, "B", b)
    recs, *_ = both(E, b, anc[name], max_band=2048, **R.b_params(name, 2048))
    assert not recs[0]["flags"] & G.BAND_CAP


# ---- C ----------------------------------------------------------------------------------------------------------------------------

def planted_runs(h, planted, paths, ops, records):
    for k, n in zip(range(h.size), records):
        lo, ro = T.record_ops(paths, ops, k)
        for side_ops, (kind, ln) in zip((lo, ro), planted[n]):
            assert (ln << 2 | (T.OP_I if kind == "I" else T.OP_D)) in side_ops.tolist(), (n, kind, ln)


def test_c_gap_runs_longer_than_a_walk_stage(engine):
    E = engine
    b, h, planted = R.block_c()
    use(E, "C", b)
    _, paths, ops, _ = both(E, b, h, **R.C_PARAMS)
    planted_runs(h, planted, paths, ops, range(h.size))
    hk = h[list(R.C_K2_RECORDS)]
    _, paths, ops, _ = both(E, b, hk, **R.C_PARAMS_K2)
    planted_runs(hk, planted, paths, ops, R.C_K2_RECORDS)


# ---- D ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(6))
def test_d_ties_under_the_unit_matrix(engine, n):
    E = engine
    b, sets = R.block_d()
    use(E, "D", b)
    name, h, kw = sets[n]
    recs, *_ = both(E, b, h, **kw)
    if name == "tiles":  # of the two tied cells the one with the smaller i
        assert np.all(recs["query_end"] - recs["query_start"] == recs["ref_end"] - recs["ref_start"] + 2) and np.all(recs["score"] > 0)
