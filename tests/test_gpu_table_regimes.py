"""GPU: the seed position table build (table.hip: two-level and three-level partition build, atomic build, the give-up path between them)
and the neighbourhood table (probe.hip: nbr_count / nbr_fill / ctx_by_index / nbr_copy_ctx / nbr_copy_ctx_sparse / nbr_fill_ctx) on the
hand-built inputs of tests/table_regimes.py, held to tests/table_model.py: the index table word for word, every bucket of up to 512
entries entry for entry (larger ones as sets), every nbr_start and every record of the neighbourhood table field for field, and what
sa_get_table_build_info says about the build that ran.  tests/test_table_regimes.py shows on the CPU that every input is in the regime
it names and that the model equals the oracle.  No pipeline runs here (DESIGN.md 4.2'')."""
import numpy as np
import pytest

import table_model as M
import table_regimes as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sub_mat(oracle):
    return oracle.build_sub_mat(910)


def build(E, sub_mat, reg, options=None, transition=True):
    """the reference's call order (src/main.cpp:297-298,613-621) up to the table"""
    E.ShutdownProcessor()
    E.reset_option(None)
    for k, v in (options or {}).items():
        E.set_option(k, v)
    E.InitializeInterface(1)
    S = reg.shape
    assert E.GenerateShapePos(S.text) == S.weight
    E.InitializeProcessor(transition, 250000, S.span, sub_mat, 910, 3000, False)
    keep = E.SendRefWriteRequest(reg.target, 0, reg.target.size)
    E.GenerateSeedPosTable(keep, 0, reg.target.size, reg.step, S.span, S.weight)
    return keep


@pytest.fixture
def E(engine):
    try:
        yield engine
    finally:
        engine.ShutdownProcessor()
        engine.reset_option(None)


def hold_table(E, sub_mat, reg, atomic):
    """index and position table against the model, and the build that made them"""
    build(E, sub_mat, reg, {"table_atomic": int(atomic), "no_td": 1})
    keys, pos = reg.entries
    info = E.table_build_info()
    assert (info["build"], info["unsorted_partitions"]) == reg.expect(atomic), (reg, atomic, info)
    assert info["nbr_fill"] == E.NBR_FILL_NONE and E.lookup_mode() == 0
    index, got = E.copy_index_table(), E.copy_pos_table()
    assert index.size == reg.shape.nkeys and got.size == E.lib().sa_get_num_index() == pos.size, (reg, got.size, pos.size)
    assert M.index_equal(index, keys), reg
    M.check_pos_table(got, pos, keys, (reg, "atomic" if atomic else "partition"))
    assert np.array_equal(E.copy_ref_codes(), reg.codes)


BUILDS = pytest.mark.parametrize("atomic", [False, True], ids=["partition", "atomic"])


@BUILDS
@pytest.mark.parametrize("name", list(R.TWO_LEVEL_REGIMES))
def test_two_level_build(E, sub_mat, name, atomic):
    hold_table(E, sub_mat, R.TWO_LEVEL_REGIMES[name](), atomic)


@BUILDS
@pytest.mark.parametrize("name", list(R.THREE_LEVEL_REGIMES))
def test_three_level_build(E, sub_mat, name, atomic):
    hold_table(E, sub_mat, R.THREE_LEVEL_REGIMES[name](), atomic)


@BUILDS
@pytest.mark.parametrize("name", list(R.WEIGHT14_REGIMES))
def test_three_level_build_14of22(E, sub_mat, name, atomic):
    hold_table(E, sub_mat, R.WEIGHT14_REGIMES[name](), atomic)


@pytest.mark.parametrize("first,lead", [(0, 0), (1000, R.TB_PART_TILE)], ids=["first tile", "second tile"])
def test_64_and_65_groups_in_a_tile_take_two_builds(E, sub_mat, first, lead):
    """64 groups in a tile are the last the third level takes; with the 65th the build gives up and the atomic build makes the table.
    Either way the table is bit for bit the one option table_atomic builds, and the 65-group table is the 64-group one and a position."""
    keys_of = {}
    for n, want in ((R.REL_GROUPS, E.TABLE_BUILD_THREE_LEVEL), (R.REL_GROUPS + 1, E.TABLE_BUILD_ATOMIC_GAVE_UP)):
        reg = R.groups_span(n, first=first, lead=lead)
        tables = []
        for atomic in (0, 1):
            build(E, sub_mat, reg, {"no_td": 1, "table_atomic": atomic})
            assert E.table_build_info()["build"] == (E.TABLE_BUILD_ATOMIC if atomic else want), (reg, E.table_build_info())
            tables.append((E.copy_index_table(), E.copy_pos_table()))
        assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1]), reg
        assert M.index_equal(tables[0][0], reg.entries[0]) and np.array_equal(tables[0][1], reg.entries[1]), reg
        keys_of[n] = reg.entries[0][reg.entries[0] >> 14 != 100]      # (without the positions in front)
    assert np.array_equal(keys_of[R.REL_GROUPS], keys_of[R.REL_GROUPS + 1][:-1])


# ---- neighbourhood table -----------------------------------------------------------------------------------------------------------------
def hold_nbr(E, sub_mat, reg, fill, want_fill):
    options, transition, mode, skip = R.FILLS[fill]
    build(E, sub_mat, reg, options, transition)
    S = reg.shape
    keys, pos = reg.entries
    assert E.lookup_mode() == mode, (reg, fill)
    info = E.table_build_info()
    assert info["nbr_fill"] == want_fill, (reg, fill, info)
    assert info["left_skip"] == skip * S.span, (reg, fill, info)
    got_pos = E.copy_pos_table()
    assert M.index_equal(E.copy_index_table(), keys)
    M.check_pos_table(got_pos, pos, keys, (reg, fill))
    want_start, src = M.neighbourhood(keys, S, transition)
    # every nbr_start, read in two ranges; the closing word is the number of entries
    half = S.nkeys // 2 + 1
    starts = np.concatenate([E.copy_neighbourhood_starts(0, half), E.copy_neighbourhood_starts(half)])
    assert starts.size == S.nkeys + 1 and np.array_equal(starts, want_start), (reg, fill)
    total = E.neighbourhood_entries()
    assert int(starts[-1]) == total == src.size
    # every record, in three ranges.  (the positions the records repeat are the DEVICE's pos_table, shown above to be the model's up to the
    # free order inside buckets above 512 entries)
    cuts = [0, total // 3, total // 3 + 1, total]
    parts = [E.copy_neighbourhood_records(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(m == mode for m, _ in parts)
    recs = np.concatenate([r for _, r in parts])
    want_pos = got_pos[src]
    if mode == 1:
        assert recs.dtype == np.uint32 and np.array_equal(recs, want_pos), (reg, fill)
    else:
        want = M.context_records(reg.codes, got_pos, S.span, skip * S.span)[src]
        assert np.array_equal(recs["pos"], want["pos"]), (reg, fill)
        bad = np.flatnonzero((recs["w"] != want["w"]).any(axis=1))
        assert bad.size == 0, (reg, fill, "%d records differ, first at entry %d (seed start %d): %s != %s"
                               % (bad.size, bad[0], recs["pos"][bad[0]], recs["w"][bad[0]], want["w"][bad[0]]))
    # ranges that leave the table are refused, not read
    with pytest.raises(RuntimeError):
        E.copy_neighbourhood_starts(S.nkeys, 2)
    with pytest.raises(RuntimeError):
        E.copy_neighbourhood_records(total, 1)


def fill_of(E, fill, reg):
    two_stage = E.NBR_FILL_CTX_SPARSE if reg.entries[0].size < reg.shape.nkeys else E.NBR_FILL_CTX_DENSE
    return {"default": two_stage, "anchor context": two_stage, "one stage": E.NBR_FILL_CTX_ONE_STAGE, "positions": E.NBR_FILL_POSITIONS,
            "notransition": E.NBR_FILL_CTX_ONE_STAGE, "notransition positions": E.NBR_FILL_ALIAS}[fill]


@pytest.mark.parametrize("fill", list(R.FILLS))
@pytest.mark.parametrize("name", list(R.NBR_REGIMES))
def test_neighbourhood_table(E, sub_mat, name, fill):
    reg = R.NBR_REGIMES[name]()
    hold_nbr(E, sub_mat, reg, fill, fill_of(E, fill, reg))


@pytest.mark.parametrize("fill", ["default", "one stage", "positions"])
@pytest.mark.parametrize("dense", [False, True], ids=["nkeys - 1: lane per key", "nkeys: wave per key"])
def test_neighbourhood_copy_switches_at_one_position_per_key(E, sub_mat, dense, fill):
    reg = R.nbr_density((1 << 18) - (0 if dense else 1))
    want = fill_of(E, fill, reg)
    if fill == "default":
        assert want == (E.NBR_FILL_CTX_DENSE if dense else E.NBR_FILL_CTX_SPARSE)
    hold_nbr(E, sub_mat, reg, fill, want)


def test_neighbourhood_of_an_empty_table(E, sub_mat):
    """num_index = 0: every run is empty, nothing to copy, nothing faults"""
    reg = R.valid_among(0)
    build(E, sub_mat, reg)
    assert E.lookup_mode() in (1, 2)
    assert E.neighbourhood_entries() == 0
    assert not E.copy_neighbourhood_starts().any()
    assert E.copy_neighbourhood_records()[1].size == 0


def test_copies_fail_with_a_message_before_the_table_is_built(E, sub_mat):
    E.ShutdownProcessor()
    E.InitializeInterface(1)
    info = E.table_build_info()
    assert info == {"build": E.TABLE_BUILD_NONE, "unsorted_partitions": 0, "nbr_fill": E.NBR_FILL_NONE, "left_skip": 0}
    with pytest.raises(RuntimeError):
        E.copy_neighbourhood_starts(0, 1)
    with pytest.raises(RuntimeError):
        E.copy_neighbourhood_records(0, 1)
    # a table without a neighbourhood table (option no_td): the same
    build(E, sub_mat, R.steps(1), {"no_td": 1})
    assert E.table_build_info()["build"] == E.TABLE_BUILD_TWO_LEVEL
    with pytest.raises(RuntimeError):
        E.copy_neighbourhood_starts(0, 1)
