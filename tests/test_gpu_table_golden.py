"""GPU: the device-built seed position table (table.hip; every step) against tables built by the reference's own GenerateSeedPosTable
text (tests/golden/table_golden.json).  Which build makes each table is asserted through sa_get_table_build_info: the 12of19 and
11of18 cases take the two-level radix-partition build; the 14of22 cases -- 5 000 bases, so the first tile of the third level already
spans hundreds of the 4096 twelve-bit groups -- make the three-level build give up and are built by the atomic build, like every
case under option table_atomic.  The three-level build itself is held to a model in tests/test_gpu_table_regimes.py."""
import numpy as np
import pytest

import table_golden as G
import table_regimes as R
from helpers import canonical_pos_table

pytestmark = pytest.mark.gpu

CASES = list(G.cases())


def expected_build(c):
    """the build the partition path takes for this case, from the case's own histogram (tests/table_regimes.py Regime.facts)"""
    reg = R.Regime("golden", c["shape"], c["step"], c["target"], None)
    w = reg.shape.weight
    if not 9 <= w <= 14:
        return R.ATOMIC
    if w <= 12:
        return R.TWO_LEVEL
    return R.THREE_LEVEL if reg.facts().get("rel_groups_max", 0) < R.REL_GROUPS else R.GAVE_UP


def test_the_golden_14of22_cases_are_too_small_for_the_three_level_build():
    builds = {(len(c["shape"]), expected_build(c)) for c in CASES}
    assert (22, R.GAVE_UP) in builds and (22, R.THREE_LEVEL) not in builds and (19, R.TWO_LEVEL) in builds


@pytest.mark.parametrize("atomic", [0, 1], ids=["partition build", "atomic build"])
def test_device_table_equals_the_reference_functions_table(oracle, engine, atomic):
    E = engine
    try:
        for c in CASES:
            E.reset_option(None)
            E.set_option("table_atomic", atomic)
            E.InitializeInterface(1)
            k = E.GenerateShapePos(c["shape"])
            assert k == c["kmer_size"]
            E.InitializeProcessor(True, 250000, len(c["shape"]), oracle.build_sub_mat(910), 910, 3000, False)
            keep = E.SendRefWriteRequest(c["target"], 0, c["target"].size)
            E.GenerateSeedPosTable(keep, 0, c["target"].size, c["step"], len(c["shape"]), k)
            assert E.table_build_info()["build"] == (R.ATOMIC if atomic else expected_build(c)), (c["shape"], c["step"])
            index, pos = E.copy_index_table(), E.copy_pos_table()
            G.check_table(c, index, canonical_pos_table(index, pos))
            E.ShutdownProcessor()
    finally:
        E.ShutdownProcessor()
        E.reset_option(None)
