"""CPU: sa_lift_intervals as built (segalign_amd/csrc/lift.hip, api_lift.hip): the library exports the two entries, the
records have the sizes and offsets the header asserts, every kernel is there and none spills to scratch memory or uses LDS, and
`python -m segalign_amd.build --resources lift.hip` prints them."""
import ctypes as C
import os
import subprocess
import sys

import lift_model as L
from segalign_amd import engine as E
from segalign_amd.build import LIB_PATH, SOURCES, build_lib, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["lift_block_len_kernel", "lift_keys_kernel", "lift_gather_kernel", "lift_count_kernel", "lift_emit_kernel", "lift_blocks_kernel"]


def test_the_library_exports_the_entries():
    build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert "sa_lift_intervals" in syms and "sa_free_lift" in syms
    assert "sa_lift_intervals" in E.C_ABI_SYMBOLS and "sa_free_lift" in E.C_ABI_SYMBOLS


def test_the_struct_sizes_and_offsets():
    assert E.LIFT_RECORD_DTYPE.itemsize == 48 and E.LIFT_HIT_DTYPE.itemsize == 32 and E.LIFT_BLOCK_DTYPE.itemsize == 16
    assert C.sizeof(E.LiftParams) == 8 and C.sizeof(E.LiftStats) == 96
    assert E.LIFT_RECORD_DTYPE == L.RECORD and E.LIFT_HIT_DTYPE == L.HIT and E.LIFT_BLOCK_DTYPE == L.BLOCK
    f = E.LIFT_RECORD_DTYPE.fields
    assert [f[k][1] for k in ("status", "first_hit", "chain", "ostart", "mapped", "n_blocks", "strand", "pad")] == [0, 12, 16, 24, 32, 40, 44, 45]
    assert E.LIFT_HIT_DTYPE.fields["mapped"][1] == 16 and E.LIFT_HIT_DTYPE.fields["out_block"][1] == 28
    assert E.LiftStats.candidates.offset == 24 and E.LiftStats.n_status.offset == 40 and E.LiftStats.hits.offset == 72
    assert E.LiftStats.prep_ms.offset == 88 and E.LiftStats.lift_ms.offset == 92 and E.LiftParams.den.offset == 4
    header = open(os.path.join(ROOT, "include", "segalign_amd.h")).read()
    for name, size in (("sa_lift_params", 8), ("sa_lift_record", 48), ("sa_lift_hit", 32), ("sa_lift_block", 16), ("sa_lift_stats", 96)):
        assert header.count("sizeof(%s) == %d" % (name, size)) == 2, name
    assert (E.LIFT_MULTIPLE, E.LIFT_BLOCKS) == (1, 2) and "#define SA_LIFT_MULTIPLE 1u" in header and "#define SA_LIFT_BLOCKS 2u" in header
    assert (E.LIFT_UNMAPPED, E.LIFT_PARTIAL, E.LIFT_MAPPED, E.LIFT_DUPLICATED) == (0, 1, 2, 3) == (L.UNMAPPED, L.PARTIAL, L.MAPPED, L.DUPLICATED)
    assert E.LIFT_NAMES == ("unmapped", "partial", "mapped", "duplicated") == L.NAMES
    for k, name in enumerate(("UNMAPPED", "PARTIAL", "MAPPED", "DUPLICATED")):
        assert "#define SA_LIFT_%s %d" % (name, k) in header


def test_the_kernels_use_no_scratch_and_no_lds():
    assert "lift.hip" in SOURCES and "api_lift.hip" in SOURCES
    res = kernel_resources("lift.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 64 and r["lds"] == 0, (k, r)  # 64: full occupancy of a 256-thread workgroup


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "lift.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert sorted(ln.split()[0] for ln in lines) == sorted(KERNELS) and all(" scratch=0 " in ln for ln in lines)
