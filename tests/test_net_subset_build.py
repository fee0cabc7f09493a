"""CPU: sa_net_subset as built (segalign_amd/csrc/netsubset.hip, api_netsubset.hip): the library exports the two entries,
the records have the sizes the header asserts, every kernel is there and none spills to scratch memory, and
`python -m segalign_amd.build --resources netsubset.hip` prints them."""
import ctypes as C
import os
import subprocess
import sys

from segalign_amd import engine as E
from segalign_amd.build import LIB_PATH, SOURCES, build_lib, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["netsubset_counts_kernel", "netsubset_mark_kernel", "netsubset_emit_kernel", "netsubset_cut_list_kernel",
           "netsubset_rescore_kernel", "netsubset_terms_kernel", "netsubset_chains_kernel"]


def test_the_library_exports_the_entries():
    build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert "sa_net_subset" in syms and "sa_free_net_subset" in syms
    assert "sa_net_subset" in E.C_ABI_SYMBOLS and "sa_free_net_subset" in E.C_ABI_SYMBOLS


def test_the_struct_sizes():
    assert E.SUBSET_CHAIN_DTYPE.itemsize == 56 and C.sizeof(E.SubsetStats) == 56 and E.SUBSET_SPLIT == 1
    assert E.SUBSET_CHAIN_DTYPE.fields["score"][1] == 40 and E.SUBSET_CHAIN_DTYPE.fields["clipped"][1] == 48
    header = open(os.path.join(ROOT, "include", "segalign_amd.h")).read()
    assert "sizeof(sa_subset_chain) == 56" in header and "sizeof(sa_subset_stats) == 56" in header


def test_the_kernels_use_no_scratch():
    assert "netsubset.hip" in SOURCES and "api_netsubset.hip" in SOURCES
    res = kernel_resources("netsubset.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 64, (k, r)  # 64: full occupancy of a 256-thread workgroup
        assert r["lds"] == (256 if k == "netsubset_rescore_kernel" else 0), (k, r)  # the 64-entry matrix


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "netsubset.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert sorted(ln.split()[0] for ln in lines) == sorted(KERNELS) and all(" scratch=0 " in ln for ln in lines)
