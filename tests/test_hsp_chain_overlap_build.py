"""CPU: the overlap instances of the chain DP (segalign_amd/csrc/hspovl.hip) as the compiler reports them, and the
entries they serve as the library exports them.  The DP kernels are hspchain_dp.h's bodies with OVL on: they must fit a workgroup of
1 024 threads, spill nothing and keep their tile image in dynamic LDS, like the plain instances beside them."""
import os
import re

from segalign_amd.build import SOURCES, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["hspovl_cross_kernel<false>", "hspovl_cross_kernel<true>", "hspovl_resolve_kernel<false>", "hspovl_resolve_kernel<true>",
           "hspovl_weight_kernel"]


def test_overlap_kernels_fit_1024_threads_without_scratch():
    assert "hspovl.hip" in SOURCES
    res = kernel_resources("hspovl.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 128 and r["agprs"] == 0, (k, r)  # 128: what 1024 threads leave a lane
        assert r["lds"] == 0, (k, r)  # 48 bytes per node and the cost image are dynamic LDS, sized at launch


def test_the_dp_exists_once_as_text():
    """hspchain.hip and hspovl.hip hold wrappers only: the pair evaluation is hspchain_dp.h's."""
    csrc = os.path.join(ROOT, "segalign_amd", "csrc")
    for unit in ("hspchain.hip", "hspovl.hip"):
        txt = open(os.path.join(csrc, unit)).read()
        assert "hspchain_dp.h" in txt and "gap_r" not in txt and "__shfl" not in txt.split("hspchain_ends_kernel")[0], unit
    assert open(os.path.join(csrc, "hspchain_dp.h")).read().count("void consider(") == 1


def test_overlap_entries_are_exported_and_listed():
    from segalign_amd import engine as E
    from segalign_amd.build import build_lib
    build_lib()
    L = E.lib()
    for s in ("sa_chain_hsps_ovl", "sa_chain_hsps_all_ovl"):
        assert hasattr(L, s) and s in E.C_ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "segalign_amd.h")).read()
    assert re.search(r"#define SA_CHAIN_MAX_OVERLAP %d\b" % E.CHAIN_MAX_OVERLAP, hdr)
    import ctypes as C
    assert C.sizeof(E.ChainOverlap) == 8 and [n for n, _ in E.ChainOverlap._fields_] == ["max_overlap", "reserved"]


def test_python_refuses_an_allowance_out_of_range_before_the_library_does():
    import numpy as np
    import pytest
    from segalign_amd import engine as E
    h = np.zeros(0, dtype=E.SEG_DTYPE)
    for bad in (-1, E.CHAIN_MAX_OVERLAP + 1, 2 ** 32):
        for entry in (E.ChainHsps, E.ChainHspsAll):
            with pytest.raises(ValueError, match="max_overlap"):
                entry(h, None, max_overlap=bad)


def test_the_crossover_kernel_and_the_trim_entries():
    from segalign_amd import engine as E
    res = kernel_resources("chaintrim.hip")
    assert sorted(res) == ["chaintrim_crossover_kernel"] and "chaintrim.hip" in SOURCES and "api_chaintrim.hip" in SOURCES
    r = res["chaintrim_crossover_kernel"]
    assert r["scratch"] == 0 and r["lds"] == 256 and 0 < r["vgprs"] <= 128, r  # LDS: the 64 matrix entries
    import ctypes as C
    assert E.TRIM_CHAIN_DTYPE.itemsize == 16 and E.TRIM_LINK_DTYPE.itemsize == 16 and C.sizeof(E.TrimStats) == 56
    for s in ("sa_trim_chains", "sa_free_trim"):
        assert hasattr(E.lib(), s) and s in E.C_ABI_SYMBOLS
