"""CPU: sa_net_classify as built (segalign_amd/csrc/netclass.hip, api_netclass.hip): the library exports the two entries,
the records have the sizes the header asserts, every kernel is there and none spills to scratch memory, and
`python -m segalign_amd.build --resources netclass.hip` prints them."""
import ctypes as C
import os
import subprocess
import sys

from segalign_amd import engine as E
from segalign_amd.build import LIB_PATH, SOURCES, build_lib, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["netclass_counts_kernel", "netclass_emit_kernel", "netclass_flags_kernel", "netclass_segments_kernel",
           "netclass_block_dup_kernel", "netclass_classes_kernel", "netclass_keep_kernel"]


def test_the_library_exports_the_entries():
    build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert "sa_net_classify" in syms and "sa_free_net_class" in syms
    assert "sa_net_classify" in E.C_ABI_SYMBOLS and "sa_free_net_class" in E.C_ABI_SYMBOLS


def test_the_struct_sizes():
    assert E.NET_CLASS_DTYPE.itemsize == 32 and C.sizeof(E.NetClassParams) == 32 and C.sizeof(E.NetClassStats) == 88 and E.NETCLASS_FILTER == 1
    assert E.NET_CLASS_DTYPE.fields["ogroup"][1] == 20 and E.NET_CLASS_DTYPE.fields["type"][1] == 24 and E.NET_CLASS_DTYPE.fields["keep"][1] == 26
    assert E.NetClassParams.min_size.offset == 16 and E.NetClassStats.n_type.offset == 32 and E.NetClassStats.class_ms.offset == 80
    header = open(os.path.join(ROOT, "include", "segalign_amd.h")).read()
    assert header.count("sizeof(sa_net_class) == 32") == 2 and header.count("sizeof(sa_net_class_params) == 32") == 2
    assert header.count("sizeof(sa_net_class_stats) == 88") == 2
    assert (E.NETCLASS_TOP, E.NETCLASS_SYN, E.NETCLASS_INV, E.NETCLASS_NONSYN) == (0, 1, 2, 3) and E.NETCLASS_NAMES == ("top", "syn", "inv", "nonSyn")


def test_the_kernels_use_no_scratch():
    assert "netclass.hip" in SOURCES and "api_netclass.hip" in SOURCES
    res = kernel_resources("netclass.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 64 and r["lds"] == 0, (k, r)  # 64: full occupancy of a 256-thread workgroup


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "netclass.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert sorted(ln.split()[0] for ln in lines) == sorted(KERNELS) and all(" scratch=0 " in ln for ln in lines)
