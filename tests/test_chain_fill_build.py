"""CPU: the sa_fill_chains units compile for gfx950 without scratch, the library exports the entry, and the Python layouts are the
header's (include/segalign_amd.h)."""
import ctypes as C
import os
import subprocess
import sys

import chain_fill_model as F
from segalign_amd import engine as E
from segalign_amd.build import LIB_PATH, SOURCES, build_lib, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["fill_sweep_kernel<false>", "fill_sweep_kernel<true>", "fill_gather_kernel"]


def test_the_library_exports_the_entries():
    build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert "sa_fill_chains" in syms and "sa_free_fill" in syms
    assert "sa_fill_chains" in E.C_ABI_SYMBOLS and "sa_free_fill" in E.C_ABI_SYMBOLS


def test_the_struct_sizes_and_offsets():
    assert E.FILL_CHAIN_DTYPE.itemsize == 16 and E.FILL_LINK_DTYPE.itemsize == 32 and E.FILL_HSP_DTYPE.itemsize == 24
    assert C.sizeof(E.FillParams) == 32 and C.sizeof(E.FillStats) == 96
    assert E.FILL_CHAIN_DTYPE == F.CHAIN and E.FILL_LINK_DTYPE == F.LINK and E.FILL_HSP_DTYPE == F.HSP
    assert E.FILL_LINK_DTYPE.fields["cells"][1] == 24 and E.FILL_HSP_DTYPE.fields["link"][1] == 16
    assert E.FillParams.max_cells.offset == 16 and E.FillParams.min_fill.offset == 24 and E.FillStats.count_ms.offset == 72
    header = open(os.path.join(ROOT, "include", "segalign_amd.h")).read()
    for name, size in (("sa_fill_params", 32), ("sa_fill_chain", 16), ("sa_fill_link", 32), ("sa_fill_hsp", 24), ("sa_fill_stats", 96)):
        assert header.count("sizeof(%s) == %d" % (name, size)) == 2, name
    assert (E.FILL_LINKS, E.FILL_HSPS) == (1, 2) and "#define SA_FILL_LINKS 1u" in header and "#define SA_FILL_HSPS 2u" in header
    assert (E.FILL_LONG, E.FILL_LARGE, E.FILL_CROWDED) == (1, 2, 4) == (F.LONG, F.LARGE, F.CROWDED)
    for name, v in (("LONG", 1), ("LARGE", 2), ("CROWDED", 4)):
        assert "#define SA_FILL_%s %du" % (name, v) in header
    assert E.FILL_NONE == F.NONE == 0xFFFFFFFF and "#define SA_FILL_NONE 0xFFFFFFFFu" in header


def test_the_kernels_use_no_scratch():
    assert "fill.hip" in SOURCES and "api_fill.hip" in SOURCES
    res = kernel_resources("fill.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        # 64 registers: full occupancy of a 256-thread workgroup; the LDS is the 64 matrix entries
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 64 and r["lds"] in (0, 256), (k, r)


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "fill.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert len(lines) == 3 and all(ln.startswith("fill_") and " scratch=0 " in ln for ln in lines)
