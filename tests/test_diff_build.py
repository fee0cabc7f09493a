"""CPU: the sa_diff_alignments units compile for gfx950 without scratch, the library exports the entry, and the Python layouts are the
header's (include/segalign_amd.h)."""
import ctypes as C
import os
import subprocess
import sys

import diff_model as D
from segalign_amd import engine as E
from segalign_amd.build import LIB_PATH, SOURCES, build_lib, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["diff_span_of_kernel", "diff_values_kernel", "diff_items_kernel", "diff_pass_kernel<false>", "diff_pass_kernel<true>",
           "diff_finish_kernel", "diff_summaries_kernel"]


def test_the_library_exports_the_entries():
    build_lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert "sa_diff_alignments" in syms and "sa_free_diff" in syms
    assert "sa_diff_alignments" in E.C_ABI_SYMBOLS and "sa_free_diff" in E.C_ABI_SYMBOLS


def test_the_struct_sizes_and_offsets():
    assert E.DIFF_SPAN_DTYPE.itemsize == 24 and E.DIFF_EVENT_DTYPE.itemsize == 24 and E.DIFF_SUMMARY_DTYPE.itemsize == 48
    assert C.sizeof(E.DiffParams) == 8 and C.sizeof(E.DiffStats) == 568
    assert E.DIFF_SPAN_DTYPE == D.SPAN_DTYPE and E.DIFF_EVENT_DTYPE == D.EVENT_DTYPE and E.DIFF_SUMMARY_DTYPE == D.SUMMARY_DTYPE
    assert E.DIFF_SPAN_DTYPE.fields["op_offset"][1] == 8 and E.DIFF_EVENT_DTYPE.fields["kind"][1] == 20
    assert E.DIFF_SUMMARY_DTYPE.fields["n_events"][1] == 8 and E.DIFF_SUMMARY_DTYPE.fields["del_bases"][1] == 44
    assert E.DiffStats.pairs.offset == 40 and E.DiffStats.prep_ms.offset == 552 and E.DiffStats.emit_ms.offset == 560
    header = open(os.path.join(ROOT, "include", "segalign_amd.h")).read()
    for name, size in (("sa_diff_span", 24), ("sa_diff_params", 8), ("sa_diff_event", 24), ("sa_diff_summary", 48), ("sa_diff_stats", 568)):
        assert header.count("sizeof(%s) == %d" % (name, size)) == 2, name
    assert (E.DIFF_PER_BASE, E.DIFF_NO_EVENTS) == (1, 2) and "#define SA_DIFF_PER_BASE 1u" in header and "#define SA_DIFF_NO_EVENTS 2u" in header
    for name, v in (("SUB", 0), ("OTHER", 1), ("INS", 2), ("DEL", 3), ("NO_CODE", 8)):
        assert "#define SA_DIFF_%s %du" % (name, v) in header and getattr(E, "DIFF_" + name) == getattr(D, name) == v


def test_the_kernels_use_no_scratch():
    assert "diff.hip" in SOURCES and "api_diff.hip" in SOURCES
    res = kernel_resources("diff.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        # 64 registers: full occupancy of a 256-thread workgroup; the pair counts stay in registers, so no LDS
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 64 and r["lds"] == 0, (k, r)


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "diff.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert len(lines) == len(KERNELS) and all(ln.startswith("diff_") and " scratch=0 " in ln for ln in lines)
