"""CPU: the net kernels (segalign_amd/csrc/net.hip) as the compiler reports them: every kernel is there, none spills to
scratch memory or uses LDS, and `python -m segalign_amd.build --resources net.hip` prints them."""
import os
import subprocess
import sys

from segalign_amd.build import SOURCES, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["net_block_len_kernel", "net_key_minor_kernel", "net_key_major_kernel", "net_gather_kernel", "net_group_starts_kernel",
           "net_roots_kernel", "net_search_kernel", "net_count_kernel", "net_emit_kernel", "net_fill_key_kernel", "net_inverse_kernel",
           "net_finish_kernel"]


def test_net_kernels_use_no_scratch():
    assert "net.hip" in SOURCES and "api_net.hip" in SOURCES
    res = kernel_resources("net.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and r["lds"] == 0 and 0 < r["vgprs"] <= 64, (k, r)  # 64: full occupancy of a 256-thread workgroup


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "net.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert sorted(ln.split()[0] for ln in lines) == sorted(KERNELS) and all(" scratch=0 " in ln for ln in lines)
