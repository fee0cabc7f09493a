"""CPU: the peeling kernels (segalign_amd/csrc/hsppeel.hip) as the compiler reports them: every kernel is there, none
spills to scratch memory or uses LDS, and `python -m segalign_amd.build --resources hsppeel.hip` prints them."""
import os
import subprocess
import sys

from segalign_amd.build import SOURCES, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["hsppeel_prio_key_kernel", "hsppeel_init_kernel", "hsppeel_round_kernel", "hsppeel_tails_kernel", "hsppeel_chain_key_minor_kernel",
           "hsppeel_chain_key_major_kernel", "hsppeel_keep_kernel", "hsppeel_assign_kernel", "hsppeel_node_key_kernel",
           "hsppeel_members_kernel", "hsppeel_records_kernel"]


def test_peel_kernels_use_no_scratch():
    assert "hsppeel.hip" in SOURCES
    res = kernel_resources("hsppeel.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and r["lds"] == 0 and 0 < r["vgprs"] <= 64, (k, r)  # 64: full occupancy of a 256-thread workgroup


def test_the_build_module_prints_a_named_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "hsppeel.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert sorted(ln.split()[0] for ln in lines) == sorted(KERNELS) and all(" scratch=0 " in ln for ln in lines)
