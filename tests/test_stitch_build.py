"""CPU: the stitching kernels (segalign_amd/csrc/stitch.hip) as the compiler reports them: the member kernel and one sweep
instance per K are there, none spills to scratch memory, each fits the registers of a 256-thread workgroup, and
`python -m segalign_amd.build --resources stitch.hip` prints them."""
import os
import subprocess
import sys

from segalign_amd.build import SOURCES, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["stitch_member_kernel"] + ["stitch_sweep_kernel<%d>" % k for k in (2, 4, 8, 17, 33)]


def test_stitch_kernels_use_no_scratch():
    assert "stitch.hip" in SOURCES and "api_stitch.hip" in SOURCES
    res = kernel_resources("stitch.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        # 512 registers per lane is what one wave per SIMD can have: four waves of a 256-thread workgroup on four SIMDs
        assert r["scratch"] == 0 and r["lds"] == 256 and 0 < r["vgprs"] + r["agprs"] <= 512 and r["occupancy"] >= 1, (k, r)
    assert res["stitch_sweep_kernel<2>"]["vgprs"] <= 64  # the small instance keeps full occupancy


def test_the_build_module_prints_the_unit():
    out = subprocess.run([sys.executable, "-m", "segalign_amd.build", "--resources", "stitch.hip"], cwd=ROOT, stdout=subprocess.PIPE, check=True)
    lines = out.stdout.decode().splitlines()
    assert sorted(ln.split()[0] for ln in lines) == sorted(KERNELS) and all(" scratch=0 " in ln for ln in lines)
