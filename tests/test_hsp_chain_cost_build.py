"""CPU: the gap-cost DP kernels (segalign_amd/csrc/hspcost.hip) as the compiler reports them: both kernels are there,
neither spills to scratch memory, and both fit a workgroup of 1 024 threads."""
from segalign_amd.build import SOURCES, kernel_resources

KERNELS = ["hspcost_cross_kernel", "hspcost_resolve_kernel"]


def test_cost_kernels_use_no_scratch():
    assert "hspcost.hip" in SOURCES
    res = kernel_resources("hspcost.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 128, (k, r)  # 128: what a workgroup of 1024 threads leaves a lane
        assert r["lds"] == 0, (k, r)  # the tile image and the cost image are dynamic LDS
