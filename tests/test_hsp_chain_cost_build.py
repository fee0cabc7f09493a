"""CPU: the gap-cost instances of the DP kernels (the <true> instances in segalign_amd/csrc/hspchain.hip) as the compiler
reports them: both are there, neither spills to scratch memory, and both fit a workgroup of 1 024 threads."""
from segalign_amd.build import kernel_resources

KERNELS = ["hspchain_cross_kernel<true>", "hspchain_resolve_kernel<true>"]


def test_cost_kernels_use_no_scratch():
    res = kernel_resources("hspchain.hip")
    for k in KERNELS:
        assert k in res, (k, sorted(res))
        r = res[k]
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 128, (k, r)  # 128: what a workgroup of 1024 threads leaves a lane
        assert r["lds"] == 0, (k, r)  # the tile image and the cost image are dynamic LDS
