"""CPU: the chaining kernels (segalign_amd/csrc/hspchain.hip) as the compiler reports them: every kernel is there and none
spills to scratch memory.  The two DP kernels are templates on whether a gap-cost table is in force: both instances count."""
from segalign_amd.build import kernel_resources

KERNELS = ["hspchain_cross_kernel<false>", "hspchain_cross_kernel<true>", "hspchain_resolve_kernel<false>", "hspchain_resolve_kernel<true>",
           "hspchain_key_minor_kernel", "hspchain_key_major_kernel",
           "hspchain_gather_kernel", "hspchain_first_kernel", "hspchain_group_starts_kernel", "hspchain_ends_kernel",
           "hspchain_members_kernel", "hspchain_nodes_kernel"]


def test_chain_kernels_use_no_scratch():
    res = kernel_resources("hspchain.hip")
    assert sorted(res) == sorted(KERNELS)
    for k, r in res.items():
        assert r["scratch"] == 0 and 0 < r["vgprs"] <= 128, (k, r)  # 128: what a workgroup of 1024 threads leaves a lane
