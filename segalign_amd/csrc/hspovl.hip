// hspovl.hip -- the DP kernels of sa_chain_hsps_ovl and sa_chain_hsps_all_ovl (contract: include/segalign_amd.h): the
// <COSTS, true> instances of hspchain_dp.h's cross and resolve, under which HSPs that share up to max_overlap bases still link, and the
// weight kernel that makes what those instances know of a node beyond sa_chain_hsps's fields.  Rank, finish and peel are hspchain.hip's
// and hsppeel.hip's as they are.
#include "hspchain_dp.h"

namespace sa {

namespace {

template <bool COSTS>
__global__ void __launch_bounds__(1024) hspovl_cross_kernel(HspChainArgs a, HspOvlNodes o, uint32_t b, uint32_t c0, HspChainPartial* partial,
                                                            const uint32_t* image) {
    hspdp::cross_body<COSTS, true>(a, o, b, c0, partial, image);
}

template <bool COSTS>
__global__ void __launch_bounds__(1024) hspovl_resolve_kernel(HspChainArgs a, HspOvlNodes o, uint32_t b, uint32_t c0, const HspChainPartial* partial,
                                                              const uint32_t* image) {
    hspdp::resolve_body<COSTS, true>(a, o, b, c0, partial, image);
}

// One thread per node: the only division of the overlap DP.  max(score, 0) < 2^31, so the dividend is below 2^47.
__global__ void __launch_bounds__(256) hspovl_weight_kernel(const uint32_t* ln, const int32_t* sc, uint32_t n, uint32_t max_overlap, int64_t* w,
                                                            uint32_t* lim) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t len = ln[r];
    const int64_t score = sc[r] > 0 ? sc[r] : 0;
    w[r] = (int64_t)((uint64_t)(score << 16) / ((uint64_t)len + 1));
    lim[r] = min(len >> 1, max_overlap);  // 2 o < bases = len + 1 is o <= len >> 1
}

}  // namespace

void launch_hspovl_weight(const HspChainArgs& a, uint32_t max_overlap, int64_t* w, uint32_t* lim, hipStream_t s) {
    hipLaunchKernelGGL(hspovl_weight_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a.ln, a.sc, a.n, max_overlap, w, lim);
}

void launch_hspovl_cross(const HspChainArgs& a, const HspOvlNodes& o, uint32_t b, uint32_t c0, HspChainPartial* partial, const uint32_t* image,
                         hipStream_t s) {
    if (b <= c0) return;
    const auto kernel = image ? hspovl_cross_kernel<true> : hspovl_cross_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(b - c0), dim3(a.tile), hspdp::tile_lds(a.tile, image, true), s, a, o, b, c0, partial, image);
}

void launch_hspovl_resolve(const HspChainArgs& a, const HspOvlNodes& o, uint32_t b, uint32_t c0, const HspChainPartial* partial,
                           const uint32_t* image, hipStream_t s) {
    const auto kernel = image ? hspovl_resolve_kernel<true> : hspovl_resolve_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(a.tile), hspdp::tile_lds(a.tile, image, true), s, a, o, b, c0, partial, image);
}

}  // namespace sa
