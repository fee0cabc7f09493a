// hspchain.hip -- the kernels of sa_chain_hsps and, with a gap-cost table, of sa_chain_hsps_costs (contract: include/segalign_amd.h,
// DESIGN.md 15 and 20): rank, the DP's cross and resolve, and the finish.
//
// The DP itself (how a pair of nodes is offered, the LDS image of a tile, the bodies of cross and resolve) is hspchain_dp.h's, which
// also describes it; the two kernels here are its <COSTS, false> instances, COSTS being whether a gap-cost table is in force.  The
// <false, false> instances are sa_chain_hsps's kernels as they were, with no trace of the table.  The instances that let HSPs overlap
// are hspovl.hip's.
#include "hspchain_dp.h"

namespace sa {

namespace {

template <bool COSTS>
__global__ void __launch_bounds__(1024) hspchain_cross_kernel(HspChainArgs a, uint32_t b, uint32_t c0, HspChainPartial* partial, const uint32_t* image) {
    hspdp::cross_body<COSTS, false>(a, HspOvlNodes{nullptr, nullptr}, b, c0, partial, image);
}

template <bool COSTS>
__global__ void __launch_bounds__(1024) hspchain_resolve_kernel(HspChainArgs a, uint32_t b, uint32_t c0, const HspChainPartial* partial,
                                                                const uint32_t* image) {
    hspdp::resolve_body<COSTS, false>(a, HspOvlNodes{nullptr, nullptr}, b, c0, partial, image);
}

__global__ void __launch_bounds__(256) hspchain_key_minor_kernel(const sa_segment_pair* hsps, uint32_t n, uint64_t* key, uint32_t* idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = (uint64_t)hsps[i].query_start << 32 | hsps[i].len;
    idx[i] = i;
}

__global__ void __launch_bounds__(256) hspchain_key_major_kernel(const sa_segment_pair* hsps, const uint32_t* group, const uint32_t* idx, uint32_t n,
                                                                 uint64_t* key) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = idx[p];
    key[p] = (uint64_t)(group ? group[i] : 0u) << 32 | hsps[i].ref_start;
}

__global__ void __launch_bounds__(256) hspchain_gather_kernel(const sa_segment_pair* hsps, const uint32_t* group, const uint32_t* order, uint32_t n,
                                                              uint32_t* rs, uint32_t* qs, uint32_t* ln, int32_t* sc, uint32_t* gr, uint32_t* head) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        head[n] = 0;
        return;
    }
    const uint32_t i = order[r];
    const sa_segment_pair h = hsps[i];
    const uint32_t g = group ? group[i] : 0u;
    rs[r] = h.ref_start;
    qs[r] = h.query_start;
    ln[r] = h.len;
    sc[r] = h.score;
    gr[r] = g;
    head[r] = (r == 0 || (group && group[order[r - 1]] != g)) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) hspchain_first_kernel(const uint32_t* gr, uint32_t n, uint32_t tile, uint32_t* first) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if ((uint64_t)b * tile >= n) return;
    const uint32_t g = gr[b * tile];
    uint32_t lo = 0, hi = b * tile;  // first rank of group g: gr is ascending
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (gr[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    first[b] = lo / tile;
}

__global__ void __launch_bounds__(256) hspchain_group_starts_kernel(const uint32_t* head, const uint64_t* gidx, uint32_t n, uint32_t* gstart) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && head[r]) gstart[gidx[r]] = r;
}

__global__ void __launch_bounds__(256) hspchain_ends_kernel(HspChainArgs a, const uint32_t* gstart, uint32_t groups, int64_t min_score, uint32_t* gend,
                                                            uint32_t* glen) {
    const uint32_t g = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (g > groups) return;
    if (g == groups) {
        if (lane == 0) glen[g] = 0;
        return;
    }
    const uint32_t lo = gstart[g], hi = g + 1 < groups ? gstart[g + 1] : a.n;
    int64_t bf = INT64_MIN;
    uint32_t br = HSPCHAIN_NONE;
    for (uint32_t r = lo + lane; r < hi; r += 64) {  // ascending per lane: strictly larger keeps the lowest rank
        const int64_t x = a.f[r];
        if (br == HSPCHAIN_NONE || x > bf) {
            bf = x;
            br = r;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t of = __shfl_xor(bf, d);
        const uint32_t orank = __shfl_xor(br, d);
        if (orank != HSPCHAIN_NONE && (br == HSPCHAIN_NONE || of > bf || (of == bf && orank < br))) {
            bf = of;
            br = orank;
        }
    }
    if (lane != 0) return;
    uint32_t len = 0;
    if (bf >= min_score)
        for (uint32_t r = br; r != HSPCHAIN_NONE && len < hi - lo; r = a.pred[r]) len++;  // a chain has at most the group's nodes
    gend[g] = br;
    glen[g] = len;
}

__global__ void __launch_bounds__(256) hspchain_members_kernel(HspChainArgs a, const uint32_t* order, const uint32_t* gend, const uint32_t* glen,
                                                               const uint64_t* goff, uint32_t groups, sa_chain_member* out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    const uint64_t off = goff[g];
    uint32_t r = gend[g];
    for (uint32_t k = glen[g]; k > 0; k--) {  // the walk runs from the end: fill from the back
        sa_chain_member m;
        m.hsp_index = order[r];
        m.group = a.gr[r];
        m.f = a.f[r];
        out[off + k - 1] = m;
        r = a.pred[r];
    }
}

__global__ void __launch_bounds__(256) hspchain_nodes_kernel(HspChainArgs a, const uint32_t* order, sa_chain_node* nodes) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    sa_chain_node x;
    x.f = a.f[r];
    x.pred = a.pred[r] == HSPCHAIN_NONE ? -1 : (int32_t)order[a.pred[r]];
    x.pad = 0;
    nodes[order[r]] = x;
}

inline dim3 blocks(uint32_t n) { return dim3((n + 255) / 256); }
}  // namespace

void launch_hspchain_key_minor(const sa_segment_pair* hsps, uint32_t n, uint64_t* key, uint32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_key_minor_kernel, blocks(n), dim3(256), 0, s, hsps, n, key, idx);
}

void launch_hspchain_key_major(const sa_segment_pair* hsps, const uint32_t* group, const uint32_t* idx, uint32_t n, uint64_t* key, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_key_major_kernel, blocks(n), dim3(256), 0, s, hsps, group, idx, n, key);
}

void launch_hspchain_gather(const sa_segment_pair* hsps, const uint32_t* group, const uint32_t* order, uint32_t n, uint32_t* rs, uint32_t* qs,
                            uint32_t* ln, int32_t* sc, uint32_t* gr, uint32_t* head, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_gather_kernel, blocks(n + 1), dim3(256), 0, s, hsps, group, order, n, rs, qs, ln, sc, gr, head);
}

void launch_hspchain_first(const uint32_t* gr, uint32_t n, uint32_t tile, uint32_t* first, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_first_kernel, blocks((n + tile - 1) / tile), dim3(256), 0, s, gr, n, tile, first);
}

void launch_hspchain_cross(const HspChainArgs& a, uint32_t b, uint32_t c0, HspChainPartial* partial, const uint32_t* image, hipStream_t s) {
    if (b <= c0) return;
    const auto kernel = image ? hspchain_cross_kernel<true> : hspchain_cross_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(b - c0), dim3(a.tile), hspdp::tile_lds(a.tile, image, false), s, a, b, c0, partial, image);
}

void launch_hspchain_resolve(const HspChainArgs& a, uint32_t b, uint32_t c0, const HspChainPartial* partial, const uint32_t* image, hipStream_t s) {
    const auto kernel = image ? hspchain_resolve_kernel<true> : hspchain_resolve_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(a.tile), hspdp::tile_lds(a.tile, image, false), s, a, b, c0, partial, image);
}

void launch_hspchain_group_starts(const uint32_t* head, const uint64_t* gidx, uint32_t n, uint32_t* gstart, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_group_starts_kernel, blocks(n), dim3(256), 0, s, head, gidx, n, gstart);
}

void launch_hspchain_ends(const HspChainArgs& a, const uint32_t* gstart, uint32_t groups, int64_t min_score, uint32_t* gend, uint32_t* glen,
                          hipStream_t s) {
    hipLaunchKernelGGL(hspchain_ends_kernel, dim3((groups + 1 + 3) / 4), dim3(256), 0, s, a, gstart, groups, min_score, gend, glen);
}

void launch_hspchain_members(const HspChainArgs& a, const uint32_t* order, const uint32_t* gend, const uint32_t* glen, const uint64_t* goff,
                             uint32_t groups, sa_chain_member* out, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_members_kernel, blocks(groups), dim3(256), 0, s, a, order, gend, glen, goff, groups, out);
}

void launch_hspchain_nodes(const HspChainArgs& a, const uint32_t* order, sa_chain_node* nodes, hipStream_t s) {
    hipLaunchKernelGGL(hspchain_nodes_kernel, blocks(a.n), dim3(256), 0, s, a, order, nodes);
}

}  // namespace sa
