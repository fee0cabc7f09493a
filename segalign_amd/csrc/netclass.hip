// netclass.hip -- the kernels of sa_net_classify (contract: include/segalign_amd.h): where every fill of a net lands on the
// other axis relative to its parent, and how many of its bases there another fill claims too.
//
// Everything is one thread per fill, per clipped block or per event.  What orders the steps is the stream, one sort (cover.hip's
// wrapper) and four prefix sums (scan.hip) between them:
//
//   counts -> scan -> off        a fill's first position among the clipped blocks
//   emit                         the clipped other interval of a block, and its two events keyed (ogroup, coordinate, is_start)
//   sort                         at one coordinate of one ogroup an end comes before a start: abutting blocks share no base
//   flags -> scan -> starts      the depth after sorted event i is 2 starts[i + 1] - (i + 1): every ogroup's events balance
//   segments -> scan -> dup      the bases of depth >= 2 before every event
//   block_dup -> scan -> bsum    per block the difference of two prefix values, per fill again
//   classes, keep                the record; with the filter a walk up the parents, at most depth steps
//
// Plain C++ on uint32 / uint64 / int64, no atomics, no scratch; every loop is bounded at launch (a binary search: at most 32 steps; the
// walk: the fill's depth).  The host has validated every index the kernels form (netclass.h).
#include "netclass.h"

namespace sa {

namespace {

constexpr int THREADS = 256;

struct Hull {
    uint32_t s, e;
};

__device__ __forceinline__ uint32_t group_of(const NetClassArgs& a, uint32_t chain) { return a.ogroup ? a.ogroup[chain] : 0u; }
__device__ __forceinline__ uint32_t strand_of(const NetClassArgs& a, uint32_t chain) { return a.ostrand ? (uint32_t)a.ostrand[chain] : 0u; }

// The other hull of fill k: the outer ends of its first and last clipped block, which of the two depending on the strand.
__device__ __forceinline__ Hull hull_of(const NetClassArgs& a, uint32_t k, uint32_t strand) {
    const uint32_t b = (uint32_t)a.off[k], e = (uint32_t)a.off[k + 1] - 1;
    return strand ? Hull{a.cs[e], a.ce[b]} : Hull{a.cs[b], a.ce[e]};
}

__global__ __launch_bounds__(THREADS) void netclass_counts_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i < a.F) a.cnt[i] = a.fills[i].n_blocks;
}

__global__ __launch_bounds__(THREADS) void netclass_emit_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.M) return;
    uint32_t lo = 0, hi = a.F;  // the fill: the last one with off <= i; off ascends strictly, every fill having a block
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const sa_net_fill f = a.fills[lo];
    const uint32_t k = f.first_block + (i - (uint32_t)a.off[lo]);
    const uint32_t bs = a.bs[k], be = a.be[k];
    const uint32_t dl = max(bs, f.start) - bs, dr = be - min(be, f.end);
    const bool minus = strand_of(a, f.chain) != 0;
    const uint32_t s = a.obs[k] + (minus ? dr : dl), e = a.obe[k] - (minus ? dl : dr);
    const uint64_t g = (uint64_t)group_of(a, f.chain) << 32;
    a.cs[i] = s;
    a.ce[i] = e;
    a.key[2 * i] = g | ((uint64_t)s << 1) | 1u;
    a.key[2 * i + 1] = g | ((uint64_t)e << 1);
    a.val[2 * i] = 2 * i;
    a.val[2 * i + 1] = 2 * i + 1;
}

__global__ __launch_bounds__(THREADS) void netclass_flags_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.E) return;
    a.flag[i] = (uint32_t)a.skey[i] & 1u;
    a.pos[a.sval[i]] = i;  // a permutation: every slot is written once
}

__global__ __launch_bounds__(THREADS) void netclass_segments_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.E) return;
    uint32_t seg = 0;
    if (i + 1 < a.E) {
        const uint64_t x = a.skey[i], y = a.skey[i + 1];
        const uint32_t depth = 2 * a.starts[i + 1] - (i + 1);
        if (depth >= 2 && (x >> 32) == (y >> 32)) seg = ((uint32_t)y >> 1) - ((uint32_t)x >> 1);
    }
    a.seg[i] = seg;
}

__global__ __launch_bounds__(THREADS) void netclass_block_dup_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i < a.M) a.bdup[i] = (uint32_t)(a.dup[a.pos[2 * i + 1]] - a.dup[a.pos[2 * i]]);  // at most the block's length
}

__global__ __launch_bounds__(THREADS) void netclass_classes_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.F) return;
    const sa_net_fill f = a.fills[i];
    const uint32_t strand = strand_of(a, f.chain), group = group_of(a, f.chain);
    const Hull h = hull_of(a, i, strand);
    uint32_t type = SA_NETCLASS_TOP, over = 0, far = 0;
    if (f.parent >= 0) {
        const uint32_t pc = a.fills[f.parent].chain, ps = strand_of(a, pc);
        if (group_of(a, pc) != group) {
            type = SA_NETCLASS_NONSYN;
        } else {
            const Hull p = hull_of(a, (uint32_t)f.parent, ps);
            const int64_t x = (int64_t)min(h.e, p.e) - (int64_t)max(h.s, p.s);
            if (x > 0) over = (uint32_t)x;
            else far = (uint32_t)-x;
            type = ps == strand ? SA_NETCLASS_SYN : SA_NETCLASS_INV;
        }
    }
    bool self = true;
    if (a.filter) {
        self = f.score >= a.p.min_score && f.end - f.start >= a.p.min_size && f.ali >= a.p.min_ali;
        if (type == SA_NETCLASS_TOP) self = self && f.score >= a.p.min_top_score;
        else if (type == SA_NETCLASS_NONSYN) self = false;
        else self = self && far <= a.p.max_far;
    }
    a.self[i] = self ? 1 : 0;
    const uint32_t odup = (uint32_t)(a.bsum[a.off[i + 1]] - a.bsum[a.off[i]]);
    uint4* o = reinterpret_cast<uint4*>(a.out + i);  // the 32-byte record as two 16-byte stores
    o[0] = make_uint4(h.s, h.e, over, far);
    o[1] = make_uint4(odup, group, type | (strand << 8) | ((self ? 1u : 0u) << 16), 0u);
}

__global__ __launch_bounds__(THREADS) void netclass_keep_kernel(NetClassArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.F) return;
    uint32_t keep = a.self[i];
    int32_t p = a.fills[i].parent;
    for (uint32_t d = a.fills[i].depth; keep && d > 0 && p >= 0; d--) {  // depth steps reach the root (the host has checked it)
        keep = a.self[p];
        p = a.fills[p].parent;
    }
    a.out[i].keep = (uint8_t)keep;
}

inline dim3 grid_for(uint32_t n) { return dim3((n + THREADS - 1) / THREADS); }

}  // namespace

void launch_netclass_counts(const NetClassArgs& a, hipStream_t s) {
    if (a.F) hipLaunchKernelGGL(netclass_counts_kernel, grid_for(a.F), dim3(THREADS), 0, s, a);
}

void launch_netclass_emit(const NetClassArgs& a, hipStream_t s) {
    if (a.M) hipLaunchKernelGGL(netclass_emit_kernel, grid_for(a.M), dim3(THREADS), 0, s, a);
}

void launch_netclass_flags(const NetClassArgs& a, hipStream_t s) {
    if (a.E) hipLaunchKernelGGL(netclass_flags_kernel, grid_for(a.E), dim3(THREADS), 0, s, a);
}

void launch_netclass_segments(const NetClassArgs& a, hipStream_t s) {
    if (a.E) hipLaunchKernelGGL(netclass_segments_kernel, grid_for(a.E), dim3(THREADS), 0, s, a);
}

void launch_netclass_block_dup(const NetClassArgs& a, hipStream_t s) {
    if (a.M) hipLaunchKernelGGL(netclass_block_dup_kernel, grid_for(a.M), dim3(THREADS), 0, s, a);
}

void launch_netclass_classes(const NetClassArgs& a, hipStream_t s) {
    if (a.F) hipLaunchKernelGGL(netclass_classes_kernel, grid_for(a.F), dim3(THREADS), 0, s, a);
}

void launch_netclass_keep(const NetClassArgs& a, hipStream_t s) {
    if (a.F) hipLaunchKernelGGL(netclass_keep_kernel, grid_for(a.F), dim3(THREADS), 0, s, a);
}

}  // namespace sa
