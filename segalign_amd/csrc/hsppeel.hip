// hsppeel.hip -- the kernels of sa_chain_hsps_all (contract: include/segalign_amd.h): the DP's pred forest peeled into
// all of its chains, best first.
//
// The sequential rule takes the nodes by priority (f descending, rank ascending) and gives every unused node its pred walk up to the
// first used node.  The device computes the same partition without that order: head(v) is the node of highest priority in v's subtree
// of the pred forest (v and every node whose pred walk reaches v; DESIGN.md 16 has the proof).  With prio[r] = r's position in the
// priority order that is a minimum over a subtree, found by pointer doubling: in round k a node hands the minimum it holds to the node
// 2^k links up its walk and then points 2^(k + 1) links up.  ceil(log2 n) rounds cover every walk, since a walk has fewer than n links.
//   The minimum is taken with atomicMin on uint32, the only atomic here.  A minimum does not depend on the order of its operands, so
// neither the order of the atomics nor the scheduling of the workgroups changes a result.  val is updated in place: a value a thread
// reads from val[r] during a round is the minimum of a set of nodes of r's subtree that holds every node the round's start value
// covered (values only fall, and every value that reaches val[r] comes from r's subtree), and r's subtree lies inside that of the node
// it is handed to.  So a round covers at least what the double-buffered round covers and never leaves the subtree: the final values are
// the same.  ptr is double-buffered, as a round reads the pointers of other nodes.
//   Everything else is one thread per node or per chain around rocPRIM's sorts and scans.  All arithmetic is int64 and uint32; no kernel
// waits for another workgroup, and every loop is bounded by the node count known at launch.
#include "hsppeel.h"

namespace sa {

namespace {

constexpr uint64_t SIGN = (uint64_t)1 << 63;

// Ascending order of the key is descending order of x.
__device__ __forceinline__ uint64_t descending(int64_t x) { return ~((uint64_t)x ^ SIGN); }

__global__ void __launch_bounds__(256) hsppeel_prio_key_kernel(HspPeelArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    a.key_a[r] = descending(a.f[r]);
    a.idx_a[r] = r;
}

__global__ void __launch_bounds__(256) hsppeel_init_kernel(HspPeelArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    a.val[a.byprio[p]] = p;
}

__global__ void __launch_bounds__(256) hsppeel_round_kernel(HspPeelArgs a, const uint32_t* ptr, uint32_t* ptr_next) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const uint32_t up = ptr[r];
    if (up == HSPCHAIN_NONE) {
        ptr_next[r] = HSPCHAIN_NONE;
        return;
    }
    atomicMin(&a.val[up], a.val[r]);
    ptr_next[r] = ptr[up];
}

__global__ void __launch_bounds__(256) hsppeel_tails_kernel(HspPeelArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const uint32_t h = a.byprio[a.val[r]], p = a.pred[r];
    a.head[r] = h;
    if (p != HSPCHAIN_NONE && a.byprio[a.val[p]] == h) return;
    a.cscore[h] = a.f[h] - (p != HSPCHAIN_NONE ? a.f[p] : 0);  // r is the chain's tail: the walk of h stopped at p, or ran out
    a.cjoin[h] = p;
}

__global__ void __launch_bounds__(256) hsppeel_chain_key_minor_kernel(HspPeelArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    a.key_a[r] = a.head[r] == r ? descending(a.cscore[r]) : ~(uint64_t)0;
    a.idx_a[r] = r;
}

__global__ void __launch_bounds__(256) hsppeel_chain_key_major_kernel(HspPeelArgs a, const uint32_t* idx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t r = idx[p];
    a.key_a[p] = (uint64_t)(a.head[r] == r ? 0u : 1u) << 32 | a.gr[r];
}

__global__ void __launch_bounds__(256) hsppeel_keep_kernel(HspPeelArgs a) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > a.n) return;
    if (c == a.n) {
        a.keep[c] = 0;
        return;
    }
    const uint32_t r = a.corder[c];
    const bool is_head = a.head[r] == r;
    a.keep[c] = (is_head && a.cscore[r] >= a.min_score) ? 1u : 0u;
    if (is_head) {  // the heads come first: the last of them knows their number
        bool last = c + 1 == a.n;
        if (!last) {
            const uint32_t nx = a.corder[c + 1];
            last = a.head[nx] != nx;
        }
        if (last) a.tot[2] = (uint64_t)c + 1;
    }
}

__global__ void __launch_bounds__(256) hsppeel_assign_kernel(HspPeelArgs a) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n) return;
    const uint32_t r = a.corder[c];
    a.cpos[r] = c;
    if (a.keep[c]) a.khead[a.kidx[c]] = r;
}

__global__ void __launch_bounds__(256) hsppeel_node_key_kernel(HspPeelArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    const uint32_t c = a.cpos[a.head[r]];
    const uint32_t k = a.keep[c] ? (uint32_t)a.kidx[c] : HSPCHAIN_NONE;
    a.key_a[r] = k;
    a.idx_a[r] = r;
    a.chain_of[a.order[r]] = k;
}

__global__ void __launch_bounds__(256) hsppeel_members_kernel(HspPeelArgs a, const uint64_t* key, const uint32_t* idx) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.n) return;
    const uint32_t k = (uint32_t)key[m], kept = (uint32_t)a.kidx[a.n];
    if (m == 0 || (uint32_t)key[m - 1] != k) a.first[k != HSPCHAIN_NONE ? k : kept] = m;  // k < kept <= n: first[] has n + 1 entries
    if (k == HSPCHAIN_NONE) return;
    if (m + 1 == a.n) a.first[kept] = a.n;  // no node of a dropped chain: the members end with the nodes
    const uint32_t r = idx[m];
    sa_chain_all_member x;
    x.hsp_index = a.order[r];
    x.group = a.gr[r];
    x.chain = k;
    x.pad = 0;
    x.f = a.f[r];
    a.members[m] = x;
}

__global__ void __launch_bounds__(256) hsppeel_records_kernel(HspPeelArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t kept = (uint32_t)a.kidx[a.n];
    if (k == 0) {
        a.tot[0] = kept;
        a.tot[1] = a.first[kept];
    }
    if (k >= kept) return;
    const uint32_t h = a.khead[k], j = a.cjoin[h];
    sa_chain_record x;
    x.group = a.gr[h];
    x.head = a.order[h];
    x.first_member = a.first[k];
    x.n_members = a.first[k + 1] - a.first[k];
    x.score = a.cscore[h];
    x.joined = j == HSPCHAIN_NONE ? -1 : (int32_t)a.order[j];
    x.pad = 0;
    a.chains[k] = x;
}

inline dim3 blocks(uint32_t n) { return dim3((n + 255) / 256); }

}  // namespace

void launch_hsppeel_prio_key(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_prio_key_kernel, blocks(a.n), dim3(256), 0, s, a); }

void launch_hsppeel_init(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_init_kernel, blocks(a.n), dim3(256), 0, s, a); }

void launch_hsppeel_round(const HspPeelArgs& a, const uint32_t* ptr, uint32_t* ptr_next, hipStream_t s) {
    hipLaunchKernelGGL(hsppeel_round_kernel, blocks(a.n), dim3(256), 0, s, a, ptr, ptr_next);
}

void launch_hsppeel_tails(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_tails_kernel, blocks(a.n), dim3(256), 0, s, a); }

void launch_hsppeel_chain_key_minor(const HspPeelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(hsppeel_chain_key_minor_kernel, blocks(a.n), dim3(256), 0, s, a);
}

void launch_hsppeel_chain_key_major(const HspPeelArgs& a, const uint32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(hsppeel_chain_key_major_kernel, blocks(a.n), dim3(256), 0, s, a, idx);
}

void launch_hsppeel_keep(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_keep_kernel, blocks(a.n + 1), dim3(256), 0, s, a); }

void launch_hsppeel_assign(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_assign_kernel, blocks(a.n), dim3(256), 0, s, a); }

void launch_hsppeel_node_key(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_node_key_kernel, blocks(a.n), dim3(256), 0, s, a); }

void launch_hsppeel_members(const HspPeelArgs& a, const uint64_t* key, const uint32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(hsppeel_members_kernel, blocks(a.n), dim3(256), 0, s, a, key, idx);
}

void launch_hsppeel_records(const HspPeelArgs& a, hipStream_t s) { hipLaunchKernelGGL(hsppeel_records_kernel, blocks(a.n), dim3(256), 0, s, a); }

}  // namespace sa
