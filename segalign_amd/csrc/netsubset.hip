// netsubset.hip -- the kernels of sa_net_subset (contract: include/segalign_amd.h): the fills of a net cut into sub-chains.
//
// Everything is one thread per fill, per output member or per run, but the rescore, which is one wavefront per cut member in
// stitch.hip's member-kernel shape.  What orders the steps is the stream and three prefix sums (scan.hip) between them:
//
//   counts -> scan -> off        a fill's first position in the output
//   mark                         a fill with a parent stores 1 behind the parent's block it follows; equal stores, no atomic
//   emit                         the clipped member, which sides were cut, whether it heads a run
//   scans of head and is_cut     run indices, and the cut members as a dense list so that uncut members launch no wave
//   rescore                      the matrix summed over the kept diagonal, int64
//   terms -> two scans           score - pen' as two 32-bit halves: the scan takes uint32 and sums in uint64, and
//                                sum(lo) + (sum(hi) << 32) is the sum in two's complement, modulo 2^64
//   chains                       a run's record: the difference of two prefix values, the hull, the flags
//
// Plain C++ on uint32 / int64, no atomics, no scratch; every loop is bounded at launch (a binary search: at most 32 steps; the rescore:
// the member's length).  The host has validated every index the kernels form (netsubset.h).
#include "netsubset.h"

namespace sa {

namespace {

constexpr int THREADS = 256;

struct Block {  // a member's interval on the axis
    uint32_t s, e;
};

__device__ __forceinline__ sa_segment_pair load_hsp(const sa_segment_pair* p) {  // one 16-byte load
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    sa_segment_pair h;
    h.ref_start = v.x;
    h.query_start = v.y;
    h.len = v.z;
    h.score = (int32_t)v.w;
    return h;
}

__device__ __forceinline__ Block block_of(const sa_segment_pair& h, uint32_t axis) {
    const uint32_t s = axis ? h.query_start : h.ref_start;
    return {s, s + h.len + 1};
}

__global__ __launch_bounds__(THREADS) void netsubset_counts_kernel(NetSubsetArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i < a.F) a.cnt[i] = a.fills[i].n_blocks;
}

__global__ __launch_bounds__(THREADS) void netsubset_mark_kernel(NetSubsetArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.F) return;
    const int32_t parent = a.fills[i].parent;
    if (parent < 0) return;
    const uint32_t start = a.fills[i].start;
    const sa_net_fill P = a.fills[parent];
    if (P.n_blocks < 2) return;  // (the host has refused it)
    // the last block k of 0 .. n_blocks - 2 whose clipped end is at or before start; block 0 is one, as the fill lies in a gap of P
    uint32_t lo = 0, hi = P.n_blocks - 1;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t e = min(block_of(load_hsp(a.mh + P.first_block + mid), a.axis).e, P.end);
        if (e <= start) lo = mid;
        else hi = mid;
    }
    a.mark[a.off[parent] + lo] = 1;
}

__global__ __launch_bounds__(THREADS) void netsubset_emit_kernel(NetSubsetArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.N) return;
    uint32_t lo = 0, hi = a.F;  // the fill: the last one with off <= i; off ascends strictly, every fill having a block
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const sa_net_fill f = a.fills[lo];
    const uint32_t j = i - (uint32_t)a.off[lo];
    const sa_segment_pair h = load_hsp(a.mh + f.first_block + j);
    const Block b = block_of(h, a.axis);
    const uint32_t s = max(b.s, f.start), e = min(b.e, f.end), d = s - b.s;
    const uint32_t side = (b.s < f.start ? 1u : 0u) | (b.e > f.end ? 2u : 0u);
    *reinterpret_cast<uint4*>(a.out + i) = make_uint4(h.ref_start + d, h.query_start + d, e - s - 1, (uint32_t)h.score);
    a.fill_of[i] = lo;
    a.side[i] = side;
    a.is_cut[i] = side ? 1u : 0u;
    a.head[i] = (j == 0 || a.mark[i - 1]) ? 1u : 0u;
    a.score[i] = h.score;
}

__global__ __launch_bounds__(THREADS) void netsubset_cut_list_kernel(NetSubsetArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i < a.N && a.is_cut[i]) a.cut_list[a.cut_at[i]] = i;
}

__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(THREADS) void netsubset_rescore_kernel(NetSubsetArgs a, uint32_t n_cut) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t w = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (w >= n_cut) return;
    const int lane = threadIdx.x & 63;
    const uint32_t i = a.cut_list[w];
    const sa_segment_pair h = load_hsp(a.out + i);
    const uint8_t* x = a.ref + h.ref_start;
    const uint8_t* y = a.query + h.query_start;
    const uint64_t bases = (uint64_t)h.len + 1;
    long long sum = 0;
    for (uint64_t k = lane; k < bases; k += 64) sum += s_sub[(x[k] & 7) * 8 + (y[k] & 7)];
    sum = wave_sum64(sum);
    if (lane == 0) {
        a.score[i] = sum;
        a.out[i].score = (int32_t)min(max(sum, (long long)INT32_MIN), (long long)INT32_MAX);
    }
}

__global__ __launch_bounds__(THREADS) void netsubset_terms_kernel(NetSubsetArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i == 0) a.run_start[a.run[a.N]] = a.N;
    if (i >= a.N) return;
    int64_t v = a.score[i];
    if (a.head[i]) {
        a.run_start[a.run[i]] = i;
    } else {
        const sa_segment_pair p = load_hsp(a.out + i - 1), m = load_hsp(a.out + i);
        const int64_t re = (int64_t)p.ref_start + p.len + 1, qe = (int64_t)p.query_start + p.len + 1;
        const int64_t rs = m.ref_start, qs = m.query_start;
        const int64_t dd = (rs - qs) - ((int64_t)p.ref_start - (int64_t)p.query_start);
        int64_t pen = (int64_t)a.diag_pen * (dd < 0 ? -dd : dd) + (int64_t)a.anti_pen * ((rs + qs) - (re + qe));
        if (a.image) pen += hspcost_gapcost(a.image, rs - re, qs - qe);  // from global memory: one thread per link, no tile to share the image with
        v -= pen;
    }
    a.lo[i] = (uint32_t)(uint64_t)v;
    a.hi[i] = (uint32_t)((uint64_t)v >> 32);
}

__global__ __launch_bounds__(THREADS) void netsubset_chains_kernel(NetSubsetArgs a, uint32_t runs) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= runs) return;
    const uint32_t b = a.run_start[r], e = a.run_start[r + 1];
    const uint32_t fill = a.fill_of[b];
    const sa_net_fill f = a.fills[fill];
    const sa_segment_pair x = load_hsp(a.out + b), y = load_hsp(a.out + e - 1);
    sa_subset_chain c;
    c.fill = fill;
    c.chain = f.chain;
    c.group = f.group;
    c.run = r - (uint32_t)a.run[a.off[fill]];
    c.first_member = b;
    c.n_members = e - b;
    c.ref_start = x.ref_start;
    c.ref_end = y.ref_start + y.len + 1;
    c.query_start = x.query_start;
    c.query_end = y.query_start + y.len + 1;
    c.score = (int64_t)((a.sum_lo[e] + (a.sum_hi[e] << 32)) - (a.sum_lo[b] + (a.sum_hi[b] << 32)));
    c.clipped = (a.side[b] & 1u) | (a.side[e - 1] & 2u);
    c.pad = 0;
    a.chains[r] = c;
}

inline dim3 grid_for(uint32_t n) { return dim3((n + THREADS - 1) / THREADS); }

}  // namespace

void launch_netsubset_counts(const NetSubsetArgs& a, hipStream_t s) {
    if (a.F) hipLaunchKernelGGL(netsubset_counts_kernel, grid_for(a.F), dim3(THREADS), 0, s, a);
}

void launch_netsubset_mark(const NetSubsetArgs& a, hipStream_t s) {
    if (a.F) hipLaunchKernelGGL(netsubset_mark_kernel, grid_for(a.F), dim3(THREADS), 0, s, a);
}

void launch_netsubset_emit(const NetSubsetArgs& a, hipStream_t s) {
    if (a.N) hipLaunchKernelGGL(netsubset_emit_kernel, grid_for(a.N), dim3(THREADS), 0, s, a);
}

void launch_netsubset_cut_list(const NetSubsetArgs& a, hipStream_t s) {
    if (a.N) hipLaunchKernelGGL(netsubset_cut_list_kernel, grid_for(a.N), dim3(THREADS), 0, s, a);
}

void launch_netsubset_rescore(const NetSubsetArgs& a, uint32_t n_cut, hipStream_t s) {
    if (n_cut) hipLaunchKernelGGL(netsubset_rescore_kernel, dim3((n_cut + THREADS / 64 - 1) / (THREADS / 64)), dim3(THREADS), 0, s, a, n_cut);
}

void launch_netsubset_terms(const NetSubsetArgs& a, hipStream_t s) {
    if (a.N) hipLaunchKernelGGL(netsubset_terms_kernel, grid_for(a.N), dim3(THREADS), 0, s, a);
}

void launch_netsubset_chains(const NetSubsetArgs& a, uint32_t runs, hipStream_t s) {
    if (runs) hipLaunchKernelGGL(netsubset_chains_kernel, grid_for(runs), dim3(THREADS), 0, s, a, runs);
}

}  // namespace sa
