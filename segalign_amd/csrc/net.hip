// net.hip -- the kernels of sa_net_chains (contract: include/segalign_amd.h): the chains of every group laid on one axis
// best first, each filling what is still open, the gaps inside a fill open one level down.
//
// The sequential rule takes the chains by priority and offers each to every open space.  The device runs the equivalent recursive rule
// level by level: the filler of a space is the chain of best priority that holds at least min_fill bases in it, and a chain that
// qualifies in a remainder or a gap of a space qualifies in the space itself (clipped bases only shrink with the space), so it comes
// after the space's filler.  A new space therefore starts its scan one position behind its opener's (DESIGN.md 19 has the argument).
//   Prepare: the chains in priority order (two stable radix sorts), per position the chain's hull, per group its range of positions,
// and the prefix sums of the block lengths.  A round is three kernels of one wavefront per space around one scan:
//   search  lane l of tile t tests the chain at position from + 64 t + l: the hull first, then two binary searches in the chain's blocks
//           (the first with end > a, the last with start < b) and the bases between them from the prefix sums, less what the two edge
//           blocks lose to the clip.  __ballot's lowest lane of the first non-empty tile is the filler.
//   count   the children that will be searched: the two remainders and every gap between clipped blocks, each if >= min_space.
//   emit    the fill, and those children as the next round's spaces, at the offsets the scan gave.
// A wavefront works on one space from start to end, so every branch on the space is uniform and __ballot sees all 64 lanes.  Plain
// uint32 / uint64 arithmetic; no kernel waits for another workgroup, every loop is bounded by a count known at launch, nothing is
// allocated, no atomics.
#include "net.h"

namespace sa {

namespace {

constexpr uint64_t SIGN = (uint64_t)1 << 63;
constexpr uint32_t WAVES = 4;  // wavefronts, and so spaces, per workgroup of the round kernels

// Ascending order of the key is descending order of x.
__device__ __forceinline__ uint64_t descending(int64_t x) { return ~((uint64_t)x ^ SIGN); }

__global__ void __launch_bounds__(256) net_block_len_kernel(NetArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.blocks) return;
    a.len[k] = a.be[k] - a.bs[k];
}

__global__ void __launch_bounds__(256) net_key_minor_kernel(NetArgs a) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n) return;
    a.key_a[c] = descending(a.score[c]);
    a.idx_a[c] = c;
}

__global__ void __launch_bounds__(256) net_key_major_kernel(NetArgs a, const uint32_t* idx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    a.key_a[p] = a.group ? a.group[idx[p]] : 0u;
}

__global__ void __launch_bounds__(256) net_gather_kernel(NetArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > a.n) return;
    if (p == a.n) {
        a.head[p] = 0;
        return;
    }
    const uint32_t c = a.byprio[p], f = a.first[c], e = a.first[c + 1];
    a.hull_s[p] = e > f ? a.bs[f] : 0u;
    a.hull_e[p] = e > f ? a.be[e - 1] : 0u;
    a.head[p] = (p == 0 || (a.group && a.group[c] != a.group[a.byprio[p - 1]])) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) net_group_starts_kernel(NetArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > a.n) return;
    if (p == a.n || a.head[p]) a.gstart[a.gidx[p]] = p;  // gidx[p] <= groups: gstart has groups + 1 entries
}

__global__ void __launch_bounds__(256) net_roots_kernel(NetArgs a, uint32_t groups, NetSpace* spaces) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    NetSpace sp;
    sp.a = 0;
    sp.b = NET_TOP;
    sp.from = a.gstart[g];
    sp.hi = a.gstart[g + 1];
    sp.parent = -1;
    sp.depth = 0;
    spaces[g] = sp;
}

__global__ void __launch_bounds__(64 * WAVES) net_search_kernel(NetArgs a, NetRound r) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= r.S) return;
    const NetSpace sp = r.spaces[k];
    for (uint32_t base = sp.from; base < sp.hi; base += 64) {
        const uint32_t p = base + lane;
        NetHit h = {p, 0, 0, 0};
        bool ok = false;
        if (p < sp.hi && a.hull_s[p] < sp.b && a.hull_e[p] > sp.a) {
            const uint32_t c = a.byprio[p], e = a.first[c + 1];
            uint32_t lo = a.first[c], hi = e;
            while (lo < hi) {  // the first block with end > a
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.be[mid] > sp.a) hi = mid; else lo = mid + 1;
            }
            h.i = lo;
            hi = e;
            while (lo < hi) {  // the first block from there with start >= b
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.bs[mid] >= sp.b) hi = mid; else lo = mid + 1;
            }
            if (lo > h.i) {
                h.j = lo - 1;
                const uint32_t s0 = a.bs[h.i], e1 = a.be[h.j];
                const uint64_t bases = a.pre[lo] - a.pre[h.i] - (sp.a > s0 ? sp.a - s0 : 0u) - (e1 > sp.b ? e1 - sp.b : 0u);
                h.ali = (uint32_t)bases;  // at most b - a
                ok = bases >= a.min_fill;
            }
        }
        const unsigned long long m = __ballot(ok);
        if (m) {
            if (lane == (uint32_t)(__ffsll(m) - 1)) r.hit[k] = h;
            return;
        }
    }
    if (lane == 0) r.hit[k] = NetHit{NET_NONE, 0, 0, 0};
}

// The extent of the fill of space sp by hit h.
__device__ __forceinline__ void fill_extent(const NetArgs& a, const NetSpace& sp, const NetHit& h, uint32_t& start, uint32_t& end) {
    const uint32_t s0 = a.bs[h.i], e1 = a.be[h.j];
    start = sp.a > s0 ? sp.a : s0;
    end = e1 > sp.b ? sp.b : e1;
}

__global__ void __launch_bounds__(64 * WAVES) net_count_kernel(NetArgs a, NetRound r) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= r.S) return;
    const NetHit h = r.hit[k];
    if (h.pos == NET_NONE) {
        if (lane == 0) r.cnt[k] = r.cnt[(size_t)r.S + k] = 0;
        return;
    }
    const NetSpace sp = r.spaces[k];
    uint32_t start, end, total = 0;
    fill_extent(a, sp, h, start, end);
    for (uint32_t base = h.i; base < h.j; base += 64) {
        const uint32_t g = base + lane;
        const bool ok = g < h.j && a.bs[g + 1] - a.be[g] >= a.min_space;
        total += (uint32_t)__popcll(__ballot(ok));
    }
    if (lane == 0) {
        r.cnt[k] = total + (start - sp.a >= a.min_space ? 1u : 0u) + (sp.b - end >= a.min_space ? 1u : 0u);
        r.cnt[(size_t)r.S + k] = 1;
    }
}

__global__ void __launch_bounds__(64 * WAVES) net_emit_kernel(NetArgs a, NetRound r) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= r.S) return;
    const NetHit h = r.hit[k];
    if (h.pos == NET_NONE) return;
    const NetSpace sp = r.spaces[k];
    const uint32_t c = a.byprio[h.pos];
    const uint32_t fi = r.fill_base + (uint32_t)(r.off[(size_t)r.S + k] - r.off[r.S]);
    uint64_t slot = r.off[k];
    uint32_t start, end;
    fill_extent(a, sp, h, start, end);
    NetSpace ch;
    ch.from = h.pos + 1;
    ch.hi = sp.hi;
    const bool left = start - sp.a >= a.min_space;
    if (lane == 0) {
        sa_net_fill f;
        f.group = a.group ? a.group[c] : 0u;
        f.chain = c;
        f.parent = sp.parent;
        f.depth = sp.depth;
        f.start = start;
        f.end = end;
        f.ali = h.ali;
        f.first_block = h.i;
        f.n_blocks = h.j - h.i + 1;
        f.pad = 0;
        f.score = a.score[c];
        r.fills[fi] = f;
        if (left) {
            ch.a = sp.a;
            ch.b = start;
            ch.parent = sp.parent;
            ch.depth = sp.depth;
            r.next[slot] = ch;
        }
    }
    slot += left ? 1 : 0;
    ch.parent = (int32_t)fi;
    ch.depth = sp.depth + 1;
    for (uint32_t base = h.i; base < h.j; base += 64) {
        const uint32_t g = base + lane;
        bool ok = false;
        if (g < h.j) {
            ch.a = a.be[g];
            ch.b = a.bs[g + 1];
            ok = ch.b - ch.a >= a.min_space;
        }
        const unsigned long long m = __ballot(ok);
        if (ok) r.next[slot + (uint32_t)__popcll(m & (((unsigned long long)1 << lane) - 1))] = ch;
        slot += (uint32_t)__popcll(m);
    }
    if (lane == 0 && sp.b - end >= a.min_space) {
        ch.a = end;
        ch.b = sp.b;
        ch.parent = sp.parent;
        ch.depth = sp.depth;
        r.next[slot] = ch;
    }
}

__global__ void __launch_bounds__(256) net_fill_key_kernel(const sa_net_fill* fills, uint32_t F, uint64_t* key, uint32_t* idx) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    key[f] = (uint64_t)fills[f].group << 32 | fills[f].start;
    idx[f] = f;
}

__global__ void __launch_bounds__(256) net_inverse_kernel(const uint32_t* order, uint32_t F, uint32_t* inv) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= F) return;
    inv[order[k]] = k;
}

__global__ void __launch_bounds__(256) net_finish_kernel(const sa_net_fill* fills, const uint32_t* order, const uint32_t* inv, uint32_t F,
                                                         sa_net_fill* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= F) return;
    // a fill as three 16-byte words (the arrays are 256-byte aligned, a fill is 48 bytes); parent is the third field
    const uint4* src = reinterpret_cast<const uint4*>(fills + order[k]);
    uint4* dst = reinterpret_cast<uint4*>(out + k);
    uint4 w = src[0];
    if ((int32_t)w.z >= 0) w.z = inv[w.z];
    dst[0] = w;
    dst[1] = src[1];
    dst[2] = src[2];
}

inline dim3 blocks(uint32_t n) { return dim3((n + 255) / 256); }
inline dim3 waves(uint32_t n) { return dim3((n + WAVES - 1) / WAVES); }

}  // namespace

void launch_net_block_len(const NetArgs& a, hipStream_t s) {
    if (a.blocks) hipLaunchKernelGGL(net_block_len_kernel, blocks(a.blocks), dim3(256), 0, s, a);
}

void launch_net_key_minor(const NetArgs& a, hipStream_t s) { hipLaunchKernelGGL(net_key_minor_kernel, blocks(a.n), dim3(256), 0, s, a); }

void launch_net_key_major(const NetArgs& a, const uint32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(net_key_major_kernel, blocks(a.n), dim3(256), 0, s, a, idx);
}

void launch_net_gather(const NetArgs& a, hipStream_t s) { hipLaunchKernelGGL(net_gather_kernel, blocks(a.n + 1), dim3(256), 0, s, a); }

void launch_net_group_starts(const NetArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(net_group_starts_kernel, blocks(a.n + 1), dim3(256), 0, s, a);
}

void launch_net_roots(const NetArgs& a, uint32_t groups, NetSpace* spaces, hipStream_t s) {
    hipLaunchKernelGGL(net_roots_kernel, blocks(groups), dim3(256), 0, s, a, groups, spaces);
}

void launch_net_search(const NetArgs& a, const NetRound& r, hipStream_t s) {
    hipLaunchKernelGGL(net_search_kernel, waves(r.S), dim3(64 * WAVES), 0, s, a, r);
}

void launch_net_count(const NetArgs& a, const NetRound& r, hipStream_t s) {
    hipLaunchKernelGGL(net_count_kernel, waves(r.S), dim3(64 * WAVES), 0, s, a, r);
}

void launch_net_emit(const NetArgs& a, const NetRound& r, hipStream_t s) {
    hipLaunchKernelGGL(net_emit_kernel, waves(r.S), dim3(64 * WAVES), 0, s, a, r);
}

void launch_net_fill_key(const sa_net_fill* fills, uint32_t F, uint64_t* key, uint32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(net_fill_key_kernel, blocks(F), dim3(256), 0, s, fills, F, key, idx);
}

void launch_net_inverse(const uint32_t* order, uint32_t F, uint32_t* inv, hipStream_t s) {
    hipLaunchKernelGGL(net_inverse_kernel, blocks(F), dim3(256), 0, s, order, F, inv);
}

void launch_net_finish(const sa_net_fill* fills, const uint32_t* order, const uint32_t* inv, uint32_t F, sa_net_fill* out, hipStream_t s) {
    hipLaunchKernelGGL(net_finish_kernel, blocks(F), dim3(256), 0, s, fills, order, inv, F, out);
}

}  // namespace sa
