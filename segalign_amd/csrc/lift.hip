// lift.hip -- the kernels of sa_lift_intervals (contract: include/segalign_amd.h): intervals of one axis carried through
// chains to the other axis.
//
// Prepare, once per call: the block lengths and their prefix sums; the chains sorted by (group, hull start), stable, so that equal keys
// stay in chain order, which is the hit order; over the sorted positions the running maximum of (group << 32) | hull end (cover.hip's
// rocPRIM scan), which the group in the high bits makes a maximum per group.
//   count   one wavefront per interval.  Three binary searches, the same in every lane, give the positions [p_lo, p_hi) that can touch
//           it: the chains of its group whose hull starts before its end, from the first whose running maximum passes its start.  Lane l
//           of tile t tests position p_lo + 64 t + l: the hull first, then two binary searches in the chain's blocks (the first with end
//           > s, from there the first with start >= e) and the bases between them from the prefix sums, less what the two edge blocks
//           lose.  __ballot counts the touching and the qualifying chains; every lane keeps its best (mapped descending, position
//           ascending), one wave reduction picks the interval's, lane 0 writes the record and the hit count.
//   emit    after the scan of the hit counts: the same walk, the qualifying chains' hits at first_hit + the ballot rank.
//   blocks  after the scan of the hits' n_blocks: one thread per output block, its hit by a binary search in the offsets.
// A wavefront works on one interval from start to end, so every branch on the interval is uniform and __ballot sees all 64 lanes.  Plain
// C++ on uint32 / uint64 / int64; no kernel waits for another workgroup, every loop is bounded by a count known at launch (a binary
// search: at most 32 steps; the walk: the chains), nothing is allocated, no atomics.  The host has validated every index the kernels
// form (lift.h).
#include "lift.h"

namespace sa {

namespace {

constexpr int THREADS = 256;
constexpr uint32_t WAVES = 4;  // wavefronts, and so intervals, per workgroup of count and emit

// What a chain holds of an interval: its clipped blocks i .. j and their bases.
struct Probe {
    uint32_t i, j, mapped;
};

// The other hull of the clipped blocks i .. j of a chain.
struct Image {
    uint32_t ostart, oend;
};

__device__ __forceinline__ uint32_t strand_of(const LiftArgs& a, uint32_t chain) { return a.ostrand ? (uint32_t)a.ostrand[chain] : 0u; }

// The first position in [lo, hi) whose key is >= x.
__device__ __forceinline__ uint32_t first_at_least(const uint64_t* key, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The candidate range of the interval [s, e) of group g.
__device__ __forceinline__ LiftRange range_of(const LiftArgs& a, uint32_t g, uint32_t s, uint32_t e) {
    const uint64_t gk = (uint64_t)g << 32;
    const uint32_t g_lo = first_at_least(a.skey, 0, a.N, gk);
    LiftRange r;
    r.hi = first_at_least(a.skey, g_lo, a.N, gk | e);
    r.lo = first_at_least(a.run, g_lo, r.hi, (gk | s) + 1);  // run ascends: the first running maximum that exceeds (g, s)
    return r;
}

// Does the chain at position p hold a base of [s, e)?  The hull test, then the two searches in its blocks.
__device__ __forceinline__ bool probe(const LiftArgs& a, uint32_t p, uint32_t s, uint32_t e, Probe& r) {
    if (!((uint32_t)a.skey[p] < e && a.hull_e[p] > s)) return false;
    const uint32_t c = a.order[p], end = a.first[c + 1];
    uint32_t lo = a.first[c], hi = end;
    while (lo < hi) {  // the first block with end > s
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.be[mid] > s) hi = mid; else lo = mid + 1;
    }
    r.i = lo;
    hi = end;
    while (lo < hi) {  // the first block from there with start >= e
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.bs[mid] >= e) hi = mid; else lo = mid + 1;
    }
    if (lo <= r.i) return false;  // the interval lies in a gap of the chain
    r.j = lo - 1;
    const uint32_t s0 = a.bs[r.i], e1 = a.be[r.j];
    r.mapped = (uint32_t)(a.pre[lo] - a.pre[r.i] - (s > s0 ? s - s0 : 0u) - (e1 > e ? e1 - e : 0u));  // at least 1, at most e - s
    return true;
}

// Block k cut to [s, e) on the axis loses dl bases on its left and dr on its right; on the other axis a strand-1 block loses them on
// the opposite sides.
__device__ __forceinline__ Image clip_other(const LiftArgs& a, uint32_t k, uint32_t s, uint32_t e, bool minus) {
    const uint32_t bs = a.bs[k], be = a.be[k];
    const uint32_t dl = max(bs, s) - bs, dr = be - min(be, e);
    return Image{a.obs[k] + (minus ? dr : dl), a.obe[k] - (minus ? dl : dr)};
}

// By monotonicity the hull is two of the four outer ends of the first and the last clipped block.
__device__ __forceinline__ Image image_of(const LiftArgs& a, uint32_t chain, const Probe& r, uint32_t s, uint32_t e) {
    const bool minus = strand_of(a, chain) != 0;
    const Image x = clip_other(a, r.i, s, e, minus), y = clip_other(a, r.j, s, e, minus);
    return minus ? Image{y.ostart, x.oend} : Image{x.ostart, y.oend};
}

__device__ __forceinline__ bool qualifies(const LiftArgs& a, uint32_t mapped, uint32_t s, uint32_t e) {
    return (int64_t)mapped * (int64_t)a.den >= (int64_t)a.num * (int64_t)(e - s);  // below 2^51 on both sides
}

__global__ __launch_bounds__(THREADS) void lift_block_len_kernel(LiftArgs a) {
    const uint32_t k = blockIdx.x * THREADS + threadIdx.x;
    if (k < a.B) a.len[k] = a.be[k] - a.bs[k];
}

__global__ __launch_bounds__(THREADS) void lift_keys_kernel(LiftArgs a) {
    const uint32_t c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= a.N) return;
    const uint32_t f = a.first[c], e = a.first[c + 1];
    a.key[c] = (uint64_t)(a.group ? a.group[c] : 0u) << 32 | (e > f ? a.bs[f] : 0u);
    a.val[c] = c;
}

__global__ __launch_bounds__(THREADS) void lift_gather_kernel(LiftArgs a) {
    const uint32_t p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.N) return;
    const uint32_t c = a.order[p], f = a.first[c], e = a.first[c + 1];
    const uint32_t he = e > f ? a.be[e - 1] : 0u;  // an empty chain: the hull (0, 0), which no interval meets
    a.hull_e[p] = he;
    a.hmax[p] = (a.skey[p] & 0xFFFFFFFF00000000ull) | he;
}

__global__ __launch_bounds__(64 * WAVES) void lift_count_kernel(LiftArgs a) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= a.I) return;
    const uint32_t g = a.iv_group ? a.iv_group[k] : 0u, s = a.iv_s[k], e = a.iv_e[k];
    const LiftRange rg = range_of(a, g, s, e);
    uint32_t n_touch = 0, n_qualify = 0;
    uint64_t best = 0;  // (mapped << 32) | ~position: the greatest is the best chain; 0: none, mapped being at least 1
    for (uint32_t base = rg.lo; base < rg.hi; base += 64) {
        const uint32_t p = base + lane;
        Probe r;
        const bool touch = p < rg.hi && probe(a, p, s, e, r);
        bool ok = false;
        if (touch) {
            ok = qualifies(a, r.mapped, s, e);
            const uint64_t x = (uint64_t)r.mapped << 32 | (LIFT_NONE - p);
            if (x > best) best = x;
        }
        n_touch += (uint32_t)__popcll(__ballot(touch));
        n_qualify += (uint32_t)__popcll(__ballot(ok));
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t x = __shfl_xor((unsigned long long)best, d);
        if (x > best) best = x;
    }
    if (lane != 0) return;
    a.range[k] = rg;
    a.cnt[k] = a.multiple ? n_qualify : (n_qualify == 1 ? 1u : 0u);
    uint4* o = reinterpret_cast<uint4*>(a.rec + k);  // the 48-byte record as three 16-byte stores; first_hit comes from lift_emit_kernel
    if (best == 0) {
        o[0] = make_uint4(SA_LIFT_UNMAPPED, 0u, 0u, 0u);
        o[1] = make_uint4(LIFT_NONE, 0u, 0u, 0u);
        o[2] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t p = LIFT_NONE - (uint32_t)best, c = a.order[p];
    Probe r;
    probe(a, p, s, e, r);  // it touched
    const Image im = image_of(a, c, r, s, e);
    const uint32_t status = n_qualify == 0 ? SA_LIFT_PARTIAL : n_qualify == 1 ? SA_LIFT_MAPPED : SA_LIFT_DUPLICATED;
    o[0] = make_uint4(status, n_touch, n_qualify, 0u);
    o[1] = make_uint4(c, a.ogroup ? a.ogroup[c] : 0u, im.ostart, im.oend);
    o[2] = make_uint4(r.mapped, r.i, r.j - r.i + 1, strand_of(a, c));
}

__global__ __launch_bounds__(64 * WAVES) void lift_emit_kernel(LiftArgs a) {
    const uint32_t k = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= a.I) return;
    uint32_t slot = (uint32_t)a.off[k];  // at most 2^31 - 1 hits: the host has read the total
    if (lane == 0) a.rec[k].first_hit = slot;
    if (a.cnt[k] == 0) return;  // with SA_LIFT_MULTIPLE no chain qualifies; without it the interval is not MAPPED
    const uint32_t s = a.iv_s[k], e = a.iv_e[k];
    const LiftRange rg = a.range[k];
    for (uint32_t base = rg.lo; base < rg.hi; base += 64) {
        const uint32_t p = base + lane;
        Probe r;
        const bool ok = p < rg.hi && probe(a, p, s, e, r) && qualifies(a, r.mapped, s, e);
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const uint32_t h = slot + (uint32_t)__popcll(m & (((unsigned long long)1 << lane) - 1)), c = a.order[p];
            const Image im = image_of(a, c, r, s, e);
            uint4* o = reinterpret_cast<uint4*>(a.hits + h);  // the 32-byte hit as two 16-byte stores; out_block comes from lift_blocks_kernel
            o[0] = make_uint4(k, c, im.ostart, im.oend);
            o[1] = make_uint4(r.mapped, r.i, r.j - r.i + 1, 0u);
            if (a.with_blocks) a.hn[h] = r.j - r.i + 1;
        }
        slot += (uint32_t)__popcll(m);
    }
}

__global__ __launch_bounds__(THREADS) void lift_blocks_kernel(LiftArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.O) return;
    uint32_t lo = 0, hi = a.H;  // the hit: the last one with hoff <= i; hoff ascends strictly, every hit having a block
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.hoff[mid] <= i) lo = mid; else hi = mid;
    }
    const uint32_t at = (uint32_t)a.hoff[lo];
    const sa_lift_hit& h = a.hits[lo];
    const uint32_t iv = h.interval, chain = h.chain, k = h.first_block + (i - at);
    const uint32_t s = a.iv_s[iv], e = a.iv_e[iv];
    const Image im = clip_other(a, k, s, e, strand_of(a, chain) != 0);
    *reinterpret_cast<uint4*>(a.out + i) = make_uint4(max(a.bs[k], s), min(a.be[k], e), im.ostart, im.oend);
    if (i == at) a.hits[lo].out_block = i;  // a field no thread reads
}

inline dim3 grid_for(uint32_t n) { return dim3((n + THREADS - 1) / THREADS); }
inline dim3 waves(uint32_t n) { return dim3((n + WAVES - 1) / WAVES); }

}  // namespace

void launch_lift_block_len(const LiftArgs& a, hipStream_t s) {
    if (a.B) hipLaunchKernelGGL(lift_block_len_kernel, grid_for(a.B), dim3(THREADS), 0, s, a);
}

void launch_lift_keys(const LiftArgs& a, hipStream_t s) {
    if (a.N) hipLaunchKernelGGL(lift_keys_kernel, grid_for(a.N), dim3(THREADS), 0, s, a);
}

void launch_lift_gather(const LiftArgs& a, hipStream_t s) {
    if (a.N) hipLaunchKernelGGL(lift_gather_kernel, grid_for(a.N), dim3(THREADS), 0, s, a);
}

void launch_lift_count(const LiftArgs& a, hipStream_t s) {
    if (a.I) hipLaunchKernelGGL(lift_count_kernel, waves(a.I), dim3(64 * WAVES), 0, s, a);
}

void launch_lift_emit(const LiftArgs& a, hipStream_t s) {
    if (a.I) hipLaunchKernelGGL(lift_emit_kernel, waves(a.I), dim3(64 * WAVES), 0, s, a);
}

void launch_lift_blocks(const LiftArgs& a, hipStream_t s) {
    if (a.O) hipLaunchKernelGGL(lift_blocks_kernel, grid_for(a.O), dim3(THREADS), 0, s, a);
}

}  // namespace sa
