// hspchain.hip -- the kernels of sa_chain_hsps and, with a gap-cost table, of sa_chain_hsps_costs (contract: include/segalign_amd.h,
// DESIGN.md 15 and 20).
//
// The HSPs are ranked by (group, ref_start, query_start, len, input index); a predecessor always has the lower rank, so rank order is an
// evaluation order.  The ranked nodes are cut into tiles of `tile` nodes.  For tile b the host launches
//   cross    one workgroup per earlier tile c that can hold a predecessor: thread t sweeps c's nodes (staged in LDS, every lane reads the
//            same node: a broadcast) for node b * tile + t and writes the best candidate of that tile to partial[];
//   resolve  one workgroup: thread t reduces its partials over c in ascending order, then the tile settles its own dependencies, 64-node
//            sub-tile after sub-tile: the sub-tile's wave finalises lane 0, 1, ... 63 in turn, handing each finished f to the later lanes
//            by a lane broadcast (no barrier); one barrier later every thread of the later sub-tiles sweeps the finished sub-tile.
// Every candidate of a node is met in ascending rank and replaces the best only when it is strictly larger, and a node starts from
// (0, no predecessor): "value > 0, lowest rank among equals" holds by construction, without atomics.  All arithmetic is int64.
// No kernel waits for another workgroup; every loop is bounded by the tile, the tile count or the node count known at launch.
//
// The penalty of a link has an optional term, the piecewise-linear gap cost of a sa_chain_gap_costs: cross and resolve are
// templates on COSTS, and the <false> instances are sa_chain_hsps's kernels as they were, with no trace of the table.  The table is
// uniform, the gap is per lane.  The host folds the three cost arrays into one image (hspcost.h) that every workgroup of a <true>
// instance copies into LDS behind the tile image; a lane then picks the case by an offset of 0, 16 or 32 rows, looks x = dt + dq up (x is
// dq where dt is 0 and dt where dq is 0, so one x serves the three cases) by a four-step binary search over the 16 shared break points,
// and reads its row (cost, slope, pos) in one 16-byte access (hspcost_gapcost).  No division, no scratch, no atomics; every LDS index is
// (0 | 16 | 32) + (0 .. 15) whatever the lane's values are, so no lookup can leave the image.
#include "hspchain.h"
#include "hspcost.h"

namespace sa {

namespace {

constexpr int64_t FAR = (int64_t)1 << 40;  // end coordinate of a slot past the last node: precedes nothing, and keeps every product in range

struct Pen {
    int64_t diag_pen, anti_pen, max_gap;
};

struct Me {  // the node a thread owns
    int64_t rs, qs, dg;
    uint32_t gr;
};

// Offers node j (end coordinates re, qe, diagonal dg, final f fj, group gj, rank `rank`) to the node `m`; img is the cost image in LDS
// and is read only with COSTS.
template <bool COSTS>
__device__ __forceinline__ void consider(const Me& m, int64_t re, int64_t qe, int64_t dg, int64_t fj, uint32_t gj, uint32_t rank, const Pen& P,
                                         const uint32_t* img, int64_t& best, uint32_t& bj) {
    const int64_t gap_r = m.rs - re, gap_q = m.qs - qe;
    bool ok = gj == m.gr && gap_r >= 0 && gap_q >= 0;
    if (P.max_gap) ok = ok && gap_r <= P.max_gap && gap_q <= P.max_gap;
    const int64_t dd = m.dg - dg;
    int64_t pen = P.diag_pen * (dd < 0 ? -dd : dd) + P.anti_pen * (gap_r + gap_q);
    if (COSTS) pen += hspcost_gapcost(img, gap_r, gap_q);
    const int64_t v = fj - pen;
    if (ok && v > best) {
        best = v;
        bj = rank;
    }
}

// LDS image of one tile: re, qe, diagonal and f as int64[tile] each, then the group as uint32[tile] (36 bytes per node, a multiple of
// 16 in all since tile is a multiple of 64); behind it, with COSTS only, the cost image, its rows 16-byte aligned.
struct TileLds {
    int64_t *re, *qe, *dg, *f;
    uint32_t *gr, *img;
    __device__ TileLds(int64_t* base, uint32_t tile)
        : re(base), qe(base + tile), dg(base + 2 * tile), f(base + 3 * tile), gr((uint32_t*)(base + 4 * tile)), img(gr + tile) {}
};

__device__ __forceinline__ void stage_image(const TileLds& L, const uint32_t* image, uint32_t T, uint32_t t) {
    for (uint32_t w = t; w < HSPCOST_WORDS; w += T) L.img[w] = image[w];
}

template <bool COSTS>
__global__ void __launch_bounds__(1024) hspchain_cross_kernel(HspChainArgs a, uint32_t b, uint32_t c0, HspChainPartial* partial, const uint32_t* image) {
    extern __shared__ int64_t lds[];
    const uint32_t T = a.tile, t = threadIdx.x;
    const uint32_t c = c0 + blockIdx.x;  // c < b: a full tile
    TileLds L(lds, T);
    {
        const uint32_t j = c * T + t;
        const int64_t rs = a.rs[j], qs = a.qs[j], span = (int64_t)a.ln[j] + 1;
        L.re[t] = rs + span;
        L.qe[t] = qs + span;
        L.dg[t] = rs - qs;
        L.f[t] = a.f[j];
        L.gr[t] = a.gr[j];
    }
    if (COSTS) stage_image(L, image, T, t);
    __syncthreads();
    const uint32_t i = b * T + t;
    if (i >= a.n) return;
    Me m;
    m.rs = a.rs[i];
    m.qs = a.qs[i];
    m.dg = m.rs - m.qs;
    m.gr = a.gr[i];
    const Pen P = {a.diag_pen, a.anti_pen, a.max_gap};
    int64_t best = 0;
    uint32_t bj = HSPCHAIN_NONE;
    // two pairs per iteration, which is what the compiler makes of the linear loop on its own: with COSTS the two searches are
    // independent, so each of their four dependent LDS reads is issued beside the other pair's
#pragma unroll 2
    for (uint32_t k = 0; k < T; k++) consider<COSTS>(m, L.re[k], L.qe[k], L.dg[k], L.f[k], L.gr[k], c * T + k, P, L.img, best, bj);
    HspChainPartial r;
    r.v = best;
    r.rank = bj;
    r.pad = 0;
    partial[(size_t)blockIdx.x * T + t] = r;
}

template <bool COSTS>
__global__ void __launch_bounds__(1024) hspchain_resolve_kernel(HspChainArgs a, uint32_t b, uint32_t c0, const HspChainPartial* partial,
                                                                const uint32_t* image) {
    extern __shared__ int64_t lds[];
    const uint32_t T = a.tile, t = threadIdx.x, wave = t >> 6;
    const uint32_t base = b * T, i = base + t;
    const bool live = i < a.n;
    const uint32_t nb = min(T, a.n - base), subs = (nb + 63) / 64;
    TileLds L(lds, T);
    Me m = {0, 0, 0, 0};
    int64_t score = 0;
    if (live) {
        m.rs = a.rs[i];
        m.qs = a.qs[i];
        m.dg = m.rs - m.qs;
        m.gr = a.gr[i];
        score = a.sc[i];
        const int64_t span = (int64_t)a.ln[i] + 1;
        L.re[t] = m.rs + span;
        L.qe[t] = m.qs + span;
        L.dg[t] = m.dg;
        L.gr[t] = m.gr;
    } else {
        L.re[t] = L.qe[t] = FAR;
        L.dg[t] = 0;
        L.gr[t] = 0;
    }
    L.f[t] = 0;
    if (COSTS) stage_image(L, image, T, t);
    const Pen P = {a.diag_pen, a.anti_pen, a.max_gap};
    int64_t best = 0;
    uint32_t bj = HSPCHAIN_NONE;
    if (live)
        for (uint32_t k = 0; k < b - c0; k++) {  // earlier tiles, ascending
            const HspChainPartial p = partial[(size_t)k * T + t];
            if (p.v > best) {
                best = p.v;
                bj = p.rank;
            }
        }
    __syncthreads();
    for (uint32_t s = 0; s < subs; s++) {
        if (wave == s) {
            // lane k's f is final at step k: every node of lower rank has been offered to it.  A lane at or before k is never a
            // successor of k (its start does not lie behind k's end), so the offer needs no lane test.
            for (uint32_t k = 0; k < 64; k++) {
                const int64_t fk = __shfl(score + best, (int)k);
                const uint32_t j = s * 64 + k;
                consider<COSTS>(m, L.re[j], L.qe[j], L.dg[j], fk, L.gr[j], base + j, P, L.img, best, bj);
            }
            L.f[t] = score + best;
        }
        __syncthreads();
        if (wave > s && wave < subs)
#pragma unroll 2  // as in the cross loop
            for (uint32_t k = 0; k < 64; k++) {
                const uint32_t j = s * 64 + k;
                consider<COSTS>(m, L.re[j], L.qe[j], L.dg[j], L.f[j], L.gr[j], base + j, P, L.img, best, bj);
            }
    }
    if (live) {
        a.f[i] = score + best;
        a.pred[i] = bj;
    }
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
// Dynamic LDS of cross and resolve: the tile image, and the cost image only where there is one.
inline size_t tile_lds(uint32_t tile, const uint32_t* image) {
    return (size_t)tile * (4 * sizeof(int64_t) + sizeof(uint32_t)) + (image ? HSPCOST_WORDS * sizeof(uint32_t) : 0);
}

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
    hipLaunchKernelGGL(kernel, dim3(b - c0), dim3(a.tile), tile_lds(a.tile, image), s, a, b, c0, partial, image);
}

void launch_hspchain_resolve(const HspChainArgs& a, uint32_t b, uint32_t c0, const HspChainPartial* partial, const uint32_t* image, hipStream_t s) {
    const auto kernel = image ? hspchain_resolve_kernel<true> : hspchain_resolve_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(a.tile), tile_lds(a.tile, image), s, a, b, c0, partial, image);
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
