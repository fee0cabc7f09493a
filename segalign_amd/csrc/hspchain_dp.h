// hspchain_dp.h -- the chaining DP's device code, once: what a pair of nodes is offered as (consider), the LDS image of a tile (TileLds)
// and the bodies of the cross and the resolve kernel, as __device__ __forceinline__ templates on <COSTS, OVL>.  hspchain.hip instantiates
// <COSTS, false> as sa_chain_hsps's and sa_chain_hsps_costs's kernels, hspovl.hip <COSTS, true> as those of sa_chain_hsps_ovl and
// sa_chain_hsps_all_ovl (contract: include/segalign_amd.h).
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
// COSTS: the penalty of a link has one more term, the piecewise-linear gap cost of a sa_chain_gap_costs.  The table is
// uniform, the gap is per lane.  The host folds the three cost arrays into one image (hspcost.h) that every workgroup of a COSTS
// instance copies into LDS behind the tile image; a lane then picks the case by an offset of 0, 16 or 32 rows, looks x = dt + dq up (x is
// dq where dt is 0 and dt where dq is 0, so one x serves the three cases) by a four-step binary search over the 16 shared break points,
// and reads its row (cost, slope, pos) in one 16-byte access (hspcost_gapcost).  No division, no scratch, no atomics; every LDS index is
// (0 | 16 | 32) + (0 .. 15) whatever the lane's values are, so no lookup can leave the image.
//
// OVL: j may precede i although they share up to max_overlap bases.  Two more values per node are staged beside the
// others, both made once per node by hspovl.hip's weight kernel: w (the node's score per base in 1/65536) and lim = min(len >> 1,
// max_overlap), the largest overlap the node takes part in: 2 o < bases is o <= (bases - 1) >> 1 = len >> 1.  A lane derives the
// overlap o of its pair, tests o <= min(lim_j, lim_i), moves i's start o bases on for the gaps and charges (o * min(w_j, w_i)) >> 16.
// The <COSTS, false> instances read none of this and are the kernels they were before the template had the parameter.
#pragma once
#include "hspchain.h"
#include "hspcost.h"

namespace sa {

namespace hspdp {

constexpr int64_t FAR = (int64_t)1 << 40;  // end coordinate of a slot past the last node: precedes nothing, and keeps every product in range

struct Pen {
    int64_t diag_pen, anti_pen, max_gap;
};

template <bool OVL>
struct Me {  // the node a thread owns
    int64_t rs, qs, dg;
    uint32_t gr;
    __device__ int64_t weight() const { return 0; }
    __device__ uint32_t limit() const { return 0u; }
};
template <>
struct Me<true> {  // and its weight and overlap limit
    int64_t rs, qs, dg;
    uint32_t gr, lim;
    int64_t w;
    __device__ int64_t weight() const { return w; }
    __device__ uint32_t limit() const { return lim; }
};

// Offers node j (end coordinates re, qe, diagonal dg, final f fj, group gj, rank `rank`; with OVL its weight wj and overlap limit limj)
// to the node `m`; img is the cost image in LDS and is read only with COSTS.
template <bool COSTS, bool OVL>
__device__ __forceinline__ void consider(const Me<OVL>& m, int64_t re, int64_t qe, int64_t dg, int64_t fj, uint32_t gj, uint32_t rank, int64_t wj,
                                         uint32_t limj, const Pen& P, const uint32_t* img, int64_t& best, uint32_t& bj) {
    // with OVL: o = max(0, re_j - rs_i, qe_j - qs_i), and the gaps are those left once o bases are cut off i's head, both >= 0.
    // pen is computed for every pair and used only under ok.  For a pair that is no link every step still stays in range: starts are
    // below 2^32 and ends at most FAR = 2^40, so |head|, o and the gaps are below 2^41 + 2^32; with diag_pen, anti_pen <= 2^20 (checked
    // by the entry) both signed products are below 2^63; hspcost_gapcost clamps its search into 32 bits and reads rows
    // (0 | 16 | 32) + (0 .. 15) of the image whatever the gaps are, and its products are unsigned.
    const int64_t head_r = m.rs - re, head_q = m.qs - qe, lo = head_r < head_q ? head_r : head_q;
    const int64_t o = OVL && lo < 0 ? -lo : 0;
    const int64_t gap_r = head_r + o, gap_q = head_q + o;
    bool ok = gj == m.gr && (OVL ? o <= (int64_t)(limj < m.limit() ? limj : m.limit()) : gap_r >= 0 && gap_q >= 0);
    if (P.max_gap) ok = ok && gap_r <= P.max_gap && gap_q <= P.max_gap;
    const int64_t dd = m.dg - dg;
    int64_t pen = P.diag_pen * (dd < 0 ? -dd : dd) + P.anti_pen * (gap_r + gap_q);
    if (COSTS) pen += hspcost_gapcost(img, gap_r, gap_q);
    // the overlap charge: for a link o <= 2^12 and w < 2^47, so the product is below 2^59; for a pair that is no link (o up to 2^41)
    // the unsigned product wraps, and the value, below 2^48 either way, is not used
    if (OVL) pen += (int64_t)(((uint64_t)o * (uint64_t)(wj < m.weight() ? wj : m.weight())) >> 16);
    const int64_t v = fj - pen;
    if (ok && v > best) {
        best = v;
        bj = rank;
    }
}

// LDS image of one tile: re, qe, diagonal and f as int64[tile] each, then the group as uint32[tile] (36 bytes per node, a multiple of
// 16 in all since tile is a multiple of 64); behind it, with COSTS only, the cost image, its rows 16-byte aligned.  With OVL a fifth
// int64 array, w, follows f, and lim follows the group as uint32[tile]: 48 bytes per node, 48 KB at tile = 1024.
template <bool OVL>
struct TileLds;
template <>
struct TileLds<false> {
    int64_t *re, *qe, *dg, *f;
    uint32_t *gr, *img;
    __device__ TileLds(int64_t* base, uint32_t tile)
        : re(base), qe(base + tile), dg(base + 2 * tile), f(base + 3 * tile), gr((uint32_t*)(base + 4 * tile)), img(gr + tile) {}
    __device__ int64_t weight(uint32_t) const { return 0; }
    __device__ uint32_t limit(uint32_t) const { return 0u; }
};
template <>
struct TileLds<true> {
    int64_t *re, *qe, *dg, *f, *w;
    uint32_t *gr, *lim, *img;
    __device__ TileLds(int64_t* base, uint32_t tile)
        : re(base), qe(base + tile), dg(base + 2 * tile), f(base + 3 * tile), w(base + 4 * tile), gr((uint32_t*)(base + 5 * tile)),
          lim(gr + tile), img(lim + tile) {}
    __device__ int64_t weight(uint32_t k) const { return w[k]; }
    __device__ uint32_t limit(uint32_t k) const { return lim[k]; }
};

// Bytes of dynamic LDS of cross and resolve: the tile image, and the cost image only where there is one.
inline size_t tile_lds(uint32_t tile, const uint32_t* image, bool ovl) {
    const size_t node = 4 * sizeof(int64_t) + sizeof(uint32_t) + (ovl ? sizeof(int64_t) + sizeof(uint32_t) : 0);
    return (size_t)tile * node + (image ? HSPCOST_WORDS * sizeof(uint32_t) : 0);
}

template <bool OVL>
__device__ __forceinline__ void stage_image(const TileLds<OVL>& L, const uint32_t* image, uint32_t T, uint32_t t) {
    for (uint32_t w = t; w < HSPCOST_WORDS; w += T) L.img[w] = image[w];
}

// The body of the cross kernel: workgroup blockIdx.x offers tile c0 + blockIdx.x to tile b.  o is read only with OVL.
template <bool COSTS, bool OVL>
__device__ __forceinline__ void cross_body(const HspChainArgs& a, const HspOvlNodes& o, uint32_t b, uint32_t c0, HspChainPartial* partial,
                                           const uint32_t* image) {
    extern __shared__ int64_t lds[];
    const uint32_t T = a.tile, t = threadIdx.x;
    const uint32_t c = c0 + blockIdx.x;  // c < b: a full tile
    TileLds<OVL> L(lds, T);
    {
        const uint32_t j = c * T + t;
        const int64_t rs = a.rs[j], qs = a.qs[j], span = (int64_t)a.ln[j] + 1;
        L.re[t] = rs + span;
        L.qe[t] = qs + span;
        L.dg[t] = rs - qs;
        L.f[t] = a.f[j];
        L.gr[t] = a.gr[j];
        if constexpr (OVL) {
            L.w[t] = o.w[j];
            L.lim[t] = o.lim[j];
        }
    }
    if (COSTS) stage_image(L, image, T, t);
    __syncthreads();
    const uint32_t i = b * T + t;
    if (i >= a.n) return;
    Me<OVL> m;
    m.rs = a.rs[i];
    m.qs = a.qs[i];
    m.dg = m.rs - m.qs;
    m.gr = a.gr[i];
    if constexpr (OVL) {
        m.lim = o.lim[i];
        m.w = o.w[i];
    }
    const Pen P = {a.diag_pen, a.anti_pen, a.max_gap};
    int64_t best = 0;
    uint32_t bj = HSPCHAIN_NONE;
    // two pairs per iteration, which is what the compiler makes of the linear loop on its own: with COSTS the two searches are
    // independent, so each of their four dependent LDS reads is issued beside the other pair's
#pragma unroll 2
    for (uint32_t k = 0; k < T; k++)
        consider<COSTS, OVL>(m, L.re[k], L.qe[k], L.dg[k], L.f[k], L.gr[k], c * T + k, L.weight(k), L.limit(k), P, L.img, best, bj);
    HspChainPartial r;
    r.v = best;
    r.rank = bj;
    r.pad = 0;
    partial[(size_t)blockIdx.x * T + t] = r;
}

// The body of the resolve kernel: one workgroup settles tile b.
template <bool COSTS, bool OVL>
__device__ __forceinline__ void resolve_body(const HspChainArgs& a, const HspOvlNodes& o, uint32_t b, uint32_t c0, const HspChainPartial* partial,
                                             const uint32_t* image) {
    extern __shared__ int64_t lds[];
    const uint32_t T = a.tile, t = threadIdx.x, wave = t >> 6;
    const uint32_t base = b * T, i = base + t;
    const bool live = i < a.n;
    const uint32_t nb = min(T, a.n - base), subs = (nb + 63) / 64;
    TileLds<OVL> L(lds, T);
    Me<OVL> m = {};
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
        if constexpr (OVL) {
            L.w[t] = m.w = o.w[i];
            L.lim[t] = m.lim = o.lim[i];
        }
    } else {
        L.re[t] = L.qe[t] = FAR;
        L.dg[t] = 0;
        L.gr[t] = 0;
        if constexpr (OVL) {  // a slot past the last node overlaps nothing: its limit is 0 and its ends lie FAR behind every start
            L.w[t] = 0;
            L.lim[t] = 0;
        }
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
            // successor of k, so the offer needs no lane test.  Without OVL: its start does not lie behind k's end.  With OVL: such a
            // lane i has rs_i <= rs_k, so o(k, i) >= re_k - rs_i >= re_k - rs_k = bases_k, and 2 o < bases_k fails (o > lim_k); a
            // lane past the last node has lim = 0 and, as node k, ends FAR behind every start.
            for (uint32_t k = 0; k < 64; k++) {
                const int64_t fk = __shfl(score + best, (int)k);
                const uint32_t j = s * 64 + k;
                consider<COSTS, OVL>(m, L.re[j], L.qe[j], L.dg[j], fk, L.gr[j], base + j, L.weight(j), L.limit(j), P, L.img, best, bj);
            }
            L.f[t] = score + best;
        }
        __syncthreads();
        if (wave > s && wave < subs)
#pragma unroll 2  // as in the cross loop
            for (uint32_t k = 0; k < 64; k++) {
                const uint32_t j = s * 64 + k;
                consider<COSTS, OVL>(m, L.re[j], L.qe[j], L.dg[j], L.f[j], L.gr[j], base + j, L.weight(j), L.limit(j), P, L.img, best, bj);
            }
    }
    if (live) {
        a.f[i] = score + best;
        a.pred[i] = bj;
    }
}

}  // namespace hspdp

}  // namespace sa
