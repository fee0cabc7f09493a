// hspcost.hip -- the DP kernels of sa_chain_hsps_costs / sa_chain_hsps_all_costs (contract: include/segalign_amd.h).
//
// The cross and resolve steps of hspchain.hip, word for word, with one more term in the penalty of a link: the piecewise-linear gap
// cost of a sa_chain_gap_costs.  Tiles, partials, sub-tiles, the order candidates are met in and "replace only on strictly larger" are
// unchanged, so the tie rules hold by the same construction.  hspchain.hip is not touched: these are kernels of their own, with an
// argument struct of their own.
// The table is uniform, the gap is per lane.  The host folds the three cost arrays into one image (hspcost.h) that every workgroup
// copies into LDS behind the tile image; a lane then picks the case by an offset of 0, 16 or 32 rows, looks x = dt + dq up (x is dq
// where dt is 0 and dt where dq is 0, so one x serves the three cases) by a four-step binary search over the 16 shared break points,
// and reads its row (cost, slope, pos) in one 16-byte access.  No division, no scratch, no atomics; every LDS index is
// (0 | 16 | 32) + (0 .. 15) whatever the lane's values are, so no lookup can leave the image.
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

// Offers node j (end coordinates re, qe, diagonal dg, final f fj, group gj, rank `rank`) to the node `m`.
__device__ __forceinline__ void consider(const Me& m, int64_t re, int64_t qe, int64_t dg, int64_t fj, uint32_t gj, uint32_t rank, const Pen& P,
                                         const uint32_t* img, int64_t& best, uint32_t& bj) {
    const int64_t gap_r = m.rs - re, gap_q = m.qs - qe;
    bool ok = gj == m.gr && gap_r >= 0 && gap_q >= 0;
    if (P.max_gap) ok = ok && gap_r <= P.max_gap && gap_q <= P.max_gap;
    const int64_t dd = m.dg - dg;
    const int64_t v = fj - (P.diag_pen * (dd < 0 ? -dd : dd) + P.anti_pen * (gap_r + gap_q) + hspcost_gapcost(img, gap_r, gap_q));
    if (ok && v > best) {
        best = v;
        bj = rank;
    }
}

// LDS: the tile image of hspchain.hip (re, qe, diagonal and f as int64[tile] each, the group as uint32[tile]: 36 bytes per node, a
// multiple of 16 in all since tile is one of 64), then the cost image.
struct TileLds {
    int64_t *re, *qe, *dg, *f;
    uint32_t *gr, *img;
    __device__ TileLds(int64_t* base, uint32_t tile)
        : re(base), qe(base + tile), dg(base + 2 * tile), f(base + 3 * tile), gr((uint32_t*)(base + 4 * tile)), img((uint32_t*)(base + 4 * tile) + tile) {}
};

__device__ __forceinline__ void stage_image(const TileLds& L, const uint32_t* image, uint32_t T, uint32_t t) {
    for (uint32_t w = t; w < HSPCOST_WORDS; w += T) L.img[w] = image[w];
}

__global__ void __launch_bounds__(1024) hspcost_cross_kernel(HspCostArgs ca, uint32_t b, uint32_t c0, HspChainPartial* partial) {
    extern __shared__ int64_t lds[];
    const HspChainArgs& a = ca.c;
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
    stage_image(L, ca.image, T, t);
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
    // two pairs per iteration, as the compiler unrolls the linear kernel on its own: the two searches are independent, so each of
    // their four dependent LDS reads is issued beside the other pair's
#pragma unroll 2
    for (uint32_t k = 0; k < T; k++) consider(m, L.re[k], L.qe[k], L.dg[k], L.f[k], L.gr[k], c * T + k, P, L.img, best, bj);
    HspChainPartial r;
    r.v = best;
    r.rank = bj;
    r.pad = 0;
    partial[(size_t)blockIdx.x * T + t] = r;
}

__global__ void __launch_bounds__(1024) hspcost_resolve_kernel(HspCostArgs ca, uint32_t b, uint32_t c0, const HspChainPartial* partial) {
    extern __shared__ int64_t lds[];
    const HspChainArgs& a = ca.c;
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
    stage_image(L, ca.image, T, t);
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
                consider(m, L.re[j], L.qe[j], L.dg[j], fk, L.gr[j], base + j, P, L.img, best, bj);
            }
            L.f[t] = score + best;
        }
        __syncthreads();
        if (wave > s && wave < subs)
#pragma unroll 2
            for (uint32_t k = 0; k < 64; k++) {
                const uint32_t j = s * 64 + k;
                consider(m, L.re[j], L.qe[j], L.dg[j], L.f[j], L.gr[j], base + j, P, L.img, best, bj);
            }
    }
    if (live) {
        a.f[i] = score + best;
        a.pred[i] = bj;
    }
}

inline size_t cost_lds(uint32_t tile) { return (size_t)tile * (4 * sizeof(int64_t) + sizeof(uint32_t)) + HSPCOST_WORDS * sizeof(uint32_t); }

}  // namespace

void launch_hspcost_cross(const HspCostArgs& a, uint32_t b, uint32_t c0, HspChainPartial* partial, hipStream_t s) {
    if (b > c0) hipLaunchKernelGGL(hspcost_cross_kernel, dim3(b - c0), dim3(a.c.tile), cost_lds(a.c.tile), s, a, b, c0, partial);
}

void launch_hspcost_resolve(const HspCostArgs& a, uint32_t b, uint32_t c0, const HspChainPartial* partial, hipStream_t s) {
    hipLaunchKernelGGL(hspcost_resolve_kernel, dim3(1), dim3(a.c.tile), cost_lds(a.c.tile), s, a, b, c0, partial);
}

}  // namespace sa
