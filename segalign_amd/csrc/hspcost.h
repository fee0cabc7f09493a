// hspcost.h -- the device image of a gap-cost table and its lookup: what hspchain.hip (the DP's <true> instances), netsubset.hip and
// post_host.h (which builds the image) share.  Contract: include/segalign_amd.h, DESIGN.md 20.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

// The device image of a sa_chain_gap_costs, uint32 words:
//   [0, 16)    pos[k], rows past n repeating row n - 1: a search that runs past n lands on a copy of the last row
//   [16, 208)  48 rows of (cost low, cost high, slope, pos): rows 0-15 q_gap, 16-31 t_gap, 32-47 both_gap, padded alike
// pos is one array for the three tables, so the search reads 16 words whatever the case; the row is one 16-byte read.
constexpr uint32_t HSPCOST_POINTS = SA_CHAIN_GAP_POINTS;
constexpr uint32_t HSPCOST_ROW0 = HSPCOST_POINTS;                       // first word of the rows
constexpr uint32_t HSPCOST_WORDS = HSPCOST_POINTS + 3 * HSPCOST_POINTS * 4;  // 208 words, 832 bytes
constexpr uint32_t HSPCOST_SLOPE_LIMIT = 1u << 27;

// The gap cost of a link with gaps dt, dq from an image, in LDS (hspchain.hip) or in global memory (netsubset.hip): the one lookup both
// units use, so that a sub-chain is priced as its chain was.  For a pair that is no link (a negative gap) the value is arbitrary but
// every step stays in range: the search clamps x into 32 bits, the distance past the break point is clamped at 0.
__host__ __device__ __forceinline__ int64_t hspcost_gapcost(const uint32_t* img, int64_t dt, int64_t dq) {
    const int64_t x = dt + dq;
    const uint32_t off = dt == 0 ? 0u : dq == 0 ? HSPCOST_POINTS : 2 * HSPCOST_POINTS;
    const uint32_t xc = ((uint64_t)x >> 32) ? 0xFFFFFFFFu : (uint32_t)x;  // pos < 2^32: the search gives the same row as with x
    uint32_t k = 0;  // the largest k with pos[k] <= x, or 0
    k += img[k + 8] <= xc ? 8u : 0u;
    k += img[k + 4] <= xc ? 4u : 0u;
    k += img[k + 2] <= xc ? 2u : 0u;
    k += img[k + 1] <= xc ? 1u : 0u;
    const uint4 row = ((const uint4*)(img + HSPCOST_ROW0))[off + k];  // cost low, cost high, slope, pos
    int64_t d = x - (int64_t)row.w;
    if (d < 0) d = 0;  // x below pos[0]: the cost of pos[0]
    // d < 2^34 and slope < 2^27: the product from two 32-bit multiplies, below 2^61
    const uint64_t prod = (uint64_t)(uint32_t)d * row.z + ((uint64_t)((uint32_t)((uint64_t)d >> 32) * row.z) << 32);
    const int64_t g = (int64_t)((uint64_t)row.x | (uint64_t)row.y << 32) + (int64_t)(prod >> 16);
    return x == 0 ? 0 : g;
}

}  // namespace sa
