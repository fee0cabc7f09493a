// hspcost.h -- what hspcost.hip (the DP kernels under a gap-cost table) and api_hspchain.hip (sa_chain_hsps_costs, sa_chain_hsps_all_costs)
// share.  Contract: include/segalign_amd.h, DESIGN.md 20.
#pragma once
#include "hspchain.h"

namespace sa {

// The device image of a sa_chain_gap_costs, uint32 words:
//   [0, 16)    pos[k], rows past n repeating row n - 1: a search that runs past n lands on a copy of the last row
//   [16, 208)  48 rows of (cost low, cost high, slope, pos): rows 0-15 q_gap, 16-31 t_gap, 32-47 both_gap, padded alike
// pos is one array for the three tables, so the search reads 16 words whatever the case; the row is one 16-byte read.
constexpr uint32_t HSPCOST_POINTS = SA_CHAIN_GAP_POINTS;
constexpr uint32_t HSPCOST_ROW0 = HSPCOST_POINTS;                       // first word of the rows
constexpr uint32_t HSPCOST_WORDS = HSPCOST_POINTS + 3 * HSPCOST_POINTS * 4;  // 208 words, 832 bytes
constexpr uint32_t HSPCOST_SLOPE_LIMIT = 1u << 27;

struct HspCostArgs {
    HspChainArgs c;         // the ranked HSPs, f and pred, the tile and the linear terms: as the linear kernels take them
    const uint32_t* image;  // HSPCOST_WORDS words, 16-byte aligned
};

// The cross and resolve steps of hspchain.h with the gap cost added to the penalty; same grid, same partials.
void launch_hspcost_cross(const HspCostArgs& a, uint32_t b, uint32_t c0, HspChainPartial* partial, hipStream_t s);
void launch_hspcost_resolve(const HspCostArgs& a, uint32_t b, uint32_t c0, const HspChainPartial* partial, hipStream_t s);

}  // namespace sa
