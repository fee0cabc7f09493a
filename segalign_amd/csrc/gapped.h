// gapped.h -- what gapped.hip (the kernel) and api_gapped.hip (sa_gapped_extend) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

struct GappedSide {  // result of one one-sided extension
    int32_t best;    // best score (>= 0: the anchor cell scores 0)
    int32_t best_i;  // target bases of the best cell
    int32_t best_j;  // query bases of the best cell
    uint32_t cells;  // live cells, the anchor cell included
    uint32_t flags;  // SA_GAPPED_*
    uint32_t pad[3];
};

struct GappedArgs {
    const uint8_t* ref;  // plain codes of the resident target block (dc->ref)
    uint32_t ref_len;
    const uint8_t* query;  // plain codes of the query strand
    uint32_t query_len;
    const int* sub_mat;  // 64 entries on the device
    const sa_segment_pair* hsps;  // the batch's HSPs
    uint32_t num_tasks;  // 2 x HSPs of the batch: task 2h extends HSP h to the left, 2h + 1 to the right
    int gap_open, gap_extend, ydrop, max_extent, max_band;
    GappedSide* out;  // [num_tasks]
};

int gapped_cells_per_lane(int max_band);  // K of the kernel instance a band needs (64 K >= max_band + 1); -1: too wide
void launch_gapped(const GappedArgs& a, hipStream_t s);

}  // namespace sa
