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

// ---- trace sweep and path walk (sa_gapped_align) ----
struct TraceTask {  // one side to trace: a side whose best cell is not the anchor
    uint32_t ar, aq;     // anchor (a_r, a_q)
    int32_t dir;         // -1 left, +1 right
    int32_t dstar;       // best_i + best_j of the side (pass 1): the trace covers antidiagonals 1 .. dstar
    int32_t best_i, best_j;
    uint64_t trace_off;  // byte offset of the side's trace area in the batch's trace buffer (256-aligned)
    uint64_t ops_off;    // first entry of the side's op area (dstar entries) in the batch's op buffer
};

struct TraceOut {  // what the walk of one side found
    uint32_t n_runs;  // run-length ops written, in walk order (best cell -> anchor)
    uint32_t matches, mismatches, gap_opens, gap_bases;
    uint32_t err;     // != 0: the walk left the traced cells (a broken invariant; the host aborts)
    uint32_t pad[2];
};

// Trace area of one side: dstar rows of 64 x ceil(K / 8) dwords (row d - 1 = antidiagonal d; dword w * 64 + l holds the 4-bit codes of
// lane l's cells 8 w .. 8 w + 7), then the window base of antidiagonals 0 .. dstar as int32.  Rounded up to 256 bytes.
size_t gapped_trace_bytes(int max_band, int dstar);
void launch_gapped_trace(const GappedArgs& a, const TraceTask* tasks, uint32_t n, uint8_t* area, hipStream_t s);
void launch_gapped_walk(const GappedArgs& a, const TraceTask* tasks, uint32_t n, const uint8_t* area, uint32_t* ops, TraceOut* out,
                        hipStream_t s);

}  // namespace sa
