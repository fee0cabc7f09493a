// netsubset.h -- what netsubset.hip (the kernels) and api_netsubset.hip (sa_net_subset) share.  Contract: include/segalign_amd.h, DESIGN.md 21.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"
#include "hspcost.h"  // the gap-cost image a link's penalty is looked up in

namespace sa {

constexpr uint32_t NETSUBSET_MAX_FILLS = 0x7FFFFFFFu;
constexpr uint32_t NETSUBSET_MAX_OUT = 1u << 26;      // output members
constexpr uint32_t NETSUBSET_MAX_MEMBERS = 1u << 22;  // members of the input CSR

// One call on the device.  F fills, M members of the input CSR, N output members; the host has checked everything the kernels rely on:
// every fill's blocks lie in mh[0, M), a fill with a parent lies in a gap of it, every member lies inside the block on both sequences.
struct NetSubsetArgs {
    const uint8_t* ref;  // plain codes of the resident target block
    uint32_t ref_len;
    const uint8_t* query;  // plain codes of the query strand
    uint32_t query_len;
    const int* sub_mat;  // 64 entries on the device

    const sa_net_fill* fills;   // [F]
    const sa_segment_pair* mh;  // [M]: the HSP of every member of the input CSR, in member order
    uint32_t F, M, N;
    uint32_t axis;  // 0: target, 1: query
    int32_t diag_pen, anti_pen;
    const uint32_t* image;  // HSPCOST_WORDS words, or nullptr: no gap-cost table

    uint32_t* cnt;   // [F] n_blocks of every fill; its exclusive scan is off
    uint64_t* off;   // [F + 1] position of a fill's first member in the output
    uint32_t* mark;  // [N] zeroed, then 1 where a fill is cut after this member
    uint32_t* fill_of;  // [N]
    uint32_t* side;  // [N] bit 0: cut on the left, bit 1: cut on the right
    uint32_t* head;  // [N] 1 where a run starts; its exclusive scan is run
    uint64_t* run;   // [N + 1]
    uint32_t* is_cut;  // [N] side != 0; its exclusive scan is cut_at
    uint64_t* cut_at;  // [N + 1]
    uint32_t* cut_list;  // [N] the cut members' positions, ascending
    sa_segment_pair* out;  // [N] the clipped members
    int64_t* score;  // [N] the exact member scores
    uint32_t *lo, *hi;  // [N] the halves of score - pen' to the predecessor in the run; their exclusive scans are sum_lo, sum_hi
    uint64_t *sum_lo, *sum_hi;  // [N + 1]
    uint32_t* run_start;  // [runs + 1] position of every run's first member, N at the end
    sa_subset_chain* chains;  // [runs]
};

// cnt[k] = fills[k].n_blocks.
void launch_netsubset_counts(const NetSubsetArgs& a, hipStream_t s);
// One thread per fill with a parent: mark[off[parent] + k] = 1 for the last clipped block k of the parent that ends at or before the
// fill's start.  mark is zeroed before.
void launch_netsubset_mark(const NetSubsetArgs& a, hipStream_t s);
// One thread per output member: its fill (a binary search in off), the clipped HSP with the score field kept, side, is_cut, head and
// score for an uncut member.
void launch_netsubset_emit(const NetSubsetArgs& a, hipStream_t s);
// cut_list[cut_at[i]] = i for every cut member i.
void launch_netsubset_cut_list(const NetSubsetArgs& a, hipStream_t s);
// One wavefront per cut member: score = the matrix summed over the kept diagonal, out.score = that clamped to int32.
void launch_netsubset_rescore(const NetSubsetArgs& a, uint32_t n_cut, hipStream_t s);
// One thread per member: lo, hi = the halves of score - pen'(predecessor, member), the penalty 0 at a run's head; run_start of a head.
void launch_netsubset_terms(const NetSubsetArgs& a, hipStream_t s);
// One thread per run: the record.
void launch_netsubset_chains(const NetSubsetArgs& a, uint32_t runs, hipStream_t s);

}  // namespace sa
