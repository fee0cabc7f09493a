// netclass.h -- what netclass.hip (the kernels) and api_netclass.hip (sa_net_classify) share.  Contract: include/segalign_amd.h, DESIGN.md 22.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

constexpr uint32_t NETCLASS_MAX_CHAINS = 1u << 22;
constexpr uint32_t NETCLASS_MAX_BLOCKS = 1u << 26;  // blocks of the input CSR, and clipped blocks of all fills: 2^27 events fit the sort's count
constexpr uint32_t NETCLASS_MAX_FILLS = 0x7FFFFFFFu;
constexpr uint32_t NETCLASS_TOP = 1u << 31;  // every coordinate is below it

// One call on the device.  F fills, M clipped blocks, E = 2 M events; the host has checked everything the kernels rely on: every fill's
// blocks lie in the block arrays, every clipped block holds a base, a parent is an earlier fill and depth counts the steps to the root.
struct NetClassArgs {
    const sa_net_fill* fills;  // [F]
    const uint32_t *bs, *be;   // blocks on the axis
    const uint32_t *obs, *obe;  // the same blocks on the other axis
    const uint32_t* ogroup;    // [chains] or nullptr: all 0
    const uint8_t* ostrand;    // [chains] or nullptr: all 0
    uint32_t F, M, E;
    uint32_t filter;  // SA_NETCLASS_FILTER set
    sa_net_class_params p;

    uint32_t* cnt;  // [F] n_blocks of every fill; its exclusive scan is off
    uint64_t* off;  // [F + 1] position of a fill's first clipped block
    uint32_t *cs, *ce;  // [M] the clipped other interval of every block
    uint64_t *key, *skey;  // [E] (ogroup << 32) | (coordinate << 1) | is_start, as emitted and sorted
    uint32_t *val, *sval;  // [E] the event's index: 2 j for the start of block j, 2 j + 1 for its end
    uint32_t* flag;  // [E] is_start of the sorted events; its exclusive scan is starts
    uint32_t* starts;  // [E + 1]
    uint32_t* seg;  // [E] bases from this event to the next with depth >= 2, inside one ogroup; its exclusive scan is dup
    uint64_t* dup;  // [E + 1]
    uint32_t* pos;  // [E] where event v stands in the sorted order
    uint32_t* bdup;  // [M] duplicated bases of a clipped block; its exclusive scan is bsum
    uint64_t* bsum;  // [M + 1]
    uint8_t* self;  // [F] self(f)
    sa_net_class* out;  // [F]
};

// cnt[k] = fills[k].n_blocks.
void launch_netclass_counts(const NetClassArgs& a, hipStream_t s);
// One thread per clipped block: its fill (a binary search in off), cs, ce and its two events.
void launch_netclass_emit(const NetClassArgs& a, hipStream_t s);
// One thread per sorted event: flag, and pos of the event it holds.
void launch_netclass_flags(const NetClassArgs& a, hipStream_t s);
// One thread per sorted event: seg from the depth after it, 2 starts[i + 1] - (i + 1).
void launch_netclass_segments(const NetClassArgs& a, hipStream_t s);
// One thread per clipped block: bdup = dup[pos of its end] - dup[pos of its start].
void launch_netclass_block_dup(const NetClassArgs& a, hipStream_t s);
// One thread per fill: the record but keep, and self.
void launch_netclass_classes(const NetClassArgs& a, hipStream_t s);
// One thread per fill: keep = self of the fill and of every ancestor, a walk of at most depth steps.
void launch_netclass_keep(const NetClassArgs& a, hipStream_t s);

}  // namespace sa
