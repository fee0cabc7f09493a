// lift.h -- what lift.hip (the kernels) and api_lift.hip (sa_lift_intervals) share.  Contract: include/segalign_amd.h, DESIGN.md 23.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

constexpr uint32_t LIFT_MAX_CHAINS = 1u << 22;
constexpr uint32_t LIFT_MAX_BLOCKS = 1u << 26;
constexpr uint32_t LIFT_MAX_INTERVALS = 1u << 26;
constexpr uint32_t LIFT_MAX_DEN = 1u << 20;
constexpr uint32_t LIFT_TOP = 1u << 31;          // every coordinate is below it
constexpr uint64_t LIFT_MAX_OUT = 0x7FFFFFFFu;   // hits, and output blocks, of one call
constexpr uint32_t LIFT_NONE = 0xFFFFFFFFu;

// The positions [lo, hi) of the sorted chains that an interval tests.
struct LiftRange {
    uint32_t lo, hi;
};

// One call on the device.  N chains, B blocks, I intervals, H hits, O output blocks; the host has checked everything the kernels rely
// on: first[] is a CSR over the block arrays, the blocks of a chain ascend and are disjoint, every coordinate is below 2^31 and every
// interval holds a base.
struct LiftArgs {
    const uint32_t* first;      // [N + 1]
    const uint32_t *bs, *be;    // [B] blocks on the axis
    const uint32_t *obs, *obe;  // [B] the same blocks on the other axis
    const uint32_t* group;      // [N] or nullptr: all 0
    const uint32_t* ogroup;     // [N] or nullptr: all 0
    const uint8_t* ostrand;     // [N] or nullptr: all 0
    const uint32_t* iv_group;   // [I] or nullptr: all 0
    const uint32_t *iv_s, *iv_e;  // [I]
    uint32_t N, B, I, H, O;
    uint32_t num, den;
    uint32_t multiple, with_blocks;  // the two flags

    uint32_t* len;    // [B] block lengths; their exclusive scan is pre
    uint64_t* pre;    // [B + 1]
    uint64_t *key, *skey;    // [N] (group << 32) | hull start, by chain and sorted
    uint32_t *val, *order;   // [N] the chain index, by chain and sorted: order[p] is the chain at position p
    uint32_t* hull_e;        // [N] the hull's end at position p (its start is the low half of skey[p])
    uint64_t *hmax, *run;    // [N] (group << 32) | hull end at position p, and its inclusive running maximum
    LiftRange* range;        // [I] what lift_count_kernel tested, for lift_emit_kernel
    uint32_t* cnt;           // [I] the hits of an interval under the flags; their exclusive scan is off
    uint64_t* off;           // [I + 1]
    sa_lift_record* rec;     // [I]
    sa_lift_hit* hits;       // [H]
    uint32_t* hn;            // [H] n_blocks of every hit; their exclusive scan is hoff
    uint64_t* hoff;          // [H + 1]
    sa_lift_block* out;      // [O]
};

// len[k] = be[k] - bs[k].
void launch_lift_block_len(const LiftArgs& a, hipStream_t s);
// One thread per chain: key = (group << 32) | hull start, val = the chain; an empty chain has the hull (0, 0).
void launch_lift_keys(const LiftArgs& a, hipStream_t s);
// One thread per sorted position: hull_e and hmax of the chain that stands there.
void launch_lift_gather(const LiftArgs& a, hipStream_t s);
// One wavefront per interval: its candidate range, the record but first_hit, and cnt.
void launch_lift_count(const LiftArgs& a, hipStream_t s);
// One wavefront per interval: first_hit, and the hits of the qualifying chains at off + the rank among them; with blocks also hn.
void launch_lift_emit(const LiftArgs& a, hipStream_t s);
// One thread per output block: its hit (a binary search in hoff), the clipped block pair, and the hit's out_block from its first one.
void launch_lift_blocks(const LiftArgs& a, hipStream_t s);

}  // namespace sa
