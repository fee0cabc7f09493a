// stitch.h -- what stitch.hip (the kernels) and api_stitch.hip (sa_stitch_chains) share; the link's trace area and its walk are gapped.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"
#include "gapped.h"  // TraceTask, TraceOut, gapped_trace_bytes, launch_gapped_walk: a link is walked by sa_gapped_align's walk kernel

namespace sa {

constexpr int STITCH_MAX_LINK = 2048;     // the widest instance (K = 33) holds rows 0 .. 2111
constexpr int STITCH_NEG = -(1 << 30);    // minus infinity of the sweep, gapped.hip's; a score <= STITCH_NEG / 2 is not finite

struct StitchArgs {
    const uint8_t* ref;  // plain codes of the resident target block
    uint32_t ref_len;
    const uint8_t* query;  // plain codes of the query strand
    uint32_t query_len;
    const int* sub_mat;  // 64 entries on the device
    int gap_open, gap_extend;
};

struct StitchMember {  // one entry of members[]: the HSP it names
    uint32_t rs, qs, len, pad;
};
struct StitchMemberOut {
    int64_t score;  // sub_mat summed over the member's len + 1 pairs
    uint32_t matches, mismatches;
};
// One wave per member.  The caller has checked that every member lies inside the block on both sequences.
void launch_stitch_members(const StitchArgs& a, const StitchMember* members, uint32_t n, StitchMemberOut* out, hipStream_t s);

// The global sweep of n links, one wave each, all of the instance K = gapped_cells_per_lane(max_band): task k is the rectangle of
// best_i = dt <= max_band target bases from ar by best_j = dq query bases from aq, dstar = dt + dq >= 1, dir +1.  score[k] = H(dt, dq);
// the trace area at trace_off gets gapped.h's layout for that K with window base 0 on every antidiagonal.  The caller has checked
// that both ranges lie inside the block.
void launch_stitch_sweep(const StitchArgs& a, int max_band, const TraceTask* tasks, uint32_t n, uint8_t* area, int32_t* score, hipStream_t s);

}  // namespace sa
