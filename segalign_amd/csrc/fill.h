// fill.h -- what fill.hip (the kernels) and api_fill.hip (sa_fill_chains) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"
#include "stitch.h"  // StitchArgs: the resident block as the kernels read it

namespace sa {

constexpr uint32_t FILL_BATCH_LANES = 1u << 22;  // the diagonals (padded to 64 a task) one count launch takes: 65 536 wavefronts

struct FillTask {  // 64 adjacent diagonals of one link: lane l scans d = d0 + l
    uint32_t re, qe;  // the rectangle's origin
    uint32_t dt, dq;  // its sides, both >= 1
    int32_t d0;       // -(dq - 1) + 64 * (the task's number within the link)
    uint32_t link;    // what the emit pass writes beside every HSP of the task
};

struct FillScan {
    int32_t thresh, xdrop;
};

// One wavefront per task.  cnt[64 * t + l] = the HSPs of task t's lane l (0 for a lane past the link's last diagonal).
void launch_fill_count(const StitchArgs& a, const FillScan& f, const FillTask* tasks, uint32_t n, uint32_t* cnt, hipStream_t s);
// Tasks [t0, t1): lane (t, l) writes its HSPs from out[off[64 * t + l] - base] on, in the order of its diagonal, and the task's link
// beside each.  The caller has sized out and out_link for off[64 * t1] - base entries, base = off[64 * t0].
void launch_fill_emit(const StitchArgs& a, const FillScan& f, const FillTask* tasks, uint32_t t0, uint32_t t1, const uint64_t* off,
                      uint64_t base, sa_segment_pair* out, uint32_t* out_link, hipStream_t s);
// out[k] = off[at[k]] for k < n: the offsets at the links' first lanes.
void launch_fill_gather(const uint64_t* off, const uint32_t* at, uint32_t n, uint64_t* out, hipStream_t s);

}  // namespace sa
