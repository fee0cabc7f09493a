// chaintrim.h -- what chaintrim.hip (the crossover kernel) and api_chaintrim.hip (sa_trim_chains) share.  Contract: include/segalign_amd.h,
// DESIGN.md 24.  The sequences and the scoring matrix are the stitch entry's (StitchArgs), and so is the kernel that rescores a cut member.
#pragma once
#include "stitch.h"

namespace sa {

struct TrimLinkTask {  // one overlapping link: the first of j's last o columns and of i's first o columns, on both axes
    uint32_t jr, jq, ir, iq, o, pad;
};

// One wave per link: x[k] in 0 .. o maximises S(x) = sum_{c < x} a_c + sum_{c >= x} b_c, a_c the score of j's c-th column among its
// last o and b_c that of i's c-th among its first o; the lowest x among equals.  The caller has checked that both members lie inside
// the block and that 1 <= o <= 4096.
void launch_chaintrim_crossover(const StitchArgs& a, const TrimLinkTask* tasks, uint32_t n, uint32_t* x, hipStream_t s);

}  // namespace sa
