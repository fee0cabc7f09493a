// chaintrim.hip -- the crossover kernel of sa_trim_chains (contract: include/segalign_amd.h).
//
// Two linked members j, i of a chain share o columns on an axis.  Cutting j's last o - x and i's first x columns leaves
// S(x) = sum_{c < x} a_c + sum_{c >= x} b_c of the shared stretch, which is sum_c b_c + P(x) with P(x) = sum_{c < x} (a_c - b_c) and
// P(0) = 0: the best crossover is the arg-max of a prefix sum.  One wavefront takes a link.  Its lanes run over the columns in chunks
// of 64; a lane scores its column of j and of i from the resident codes (as stitch.hip's member kernel scores a column), a wave prefix
// sum of a_c - b_c is carried from chunk to chunk, and a lane keeps the best (P, x) it has met, replacing it only by a strictly
// larger P, so that within a lane the lowest x stays.  A final shuffle reduction takes the largest P and among equals the lowest x.
// No atomics, no scratch, no LDS beyond the 64 matrix entries; the loop runs ceil(o / 64) <= 64 times.
#include "chaintrim.h"

namespace sa {

namespace {

__global__ __launch_bounds__(256) void chaintrim_crossover_kernel(StitchArgs a, const TrimLinkTask* __restrict__ tasks, uint32_t n,
                                                                  uint32_t* __restrict__ x) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= n) return;
    const int lane = threadIdx.x & 63;
    const TrimLinkTask t = tasks[l];
    const uint8_t *jr = a.ref + t.jr, *jq = a.query + t.jq, *ir = a.ref + t.ir, *iq = a.query + t.iq;
    long long carry = 0, best = 0;  // P(0) = 0 at x = 0
    uint32_t bx = 0;
    for (uint32_t base = 0; base < t.o; base += 64) {
        const uint32_t c = base + lane;
        long long d = 0;
        if (c < t.o) d = (long long)s_sub[(jr[c] & 7) * 8 + (jq[c] & 7)] - (long long)s_sub[(ir[c] & 7) * 8 + (iq[c] & 7)];
        for (int k = 1; k < 64; k <<= 1) {  // inclusive prefix sum over the wave
            const long long up = __shfl_up(d, k);
            if (lane >= k) d += up;
        }
        const long long p = carry + d;  // P(c + 1)
        if (c < t.o && p > best) {
            best = p;
            bx = c + 1;
        }
        carry = __shfl(p, 63);
    }
    for (int k = 32; k > 0; k >>= 1) {
        const long long ob = __shfl_xor(best, k);
        const uint32_t ox = __shfl_xor(bx, k);
        if (ob > best || (ob == best && ox < bx)) {
            best = ob;
            bx = ox;
        }
    }
    if (lane == 0) x[l] = bx;
}

}  // namespace

void launch_chaintrim_crossover(const StitchArgs& a, const TrimLinkTask* tasks, uint32_t n, uint32_t* x, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(chaintrim_crossover_kernel, dim3((n + 3) / 4), dim3(256), 0, s, a, tasks, n, x);
}

}  // namespace sa
