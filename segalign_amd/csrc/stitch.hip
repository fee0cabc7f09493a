// stitch.hip -- the links of sa_stitch_chains: a global affine alignment (Gotoh) of the rectangle between two consecutive members of a
// chain, fixed at both corners, one wavefront per link.
//
// The contract is written out in include/segalign_amd.h (sa_stitch_chains) and DESIGN.md 17; tests/cpp/stitch_check.c restates it
// serially.  The sweep runs the antidiagonals d = i + j = 1 .. dt + dq of the rectangle with the recurrence of gapped.hip, but the
// window never moves: lane l owns rows l K .. l K + K - 1 for the whole link, so
//
//   * X[i - 1] of every row is loaded once and stays put;
//   * the E neighbour (i, j - 1) is the slot itself on d - 1, the F neighbour (i - 1, j) and the M neighbour (i - 1, j - 1) are the slot
//     below on d - 1 and d - 2: a register move inside the lane, one cross-lane shift for the lane's edge slot;
//   * Y[j - 1] shifts one slot per antidiagonal; the one new code per step comes from a 64-lane prefetch that is refilled one coalesced
//     load ahead;
//   * there is no live range, no ballot, no reduction and no y-drop: a cell is dead outside the rectangle or at a separator, nothing else.
//
// It writes gapped.h's trace area (4 bits per cell, window base 0 everywhere), so gapped.hip's walk kernel follows the path as it stands.
#include "stitch.h"

namespace sa {

namespace {

constexpr int NEG = STITCH_NEG;
constexpr int SEP = 7;

__device__ __forceinline__ int edge_up(int v) {  // lane l receives lane l - 1's value, lane 0 NEG
    const int r = __shfl_up(v, 1);
    return (threadIdx.x & 63) == 0 ? NEG : r;
}

// The query codes of one link consumed in order: buf holds elements [base, base + 64) (lane l: base + l), nxt the 64 after them.
// Elements from n on are never used as a base and read as 0, so no load leaves the link's range.
struct Codes {
    const uint8_t* s;
    int n, buf, nxt, pos, base;
    __device__ int code(int p) const { return p < n ? (s[p] & 7) : 0; }
    __device__ void init(const uint8_t* seq, int count) {
        const int lane = threadIdx.x & 63;
        s = seq;
        n = count;
        base = 0;
        pos = 0;
        buf = code(lane);
        nxt = code(64 + lane);
    }
    __device__ int take() {
        const int v = __builtin_amdgcn_readlane(buf, pos);
        if (++pos == 64) {
            buf = nxt;
            base += 64;
            pos = 0;
            nxt = code(base + 64 + (threadIdx.x & 63));
        }
        return v;
    }
};

// Cell codes as gapped.hip writes them: bits 0-1 the source of H (0 M, 1 E, 2 F, by the tie rules of the contract), bit 2 E extends,
// bit 3 F extends.
template <int K>
__device__ void stitch_link(const StitchArgs& a, const int* __restrict__ sub, const TraceTask& t, uint32_t* __restrict__ trace,
                            int32_t* __restrict__ score) {
    constexpr int NW = (K + 7) / 8;  // trace dwords per lane per antidiagonal
    const int lane = threadIdx.x & 63;
    const int O = a.gap_open, Ext = a.gap_extend, dt = t.best_i, dq = t.best_j, dstar = t.dstar;
    const uint8_t* X = a.ref + t.ar;
    int H1[K], E1[K], F1[K], H2[K], xc[K], yc[K];
    // antidiagonal 0: the cell (0, 0); antidiagonal -1: nothing
#pragma unroll
    for (int s = 0; s < K; s++) {
        const int i = lane * K + s;
        H1[s] = i == 0 ? 0 : NEG;
        E1[s] = F1[s] = H2[s] = NEG;
        xc[s] = (i >= 1 && i <= dt) ? (X[i - 1] & 7) : 0;  // X[i - 1] of row i; rows beyond dt are dead
        yc[s] = 0;
    }
    Codes ys;
    ys.init(a.query + t.aq, dq);
    int* wbase = (int*)(trace + (size_t)dstar * 64 * NW);
    if (lane == 0) wbase[0] = 0;
    for (int d = 1; d <= dstar; d++) {
        // what slot 0 takes from the lane below: H and F of d - 1, H of d - 2 and the query code that moves up
        const int eH = edge_up(H1[K - 1]), eF = edge_up(F1[K - 1]), eM = edge_up(H2[K - 1]);
        int eY = __shfl_up(yc[K - 1], 1);
        const int fresh = ys.take();  // Y[d - 1] for the cell (0, d)
        if (lane == 0) eY = fresh;
        uint32_t pk[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) pk[k] = 0;
        // top slot first: slot s reads slot s - 1 of the antidiagonals before, which is still untouched
#pragma unroll
        for (int s = K - 1; s >= 0; s--) {
            const int i = lane * K + s, j = d - i;
            const int Fh = s ? H1[s > 0 ? s - 1 : 0] : eH, Ff = s ? F1[s > 0 ? s - 1 : 0] : eF, Mh = s ? H2[s > 0 ? s - 1 : 0] : eM;
            const int y = s ? yc[s > 0 ? s - 1 : 0] : eY;
            const int Eh = H1[s], Ee = E1[s];
            const bool dead = i > dt || j < 0 || j > dq || (i >= 1 && xc[s] == SEP) || (j >= 1 && y == SEP);
            const int e = max(max(Ee, Eh - O) - Ext, NEG);
            const int f = max(max(Ff, Fh - O) - Ext, NEG);
            const int m = (i >= 1 && j >= 1) ? max(Mh + sub[xc[s] * 8 + y], NEG) : NEG;
            const int h = max(m, max(e, f));
            const uint32_t src = m == h ? 0u : (e == h ? 1u : 2u);  // (the codes of dead cells are never read)
            const uint32_t eb = Ee > Eh - O, fb = Ff > Fh - O;
            pk[s >> 3] |= (src | eb << 2 | fb << 3) << (4 * (s & 7));
            const bool live = !dead && h > NEG / 2;
            H2[s] = H1[s];
            H1[s] = live ? h : NEG;
            E1[s] = live ? e : NEG;
            F1[s] = live ? f : NEG;
            yc[s] = y;
        }
        uint32_t* row = trace + (size_t)(d - 1) * 64 * NW;
#pragma unroll
        for (int k = 0; k < NW; k++) row[k * 64 + lane] = pk[k];
        if (lane == 0) wbase[d] = 0;
    }
    int v = NEG;
#pragma unroll
    for (int s = 0; s < K; s++)
        if (lane * K + s == dt) v = H1[s];
    if (lane == dt / K) *score = v;
}

template <int K>
__global__ __launch_bounds__(256) void stitch_sweep_kernel(StitchArgs a, const TraceTask* __restrict__ tasks, uint32_t n, uint8_t* area,
                                                          int32_t* __restrict__ score) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t task = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task >= n) return;
    const TraceTask t = tasks[task];
    stitch_link<K>(a, s_sub, t, (uint32_t*)(area + t.trace_off), score + task);
}

__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void stitch_member_kernel(StitchArgs a, const StitchMember* __restrict__ members, uint32_t n,
                                                           StitchMemberOut* __restrict__ out) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n) return;
    const int lane = threadIdx.x & 63;
    const StitchMember h = members[m];
    const uint8_t* x = a.ref + h.rs;
    const uint8_t* y = a.query + h.qs;
    const uint64_t bases = (uint64_t)h.len + 1;
    long long sum = 0, eq = 0;
    for (uint64_t k = lane; k < bases; k += 64) {
        const int cx = x[k] & 7, cy = y[k] & 7;
        sum += s_sub[cx * 8 + cy];
        eq += (cx == cy && cx < 4) ? 1 : 0;
    }
    sum = wave_sum64(sum);
    eq = wave_sum64(eq);
    if (lane == 0) {
        StitchMemberOut r;
        r.score = sum;
        r.matches = (uint32_t)eq;
        r.mismatches = (uint32_t)(bases - (uint64_t)eq);
        out[m] = r;
    }
}

}  // namespace

void launch_stitch_members(const StitchArgs& a, const StitchMember* members, uint32_t n, StitchMemberOut* out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(stitch_member_kernel, dim3((n + 3) / 4), dim3(256), 0, s, a, members, n, out);
}

void launch_stitch_sweep(const StitchArgs& a, int max_band, const TraceTask* tasks, uint32_t n, uint8_t* area, int32_t* score, hipStream_t s) {
    if (n == 0) return;
    const dim3 grid((n + 3) / 4), block(256);
    switch (gapped_cells_per_lane(max_band)) {
        case 2: hipLaunchKernelGGL(stitch_sweep_kernel<2>, grid, block, 0, s, a, tasks, n, area, score); break;
        case 4: hipLaunchKernelGGL(stitch_sweep_kernel<4>, grid, block, 0, s, a, tasks, n, area, score); break;
        case 8: hipLaunchKernelGGL(stitch_sweep_kernel<8>, grid, block, 0, s, a, tasks, n, area, score); break;
        case 17: hipLaunchKernelGGL(stitch_sweep_kernel<17>, grid, block, 0, s, a, tasks, n, area, score); break;
        default: hipLaunchKernelGGL(stitch_sweep_kernel<33>, grid, block, 0, s, a, tasks, n, area, score); break;
    }
}

}  // namespace sa
