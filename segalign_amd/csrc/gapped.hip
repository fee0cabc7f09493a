// gapped.hip -- gapped y-drop extension of HSP anchors (affine gaps, Gotoh), one wavefront per (HSP, side).
//
// The contract is written out in include/segalign_amd.h (sa_gapped_extend) and DESIGN.md 11; tests/cpp/gapped_check.c restates it
// serially.  This kernel sweeps the antidiagonals d = i + j = 1, 2, ... of one one-sided extension:
//
//   * lanes along i: the wave holds a window of W = 64 K consecutive i values, lane l owns cells l K .. l K + K - 1 in registers.  The
//     window base moves by 0 or 1 per antidiagonal (the cells that can be finite on d always fit one of the two windows, see
//     gapped_side), so the neighbours of a cell on d-1 and d-2 are at most one cell away: a register move inside the lane, one
//     cross-lane shift for the lane's edge slot;
//   * codes: X[i-1] and Y[j-1] of every cell stay in registers and shift with the window; the single new code a step needs (the
//     window's top cell when the base moves, its bottom cell otherwise) comes from a 64-lane prefetch buffer of the sequence stream
//     that is read with v_readlane and refilled one coalesced load ahead;
//   * per antidiagonal: a ballot gives the live range (band cap, next step's candidate range), a wave max-reduction the best cell.
//
// Values are int32 clamped at NEG (minus infinity); finite values stay above NEG / 2 under the parameter limits of the C-ABI.
#include "gapped.h"

namespace sa {

namespace {

constexpr int NEG = -(1 << 30);
constexpr int SEP = 7;

struct Seq {  // one direction of one sequence as seen from the anchor: element p is s[a + p] (dir +1) or s[a - 1 - p] (dir -1)
    const uint8_t* s;
    long long len, a;
    int dir;
    __device__ int code(long long p) const {
        if (p < 0) return 0;  // (index -1 of the i = 0 / j = 0 cells: never read as a base)
        const long long pos = dir > 0 ? a + p : a - 1 - p;
        return (pos < 0 || pos >= len) ? SEP : (s[pos] & 7);
    }
};

__device__ __forceinline__ int shift_in_up(int v) {  // lane l receives lane l-1's value, lane 0 NEG
    const int r = __shfl_up(v, 1);
    return (threadIdx.x & 63) == 0 ? NEG : r;
}
__device__ __forceinline__ int shift_in_down(int v) {  // lane l receives lane l+1's value, lane 63 NEG
    const int r = __shfl_down(v, 1);
    return (threadIdx.x & 63) == 63 ? NEG : r;
}
// res[c] = a[c - 1] (cell -1 of the window: NEG)
template <int K>
__device__ __forceinline__ void cells_up(const int (&a)[K], int (&r)[K]) {
    const int edge = shift_in_up(a[K - 1]);
#pragma unroll
    for (int s = K - 1; s > 0; s--) r[s] = a[s - 1];
    r[0] = edge;
}
// res[c] = a[c + 1] (cell W of the window: NEG)
template <int K>
__device__ __forceinline__ void cells_down(const int (&a)[K], int (&r)[K]) {
    const int edge = shift_in_down(a[0]);
#pragma unroll
    for (int s = 0; s < K - 1; s++) r[s] = a[s + 1];
    r[K - 1] = edge;
}
template <int K>
__device__ __forceinline__ void cells_copy(const int (&a)[K], int (&r)[K]) {
#pragma unroll
    for (int s = 0; s < K; s++) r[s] = a[s];
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o);
    return v;
}

// A sequence stream consumed one element per use, in order, from `next` on: buf holds elements [base, base + 64) (lane l: base + l),
// nxt the 64 after them (loaded one buffer ahead, so a refill waits on nothing).
struct Stream {
    int buf, nxt, pos;
    long long base;
    __device__ void init(const Seq& q, long long first) {
        const int lane = threadIdx.x & 63;
        base = first;
        pos = 0;
        buf = q.code(first + lane);
        nxt = q.code(first + 64 + lane);
    }
    __device__ int take(const Seq& q) {
        const int v = __builtin_amdgcn_readlane(buf, pos);
        if (++pos == 64) {
            buf = nxt;
            base += 64;
            pos = 0;
            nxt = q.code(base + 64 + (threadIdx.x & 63));
        }
        return v;
    }
};

template <int K>
__device__ void gapped_side(const GappedArgs& a, const int* __restrict__ sub, const Seq& X, const Seq& Y, GappedSide* out) {
    constexpr int W = 64 * K;
    const int lane = threadIdx.x & 63;
    const int O = a.gap_open, Ext = a.gap_extend, ydrop = a.ydrop, maxe = a.max_extent, maxband = a.max_band;
    int H1[K], E1[K], F1[K], H2[K], xc[K], yc[K];
    // antidiagonal 0 in the window [0, W): the anchor cell (0, 0); antidiagonal -1: nothing
#pragma unroll
    for (int s = 0; s < K; s++) {
        const int c = lane * K + s;
        H1[s] = c == 0 ? 0 : NEG;
        E1[s] = F1[s] = H2[s] = NEG;
        xc[s] = X.code(c - 1);  // X[i - 1] of cell i = c
        yc[s] = 0;              // j = -c <= 0: no Y base
    }
    Stream xs, ys;
    xs.init(X, W - 1);  // the next X code a base move brings in: X[W - 1] for cell i = W
    ys.init(Y, 0);      // the next Y code: Y[0] for cell j = 1
    int w1 = 0, w2 = 0;              // window bases of antidiagonals d-1, d-2
    int lo1 = 0, hi1 = 0, lo2 = 1, hi2 = 0;  // their live ranges (lo > hi: none)
    int best = 0, best_i = 0, best_j = 0;
    unsigned cnt = 0, ext = 0, flags = 0;
    for (int d = 1;; d++) {
        const bool e1 = lo1 > hi1, e2 = lo2 > hi2;
        if (e1 && e2) break;  // two consecutive antidiagonals without a live cell
        int lo = 0x7fffffff, hi = -0x7fffffff;
        if (!e1) { lo = min(lo, lo1); hi = max(hi, hi1 + 1); }
        if (!e2) { lo = min(lo, lo2 + 1); hi = max(hi, hi2 + 1); }
        lo = max(lo, max(0, d - maxe));
        hi = min(hi, min(d, maxe));
        if (hi - lo + 1 > maxband + 1) { flags |= SA_GAPPED_BAND_CAP; break; }
        // the candidates lie in [w1, w1 + W]: move the window by one only when the top one is outside [w1, w1 + W)
        const int delta = hi >= w1 + W ? 1 : 0;
        const int dp = w1 - w2;
        const int w = w1 + delta;
        int Eh[K], Ee[K], Fh[K], Ff[K], Mh[K];
        if (delta) {
            cells_down<K>(H1, Eh); cells_down<K>(E1, Ee);
            cells_copy<K>(H1, Fh); cells_copy<K>(F1, Ff);
            if (dp) cells_down<K>(H2, Mh); else cells_copy<K>(H2, Mh);
            int t[K];
            cells_down<K>(xc, t);
            const int fresh = xs.take(X);
            if (lane == 63) t[K - 1] = fresh;
            cells_copy<K>(t, xc);
        } else {
            cells_copy<K>(H1, Eh); cells_copy<K>(E1, Ee);
            cells_up<K>(H1, Fh); cells_up<K>(F1, Ff);
            if (dp) cells_copy<K>(H2, Mh); else cells_up<K>(H2, Mh);
            int t[K];
            cells_up<K>(yc, t);
            const int fresh = ys.take(Y);
            if (lane == 0) t[0] = fresh;
            cells_copy<K>(t, yc);
        }
        const int floor_ = best - ydrop;
        int lbest = NEG, lbest_s = 0, llo_s = -1, lhi_s = -1;
        unsigned lcnt = 0, lext = 0;
#pragma unroll
        for (int s = 0; s < K; s++) {
            const int i = w + lane * K + s, j = d - i;
            const bool dead = i < lo || i > hi || (i >= 1 && xc[s] == SEP) || (j >= 1 && yc[s] == SEP);
            const int e = max(max(Ee[s], Eh[s] - O) - Ext, NEG);
            const int f = max(max(Ff[s], Fh[s] - O) - Ext, NEG);
            const int m = (i >= 1 && j >= 1) ? max(Mh[s] + sub[xc[s] * 8 + yc[s]], NEG) : NEG;
            const int h = max(m, max(e, f));
            const bool live = !dead && h > NEG / 2 && h >= floor_;
            H2[s] = H1[s];
            H1[s] = live ? h : NEG;
            E1[s] = live ? e : NEG;
            F1[s] = live ? f : NEG;
            if (live) {
                if (llo_s < 0) llo_s = s;
                lhi_s = s;
                lcnt++;
                if (h > lbest) { lbest = h; lbest_s = s; }
                if (i == maxe || j == maxe) lext = 1;
            }
        }
        const unsigned long long mask = __ballot(llo_s >= 0);
        int nlo = 1, nhi = 0;
        if (mask) {
            const int ll = __builtin_ctzll(mask), lh = 63 - __builtin_clzll(mask);
            nlo = w + ll * K + __builtin_amdgcn_readlane(llo_s, ll);
            nhi = w + lh * K + __builtin_amdgcn_readlane(lhi_s, lh);
            if (nhi - nlo + 1 > maxband) { flags |= SA_GAPPED_BAND_CAP; break; }
            const int m = wave_max(lbest);
            if (m > best) {
                const unsigned long long bm = __ballot(lbest == m);
                const int bl = __builtin_ctzll(bm);
                best = m;
                best_i = w + bl * K + __builtin_amdgcn_readlane(lbest_s, bl);
                best_j = d - best_i;
            }
        }
        cnt += lcnt;
        ext |= lext;
        w2 = w1; w1 = w;
        lo2 = lo1; hi2 = hi1;
        lo1 = nlo; hi1 = nhi;
    }
    const unsigned cells = wave_sum(cnt) + 1;  // + the anchor cell (0, 0)
    if (wave_or(ext)) flags |= SA_GAPPED_EXTENT_CAP;
    if (lane == 0) {
        out->best = best;
        out->best_i = best_i;
        out->best_j = best_j;
        out->cells = cells;
        out->flags = flags;
    }
}

template <int K>
__global__ __launch_bounds__(256) void gapped_kernel(GappedArgs a) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t task = blockIdx.x * 4 + (threadIdx.x >> 6);  // (HSP, side): 2 h + 0 left, 2 h + 1 right
    if (task >= a.num_tasks) return;
    const sa_segment_pair hs = a.hsps[task >> 1];
    const long long ar = (long long)hs.ref_start + hs.len / 2, aq = (long long)hs.query_start + hs.len / 2;
    const int dir = (task & 1) ? 1 : -1;
    const Seq X = {a.ref, (long long)a.ref_len, ar, dir};
    const Seq Y = {a.query, (long long)a.query_len, aq, dir};
    gapped_side<K>(a, s_sub, X, Y, a.out + task);
}

}  // namespace

int gapped_cells_per_lane(int max_band) {
    for (int k : {2, 4, 8, 17, 33})
        if (64 * k >= max_band + 1) return k;
    return -1;
}

void launch_gapped(const GappedArgs& a, hipStream_t s) {
    if (a.num_tasks == 0) return;
    const dim3 grid((a.num_tasks + 3) / 4), block(256);
    switch (gapped_cells_per_lane(a.max_band)) {
        case 2: hipLaunchKernelGGL(gapped_kernel<2>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(gapped_kernel<4>, grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL(gapped_kernel<8>, grid, block, 0, s, a); break;
        case 17: hipLaunchKernelGGL(gapped_kernel<17>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(gapped_kernel<33>, grid, block, 0, s, a); break;
    }
}

}  // namespace sa
