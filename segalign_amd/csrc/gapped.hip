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
//
// sa_gapped_align adds two kernels: the TRACE instance of the same sweep, which stops at the side's best antidiagonal d*
// and stores 4 bits per cell (H source, E extend, F extend) plus the window base of every antidiagonal, and a walk kernel that
// follows those bits from the best cell back to the anchor, 64 antidiagonals at a time staged in LDS.
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

// TRACE = false: the extension (pass 1), result in *out.  TRACE = true: the same sweep over antidiagonals 1 .. dstar only, writing the
// trace area of gapped.h (4-bit cell codes: bits 0-1 the source of H -- 0 M, 1 E, 2 F, by the tie rules of the contract --, bit 2 E
// extends, bit 3 F extends) and nothing else.
template <int K, bool TRACE>
__device__ void gapped_side(const GappedArgs& a, const int* __restrict__ sub, const Seq& X, const Seq& Y, GappedSide* out,
                            uint32_t* __restrict__ trace, int dstar) {
    constexpr int W = 64 * K;
    constexpr int NW = (K + 7) / 8;  // trace dwords per lane per antidiagonal
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
    int* wbase = nullptr;
    if constexpr (TRACE) {
        wbase = (int*)(trace + (size_t)dstar * 64 * NW);
        if (lane == 0) wbase[0] = 0;
    }
    for (int d = 1;; d++) {
        if constexpr (TRACE) {
            if (d > dstar) break;  // the best cell's antidiagonal is traced: the sweep up to it is pass 1's, step for step
        }
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
        uint32_t pk[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) pk[k] = 0;
#pragma unroll
        for (int s = 0; s < K; s++) {
            const int i = w + lane * K + s, j = d - i;
            const bool dead = i < lo || i > hi || (i >= 1 && xc[s] == SEP) || (j >= 1 && yc[s] == SEP);
            const int e = max(max(Ee[s], Eh[s] - O) - Ext, NEG);
            const int f = max(max(Ff[s], Fh[s] - O) - Ext, NEG);
            const int m = (i >= 1 && j >= 1) ? max(Mh[s] + sub[xc[s] * 8 + yc[s]], NEG) : NEG;
            const int h = max(m, max(e, f));
            if constexpr (TRACE) {  // (the codes of cells that are not live are never read)
                const uint32_t src = m == h ? 0u : (e == h ? 1u : 2u);
                const uint32_t eb = Ee[s] > Eh[s] - O, fb = Ff[s] > Fh[s] - O;
                pk[s >> 3] |= (src | eb << 2 | fb << 3) << (4 * (s & 7));
            }
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
        if constexpr (TRACE) {
            uint32_t* row = trace + (size_t)(d - 1) * 64 * NW;
#pragma unroll
            for (int k = 0; k < NW; k++) row[k * 64 + lane] = pk[k];
            if (lane == 0) wbase[d] = w;
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
    if constexpr (TRACE) return;
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
    gapped_side<K, false>(a, s_sub, X, Y, a.out + task, nullptr, 0);
}

// Pass 1 of sides that start at an explicit origin (the continuation pieces of DESIGN.md 14): the same sweep, one wave per task.
template <int K>
__global__ __launch_bounds__(256) void gapped_sides_kernel(GappedArgs a, const SideTask* __restrict__ tasks, uint32_t n,
                                                           GappedSide* __restrict__ out) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t task = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task >= n) return;
    const SideTask t = tasks[task];
    const Seq X = {a.ref, (long long)a.ref_len, (long long)t.ar, t.dir};
    const Seq Y = {a.query, (long long)a.query_len, (long long)t.aq, t.dir};
    gapped_side<K, false>(a, s_sub, X, Y, out + task, nullptr, 0);
}

template <int K>
__global__ __launch_bounds__(256) void gapped_trace_kernel(GappedArgs a, const TraceTask* __restrict__ tasks, uint32_t n, uint8_t* area) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t task = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (task >= n) return;
    const TraceTask t = tasks[task];
    const Seq X = {a.ref, (long long)a.ref_len, (long long)t.ar, t.dir};
    const Seq Y = {a.query, (long long)a.query_len, (long long)t.aq, t.dir};
    gapped_side<K, true>(a, s_sub, X, Y, nullptr, (uint32_t*)(area + t.trace_off), t.dstar);
}

// One wave per traced side.  The walk state (cell, H / E / F) is wave-uniform.  Every 64 antidiagonals the wave stages the codes of
// the region the path can reach next -- antidiagonals d0 .. d0 - 63, target bases i0 - 63 .. i0 (each step lowers d by 1 or 2 and i
// by at most as much) -- into LDS, one cell per lane and antidiagonal, all loads independent of one another; the walk then reads LDS
// only.  The M pairs of a stage are matched against the codes afterwards, one pair per lane.
template <int K>
__global__ __launch_bounds__(256) void gapped_walk_kernel(GappedArgs a, const TraceTask* __restrict__ tasks, uint32_t n,
                                                         const uint8_t* __restrict__ area, uint32_t* __restrict__ ops,
                                                         TraceOut* __restrict__ out) {
    constexpr int W = 64 * K, NW = (K + 7) / 8;
    __shared__ uint8_t s_code[4][64][64];  // [wave][antidiagonal d0 - r][cell i0 - 63 + c]
    __shared__ int s_mi[4][64], s_mj[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t task = blockIdx.x * 4 + wave;
    if (task >= n) return;
    const TraceTask t = tasks[task];
    const uint32_t* tr = (const uint32_t*)(area + t.trace_off);
    const int* wbase = (const int*)(tr + (size_t)t.dstar * 64 * NW);
    uint32_t* o = ops + t.ops_off;
    const Seq X = {a.ref, (long long)a.ref_len, (long long)t.ar, t.dir};
    const Seq Y = {a.query, (long long)a.query_len, (long long)t.aq, t.dir};
    int i = t.best_i, j = t.best_j, st = 0;  // st: 0 H, 1 E, 2 F
    int cur = -1;
    uint32_t len = 0, nr = 0, opens = 0, gapb = 0, matches = 0, mism = 0, err = 0;
    auto emit = [&](int op) {
        if (op == cur) { len++; return; }
        if (len) {
            if (nr >= (uint32_t)t.dstar) { err = 1; return; }
            if (lane == 0) o[nr] = len << 2 | (uint32_t)cur;
            nr++;
            if (cur != (int)SA_GAPPED_OP_M) { opens++; gapb += len; }
        }
        cur = op;
        len = 1;
    };
    while (!err && i + j > 0) {
        const int d0 = i + j, ib = i - 63;
        const int nd = min(64, d0);  // antidiagonals d0 .. d0 - nd + 1, all >= 1
        const int wl = lane < nd ? wbase[d0 - lane] : 0;
#pragma unroll 16
        for (int r = 0; r < 64; r++) {
            const int w = __shfl(wl, r);
            const int dd = d0 - r, ii = ib + lane, slot = ii - w;
            uint32_t code = 0;  // cells the path cannot reach: never read
            if (r < nd && ii >= 0 && dd - ii >= 0 && slot >= 0 && slot < W) {
                const int l = slot / K, s = slot - l * K;
                code = (tr[(size_t)(dd - 1) * 64 * NW + (s >> 3) * 64 + l] >> (4 * (s & 7))) & 15u;
            }
            s_code[wave][r][lane] = (uint8_t)code;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int nm = 0;
        while (i + j > 0 && d0 - (i + j) < nd) {
            const int r = d0 - (i + j), c = i - ib;
            if (i < 0 || j < 0 || c < 0 || c > 63 || nm >= 64) { err = 2; break; }
            const uint32_t code = s_code[wave][r][c];
            if (st == 0) {
                const uint32_t src = code & 3u;
                if (src == 0) {
                    emit(SA_GAPPED_OP_M);
                    s_mi[wave][nm] = i;
                    s_mj[wave][nm] = j;
                    nm++;
                    i--;
                    j--;
                } else if (src == 3) {
                    err = 3;
                    break;
                } else {
                    st = (int)src;
                }
            } else if (st == 1) {
                emit(SA_GAPPED_OP_I);
                st = (code >> 2) & 1u ? 1 : 0;
                j--;
            } else {
                emit(SA_GAPPED_OP_D);
                st = (code >> 3) & 1u ? 2 : 0;
                i--;
            }
            if (err) break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        bool match = false;
        if (lane < nm) {
            const int x = X.code(s_mi[wave][lane] - 1), y = Y.code(s_mj[wave][lane] - 1);
            match = x == y && x < 4;
        }
        const uint32_t nmatch = (uint32_t)__popcll(__ballot(match));
        matches += nmatch;
        mism += (uint32_t)nm - nmatch;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (!err && (i != 0 || j != 0 || st != 0)) err = 4;
    if (!err) emit(-1);  // flush the last run
    if (lane == 0) {
        TraceOut r;
        r.n_runs = nr;
        r.matches = matches;
        r.mismatches = mism;
        r.gap_opens = opens;
        r.gap_bases = gapb;
        r.err = err;
        r.pad[0] = r.pad[1] = 0;
        out[task] = r;
    }
}

}  // namespace

int gapped_cells_per_lane(int max_band) {
    for (int k : {2, 4, 8, 17, 33})
        if (64 * k >= max_band + 1) return k;
    return -1;
}

size_t gapped_trace_bytes(int max_band, int dstar) {
    const size_t nw = (size_t)(gapped_cells_per_lane(max_band) + 7) / 8;
    return ((size_t)dstar * 64 * nw * 4 + ((size_t)dstar + 1) * 4 + 255) & ~(size_t)255;
}

void launch_gapped_trace(const GappedArgs& a, const TraceTask* tasks, uint32_t n, uint8_t* area, hipStream_t s) {
    if (n == 0) return;
    const dim3 grid((n + 3) / 4), block(256);
    switch (gapped_cells_per_lane(a.max_band)) {
        case 2: hipLaunchKernelGGL(gapped_trace_kernel<2>, grid, block, 0, s, a, tasks, n, area); break;
        case 4: hipLaunchKernelGGL(gapped_trace_kernel<4>, grid, block, 0, s, a, tasks, n, area); break;
        case 8: hipLaunchKernelGGL(gapped_trace_kernel<8>, grid, block, 0, s, a, tasks, n, area); break;
        case 17: hipLaunchKernelGGL(gapped_trace_kernel<17>, grid, block, 0, s, a, tasks, n, area); break;
        default: hipLaunchKernelGGL(gapped_trace_kernel<33>, grid, block, 0, s, a, tasks, n, area); break;
    }
}

void launch_gapped_walk(const GappedArgs& a, const TraceTask* tasks, uint32_t n, const uint8_t* area, uint32_t* ops, TraceOut* out,
                        hipStream_t s) {
    if (n == 0) return;
    const dim3 grid((n + 3) / 4), block(256);
    switch (gapped_cells_per_lane(a.max_band)) {
        case 2: hipLaunchKernelGGL(gapped_walk_kernel<2>, grid, block, 0, s, a, tasks, n, area, ops, out); break;
        case 4: hipLaunchKernelGGL(gapped_walk_kernel<4>, grid, block, 0, s, a, tasks, n, area, ops, out); break;
        case 8: hipLaunchKernelGGL(gapped_walk_kernel<8>, grid, block, 0, s, a, tasks, n, area, ops, out); break;
        case 17: hipLaunchKernelGGL(gapped_walk_kernel<17>, grid, block, 0, s, a, tasks, n, area, ops, out); break;
        default: hipLaunchKernelGGL(gapped_walk_kernel<33>, grid, block, 0, s, a, tasks, n, area, ops, out); break;
    }
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

void launch_gapped_sides(const GappedArgs& a, const SideTask* tasks, uint32_t n, GappedSide* out, hipStream_t s) {
    if (n == 0) return;
    const dim3 grid((n + 3) / 4), block(256);
    switch (gapped_cells_per_lane(a.max_band)) {
        case 2: hipLaunchKernelGGL(gapped_sides_kernel<2>, grid, block, 0, s, a, tasks, n, out); break;
        case 4: hipLaunchKernelGGL(gapped_sides_kernel<4>, grid, block, 0, s, a, tasks, n, out); break;
        case 8: hipLaunchKernelGGL(gapped_sides_kernel<8>, grid, block, 0, s, a, tasks, n, out); break;
        case 17: hipLaunchKernelGGL(gapped_sides_kernel<17>, grid, block, 0, s, a, tasks, n, out); break;
        default: hipLaunchKernelGGL(gapped_sides_kernel<33>, grid, block, 0, s, a, tasks, n, out); break;
    }
}

}  // namespace sa
