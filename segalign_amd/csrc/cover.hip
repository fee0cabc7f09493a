// cover.hip -- the cover index of sa_gapped_align_greedy (contract: include/segalign_amd.h).
//
// An accepted alignment covers the points (t, q) of its M runs and its own anchor point.  Each M run is one segment of a diagonal.  The
// index holds the accepted segments sorted by key = diag << 32 | t_begin and, per entry, the running maximum of t_end within its
// diagonal: a point is covered when the last entry with key <= its own key lies on its diagonal and that maximum exceeds its t.
// Segments of different paths overlap and nest, so the running maximum, not the entry's own t_end, answers the question.
//
// Per priority batch the host runs: query (earlier batches' index against the batch's anchors), emit (inside the trace loop, from the
// walk's own output), edges (segments of eligible survivors against the sorted survivor anchors, count / scan / scatter into CSR by
// the covered survivor), resolve (one wave, the sequential rule over the survivors), select + sort + merge + running-max scan (the
// accepted segments into the index).  The sorts and scans are rocPRIM's.
#include <atomic>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gapped.h"

namespace sa {

namespace {

__device__ __forceinline__ uint32_t lower_bound64(const uint64_t* a, uint32_t n, uint64_t x) {  // first index with a[i] >= x
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t upper_bound64(const uint64_t* a, uint32_t n, uint64_t x) {  // first index with a[i] > x
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One wave per traced side, or per piece of a continued side: (a_r, a_q) below is the task's own origin, so a piece's runs
// are placed from that piece's origin and best cell, not from the record's start.  Walk order runs from the far end to the origin:
// forward in the genome on the left side (from (a_r - best_i, a_q - best_j)), backward on the right side (from (a_r + best_i, a_q + best_j)).  A wave prefix over the runs' target and query
// lengths places every run of a 64-run chunk; the chunk's totals carry into the next.
__global__ void __launch_bounds__(256) cover_emit_kernel(const TraceTask* tasks, const TraceOut* out, const uint32_t* ops,
                                                         const CoverEmit* emit, uint32_t n, uint32_t query_len, CoverSeg* segs) {
    const uint32_t w = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (w >= n) return;
    const TraceTask T = tasks[w];
    const uint32_t nr = out[w].n_runs;
    const CoverEmit E = emit[w];
    const uint32_t* o = ops + T.ops_off;
    const bool right = T.dir > 0;
    uint32_t t0 = right ? T.ar + (uint32_t)T.best_i : T.ar - (uint32_t)T.best_i;
    uint32_t q0 = right ? T.aq + (uint32_t)T.best_j : T.aq - (uint32_t)T.best_j;
    for (uint32_t base = 0; base < nr; base += 64) {
        const uint32_t k = base + lane;
        const uint32_t x = k < nr ? o[k] : 0u;
        const uint32_t len = x >> 2, op = x & 3;
        const uint32_t dt = (k < nr && op != SA_GAPPED_OP_I) ? len : 0u, dq = (k < nr && op != SA_GAPPED_OP_D) ? len : 0u;
        uint32_t it = dt, iq = dq;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t a = __shfl_up(it, d), b = __shfl_up(iq, d);
            if ((int)lane >= d) {
                it += a;
                iq += b;
            }
        }
        if (k < nr) {
            const uint32_t et = it - dt, eq = iq - dq;  // target / query bases of the chunk's earlier runs
            CoverSeg g;
            g.owner = E.owner;
            if (op == SA_GAPPED_OP_M) {
                const uint32_t tb = right ? t0 - et - len : t0 + et, qb = right ? q0 - eq - len : q0 + eq;
                g.key = (uint64_t)(tb - qb + query_len) << 32 | tb;
                g.t_end = tb + len;
            } else {
                g.key = COVER_NONE;
                g.t_end = 0;
            }
            segs[E.seg_off + k] = g;
        }
        const uint32_t tt = __shfl(it, 63), tq = __shfl(iq, 63);
        if (right) {
            t0 -= tt;
            q0 -= tq;
        } else {
            t0 += tt;
            q0 += tq;
        }
    }
}

__global__ void __launch_bounds__(256) cover_query_kernel(const uint64_t* key, const uint64_t* run, uint32_t n_index, const uint64_t* keys,
                                                          uint32_t n, uint8_t* covered) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t x = keys[k];
    const uint32_t i = upper_bound64(key, n_index, x);
    covered[k] = (i > 0 && (run[i - 1] >> 32) == (x >> 32) && (uint32_t)run[i - 1] > (uint32_t)x) ? 1 : 0;
}

__global__ void __launch_bounds__(256) cover_edges_kernel(const CoverSeg* segs, uint32_t n_segs, const uint64_t* akey, const uint32_t* arank,
                                                          uint32_t n_anchors, const uint8_t* eligible, uint32_t lo, uint32_t hi,
                                                          uint32_t* deg, unsigned long long* cursor, uint32_t* src, int count) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    const CoverSeg g = segs[s];
    if (g.key == COVER_NONE || g.owner < lo || g.owner >= hi || !eligible[g.owner]) return;
    const uint64_t end = (g.key & ~0xffffffffull) | g.t_end;
    for (uint32_t i = lower_bound64(akey, n_anchors, g.key); i < n_anchors && akey[i] < end; i++) {
        const uint32_t h = arank[i];
        if (h <= g.owner || h >= hi) continue;
        if (count) atomicAdd(&deg[h - lo], 1u);
        else src[atomicAdd(&cursor[h - lo], 1ull)] = g.owner - lo;
    }
}

// The sequential rule, one wave.  Lanes load 64 survivors' eligibility and CSR rows at a time; for each survivor in turn they test its
// in-edges against the accepted bits in LDS, a ballot decides, and lane 0 sets the survivor's bit.  Exact by construction: survivor h
// is decided after every survivor before it.  The accepted bits take (n + 31) / 32 words of dynamic LDS.
__global__ void __launch_bounds__(64) cover_resolve_kernel(const uint8_t* eligible, const uint64_t* row, const uint32_t* src, uint32_t n,
                                                           uint8_t* state) {
    extern __shared__ uint32_t acc[];
    const uint32_t lane = threadIdx.x;
    for (uint32_t w = lane; w < (n + 31) / 32; w += 64) acc[w] = 0;
    __syncthreads();
    for (uint32_t h0 = 0; h0 < n; h0 += 64) {
        const uint32_t h = h0 + lane;
        const int el = h < n ? eligible[h] : 0;
        const uint64_t r0 = h < n ? row[h] : 0ull, r1 = h < n ? row[h + 1] : 0ull;
        uint8_t st = 0;
        const uint32_t m = min(64u, n - h0);
        for (uint32_t j = 0; j < m; j++) {
            const uint64_t b = __shfl(r0, j), e = __shfl(r1, j);
            bool cov = false;
            for (uint64_t kb = b; kb < e; kb += 64) {
                bool hit = false;
                if (kb + lane < e) {
                    const uint32_t a = src[kb + lane];
                    hit = (acc[a >> 5] >> (a & 31)) & 1u;
                }
                if (__ballot(hit)) {
                    cov = true;
                    break;
                }
            }
            const int ej = __shfl(el, j);
            if (lane == j) st = cov ? 2 : (el ? 1 : 0);
            if (!cov && ej) {
                if (lane == 0) acc[(h0 + j) >> 5] |= 1u << ((h0 + j) & 31);
                __syncthreads();
            }
        }
        if (h < n) state[h] = st;
    }
}

__global__ void __launch_bounds__(256) cover_select_kernel(const CoverSeg* segs, uint32_t n_segs, const uint8_t* state, uint32_t lo,
                                                           uint32_t hi, uint64_t* key, uint64_t* dt, uint32_t* count) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    const CoverSeg g = segs[s];
    if (g.key == COVER_NONE || g.owner < lo || g.owner >= hi || state[g.owner] != 1) return;
    const uint32_t p = atomicAdd(count, 1u);
    key[p] = g.key;
    dt[p] = (g.key & ~0xffffffffull) | g.t_end;
}

__global__ void __launch_bounds__(256) cover_merge_kernel(const uint64_t* ka, const uint64_t* va, uint32_t na, const uint64_t* kb,
                                                          const uint64_t* vb, uint32_t nb, uint64_t* ko, uint64_t* vo) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) {
        const uint32_t p = i + lower_bound64(kb, nb, ka[i]);
        ko[p] = ka[i];
        vo[p] = va[i];
    } else if (i < na + nb) {
        const uint32_t j = i - na, p = j + upper_bound64(ka, na, kb[j]);
        ko[p] = kb[j];
        vo[p] = vb[j];
    }
}

struct RunMax {  // segmented maximum over values diag << 32 | t_end sorted by diagonal: a new diagonal restarts it
    __host__ __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return (x >> 32) == (y >> 32) ? (x > y ? x : y) : y; }
};

inline dim3 blocks(uint32_t n) { return dim3((n + 255) / 256); }

}  // namespace

void launch_cover_emit(const TraceTask* tasks, const TraceOut* out, const uint32_t* ops, const CoverEmit* emit, uint32_t n,
                       uint32_t query_len, CoverSeg* segs, hipStream_t s) {
    if (n) hipLaunchKernelGGL(cover_emit_kernel, dim3((n + 3) / 4), dim3(256), 0, s, tasks, out, ops, emit, n, query_len, segs);
}

void launch_cover_query(const uint64_t* key, const uint64_t* run, uint32_t n_index, const uint64_t* keys, uint32_t n, uint8_t* covered,
                        hipStream_t s) {
    if (n) hipLaunchKernelGGL(cover_query_kernel, blocks(n), dim3(256), 0, s, key, run, n_index, keys, n, covered);
}

void launch_cover_edges(const CoverSeg* segs, uint32_t n_segs, const uint64_t* akey, const uint32_t* arank, uint32_t n_anchors,
                        const uint8_t* eligible, uint32_t lo, uint32_t hi, uint32_t* deg, uint64_t* cursor, uint32_t* src, int count,
                        hipStream_t s) {
    if (n_segs)
        hipLaunchKernelGGL(cover_edges_kernel, blocks(n_segs), dim3(256), 0, s, segs, n_segs, akey, arank, n_anchors, eligible, lo, hi, deg,
                           (unsigned long long*)cursor, src, count);
}

void launch_cover_resolve(const uint8_t* eligible, const uint64_t* row, const uint32_t* src, uint32_t n, uint8_t* state, hipStream_t s) {
    if (n == 0) return;
    // above 64 KB a launch must ask for its dynamic LDS; the attribute is per device and idempotent, so racing slot threads only repeat it
    const size_t lds = (size_t)(n + 31) / 32 * sizeof(uint32_t);
    if (lds > 64 * 1024) {
        static std::atomic<size_t> set[64];
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev >= 0 && dev < 64 && set[dev].load(std::memory_order_acquire) < lds) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cover_resolve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(COVER_RESOLVE_MAX / 8));
            set[dev].store(COVER_RESOLVE_MAX / 8, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(cover_resolve_kernel, dim3(1), dim3(64), lds, s, eligible, row, src, n, state);
}

void launch_cover_select(const CoverSeg* segs, uint32_t n_segs, const uint8_t* state, uint32_t lo, uint32_t hi, uint64_t* key, uint64_t* dt,
                         uint32_t* count, hipStream_t s) {
    if (n_segs) hipLaunchKernelGGL(cover_select_kernel, blocks(n_segs), dim3(256), 0, s, segs, n_segs, state, lo, hi, key, dt, count);
}

void launch_cover_merge(const uint64_t* ka, const uint64_t* va, uint32_t na, const uint64_t* kb, const uint64_t* vb, uint32_t nb,
                        uint64_t* ko, uint64_t* vo, hipStream_t s) {
    if (na + nb) hipLaunchKernelGGL(cover_merge_kernel, blocks(na + nb), dim3(256), 0, s, ka, va, na, kb, vb, nb, ko, vo);
}

void cover_sort_pairs(void* temp, size_t* bytes, const uint64_t* kin, uint64_t* kout, const uint64_t* vin, uint64_t* vout, uint32_t n,
                      hipStream_t s) {
    (void)rocprim::radix_sort_pairs(temp, *bytes, kin, kout, vin, vout, (size_t)n, 0, 64, s);
}

void cover_sort_anchors(void* temp, size_t* bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout, uint32_t n,
                        hipStream_t s) {
    (void)rocprim::radix_sort_pairs(temp, *bytes, kin, kout, vin, vout, (size_t)n, 0, 64, s);
}

void cover_scan_offsets(void* temp, size_t* bytes, const uint32_t* deg, uint64_t* row, uint32_t n, hipStream_t s) {
    (void)rocprim::exclusive_scan(temp, *bytes, deg, row, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), s);
}

void cover_scan_runmax(void* temp, size_t* bytes, const uint64_t* dt, uint64_t* run, uint32_t n, hipStream_t s) {
    (void)rocprim::inclusive_scan(temp, *bytes, dt, run, (size_t)n, RunMax(), s);
}

}  // namespace sa
