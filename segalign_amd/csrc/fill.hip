// fill.hip -- the diagonal sweep of sa_fill_chains (contract: include/segalign_amd.h).
//
// A task is 64 adjacent diagonals d = i - j of one link's rectangle, one wavefront per task, lane l on d0 + l.  The wave steps along
// the target rows i that any of its diagonals crosses: the target code of a row is wave-uniform, and the lanes' query codes
// j = i - d0 - l are 64 consecutive bytes.  A lane carries the scan's state (s, b, start, bend) in registers and never shares a
// diagonal, so the scan is the contract's, cell by cell.  The sweep runs twice as one template: the count pass leaves the number of
// HSPs per lane, an exclusive scan places them, and the emit pass writes every lane's HSPs from its own offset on, which is the
// contract's order (link, d, i) by construction.  No atomics, no scratch, no LDS beyond the 64 matrix entries; the loop runs at most
// min(dt, dq + 63) times.
#include "fill.h"

namespace sa {

namespace {

template <bool EMIT>
__global__ __launch_bounds__(256) void fill_sweep_kernel(StitchArgs a, FillScan f, const FillTask* __restrict__ tasks, uint32_t t0, uint32_t t1,
                                                         uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint64_t base,
                                                         sa_segment_pair* __restrict__ out, uint32_t* __restrict__ out_link) {
    __shared__ int s_sub[64];
    if (threadIdx.x < 64) s_sub[threadIdx.x] = a.sub_mat[threadIdx.x];
    __syncthreads();
    const uint32_t w = t0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= t1) return;
    const int lane = threadIdx.x & 63;
    const FillTask t = tasks[w];
    const int dt = (int)t.dt, dq = (int)t.dq;
    const int d = t.d0 + lane;
    const bool mine = d < dt;                  // the link's last task may reach past its last diagonal
    const int i0 = d > 0 ? d : 0;              // the diagonal's first cell is (i0, i0 - d)
    const int i_lo = t.d0 > 0 ? t.d0 : 0;      // lane 0's first row is the wave's first
    const int i_top = dq - 1 + t.d0 + 63;      // lane 63's last row is the wave's last
    const int i_hi = i_top < dt - 1 ? i_top : dt - 1;
    const uint8_t* tr = a.ref + t.re;
    const uint8_t* qr = a.query + t.qe;
    int s = 0, b = 0, start = 0, bend = 0;
    uint32_t n = 0;
    size_t at = 0;
    if (EMIT) at = (size_t)(off[(size_t)w * 64 + lane] - base);
    const uint32_t r0 = t.re + (uint32_t)i0, q0 = t.qe + (uint32_t)(i0 - d);
    auto flush = [&]() {
        if (b >= f.thresh) {
            if (EMIT) {
                out[at + n] = {r0 + (uint32_t)start, q0 + (uint32_t)start, (uint32_t)(bend - start), b};
                out_link[at + n] = t.link;
            }
            n++;
        }
        s = b = 0;
    };
    for (int i = i_lo; i <= i_hi; i++) {
        const int x = tr[i] & 7;
        const int j = i - d;
        if (mine && j >= 0 && j < dq) {
            const int y = qr[j] & 7;
            const int k = i - i0;
            if (x == 7 || y == 7) {
                flush();
            } else {
                if (s == 0 && b == 0) start = k;
                s += s_sub[x * 8 + y];
                if (s > b) {
                    b = s;
                    bend = k;
                }
                if (s <= 0 || b - s > f.xdrop) flush();
            }
        }
    }
    flush();  // the diagonal's end
    if (!EMIT) cnt[(size_t)w * 64 + lane] = n;
}

__global__ __launch_bounds__(256) void fill_gather_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ at, uint32_t n,
                                                          uint64_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = off[at[k]];
}

}  // namespace

void launch_fill_count(const StitchArgs& a, const FillScan& f, const FillTask* tasks, uint32_t n, uint32_t* cnt, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fill_sweep_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, s, a, f, tasks, 0u, n, cnt, nullptr, (uint64_t)0, nullptr,
                       nullptr);
}

void launch_fill_emit(const StitchArgs& a, const FillScan& f, const FillTask* tasks, uint32_t t0, uint32_t t1, const uint64_t* off,
                      uint64_t base, sa_segment_pair* out, uint32_t* out_link, hipStream_t s) {
    if (t1 <= t0) return;
    hipLaunchKernelGGL(fill_sweep_kernel<true>, dim3((t1 - t0 + 3) / 4), dim3(256), 0, s, a, f, tasks, t0, t1, nullptr, off, base, out,
                       out_link);
}

void launch_fill_gather(const uint64_t* off, const uint32_t* at, uint32_t n, uint64_t* out, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fill_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, off, at, n, out);
}

}  // namespace sa
