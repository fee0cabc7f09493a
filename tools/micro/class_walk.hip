// class_walk.hip -- round-5 verdict item 1(a): what does the class filter's WALK cost a CU when its LDS table is laid out so that a lane
// can never meet another lane on its bank, against today's 4096-entry table -- in LDS cycles AND in the kernel's own time?
//
// The class filter (segalign_amd/csrc/extend.hip 1d) walks 112 context bases per hit as 18 six-base fields + a four-base tail: 19
// ds_read_b32 with random addresses into a 16 KB + 1 KB table, 2-3 VALU per field for the walk state {T : N} and W, 1-2 for the address.
// 64 random dword reads of a wave conflict in the 32 banks a ds_read_b32 sees: SQ_LDS_BANK_CONFLICT is 68-70 % of the LDS cycles of the
// filter (profiles/r05/pmc6.txt, join_pmc*.txt), tools/micro/lds_rate: 6.1-6.5 cycles per random wave-instruction per CU against 2.95
// conflict-free.  A conflict-free layout needs every lane of a 32-lane group on its own bank, i.e. the table replicated once per bank:
//   A  today:        4096 entries (6 bases) + 256-entry tail, one copy              17 KB   19 lookups per hit
//   B  per bank:     256 entries (4 bases) x 32 copies, lane l reads copy l & 31    32 KB   28 lookups per hit   conflict-free by construction
//   C  per 4 banks:  1024 entries (5 bases) x 8 copies, copy r on banks 4r .. 4r+3  32 KB   23 lookups per hit   4 lanes share 4 banks
// Every variant runs twice: LDS ONLY (the reads and one xor each: the LDS cycles per 64 hits) and as the WALK (address extraction from
// the seven class-string dwords, cls_step with W as in the filter, the verdict's few ops) -- no global memory in either, so what is
// measured is the CU's LDS + VALU issue, the two units the key-ordered filter was bound by.
// Class strings come from a per-lane additive generator (7 VALU per hit, the same in every variant).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o class_walk class_walk.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

__device__ __forceinline__ void cls_step(const uint32_t* s_tab, uint32_t addr, uint32_t& P, uint32_t& W) {
    const uint32_t e = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(s_tab) + addr);
    asm("v_pk_add_i16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(P) : "v"(P), "v"(e));
    asm("v_min_i16_sdwa %0, %0, %1 dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:WORD_0 src1_sel:WORD_0" : "+v"(P) : "v"(e));
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    W = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(s16x2, W), __builtin_bit_cast(s16x2, P)));
}
__device__ __forceinline__ void lds_only(const uint32_t* s_tab, uint32_t addr, uint32_t& acc) {
    acc ^= *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(s_tab) + addr);
}

// field of NB bases (2 NB bits) starting at bit O of the 224-bit string x[0..6]
template <int O, int NB>
__device__ __forceinline__ uint32_t field(const uint32_t (&x)[8]) {
    constexpr int d = O >> 5, o = O & 31, bits = 2 * NB;
    constexpr uint32_t mask = (1u << bits) - 1u;
    if (o + bits <= 32) return (x[d] >> o) & mask;  // v_bfe_u32
    return __builtin_amdgcn_alignbit(x[d + 1], x[d], (uint32_t)o) & mask;
}

enum { TAB_A = 0, TAB_B = 1, TAB_C = 2 };

template <int TAB, bool WALK>
__global__ __launch_bounds__(1024, 8) void k(uint32_t* out, int iters, int xdrop) {
    extern __shared__ uint32_t s_tab[];
    constexpr uint32_t TAB_DW = TAB == TAB_A ? 4096 + 256 : 8192;
    // entries {sum : sum - mx} of the class scores 100 / -114 / -31 / -123 (HOXD70's class maxima), as in cls_table_init
    for (uint32_t i = threadIdx.x; i < TAB_DW; i += blockDim.x) {
        uint32_t f, nb;
        if (TAB == TAB_A) { nb = i < 4096 ? 6 : 4; f = i < 4096 ? i : i - 4096; }
        else if (TAB == TAB_B) { nb = 4; f = i >> 5; }                          // dword = field * 32 + copy
        else { nb = 5; f = ((i >> 5) << 2) | (i & 3); }                         // dword = (field >> 2) * 32 + copy * 4 + (field & 3)
        int sum = 0, mx = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const int c = (f >> (2 * b)) & 3;
            sum += c == 0 ? 100 : c == 1 ? -114 : c == 2 ? -31 : -123;
            mx = sum > mx ? sum : mx;
        }
        s_tab[i] = ((uint32_t)sum << 16) | ((uint32_t)(sum - mx) & 0xFFFFu);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t laneB = (lane & 31u) << 2;  // B: the lane's own bank
    const uint32_t laneC = (lane & 7u) << 4;   // C: the lane's group of four banks
    uint32_t x[8], inc[8];
    uint32_t r = (threadIdx.x + blockIdx.x * blockDim.x) * 747796405u + 12345u;
    for (int j = 0; j < 8; j++) {
        r = r * 1664525u + 1013904223u;
        x[j] = r;
        r = r * 1664525u + 1013904223u;
        inc[j] = r | 1u;
    }
    x[7] = 0;
    uint32_t acc = 0, fwd = 0;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < 7; j++) x[j] += inc[j];
        uint32_t PR = 0, WR = 0, PL = 1900u << 16, WL = 0;
        if (TAB == TAB_A) {
#define STEP_A(O, P_, W_)                                                              \
    {                                                                                  \
        const uint32_t a_ = field<O, 6>(x) << 2;                                       \
        if (WALK) cls_step(s_tab, a_, P_, W_); else lds_only(s_tab, a_, acc);          \
    }
            STEP_A(0, PR, WR) STEP_A(12, PR, WR) STEP_A(24, PR, WR) STEP_A(36, PR, WR) STEP_A(48, PR, WR) STEP_A(60, PR, WR) STEP_A(72, PR, WR)
            STEP_A(84, PR, WR) STEP_A(96, PR, WR)
            STEP_A(108, PL, WL) STEP_A(120, PL, WL) STEP_A(132, PL, WL) STEP_A(144, PL, WL) STEP_A(156, PL, WL) STEP_A(168, PL, WL)
            STEP_A(180, PL, WL) STEP_A(192, PL, WL) STEP_A(204, PL, WL)
            {
                const uint32_t a_ = 16384u + ((x[6] >> 22) & 0x3FCu);
                if (WALK) cls_step(s_tab, a_, PL, WL); else lds_only(s_tab, a_, acc);
            }
        } else if (TAB == TAB_B) {
#define STEP_B(O, P_, W_)                                                              \
    {                                                                                  \
        const uint32_t a_ = (field<O, 4>(x) << 7) | laneB;                             \
        if (WALK) cls_step(s_tab, a_, P_, W_); else lds_only(s_tab, a_, acc);          \
    }
            STEP_B(0, PR, WR) STEP_B(8, PR, WR) STEP_B(16, PR, WR) STEP_B(24, PR, WR) STEP_B(32, PR, WR) STEP_B(40, PR, WR) STEP_B(48, PR, WR)
            STEP_B(56, PR, WR) STEP_B(64, PR, WR) STEP_B(72, PR, WR) STEP_B(80, PR, WR) STEP_B(88, PR, WR) STEP_B(96, PR, WR) STEP_B(104, PR, WR)
            STEP_B(112, PL, WL) STEP_B(120, PL, WL) STEP_B(128, PL, WL) STEP_B(136, PL, WL) STEP_B(144, PL, WL) STEP_B(152, PL, WL)
            STEP_B(160, PL, WL) STEP_B(168, PL, WL) STEP_B(176, PL, WL) STEP_B(184, PL, WL) STEP_B(192, PL, WL) STEP_B(200, PL, WL)
            STEP_B(208, PL, WL) STEP_B(216, PL, WL)
        } else {
#define STEP_C(O, P_, W_)                                                              \
    {                                                                                  \
        const uint32_t f_ = field<O, 5>(x);                                            \
        const uint32_t a_ = ((f_ >> 2) << 7) | laneC | ((f_ & 3u) << 2);               \
        if (WALK) cls_step(s_tab, a_, P_, W_); else lds_only(s_tab, a_, acc);          \
    }
            STEP_C(0, PR, WR) STEP_C(10, PR, WR) STEP_C(20, PR, WR) STEP_C(30, PR, WR) STEP_C(40, PR, WR) STEP_C(50, PR, WR) STEP_C(60, PR, WR)
            STEP_C(70, PR, WR) STEP_C(80, PR, WR) STEP_C(90, PR, WR) STEP_C(100, PR, WR)
            STEP_C(110, PL, WL) STEP_C(120, PL, WL) STEP_C(130, PL, WL) STEP_C(140, PL, WL) STEP_C(150, PL, WL) STEP_C(160, PL, WL)
            STEP_C(170, PL, WL) STEP_C(180, PL, WL) STEP_C(190, PL, WL) STEP_C(200, PL, WL) STEP_C(210, PL, WL) STEP_C(214, PL, WL)
        }
        if (WALK) {  // the verdict, as in the filter: alive sides, best = T - N, the bound against the threshold, a ballot
            const bool r_alive = (int)(short)(WR & 0xFFFFu) >= -xdrop, l_alive = (int)(short)(WL & 0xFFFFu) >= -xdrop;
            const int bestR = ((int)PR >> 16) - (int)(short)(PR & 0xFFFFu), bestL = ((int)PL >> 16) - (int)(short)(PL & 0xFFFFu);
            const bool f = r_alive || l_alive || bestR + bestL >= 3000;
            fwd += (uint32_t)__popcll(__ballot(f));
        }
    }
    if ((acc ^ fwd) == 0x12345678u) out[0] = acc;
    if (WALK && threadIdx.x == 0 && blockIdx.x == 0) out[1] = fwd;
}

template <int TAB, bool WALK>
static double run(const char* name, uint32_t* out, int lookups) {
    const int iters = 4096, threads = 1024, blocks = 256 * 2;
    const uint32_t lds = (TAB == TAB_A ? 4096 + 256 : 8192) * 4;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipLaunchKernelGGL((k<TAB, WALK>), dim3(blocks), dim3(threads), lds, 0, out, 16, 910);
    hipDeviceSynchronize();
    float best = 1e30f;
    for (int rep = 0; rep < 3; rep++) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((k<TAB, WALK>), dim3(blocks), dim3(threads), lds, 0, out, iters, 910);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        best = ms < best ? ms : best;
    }
    const double steps_per_cu = 2.0 * (threads / 64) * iters;  // 64-hit steps per CU
    const double cyc = best * 1e-3 * 2.4e9 / steps_per_cu;
    const double ghits = (double)blocks * threads * iters / (best * 1e-3) / 1e9;
    uint32_t h[2] = {0, 0};
    hipMemcpy(h, out, 8, hipMemcpyDeviceToHost);
    printf("%-54s %2d lookups  %8.3f ms  %7.1f cycles per 64 hits per CU (2.4 GHz)  %6.2f cycles per lookup  %6.1f G hits/s chip-wide%s\n", name, lookups, best, cyc,
           cyc / lookups, ghits, WALK ? "" : "  [LDS only]");
    return cyc;
}

int main() {
    uint32_t* out;
    hipMalloc(&out, 8);
    hipMemset(out, 0, 8);
    const double la = run<TAB_A, false>("A today: 4096 x 6 bases + tail, one copy (17 KB)", out, 19);
    const double lb = run<TAB_B, false>("B per bank: 256 x 4 bases x 32 copies (32 KB)", out, 28);
    const double lc = run<TAB_C, false>("C per 4 banks: 1024 x 5 bases x 8 copies (32 KB)", out, 23);
    const double wa = run<TAB_A, true>("A today: 4096 x 6 bases + tail, one copy (17 KB)", out, 19);
    const double wb = run<TAB_B, true>("B per bank: 256 x 4 bases x 32 copies (32 KB)", out, 28);
    const double wc = run<TAB_C, true>("C per 4 banks: 1024 x 5 bases x 8 copies (32 KB)", out, 23);
    printf("LDS cycles per 64 hits, A / B = %.2f x, A / C = %.2f x;  the walk (LDS + VALU), A / B = %.2f x, A / C = %.2f x\n", la / lb, la / lc, wa / wb, wa / wc);
    return 0;
}
