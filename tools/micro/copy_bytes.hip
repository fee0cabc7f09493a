// copy_bytes.hip -- the time a plain device-to-device copy of N bytes takes on one stream, for DESIGN.md 21: what sa_net_subset's
// output (out_hsps and the sub-chain records) would cost to move once, beside the subset_ms that makes it.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/copy_bytes.hip -o tools/micro/copy_bytes && tools/micro/copy_bytes BYTES [REPEATS]
// Prints the least and the median time over REPEATS (default 50) copies after 5 warm-up copies, in microseconds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                       \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: copy_bytes BYTES [REPEATS]\n");
        return 2;
    }
    const size_t bytes = strtoull(argv[1], nullptr, 10);
    const int repeats = argc > 2 ? atoi(argv[2]) : 50;
    if (bytes == 0 || bytes > ((size_t)1 << 32) || repeats < 1 || repeats > 10000) {
        fprintf(stderr, "copy_bytes: BYTES in 1 .. 2^32, REPEATS in 1 .. 10000\n");
        return 2;
    }
    void *src = nullptr, *dst = nullptr;
    hipStream_t s;
    hipEvent_t a, b;
    CHECK(hipMalloc(&src, bytes));
    CHECK(hipMalloc(&dst, bytes));
    CHECK(hipMemset(src, 1, bytes));
    CHECK(hipStreamCreate(&s));
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    std::vector<float> us;
    for (int k = 0; k < repeats + 5; k++) {
        CHECK(hipEventRecord(a, s));
        CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
        CHECK(hipEventRecord(b, s));
        CHECK(hipStreamSynchronize(s));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (k >= 5) us.push_back(ms * 1000.f);
    }
    std::sort(us.begin(), us.end());
    printf("{\"bytes\": %zu, \"repeats\": %d, \"copy_min_us\": %.2f, \"copy_median_us\": %.2f}\n", bytes, repeats, us.front(), us[us.size() / 2]);
    CHECK(hipFree(src));
    CHECK(hipFree(dst));
    return 0;
}
