// post_host.h -- the host helpers that the ten post-processing units share (api_gapped.hip, api_hspchain.hip, api_stitch.hip,
// api_chaintrim.hip, api_fill.hip, api_net.hip, api_netsubset.hip, api_netclass.hip, api_lift.hip, api_diff.hip): device time between
// events, profiled and checked launches, carving a slot buffer, the checked copies to and from the device, malloc-ed arrays for the
// caller, the resident block as kernel arguments, the checked gap-cost table as its device image, and the trace batches' packing and
// runs; and through post_checks.h the input rules they share.  Host code only, everything inline or a template.
#pragma once
#include "engine_internal.h"
#include "gapped.h"
#include "hspcost.h"
#include "post_checks.h"

namespace sa {

// Device time between N events on one stream: ms(i, j) once the stream has passed mark j (where the caller synchronises, or wait()).
// tag names the entry in the error messages ("gapped timing", ...).
template <int N>
struct Timer {
    hipStream_t s;
    const char* tag;
    hipEvent_t e[N];
    Timer(hipStream_t st, const char* t) : s(st), tag(t) {
        for (hipEvent_t& x : e) ok(hipEventCreate(&x), "hipEventCreate");
    }
    Timer(const Timer&) = delete;
    ~Timer() {
        for (hipEvent_t x : e) hipEventDestroy(x);
    }
    void mark(int i) { ok(hipEventRecord(e[i], s), "hipEventRecord"); }
    double ms(int i, int j) {
        float x = 0;
        ok(hipEventElapsedTime(&x, e[i], e[j]), "hipEventElapsedTime");
        return x;
    }
    double wait(int i, int j) {
        ok(hipEventSynchronize(e[j]), "hipEventSynchronize");
        return ms(i, j);
    }
    void ok(hipError_t r, const char* what) {
        if (r != hipSuccess) die(15, what, tag, r);
    }
};

// Launches profiled as one scope and checked, both under name.
template <typename F>
void launch(Slot* sl, const char* name, F&& launches) {
    ProfScope ps(sl, name);
    launches();
    check_launch(name);
}

// 256-byte-aligned sub-buffers of buf: layout(c) calls c.take(pointer, count) in order, once to size buf and once to set the pointers.
struct Carve {
    uint8_t* base;
    size_t end = 0;
    template <typename T>
    Carve& take(T*& p, size_t n) {
        const size_t at = (end + 255) & ~(size_t)255;
        end = at + n * sizeof(T);
        p = base ? (T*)(base + at) : nullptr;
        return *this;
    }
};
template <typename F>
void carve(DevBuf<uint8_t>& buf, const char* tag, F&& layout) {
    Carve size{nullptr};
    layout(size);
    buf.ensure(size.end, tag);
    Carve c{buf.p};
    layout(c);
}

// Arrays the caller frees (sa_free_*): nullptr for none, and no return when the host is out of memory.
template <typename T>
T* host_alloc(size_t count, const char* who) {
    if (!count) return nullptr;
    T* p = (T*)malloc(count * sizeof(T));
    if (!p) {
        fprintf(stderr, "Error: %s: out of host memory\n", who);
        exit(12);
    }
    return p;
}
template <typename T>
T* malloc_copy(const std::vector<T>& v, const char* who) {
    T* p = host_alloc<T>(v.size(), who);
    if (p) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// Checked copies on a stream, typed and counted in elements; nothing is enqueued for n == 0.  tag: the copy's name in the exit-13 message.
template <typename T>
void to_device(T* dst, const T* src, size_t n, hipStream_t s, const char* tag) {
    if (n) check_memcpy(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, s), tag);
}
template <typename T>
void to_host(T* dst, const T* src, size_t n, hipStream_t s, const char* tag) {
    if (n) check_memcpy(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s), tag);
}
// An optional input array as the kernels take it: nullptr for none, else its n elements copied to dst, and dst.
template <typename T>
T* upload(T* dst, const T* src, size_t n, hipStream_t s, const char* tag) {
    if (!src) return nullptr;
    to_device(dst, src, n, s, tag);
    return dst;
}
// One total read back, with the synchronise that makes it valid.  Two totals of one step take two to_host and one check_sync instead.
inline uint64_t read_u64(const uint64_t* at, hipStream_t s, const char* tag) {
    uint64_t x = 0;
    to_host(&x, at, 1, s, tag);
    check_sync(s, tag);
    return x;
}

// The resident target block and the query strand (rev, buffer) of the slot's device into the fields that GappedArgs and StitchArgs
// begin with; who's error when either is missing.
template <typename Args>
void resident_block(const char* who, const Slot* sl, int rev, uint32_t buffer, Args& a) {
    const DevCtx* dc = sl->ctx;
    const SeqBuf& q = rev ? dc->query_rc[buffer] : dc->query[buffer];
    if (!dc->ref.codes || !q.codes) {
        fprintf(stderr, "Error: %s needs a resident target block and query buffer %u\n", who, buffer);
        exit(1);
    }
    a.ref = dc->ref.codes;
    a.ref_len = dc->ref.len;
    a.query = q.codes;
    a.query_len = q.len;
    a.sub_mat = dc->d_sub_mat;
}

// A gap-cost table as the kernels of hspchain.hip and netsubset.hip read it (layout: hspcost.h), or none.
struct CostImage {
    bool on = false;
    uint32_t w[HSPCOST_WORDS];
};

inline void bad_costs(const char* who, const char* what, unsigned k, long long v) {
    fprintf(stderr, "Error: %s: gap costs: %s[%u] = %lld out of range\n", who, what, k, v);
    exit(1);
}

// Checks a table (contract: include/segalign_amd.h, sa_chain_hsps_costs), derives the slopes and folds the three cost arrays into the
// image; who's error for a table that breaks the rules.
inline void checked_costs(const char* who, const sa_chain_gap_costs* g, CostImage& im) {
    im.on = g != nullptr;
    if (!g) return;
    const uint32_t n = g->n;
    if (n < 1 || n > SA_CHAIN_GAP_POINTS) {
        fprintf(stderr, "Error: %s: gap costs: n = %lld out of range\n", who, (long long)n);
        exit(1);
    }
    for (uint32_t k = 0; k < n; k++)
        if (k == 0 ? g->pos[0] < 1 : g->pos[k] <= g->pos[k - 1]) bad_costs(who, "pos", k, g->pos[k]);
    const int64_t* cost[3] = {g->q_gap, g->t_gap, g->both_gap};
    const char* name[3] = {"q_gap", "t_gap", "both_gap"};
    const char* slope_name[3] = {"slope of q_gap", "slope of t_gap", "slope of both_gap"};
    for (uint32_t k = 0; k < HSPCOST_POINTS; k++) im.w[k] = g->pos[std::min(k, n - 1)];
    for (int a = 0; a < 3; a++) {
        const int64_t* c = cost[a];
        uint32_t slope[SA_CHAIN_GAP_POINTS];
        for (uint32_t k = 0; k < n; k++)
            if (c[k] < 0 || c[k] > ((int64_t)1 << 40) || (k > 0 && c[k] < c[k - 1])) bad_costs(who, name[a], k, c[k]);
        for (uint32_t k = 0; k + 1 < n; k++) {
            const int64_t sl = ((c[k + 1] - c[k]) << 16) / (int64_t)(g->pos[k + 1] - g->pos[k]);  // operands >= 0: the quotient is the floor
            if (sl >= (int64_t)HSPCOST_SLOPE_LIMIT) bad_costs(who, slope_name[a], k, sl);
            slope[k] = (uint32_t)sl;
        }
        slope[n - 1] = n > 1 ? slope[n - 2] : 0;
        for (uint32_t k = 0; k < HSPCOST_POINTS; k++) {
            const uint32_t r = std::min(k, n - 1);
            uint32_t* row = im.w + HSPCOST_ROW0 + 4 * ((uint32_t)a * HSPCOST_POINTS + k);
            row[0] = (uint32_t)c[r];
            row[1] = (uint32_t)((uint64_t)c[r] >> 32);
            row[2] = slope[r];
            row[3] = g->pos[r];
        }
    }
}

// One batch of trace tasks: their trace areas (trace bytes in all) and op areas (nops entries) laid out behind each other.
struct TraceBatch {
    std::vector<TraceTask> tasks;  // trace_off and ops_off set
    size_t trace = 0, nops = 0;
    // The batch from all[b] on: tasks [b, e) with their trace areas within option gapped_trace_mb (a larger one alone).  Returns e.
    size_t pack(const std::vector<TraceTask>& all, size_t b, int max_band) {
        const size_t budget = (size_t)g_gapped_trace_mb << 20;
        size_t e = b;
        trace = nops = 0;
        tasks.clear();
        while (e < all.size()) {
            const size_t tb = gapped_trace_bytes(max_band, all[e].dstar);
            if (e > b && trace + tb > budget) break;
            TraceTask t = all[e];
            t.trace_off = trace;
            t.ops_off = nops;
            tasks.push_back(t);
            trace += tb;
            nops += (size_t)t.dstar;
            e++;
        }
        return e;
    }
};

// The runs the walk wrote for task t of a batch, in walk order, appended to runs from off on; ops: the batch's op areas on the host.
// False when the walk left the traced cells: the caller's error.
inline bool take_runs(const TraceTask& t, const TraceOut& r, const std::vector<uint32_t>& ops, std::vector<uint32_t>& runs, size_t& off) {
    if (r.err || r.n_runs > (uint32_t)t.dstar) return false;
    off = runs.size();
    runs.insert(runs.end(), ops.begin() + t.ops_off, ops.begin() + t.ops_off + r.n_runs);
    return true;
}

}  // namespace sa
