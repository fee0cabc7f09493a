// api_stitch.hip -- C-ABI sa_stitch_chains: every chain of HSPs as one gapped alignment through all its members (contract:
// include/segalign_amd.h).  The host side: checks, the links, the member scores and the link sweeps (stitch.hip) in batches
// by instance under option gapped_trace_mb, the walk of the unbroken links (gapped.hip's walk kernel), and the records' assembly.
#include <limits.h>

#include "engine_internal.h"
#include "gapped.h"
#include "stitch.h"

using namespace sa;

namespace {

void fail(const char* fmt, long long a = 0, long long b = 0) {
    fprintf(stderr, "Error: StitchChains: ");
    fprintf(stderr, fmt, a, b);
    fprintf(stderr, "\n");
    exit(1);
}

struct Params {
    int gap_open, gap_extend, max_link, min_link_score;
};

Params resolve(const sa_stitch_params* p) {
    Params r = {400, 30, STITCH_MAX_LINK, INT_MIN};
    if (p) {
        r.gap_open = p->gap_open;
        r.gap_extend = p->gap_extend;
        if (p->max_link) r.max_link = (int)std::min<uint32_t>(p->max_link, 1u << 30);
        r.min_link_score = p->min_link_score;
    }
    if (r.gap_open < 0 || r.gap_open > (1 << 20)) fail("gap_open = %lld out of range", r.gap_open);
    if (r.gap_extend < 0 || r.gap_extend > (1 << 20)) fail("gap_extend = %lld out of range", r.gap_extend);
    if (r.max_link > STITCH_MAX_LINK) fail("max_link = %lld out of range", r.max_link);
    long long A = 0;
    for (int x = 0; x < 7; x++)
        for (int y = 0; y < 7; y++) A = std::max(A, std::llabs((long long)g_sub_mat[x * 8 + y]));
    // every finite cell of a link stays above -(1 << 29): a cell is finite only when no separator lies before it, and then the path of one
    // D run and one I run reaches it, so its H is at least -(2 O + 2 max_link E_ext) and at most max_link A
    if (2ll * r.gap_open + 2ll * r.max_link * (r.gap_extend + A) >= (1ll << 29))
        fail("gap costs and max_link = %lld leave no int32 headroom (2 O + 2 max_link (E + A) >= 1 << 29)", r.max_link);
    return r;
}

// Device time between N events on one stream.
template <int N>
struct Timer {
    hipStream_t s;
    hipEvent_t e[N];
    explicit Timer(hipStream_t st) : s(st) {
        for (hipEvent_t& x : e) ok(hipEventCreate(&x));
    }
    ~Timer() {
        for (hipEvent_t x : e) hipEventDestroy(x);
    }
    void mark(int i) { ok(hipEventRecord(e[i], s)); }
    double ms(int i, int j) {  // once the stream has passed mark j
        float x = 0;
        ok(hipEventElapsedTime(&x, e[i], e[j]));
        return x;
    }
    static void ok(hipError_t r) {
        if (r != hipSuccess) die(15, "event", "stitch timing", r);
    }
};

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

template <typename T>
T* malloc_copy(const std::vector<T>& v) {  // nullptr for none
    if (v.empty()) return nullptr;
    T* p = (T*)malloc(v.size() * sizeof(T));
    if (!p) {
        fprintf(stderr, "Error: StitchChains: out of host memory\n");
        exit(12);
    }
    memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Link {
    uint32_t re, qe;  // the rectangle's origin: the end of the member before it
    int32_t score;
    uint32_t n_runs;  // its walk: n_runs entries of runs from run_off on, in walk order
    size_t run_off;
    uint32_t matches, mismatches;
};

// A record's runs while it grows: equal neighbours merge.
struct Runs {
    std::vector<std::pair<uint64_t, uint32_t>> r;  // (length, op)
    void add(uint64_t len, uint32_t op) {
        if (!len) return;
        if (!r.empty() && r.back().second == op) r.back().first += len;
        else r.push_back({len, op});
    }
};

constexpr uint64_t RUN_MAX = (1u << 30) - 1;  // the longest run one op entry holds

}  // namespace

extern "C" {

size_t sa_stitch_chains(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, const uint32_t* first, size_t n_chains, int rev,
                        uint32_t buffer, const sa_stitch_params* p, sa_stitch_record** records, uint32_t** ops, size_t* n_ops,
                        sa_stitch_link** links, size_t* n_links, sa_stitch_stats* stats) {
    *records = nullptr;
    *ops = nullptr;
    *n_ops = 0;
    if (links) *links = nullptr;
    if (n_links) *n_links = 0;
    sa_stitch_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_proc("StitchChains", buffer);
    const Params P = resolve(p);
    if (n_chains > (1u << 22)) fail("%lld chains: at most 1 << 22", (long long)n_chains);
    if (n_chains == 0) return 0;
    if (first[0] != 0) fail("first[0] = %lld, not 0", first[0]);
    for (size_t c = 0; c < n_chains; c++)
        if (first[c + 1] < first[c]) fail("first[] decreases at chain %lld", (long long)c);
    const size_t M = first[n_chains];
    if (M > (1u << 22)) fail("%lld members: at most 1 << 22", (long long)M);
    if (M == 0) return 0;

    Slot* sl = acquire_slot();
    hipStream_t s = sl->stream;
    const DevCtx* dc = sl->ctx;
    const SeqBuf& q = rev ? dc->query_rc[buffer] : dc->query[buffer];
    if (!dc->ref.codes || !q.codes) {
        fprintf(stderr, "Error: StitchChains needs a resident target block and query buffer %u\n", buffer);
        exit(1);
    }
    StitchArgs a;
    a.ref = dc->ref.codes;
    a.ref_len = dc->ref.len;
    a.query = q.codes;
    a.query_len = q.len;
    a.sub_mat = dc->d_sub_mat;
    a.gap_open = P.gap_open;
    a.gap_extend = P.gap_extend;

    // the members, checked, and the links in input order: link_of[k] follows member entry k
    std::vector<StitchMember> mem(M);
    for (size_t k = 0; k < M; k++) {
        if (members[k] >= n_hsps) fail("member %lld names HSP %lld, which is not in the input", (long long)k, members[k]);
        const sa_segment_pair& h = hsps[members[k]];
        if ((uint64_t)h.ref_start + h.len + 1 > a.ref_len || (uint64_t)h.query_start + h.len + 1 > a.query_len)
            fail("member %lld (HSP %lld) does not lie inside the block", (long long)k, members[k]);
        mem[k] = {h.ref_start, h.query_start, h.len, 0};
    }
    std::vector<sa_stitch_link> lk;
    std::vector<Link> li;
    std::vector<size_t> link_of(M, (size_t)-1);  // the link after member entry k
    for (size_t c = 0; c < n_chains; c++)
        for (size_t k = first[c]; k + 1 < first[c + 1]; k++) {
            const StitchMember &x = mem[k], &y = mem[k + 1];
            const uint64_t re = (uint64_t)x.rs + x.len + 1, qe = (uint64_t)x.qs + x.len + 1;
            if (re > y.rs || qe > y.qs) fail("chain %lld: the member at position %lld does not end before the next one starts", (long long)c, (long long)(k - first[c]));
            sa_stitch_link l;
            l.chain = (uint32_t)c;
            l.member = (uint32_t)(k - first[c]);
            l.dt = (uint32_t)(y.rs - re);
            l.dq = (uint32_t)(y.qs - qe);
            l.score = 0;
            l.flags = (l.dt > (uint32_t)P.max_link || l.dq > (uint32_t)P.max_link) ? SA_STITCH_LONG : 0;
            l.cells = l.flags ? 0 : ((uint64_t)l.dt + 1) * ((uint64_t)l.dq + 1);
            link_of[k] = lk.size();
            lk.push_back(l);
            li.push_back({(uint32_t)re, (uint32_t)qe, 0, 0, 0, 0, 0});
        }
    const size_t L = lk.size();

    // member scores
    std::vector<StitchMemberOut> mo(M);
    {
        StitchMember* d_mem;
        StitchMemberOut* d_mo;
        carve(sl->stitch, "stitch", [&](Carve& c) { c.take(d_mem, M).take(d_mo, M); });
        Timer<2> tm(s);
        check_memcpy(hipMemcpyAsync(d_mem, mem.data(), M * sizeof(StitchMember), hipMemcpyHostToDevice, s), "stitch members");
        tm.mark(0);
        {
            ProfScope ps(sl, "stitch_members");
            launch_stitch_members(a, d_mem, (uint32_t)M, d_mo, s);
            check_launch("stitch_members");
        }
        tm.mark(1);
        check_memcpy(hipMemcpyAsync(mo.data(), d_mo, M * sizeof(StitchMemberOut), hipMemcpyDeviceToHost, s), "stitch member scores");
        check_sync(s, "stitch_members");
        st.member_ms = tm.ms(0, 1);
    }

    // the links to sweep, binned by instance: the smallest K with 64 K >= dt + 1
    static const int KS[5] = {2, 4, 8, 17, 33};
    std::vector<size_t> bin[5];
    for (size_t k = 0; k < L; k++) {
        sa_stitch_link& l = lk[k];
        if (l.flags) continue;
        st.swept++;
        st.cells += l.cells;
        if (l.dt + l.dq == 0) continue;  // score 0 and no op
        int b = 0;
        while (64 * KS[b] < (int)l.dt + 1) b++;
        bin[b].push_back(k);
    }
    std::vector<uint32_t> runs;  // the walks' runs, in walk order
    const size_t budget = (size_t)g_gapped_trace_mb << 20;
    Timer<3> tm(s);
    std::vector<TraceTask> bt, wt;
    std::vector<size_t> widx;
    std::vector<int32_t> sc;
    std::vector<TraceOut> wo;
    std::vector<uint32_t> bops;
    for (int b = 0; b < 5; b++) {
        const int max_band = 64 * KS[b] - 1;
        const std::vector<size_t>& ids = bin[b];
        for (size_t at = 0; at < ids.size();) {
            // the batch: links ids[at .. e), their trace areas within the budget (a larger link alone)
            size_t e = at, trace = 0, nops = 0;
            bt.clear();
            while (e < ids.size()) {
                const sa_stitch_link& l = lk[ids[e]];
                const int dstar = (int)(l.dt + l.dq);
                const size_t tb = gapped_trace_bytes(max_band, dstar);
                if (e > at && trace + tb > budget) break;
                bt.push_back({li[ids[e]].re, li[ids[e]].qe, 1, dstar, (int32_t)l.dt, (int32_t)l.dq, trace, nops});
                trace += tb;
                nops += (size_t)dstar;
                e++;
            }
            const size_t m = e - at;
            TraceTask *d_tasks, *d_walk;
            TraceOut* d_out;
            int32_t* d_score;
            uint32_t* d_ops;
            uint8_t* d_area;
            carve(sl->stitch, "stitch",
                  [&](Carve& c) { c.take(d_tasks, m).take(d_walk, m).take(d_out, m).take(d_score, m).take(d_ops, nops).take(d_area, trace); });
            check_memcpy(hipMemcpyAsync(d_tasks, bt.data(), m * sizeof(TraceTask), hipMemcpyHostToDevice, s), "stitch tasks");
            tm.mark(0);
            {
                ProfScope ps(sl, "stitch_sweep");
                launch_stitch_sweep(a, max_band, d_tasks, (uint32_t)m, d_area, d_score, s);
                check_launch("stitch_sweep");
            }
            tm.mark(1);
            sc.resize(m);
            check_memcpy(hipMemcpyAsync(sc.data(), d_score, m * sizeof(int32_t), hipMemcpyDeviceToHost, s), "stitch scores");
            check_sync(s, "stitch_sweep");
            st.sweep_ms += tm.ms(0, 1);
            st.trace_bytes += trace;
            st.batches++;
            // the links to walk: neither dead nor low
            wt.clear();
            widx.clear();
            for (size_t k = 0; k < m; k++) {
                sa_stitch_link& l = lk[ids[at + k]];
                if (sc[k] <= STITCH_NEG / 2) {
                    l.flags = SA_STITCH_DEAD;
                    l.score = INT_MIN;
                    continue;
                }
                l.score = li[ids[at + k]].score = sc[k];
                if (sc[k] < P.min_link_score) {
                    l.flags = SA_STITCH_LOW;
                    continue;
                }
                wt.push_back(bt[k]);
                widx.push_back(ids[at + k]);
            }
            const size_t w = wt.size();
            if (w) {
                GappedArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.ref = a.ref;
                ga.ref_len = a.ref_len;
                ga.query = a.query;
                ga.query_len = a.query_len;
                ga.sub_mat = a.sub_mat;
                ga.gap_open = a.gap_open;
                ga.gap_extend = a.gap_extend;
                ga.max_band = max_band;
                check_memcpy(hipMemcpyAsync(d_walk, wt.data(), w * sizeof(TraceTask), hipMemcpyHostToDevice, s), "stitch walk tasks");
                tm.mark(1);
                {
                    ProfScope ps(sl, "stitch_walk");
                    launch_gapped_walk(ga, d_walk, (uint32_t)w, d_area, d_ops, d_out, s);
                    check_launch("stitch_walk");
                }
                tm.mark(2);
                wo.resize(w);
                bops.resize(nops);
                check_memcpy(hipMemcpyAsync(wo.data(), d_out, w * sizeof(TraceOut), hipMemcpyDeviceToHost, s), "stitch walk results");
                check_memcpy(hipMemcpyAsync(bops.data(), d_ops, nops * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "stitch ops");
                check_sync(s, "stitch_walk");
                st.walk_ms += tm.ms(1, 2);
                for (size_t k = 0; k < w; k++) {
                    const TraceOut& r = wo[k];
                    if (r.err || r.n_runs > (uint32_t)wt[k].dstar) {
                        fprintf(stderr, "Error: StitchChains: the path walk left the traced cells (link %zu, code %u)\n", widx[k], r.err);
                        exit(1);
                    }
                    Link& x = li[widx[k]];
                    x.n_runs = r.n_runs;
                    x.run_off = runs.size();
                    x.matches = r.matches;
                    x.mismatches = r.mismatches;
                    runs.insert(runs.end(), bops.begin() + wt[k].ops_off, bops.begin() + wt[k].ops_off + r.n_runs);
                }
            }
            at = e;
        }
    }
    prof_flush(sl);
    release_slot(sl);

    // the records: a chain's members and unbroken links in genome order, cut at the broken links
    std::vector<sa_stitch_record> rec;
    std::vector<uint32_t> out_ops;
    for (size_t c = 0; c < n_chains; c++) {
        for (size_t k = first[c]; k < first[c + 1];) {
            sa_stitch_record r;
            memset(&r, 0, sizeof(r));
            r.chain = (uint32_t)c;
            r.first_member = (uint32_t)(k - first[c]);
            r.ref_start = mem[k].rs;
            r.query_start = mem[k].qs;
            r.op_offset = out_ops.size();
            Runs R;
            uint64_t matches = 0, mismatches = 0;
            for (;; k++) {
                R.add((uint64_t)mem[k].len + 1, SA_GAPPED_OP_M);
                r.score += mo[k].score;
                matches += mo[k].matches;
                mismatches += mo[k].mismatches;
                r.n_members++;
                r.ref_end = mem[k].rs + mem[k].len + 1;
                r.query_end = mem[k].qs + mem[k].len + 1;
                if (k + 1 == first[c + 1]) break;
                const sa_stitch_link& l = lk[link_of[k]];
                if (l.flags) {
                    r.flags = l.flags;
                    break;
                }
                const Link& x = li[link_of[k]];
                r.score += x.score;
                matches += x.matches;
                mismatches += x.mismatches;
                for (uint32_t y = x.n_runs; y-- > 0;) {  // the walk runs from (dt, dq) back: reversed is genome order
                    const uint32_t o = runs[x.run_off + y];
                    R.add(o >> 2, o & 3u);
                }
            }
            k++;
            for (const auto& run : R.r) {
                if (run.second != SA_GAPPED_OP_M) {
                    r.gap_opens++;
                    r.gap_bases += (uint32_t)run.first;
                }
                for (uint64_t left = run.first; left;) {
                    const uint64_t piece = std::min(left, RUN_MAX);
                    out_ops.push_back((uint32_t)piece << 2 | run.second);
                    left -= piece;
                }
            }
            r.n_ops = (uint32_t)(out_ops.size() - r.op_offset);
            r.matches = (uint32_t)matches;
            r.mismatches = (uint32_t)mismatches;
            rec.push_back(r);
        }
    }
    st.links = L;
    for (const sa_stitch_link& l : lk) {
        if (l.flags & SA_STITCH_LONG) st.long_links++;
        if (l.flags & SA_STITCH_DEAD) st.dead_links++;
        if (l.flags & SA_STITCH_LOW) st.low_links++;
    }
    st.records = rec.size();
    if (stats) *stats = st;
    *records = malloc_copy(rec);
    *ops = malloc_copy(out_ops);
    *n_ops = out_ops.size();
    if (links) *links = malloc_copy(lk);
    if (n_links) *n_links = L;
    return rec.size();
}

void sa_free_stitch(sa_stitch_record* records, uint32_t* ops, sa_stitch_link* links) {
    free(records);
    free(ops);
    free(links);
}

}  // extern "C"
