// api_gapped.hip -- C-ABI sa_gapped_extend: gapped y-drop extension of HSP anchors (contract: include/segalign_amd.h),
// and sa_gapped_align: the same records plus their alignment paths.
// The host side: parameter defaults and limits, batches of anchors through the slot's stream (gapped.hip), the selection rules, and
// for the paths the batches of traced sides sized from pass 1's best antidiagonals.
#include <functional>

#include "engine_internal.h"
#include "gapped.h"

using namespace sa;

namespace {

constexpr size_t GAPPED_BATCH = 8192;  // HSPs per launch: 16384 waves, each bounded by ~2 max_extent antidiagonals

struct Params {
    int gap_open, gap_extend, ydrop, gappedthresh, max_extent, max_band;
};

Params resolve(const sa_gapped_params* p) {
    Params r = {400, 30, 9430, g_hspthresh, 65536, 1024};
    if (p) {
        r.gap_open = p->gap_open;
        r.gap_extend = p->gap_extend;
        r.ydrop = p->ydrop;
        r.gappedthresh = p->gappedthresh;
        if (p->max_extent) r.max_extent = (int)std::min<uint32_t>(p->max_extent, 1u << 30);
        if (p->max_band) r.max_band = (int)std::min<uint32_t>(p->max_band, 1u << 30);
    }
    auto bad = [](const char* what, long long v) {
        fprintf(stderr, "Error: GappedExtend: %s = %lld out of range\n", what, v);
        exit(1);
    };
    // limits that keep every finite value of the kernels' int32 arithmetic above NEG / 2 and the per-record cell count in 32 bits
    if (r.gap_open < 0 || r.gap_open > (1 << 20)) bad("gap_open", r.gap_open);
    if (r.gap_extend < 0 || r.gap_extend > (1 << 20)) bad("gap_extend", r.gap_extend);
    if (r.ydrop < 0 || r.ydrop > (1 << 28)) bad("ydrop", r.ydrop);
    if (r.max_extent > (1 << 18)) bad("max_extent", r.max_extent);
    if (r.max_band > 2048 || gapped_cells_per_lane(r.max_band) < 0) bad("max_band", r.max_band);
    return r;
}

// Pass 1 on an acquired slot: every HSP's two sides into side[2 k], side[2 k + 1]; kernel time into st.
void extend_sides(Slot* sl, const SeqBuf& q, const sa_segment_pair* hsps, size_t n, const Params& P, std::vector<GappedSide>& side,
                  sa_gapped_stats& st) {
    DevCtx* dc = sl->ctx;
    const size_t batch = std::min(n, GAPPED_BATCH);
    const size_t hsp_bytes = (batch * sizeof(sa_segment_pair) + 255) & ~(size_t)255;
    sl->gapped.ensure(hsp_bytes + 2 * batch * sizeof(GappedSide), "gapped");
    sa_segment_pair* d_hsps = (sa_segment_pair*)sl->gapped.p;
    GappedSide* d_side = (GappedSide*)(sl->gapped.p + hsp_bytes);
    side.resize(2 * n);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (size_t b = 0; b < n; b += batch) {
        const size_t m = std::min(batch, n - b);
        check_memcpy(hipMemcpyAsync(d_hsps, hsps + b, m * sizeof(sa_segment_pair), hipMemcpyHostToDevice, sl->stream), "gapped hsps");
        GappedArgs a;
        a.ref = dc->ref.codes;
        a.ref_len = dc->ref.len;
        a.query = q.codes;
        a.query_len = q.len;
        a.sub_mat = dc->d_sub_mat;
        a.hsps = d_hsps;
        a.num_tasks = (uint32_t)(2 * m);
        a.gap_open = P.gap_open;
        a.gap_extend = P.gap_extend;
        a.ydrop = P.ydrop;
        a.max_extent = P.max_extent;
        a.max_band = P.max_band;
        a.out = d_side;
        hipEventRecord(e0, sl->stream);
        {
            ProfScope ps(sl, "gapped_extend");
            launch_gapped(a, sl->stream);
            check_launch("gapped_extend");
        }
        hipEventRecord(e1, sl->stream);
        check_memcpy(hipMemcpyAsync(side.data() + 2 * b, d_side, 2 * m * sizeof(GappedSide), hipMemcpyDeviceToHost, sl->stream), "gapped results");
        check_sync(sl->stream, "gapped_extend");
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        st.kernel_ms += ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
}

// Selection rule (3): the output order of records.
bool output_order(const sa_gapped_alignment& x, const sa_gapped_alignment& y) {
    if (x.query_start != y.query_start) return x.query_start < y.query_start;
    if (x.ref_start != y.ref_start) return x.ref_start < y.ref_start;
    if (x.query_end != y.query_end) return x.query_end < y.query_end;
    if (x.ref_end != y.ref_end) return x.ref_end < y.ref_end;
    if (x.score != y.score) return x.score > y.score;
    return x.hsp_index < y.hsp_index;
}

// Records from the sides: raw (one per HSP, input order) or the selection rules.
void make_records(const sa_segment_pair* hsps, size_t n, const std::vector<GappedSide>& side, const Params& P, int raw,
                  std::vector<sa_gapped_alignment>& rec, sa_gapped_stats& st) {
    rec.resize(n);
    for (size_t k = 0; k < n; k++) {
        const GappedSide& L = side[2 * k];
        const GappedSide& R = side[2 * k + 1];
        const uint32_t ar = hsps[k].ref_start + hsps[k].len / 2, aq = hsps[k].query_start + hsps[k].len / 2;
        sa_gapped_alignment& o = rec[k];
        o.ref_start = ar - (uint32_t)L.best_i;
        o.ref_end = ar + (uint32_t)R.best_i;
        o.query_start = aq - (uint32_t)L.best_j;
        o.query_end = aq + (uint32_t)R.best_j;
        o.score = L.best + R.best;
        o.hsp_index = (uint32_t)k;
        o.flags = L.flags | R.flags;
        o.cells = L.cells + R.cells;
        st.cells += o.cells;
        if (o.flags & SA_GAPPED_EXTENT_CAP) st.extent_capped++;
        if (o.flags & SA_GAPPED_BAND_CAP) st.band_capped++;
    }
    st.anchors = n;
    if (!raw) {
        // (1) threshold, (2) one record per extent: the highest score, then the lowest index, (3) the output order
        std::vector<sa_gapped_alignment> keep;
        keep.reserve(n);
        for (const sa_gapped_alignment& r : rec)
            if (r.score >= P.gappedthresh) keep.push_back(r);
        std::sort(keep.begin(), keep.end(), output_order);
        // the sort key begins with the extent, and within one extent the record to keep sorts first
        size_t w = 0;
        for (size_t k = 0; k < keep.size(); k++) {
            const sa_gapped_alignment& r = keep[k];
            if (w > 0) {
                const sa_gapped_alignment& l = keep[w - 1];
                if (l.query_start == r.query_start && l.ref_start == r.ref_start && l.query_end == r.query_end && l.ref_end == r.ref_end)
                    continue;
            }
            keep[w++] = r;
        }
        keep.resize(w);
        rec.swap(keep);
    }
    st.returned = rec.size();
}

const SeqBuf& resident_query(Slot* sl, int rev, uint32_t buffer, const char* who) {
    DevCtx* dc = sl->ctx;
    const SeqBuf& q = rev ? dc->query_rc[buffer] : dc->query[buffer];
    if (!dc->ref.codes || !q.codes) {
        fprintf(stderr, "Error: %s needs a resident target block and query buffer %u\n", who, buffer);
        exit(1);
    }
    return q;
}

// Called per trace batch, after its walk, while the batch's tasks, walk results and ops are still in the slot's buffer: (device tasks,
// device walk results, device ops, first task, tasks in the batch).  sa_gapped_align_greedy emits its cover segments here.
using TraceHook = std::function<void(const TraceTask*, const TraceOut*, const uint32_t*, size_t, size_t)>;

// Pass 2 and the walk for the sides of the returned records.  tasks: the sides with d* > 0; their runs, in walk
// order, are appended to runs (task t's at run_off[t], run_n[t] of them) and their counts to res.
void trace_sides(Slot* sl, const SeqBuf& q, const Params& P, const std::vector<TraceTask>& tasks, std::vector<uint32_t>& runs,
                 std::vector<size_t>& run_off, std::vector<TraceOut>& res, sa_gapped_align_stats& st, const TraceHook& hook = nullptr) {
    DevCtx* dc = sl->ctx;
    GappedArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = dc->ref.codes;
    a.ref_len = dc->ref.len;
    a.query = q.codes;
    a.query_len = q.len;
    a.sub_mat = dc->d_sub_mat;
    a.gap_open = P.gap_open;
    a.gap_extend = P.gap_extend;
    a.ydrop = P.ydrop;
    a.max_extent = P.max_extent;
    a.max_band = P.max_band;
    const size_t budget = (size_t)g_gapped_trace_mb << 20;
    const size_t nt = tasks.size();
    res.resize(nt);
    run_off.resize(nt);
    hipEvent_t e0, e1, e2;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventCreate(&e2);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    std::vector<TraceTask> bt;
    std::vector<uint32_t> bops;
    for (size_t b = 0; b < nt;) {
        // the batch: tasks [b, e), their trace areas within the budget (a larger side alone)
        size_t e = b, trace = 0, nops = 0;
        bt.clear();
        while (e < nt) {
            const size_t tb = gapped_trace_bytes(P.max_band, tasks[e].dstar);
            if (e > b && trace + tb > budget) break;
            TraceTask t = tasks[e];
            t.trace_off = trace;
            t.ops_off = nops;
            bt.push_back(t);
            trace += tb;
            nops += (size_t)t.dstar;
            e++;
        }
        const size_t m = e - b;
        const size_t task_bytes = up(m * sizeof(TraceTask)), out_bytes = up(m * sizeof(TraceOut)), ops_bytes = up(nops * sizeof(uint32_t));
        sl->gapped_trace.ensure(task_bytes + out_bytes + ops_bytes + trace, "gapped trace");
        uint8_t* base = sl->gapped_trace.p;
        TraceTask* d_tasks = (TraceTask*)base;
        TraceOut* d_out = (TraceOut*)(base + task_bytes);
        uint32_t* d_ops = (uint32_t*)(base + task_bytes + out_bytes);
        uint8_t* d_area = base + task_bytes + out_bytes + ops_bytes;
        check_memcpy(hipMemcpyAsync(d_tasks, bt.data(), m * sizeof(TraceTask), hipMemcpyHostToDevice, sl->stream), "gapped trace tasks");
        hipEventRecord(e0, sl->stream);
        {
            ProfScope ps(sl, "gapped_trace");
            launch_gapped_trace(a, d_tasks, (uint32_t)m, d_area, sl->stream);
            check_launch("gapped_trace");
        }
        hipEventRecord(e1, sl->stream);
        {
            ProfScope ps(sl, "gapped_walk");
            launch_gapped_walk(a, d_tasks, (uint32_t)m, d_area, d_ops, d_out, sl->stream);
            check_launch("gapped_walk");
        }
        hipEventRecord(e2, sl->stream);
        bops.resize(nops);
        check_memcpy(hipMemcpyAsync(res.data() + b, d_out, m * sizeof(TraceOut), hipMemcpyDeviceToHost, sl->stream), "gapped walk results");
        check_memcpy(hipMemcpyAsync(bops.data(), d_ops, nops * sizeof(uint32_t), hipMemcpyDeviceToHost, sl->stream), "gapped ops");
        check_sync(sl->stream, "gapped_align");
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        st.trace_ms += ms;
        hipEventElapsedTime(&ms, e1, e2);
        st.walk_ms += ms;
        st.trace_bytes += trace;
        st.trace_batches++;
        for (size_t k = 0; k < m; k++) {
            const TraceOut& r = res[b + k];
            if (r.err || r.n_runs > (uint32_t)bt[k].dstar) {
                fprintf(stderr, "Error: GappedAlign: the path walk left the traced cells (side %zu, code %u)\n", b + k, r.err);
                exit(1);
            }
            run_off[b + k] = runs.size();
            runs.insert(runs.end(), bops.begin() + bt[k].ops_off, bops.begin() + bt[k].ops_off + r.n_runs);
        }
        if (hook) hook(d_tasks, d_out, d_ops, b, m);
        b = e;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipEventDestroy(e2);
}

// A record's path from its sides' tasks (-1: no task), its ops appended to all: genome order, the left side's runs as walked, the right
// side's reversed.
sa_gapped_path append_path(int64_t left, int64_t right, const std::vector<uint32_t>& runs, const std::vector<size_t>& run_off,
                           const std::vector<TraceOut>& res, std::vector<uint32_t>& all) {
    sa_gapped_path g;
    memset(&g, 0, sizeof(g));
    g.op_offset = all.size();
    for (int s = 0; s < 2; s++) {
        const int64_t t = s ? right : left;
        if (t < 0) continue;
        const TraceOut& r = res[(size_t)t];
        const uint32_t* w = runs.data() + run_off[(size_t)t];
        if (s == 0) all.insert(all.end(), w, w + r.n_runs);
        else for (uint32_t x = r.n_runs; x-- > 0;) all.push_back(w[x]);
        (s ? g.n_right : g.n_left) = r.n_runs;
        g.matches += r.matches;
        g.mismatches += r.mismatches;
        g.gap_opens += r.gap_opens;
        g.gap_bases += r.gap_bases;
    }
    return g;
}

// The malloc-ed outputs of sa_gapped_align and sa_gapped_align_greedy; returns the number of records.
size_t hand_out(const std::vector<sa_gapped_alignment>& rec, const std::vector<sa_gapped_path>& pa, const std::vector<uint32_t>& all,
                sa_gapped_alignment** out, sa_gapped_path** paths, uint32_t** ops, size_t* n_ops) {
    if (rec.empty()) return 0;
    *out = (sa_gapped_alignment*)malloc(rec.size() * sizeof(sa_gapped_alignment));
    memcpy(*out, rec.data(), rec.size() * sizeof(sa_gapped_alignment));
    *paths = (sa_gapped_path*)malloc(pa.size() * sizeof(sa_gapped_path));
    memcpy(*paths, pa.data(), pa.size() * sizeof(sa_gapped_path));
    if (!all.empty()) {
        *ops = (uint32_t*)malloc(all.size() * sizeof(uint32_t));
        memcpy(*ops, all.data(), all.size() * sizeof(uint32_t));
    }
    *n_ops = all.size();
    return rec.size();
}

struct GroupTimer {  // device time of groups of launches on one stream, summed
    hipEvent_t a, b;
    double ms = 0;
    GroupTimer() {
        hipEventCreate(&a);
        hipEventCreate(&b);
    }
    ~GroupTimer() {
        hipEventDestroy(a);
        hipEventDestroy(b);
    }
    void start(hipStream_t s) { hipEventRecord(a, s); }
    void stop(hipStream_t s) {
        hipEventRecord(b, s);
        hipEventSynchronize(b);
        float x = 0;
        hipEventElapsedTime(&x, a, b);
        ms += x;
    }
};

}  // namespace

extern "C" {

size_t sa_gapped_extend(const sa_segment_pair* hsps, size_t n, int rev, uint32_t buffer, const sa_gapped_params* p, int raw,
                        sa_gapped_alignment** out, sa_gapped_stats* stats) {
    require_proc("GappedExtend", buffer);
    const Params P = resolve(p);
    *out = nullptr;
    sa_gapped_stats st;
    memset(&st, 0, sizeof(st));
    if (n == 0) {
        if (stats) *stats = st;
        return 0;
    }
    Slot* sl = acquire_slot();
    const SeqBuf& q = resident_query(sl, rev, buffer, "GappedExtend");
    std::vector<GappedSide> side;
    extend_sides(sl, q, hsps, n, P, side, st);
    prof_flush(sl);
    release_slot(sl);

    std::vector<sa_gapped_alignment> rec;
    make_records(hsps, n, side, P, raw, rec, st);
    if (stats) *stats = st;
    if (rec.empty()) return 0;
    *out = (sa_gapped_alignment*)malloc(rec.size() * sizeof(sa_gapped_alignment));
    memcpy(*out, rec.data(), rec.size() * sizeof(sa_gapped_alignment));
    return rec.size();
}

void sa_free_gapped(sa_gapped_alignment* p) { free(p); }

size_t sa_gapped_align(const sa_segment_pair* hsps, size_t n, int rev, uint32_t buffer, const sa_gapped_params* p, int raw,
                       sa_gapped_alignment** out, sa_gapped_path** paths, uint32_t** ops, size_t* n_ops, sa_gapped_align_stats* stats) {
    require_proc("GappedAlign", buffer);
    const Params P = resolve(p);
    *out = nullptr;
    *paths = nullptr;
    *ops = nullptr;
    *n_ops = 0;
    sa_gapped_align_stats st;
    memset(&st, 0, sizeof(st));
    if (n == 0) {
        if (stats) *stats = st;
        return 0;
    }
    Slot* sl = acquire_slot();
    const SeqBuf& q = resident_query(sl, rev, buffer, "GappedAlign");
    std::vector<GappedSide> side;
    extend_sides(sl, q, hsps, n, P, side, st.extend);
    std::vector<sa_gapped_alignment> rec;
    make_records(hsps, n, side, P, raw, rec, st.extend);
    // the sides of the returned records with a best cell beyond the anchor, left before right
    std::vector<TraceTask> tasks;
    std::vector<int64_t> task_of(2 * rec.size(), -1);
    for (size_t k = 0; k < rec.size(); k++) {
        const size_t h = rec[k].hsp_index;
        const uint32_t ar = hsps[h].ref_start + hsps[h].len / 2, aq = hsps[h].query_start + hsps[h].len / 2;
        for (int s = 0; s < 2; s++) {
            const GappedSide& g = side[2 * h + s];
            if (g.best_i + g.best_j == 0) continue;
            task_of[2 * k + s] = (int64_t)tasks.size();
            tasks.push_back({ar, aq, s ? 1 : -1, g.best_i + g.best_j, g.best_i, g.best_j, 0, 0});
        }
    }
    std::vector<uint32_t> runs;
    std::vector<size_t> run_off;
    std::vector<TraceOut> res;
    trace_sides(sl, q, P, tasks, runs, run_off, res, st);
    prof_flush(sl);
    release_slot(sl);

    std::vector<uint32_t> all;
    all.reserve(runs.size());
    std::vector<sa_gapped_path> pa(rec.size());
    for (size_t k = 0; k < rec.size(); k++) pa[k] = append_path(task_of[2 * k], task_of[2 * k + 1], runs, run_off, res, all);
    if (stats) *stats = st;
    return hand_out(rec, pa, all, out, paths, ops, n_ops);
}

void sa_free_gapped_align(sa_gapped_alignment* out, sa_gapped_path* paths, uint32_t* ops) {
    free(out);
    free(paths);
    free(ops);
}

// Priority batches of option gapped_greedy_batch anchors: query the earlier batches' index, extend and trace the
// survivors (segments emitted per trace batch), edges between the survivors, resolve, merge the accepted segments into the index.
size_t sa_gapped_align_greedy(const sa_segment_pair* hsps, size_t n, int rev, uint32_t buffer, const sa_gapped_params* p,
                              sa_gapped_alignment** out, sa_gapped_path** paths, uint32_t** ops, size_t* n_ops,
                              sa_gapped_greedy_stats* stats) {
    require_proc("GappedAlignGreedy", buffer);
    const Params P = resolve(p);
    *out = nullptr;
    *paths = nullptr;
    *ops = nullptr;
    *n_ops = 0;
    sa_gapped_greedy_stats st;
    memset(&st, 0, sizeof(st));
    if (n == 0) {
        if (stats) *stats = st;
        return 0;
    }
    std::vector<uint32_t> pi(n);
    for (size_t k = 0; k < n; k++) pi[k] = (uint32_t)k;
    std::sort(pi.begin(), pi.end(), [&](uint32_t x, uint32_t y) { return hsps[x].score != hsps[y].score ? hsps[x].score > hsps[y].score : x < y; });

    Slot* sl = acquire_slot();
    const SeqBuf& q = resident_query(sl, rev, buffer, "GappedAlignGreedy");
    const hipStream_t s = sl->stream;
    auto anchor = [&](const sa_segment_pair& h, uint32_t* ar, uint32_t* aq) {
        *ar = h.ref_start + h.len / 2;
        *aq = h.query_start + h.len / 2;
    };
    auto point_key = [&](uint32_t t, uint32_t qq) { return (uint64_t)(t - qq + q.len) << 32 | t; };
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t B = (size_t)g_gapped_greedy_batch;
    GroupTimer tm;
    uint32_t R = 0;  // entries of the cover index, in cover_key[cur] / cover_run[cur]
    int cur = 0;
    std::vector<sa_gapped_alignment> arec;  // accepted, in acceptance order, with their paths and ops
    std::vector<sa_gapped_path> apath;
    std::vector<uint32_t> aops;
    uint64_t edges = 0, max_edges = 0, passes = 0;  // in-edges of the resolve passes (option debug prints them)
    for (size_t b0 = 0; b0 < n; b0 += B) {
        const size_t m = std::min(B, n - b0);
        st.priority_batches++;
        // (1) query: anchors on an alignment accepted in an earlier batch are final and skipped
        std::vector<uint32_t> surv;
        surv.reserve(m);
        if (R > 0) {
            std::vector<uint64_t> qk(m);
            for (size_t k = 0; k < m; k++) {
                uint32_t ar, aq;
                anchor(hsps[pi[b0 + k]], &ar, &aq);
                qk[k] = point_key(ar, aq);
            }
            sl->cover_work.ensure(up(m * 8) + m, "cover work");
            uint64_t* d_qk = (uint64_t*)sl->cover_work.p;
            uint8_t* d_cov = sl->cover_work.p + up(m * 8);
            check_memcpy(hipMemcpyAsync(d_qk, qk.data(), m * 8, hipMemcpyHostToDevice, s), "cover query keys");
            tm.start(s);
            {
                ProfScope ps(sl, "cover_query");
                launch_cover_query(sl->cover_key[cur].p, sl->cover_run[cur].p, R, d_qk, (uint32_t)m, d_cov, s);
                check_launch("cover_query");
            }
            tm.stop(s);
            std::vector<uint8_t> cov(m);
            check_memcpy(hipMemcpyAsync(cov.data(), d_cov, m, hipMemcpyDeviceToHost, s), "cover query");
            check_sync(s, "cover_query");
            for (size_t k = 0; k < m; k++) {
                if (!cov[k]) surv.push_back(pi[b0 + k]);
                else st.skipped++, st.covered++;
            }
        } else {
            surv.assign(pi.begin() + b0, pi.begin() + b0 + m);
        }
        const size_t S = surv.size();
        if (S == 0) continue;
        if (S > COVER_RESOLVE_MAX) {
            fprintf(stderr, "Error: GappedAlignGreedy: %zu survivors in one batch (at most %u)\n", S, COVER_RESOLVE_MAX);
            exit(1);
        }
        // (2) extend the survivors (rank r = position in pi within the batch) and trace the eligible ones' sides
        std::vector<sa_segment_pair> sh(S);
        for (size_t r = 0; r < S; r++) sh[r] = hsps[surv[r]];
        std::vector<GappedSide> side;
        sa_gapped_stats es;
        memset(&es, 0, sizeof(es));
        extend_sides(sl, q, sh.data(), S, P, side, es);
        std::vector<sa_gapped_alignment> rec;
        make_records(sh.data(), S, side, P, 1, rec, es);
        st.align.extend.anchors += es.anchors;
        st.align.extend.cells += es.cells;
        st.align.extend.extent_capped += es.extent_capped;
        st.align.extend.band_capped += es.band_capped;
        st.align.extend.kernel_ms += es.kernel_ms;
        std::vector<uint8_t> elig(S);
        std::vector<TraceTask> tasks;
        std::vector<uint32_t> task_owner;
        std::vector<int64_t> task_of(2 * S, -1);
        std::vector<CoverSeg> unit;  // the anchor points of the eligible survivors
        for (size_t r = 0; r < S; r++) {
            rec[r].hsp_index = surv[r];
            elig[r] = rec[r].score >= P.gappedthresh;
            if (!elig[r]) continue;
            uint32_t ar, aq;
            anchor(sh[r], &ar, &aq);
            unit.push_back({point_key(ar, aq), ar + 1, (uint32_t)r});
            for (int d = 0; d < 2; d++) {
                const GappedSide& g = side[2 * r + d];
                if (g.best_i + g.best_j == 0) continue;
                task_of[2 * r + d] = (int64_t)tasks.size();
                tasks.push_back({ar, aq, d ? 1 : -1, g.best_i + g.best_j, g.best_i, g.best_j, 0, 0});
                task_owner.push_back((uint32_t)r);
            }
        }
        std::vector<uint32_t> runs;
        std::vector<size_t> run_off;
        std::vector<TraceOut> res;
        size_t nseg = 0;
        std::vector<CoverEmit> em;
        auto emit = [&](const TraceTask* d_tasks, const TraceOut* d_out, const uint32_t* d_ops, size_t first, size_t cnt) {
            em.resize(cnt);
            size_t add = 0;
            for (size_t k = 0; k < cnt; k++) {
                em[k] = {(uint32_t)(nseg + add), task_owner[first + k]};
                add += res[first + k].n_runs;
            }
            sl->cover_segs.ensure((nseg + add) * sizeof(CoverSeg), "cover segments", true, s);
            sl->cover_work.ensure(cnt * sizeof(CoverEmit), "cover work");
            check_memcpy(hipMemcpyAsync(sl->cover_work.p, em.data(), cnt * sizeof(CoverEmit), hipMemcpyHostToDevice, s), "cover emit");
            tm.start(s);
            {
                ProfScope ps(sl, "cover_emit");
                launch_cover_emit(d_tasks, d_out, d_ops, (const CoverEmit*)sl->cover_work.p, (uint32_t)cnt, q.len,
                                  (CoverSeg*)sl->cover_segs.p, s);
                check_launch("cover_emit");
            }
            tm.stop(s);
            nseg += add;
        };
        trace_sides(sl, q, P, tasks, runs, run_off, res, st.align, emit);
        sl->cover_segs.ensure((nseg + unit.size()) * sizeof(CoverSeg), "cover segments", true, s);
        if (!unit.empty())
            check_memcpy(hipMemcpyAsync((CoverSeg*)sl->cover_segs.p + nseg, unit.data(), unit.size() * sizeof(CoverSeg),
                                        hipMemcpyHostToDevice, s), "cover anchor segments");
        nseg += unit.size();
        if (nseg > 0xffffffffull) {
            fprintf(stderr, "Error: GappedAlignGreedy: %zu cover segments in one batch\n", nseg);
            exit(1);
        }

        // (3) edges between the survivors, (4) resolve, (5) the accepted segments into the index
        std::vector<uint64_t> akey(S);
        std::vector<uint32_t> arank(S);
        for (size_t r = 0; r < S; r++) {
            uint32_t ar, aq;
            anchor(sh[r], &ar, &aq);
            akey[r] = point_key(ar, aq);
            arank[r] = (uint32_t)r;
        }
        const size_t na = R + nseg;  // entries of the merged index, at most
        size_t o = 0;
        auto carve = [&](size_t bytes) { const size_t at = o; o += up(bytes); return at; };
        const size_t o_akin = carve(S * 8), o_akey = carve(S * 8), o_rin = carve(S * 4), o_rank = carve(S * 4), o_elig = carve(S),
                     o_deg = carve((S + 1) * 4), o_row = carve((S + 1) * 8), o_cursor = carve((S + 1) * 8), o_state = carve(S),
                     o_qcov = carve(S), o_cnt = carve(4), o_sk = carve(nseg * 8), o_sdt = carve(nseg * 8), o_sk2 = carve(nseg * 8),
                     o_sdt2 = carve(nseg * 8), o_mv = carve(na * 8);
        sl->cover_work.ensure(o, "cover work");
        uint8_t* w = sl->cover_work.p;
        uint64_t *d_akin = (uint64_t*)(w + o_akin), *d_akey = (uint64_t*)(w + o_akey), *d_sk = (uint64_t*)(w + o_sk),
                 *d_sdt = (uint64_t*)(w + o_sdt), *d_sk2 = (uint64_t*)(w + o_sk2), *d_sdt2 = (uint64_t*)(w + o_sdt2), *d_mv = (uint64_t*)(w + o_mv),
                 *d_row = (uint64_t*)(w + o_row), *d_cursor = (uint64_t*)(w + o_cursor);
        uint32_t *d_rin = (uint32_t*)(w + o_rin), *d_rank = (uint32_t*)(w + o_rank), *d_deg = (uint32_t*)(w + o_deg), *d_cnt = (uint32_t*)(w + o_cnt);
        uint8_t *d_elig = w + o_elig, *d_state = w + o_state, *d_qcov = w + o_qcov;
        const CoverSeg* d_segs = (const CoverSeg*)sl->cover_segs.p;
        size_t tb = 0, x = 0;
        cover_sort_anchors(nullptr, &x, nullptr, nullptr, nullptr, nullptr, (uint32_t)S, s), tb = std::max(tb, x);
        cover_scan_offsets(nullptr, &(x = 0), nullptr, nullptr, (uint32_t)S, s), tb = std::max(tb, x);
        cover_sort_pairs(nullptr, &(x = 0), nullptr, nullptr, nullptr, nullptr, (uint32_t)nseg, s), tb = std::max(tb, x);
        cover_scan_runmax(nullptr, &(x = 0), nullptr, nullptr, (uint32_t)na, s), tb = std::max(tb, x);
        sl->cover_temp.ensure(tb + 256, "cover temp");
        size_t tbytes = sl->cover_temp.cap;
        void* d_temp = sl->cover_temp.p;
        check_memcpy(hipMemcpyAsync(d_akin, akey.data(), S * 8, hipMemcpyHostToDevice, s), "cover anchors");
        check_memcpy(hipMemcpyAsync(d_rin, arank.data(), S * 4, hipMemcpyHostToDevice, s), "cover anchors");
        hipMemsetAsync(d_state, 0, S, s);
        tm.start(s);
        {
            ProfScope ps(sl, "cover_edges");
            cover_sort_anchors(d_temp, &(tbytes = sl->cover_temp.cap), d_akin, d_akey, d_rin, d_rank, (uint32_t)S, s);
            check_launch("cover_edges");
        }
        tm.stop(s);
        // Resolve passes over the ranks [lo, hi): the edges of one pass stay within option gapped_greedy_edges (a cluster of anchors
        // that cover each other pairwise gives quadratically many), unless one survivor alone has more in-edges.  Survivors below lo
        // are decided; the accepted ones among them are in the index, so a query decides their cover of the ranks >= lo and the edges
        // need only owners >= lo.  One pass is the common case; every split gives the same result.
        std::vector<uint8_t> state(S, 0), pre(S, 0), el(elig);
        std::vector<uint64_t> row_h;
        const uint64_t cap = (uint64_t)g_gapped_greedy_edges;
        for (size_t lo = 0; lo < S;) {
            const size_t nr = S - lo;
            if (lo > 0) {
                tm.start(s);
                {
                    ProfScope ps(sl, "cover_query");
                    launch_cover_query(sl->cover_key[cur].p, sl->cover_run[cur].p, R, d_akin + lo, (uint32_t)nr, d_qcov, s);
                    check_launch("cover_query");
                }
                tm.stop(s);
                check_memcpy(hipMemcpyAsync(pre.data() + lo, d_qcov, nr, hipMemcpyDeviceToHost, s), "cover query");
                check_sync(s, "cover_query");
                for (size_t r = lo; r < S; r++)
                    if (pre[r]) el[r] = 0;  // covered by an accepted survivor of an earlier pass: final, never accepted, no edges
            }
            check_memcpy(hipMemcpyAsync(d_elig + lo, el.data() + lo, nr, hipMemcpyHostToDevice, s), "cover eligible");
            uint64_t total = 0;
            tm.start(s);
            {
                ProfScope ps(sl, "cover_edges");
                hipMemsetAsync(d_deg, 0, (nr + 1) * 4, s);
                launch_cover_edges(d_segs, (uint32_t)nseg, d_akey, d_rank, (uint32_t)S, d_elig, (uint32_t)lo, (uint32_t)S, d_deg, nullptr, nullptr, 1, s);
                cover_scan_offsets(d_temp, &(tbytes = sl->cover_temp.cap), d_deg, d_row, (uint32_t)nr, s);
                check_launch("cover_edges");
            }
            tm.stop(s);
            check_memcpy(hipMemcpyAsync(&total, d_row + nr, 8, hipMemcpyDeviceToHost, s), "cover edges");
            check_sync(s, "cover_edges");
            size_t hi = S;
            uint64_t n_edges = total;
            if (total > cap) {  // the longest prefix of ranks whose edges fit, at least one survivor
                row_h.resize(nr + 1);
                check_memcpy(hipMemcpyAsync(row_h.data(), d_row, (nr + 1) * 8, hipMemcpyDeviceToHost, s), "cover edges");
                check_sync(s, "cover_edges");
                size_t k = (size_t)(std::upper_bound(row_h.begin(), row_h.end(), cap) - row_h.begin()) - 1;
                if (k < 1) k = 1;
                hi = lo + k;
                n_edges = row_h[k];
            }
            const size_t nh = hi - lo;
            sl->cover_edges.ensure(std::max<size_t>(n_edges, 1), "cover edges");
            tm.start(s);
            {
                ProfScope ps(sl, "cover_resolve");
                check_memcpy(hipMemcpyAsync(d_cursor, d_row, nh * 8, hipMemcpyDeviceToDevice, s), "cover edges");
                launch_cover_edges(d_segs, (uint32_t)nseg, d_akey, d_rank, (uint32_t)S, d_elig, (uint32_t)lo, (uint32_t)hi, nullptr, d_cursor,
                                   sl->cover_edges.p, 0, s);
                launch_cover_resolve(d_elig + lo, d_row, sl->cover_edges.p, (uint32_t)nh, d_state + lo, s);
                hipMemsetAsync(d_cnt, 0, 4, s);
                launch_cover_select(d_segs, (uint32_t)nseg, d_state, (uint32_t)lo, (uint32_t)hi, d_sk, d_sdt, d_cnt, s);
                check_launch("cover_resolve");
            }
            tm.stop(s);
            uint32_t M = 0;
            check_memcpy(hipMemcpyAsync(state.data() + lo, d_state + lo, nh, hipMemcpyDeviceToHost, s), "cover resolve");
            check_memcpy(hipMemcpyAsync(&M, d_cnt, 4, hipMemcpyDeviceToHost, s), "cover resolve");
            check_sync(s, "cover_resolve");
            if (M > 0) {
                sl->cover_key[1 - cur].ensure(R + M, "cover index");
                sl->cover_run[1 - cur].ensure(R + M, "cover index");
                tm.start(s);
                {
                    ProfScope ps(sl, "cover_merge");
                    cover_sort_pairs(d_temp, &(tbytes = sl->cover_temp.cap), d_sk, d_sk2, d_sdt, d_sdt2, M, s);
                    launch_cover_merge(sl->cover_key[cur].p, sl->cover_run[cur].p, R, d_sk2, d_sdt2, M, sl->cover_key[1 - cur].p, d_mv, s);
                    cover_scan_runmax(d_temp, &(tbytes = sl->cover_temp.cap), d_mv, sl->cover_run[1 - cur].p, R + M, s);
                    check_launch("cover_merge");
                }
                tm.stop(s);
                cur = 1 - cur;
                R += M;
            }
            for (size_t r = lo; r < hi; r++)
                if (pre[r]) state[r] = 2;
            edges += n_edges;
            max_edges = std::max(max_edges, n_edges);
            passes++;
            lo = hi;
        }
        for (size_t r = 0; r < S; r++) {
            if (state[r] == 1) {
                arec.push_back(rec[r]);
                apath.push_back(append_path(task_of[2 * r], task_of[2 * r + 1], runs, run_off, res, aops));
            } else if (state[r] == 2) {
                st.covered++;
            } else {
                st.below_thresh++;
            }
        }
    }
    prof_flush(sl);
    release_slot(sl);

    if (opt_value("debug"))
        fprintf(stderr, "GappedAlignGreedy: %zu HSPs, %llu priority batches, %llu resolve passes, %llu edges (at most %llu in one pass)\n", n,
                (unsigned long long)st.priority_batches, (unsigned long long)passes, (unsigned long long)edges, (unsigned long long)max_edges);
    st.align.extend.returned = arec.size();
    st.cover_segments = R;
    st.cover_ms = tm.ms;
    std::vector<size_t> ord(arec.size());
    for (size_t k = 0; k < ord.size(); k++) ord[k] = k;
    std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return output_order(arec[x], arec[y]); });
    std::vector<sa_gapped_alignment> rec(ord.size());
    std::vector<sa_gapped_path> pa(ord.size());
    std::vector<uint32_t> all;
    all.reserve(aops.size());
    for (size_t k = 0; k < ord.size(); k++) {
        rec[k] = arec[ord[k]];
        pa[k] = apath[ord[k]];
        const uint32_t* w = aops.data() + pa[k].op_offset;
        pa[k].op_offset = all.size();
        all.insert(all.end(), w, w + pa[k].n_left + pa[k].n_right);
    }
    if (stats) *stats = st;
    return hand_out(rec, pa, all, out, paths, ops, n_ops);
}

}  // extern "C"
