// api_gapped.hip -- C-ABI sa_gapped_extend: gapped y-drop extension of HSP anchors (contract: include/segalign_amd.h),
// and sa_gapped_align: the same records plus their alignment paths.
// The host side: parameter defaults and limits, batches of anchors through the slot's stream (gapped.hip), the selection rules, and
// for the paths the batches of traced sides sized from pass 1's best antidiagonals.
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
        std::sort(keep.begin(), keep.end(), [](const sa_gapped_alignment& x, const sa_gapped_alignment& y) {
            if (x.query_start != y.query_start) return x.query_start < y.query_start;
            if (x.ref_start != y.ref_start) return x.ref_start < y.ref_start;
            if (x.query_end != y.query_end) return x.query_end < y.query_end;
            if (x.ref_end != y.ref_end) return x.ref_end < y.ref_end;
            if (x.score != y.score) return x.score > y.score;
            return x.hsp_index < y.hsp_index;
        });
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

// Pass 2 and the walk for the sides of the returned records.  tasks: the sides with d* > 0; their runs, in walk
// order, are appended to runs (task t's at run_off[t], run_n[t] of them) and their counts to res.
void trace_sides(Slot* sl, const SeqBuf& q, const Params& P, const std::vector<TraceTask>& tasks, std::vector<uint32_t>& runs,
                 std::vector<size_t>& run_off, std::vector<TraceOut>& res, sa_gapped_align_stats& st) {
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
        b = e;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipEventDestroy(e2);
}

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

    // genome order: the left side's runs as walked, the right side's reversed
    std::vector<uint32_t> all;
    all.reserve(runs.size());
    std::vector<sa_gapped_path> pa(rec.size());
    for (size_t k = 0; k < rec.size(); k++) {
        sa_gapped_path& g = pa[k];
        memset(&g, 0, sizeof(g));
        g.op_offset = all.size();
        for (int s = 0; s < 2; s++) {
            const int64_t t = task_of[2 * k + s];
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
    }
    if (stats) *stats = st;
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

void sa_free_gapped_align(sa_gapped_alignment* out, sa_gapped_path* paths, uint32_t* ops) {
    free(out);
    free(paths);
    free(ops);
}

}  // extern "C"
