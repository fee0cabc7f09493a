// api_gapped.hip -- C-ABI sa_gapped_extend: gapped y-drop extension of HSP anchors (contract: include/segalign_amd.h),
// sa_gapped_align: the same records plus their alignment paths, sa_gapped_align_greedy: anchors on earlier alignments
// skipped.  The host side as steps the entries share: the call frame, pass 1 (gapped.hip), the continuation of sides that
// ended at max_extent (option gapped_pieces), the selection rules, trace tasks, the trace batches sized from pass 1's
// best antidiagonals, the output; then greedy's cover index and resolve passes (cover.hip).
#include <functional>
#include <unordered_map>

#include "post_host.h"

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

// One entry's checks and parameters, and for n > 0 its slot, query strand and the kernel arguments every launch shares.  release(), at
// the latest on leaving scope, flushes the slot's profile and gives the slot back.
struct Frame {
    const char* who;
    Params P;
    Slot* sl = nullptr;
    GappedArgs a;  // hsps, num_tasks and out are set per launch
    Frame(const char* name, size_t n, int rev, uint32_t buffer, const sa_gapped_params* p) : who(name) {
        require_proc(who, buffer);
        P = resolve(p);
        memset(&a, 0, sizeof(a));
        if (n == 0) return;
        sl = acquire_slot();
        resident_block(who, sl, rev, buffer, a);
        a.gap_open = P.gap_open;
        a.gap_extend = P.gap_extend;
        a.ydrop = P.ydrop;
        a.max_extent = P.max_extent;
        a.max_band = P.max_band;
    }
    Frame(const Frame&) = delete;
    ~Frame() { release(); }
    void release() {
        if (!sl) return;
        prof_flush(sl);
        release_slot(sl);
        sl = nullptr;
    }
};

// An HSP's anchor point (t, q), and the key of a point in the cover index: diag << 32 | t with diag = t - q + query_len.
struct Point {
    uint32_t t, q;
};
Point anchor(const sa_segment_pair& h) { return {h.ref_start + h.len / 2, h.query_start + h.len / 2}; }
uint64_t point_key(Point p, uint32_t query_len) { return (uint64_t)(p.t - p.q + query_len) << 32 | p.t; }

// One piece of a continued side: its origin and its best cell relative to that origin.
struct Piece {
    uint32_t ar, aq;
    int32_t best_i, best_j;
};

// Pass 1's results: HSP k's sides side[2 k] (left) and side[2 k + 1] (right).  A side that was continued (continue_sides) holds the
// join of its pieces, and chain[its index] lists them, piece 0 first; a side of one piece has no chain.
struct Sides {
    std::vector<GappedSide> side;
    std::unordered_map<size_t, std::vector<Piece>> chain;
};

// Pass 1: every HSP's two sides, side[2 k] and side[2 k + 1]; kernel time added to st.
std::vector<GappedSide> extend_sides(Frame& f, const sa_segment_pair* hsps, size_t n, sa_gapped_stats& st) {
    Slot* sl = f.sl;
    const size_t batch = std::min(n, GAPPED_BATCH);
    sa_segment_pair* d_hsps;
    GappedSide* d_side;
    carve(sl->gapped, "gapped", [&](Carve& c) { c.take(d_hsps, batch).take(d_side, 2 * batch); });
    std::vector<GappedSide> side(2 * n);
    Timer<2> tm(sl->stream, "gapped timing");
    GappedArgs a = f.a;
    a.hsps = d_hsps;
    a.out = d_side;
    for (size_t b = 0; b < n; b += batch) {
        const size_t m = std::min(batch, n - b);
        to_device(d_hsps, hsps + b, m, sl->stream, "gapped hsps");
        a.num_tasks = (uint32_t)(2 * m);
        tm.mark(0);
        launch(sl, "gapped_extend", [&] { launch_gapped(a, sl->stream); });
        tm.mark(1);
        to_host(side.data() + 2 * b, d_side, 2 * m, sl->stream, "gapped results");
        check_sync(sl->stream, "gapped_extend");
        st.kernel_ms += tm.ms(0, 1);
    }
    return side;
}

// Continues the sides that ended at max_extent, piece after piece, up to option gapped_pieces pieces per side (the contract of
// DESIGN.md 14 / include/segalign_amd.h).  Round r extends piece r of every side that still continues, in launches of the one-sided
// kernel; the rounds end when none does.  With gapped_pieces = 1 nothing is launched and S.side stays pass 1's.
void continue_sides(Frame& f, const sa_segment_pair* hsps, Sides& S, sa_gapped_stats& st) {
    const int P = (int)g_gapped_pieces;
    if (P <= 1) return;
    struct Open {
        size_t s;  // index in S.side
        SideTask t;
    };
    auto continues = [&](const GappedSide& piece, size_t pieces, int32_t total) {
        return pieces < (size_t)P && (piece.flags & SA_GAPPED_EXTENT_CAP) && !(piece.flags & SA_GAPPED_BAND_CAP) &&
               (piece.best_i != 0 || piece.best_j != 0) && total < (1 << 29);
    };
    auto next_task = [](const SideTask& t, const GappedSide& g) {
        return SideTask{t.dir > 0 ? t.ar + (uint32_t)g.best_i : t.ar - (uint32_t)g.best_i,
                        t.dir > 0 ? t.aq + (uint32_t)g.best_j : t.aq - (uint32_t)g.best_j, t.dir, 0};
    };
    std::vector<Open> open, next;
    for (size_t s = 0; s < S.side.size(); s++) {
        const GappedSide& g = S.side[s];
        if (!continues(g, 1, g.best)) continue;
        const Point a = anchor(hsps[s / 2]);
        const SideTask t0 = {a.t, a.q, (s & 1) ? 1 : -1, 0};
        S.chain[s] = {{a.t, a.q, g.best_i, g.best_j}};
        open.push_back({s, next_task(t0, g)});
    }
    if (open.empty()) return;
    Slot* sl = f.sl;
    const size_t continued = open.size(), batch = std::min(open.size(), 2 * GAPPED_BATCH);
    SideTask* d_tasks;
    GappedSide* d_side;
    carve(sl->gapped, "gapped", [&](Carve& c) { c.take(d_tasks, batch).take(d_side, batch); });
    Timer<2> tm(sl->stream, "gapped timing");
    std::vector<SideTask> tasks;
    std::vector<GappedSide> res;
    size_t pieces = 0, rounds = 0;
    for (; !open.empty(); open.swap(next), rounds++) {
        const size_t m = open.size();
        tasks.resize(m);
        res.resize(m);
        for (size_t k = 0; k < m; k++) tasks[k] = open[k].t;
        for (size_t b = 0; b < m; b += batch) {
            const size_t c = std::min(batch, m - b);
            to_device(d_tasks, tasks.data() + b, c, sl->stream, "gapped pieces");
            tm.mark(0);
            launch(sl, "gapped_pieces", [&] { launch_gapped_sides(f.a, d_tasks, (uint32_t)c, d_side, sl->stream); });
            tm.mark(1);
            to_host(res.data() + b, d_side, c, sl->stream, "gapped pieces");
            check_sync(sl->stream, "gapped_pieces");
            st.kernel_ms += tm.ms(0, 1);
        }
        next.clear();
        for (size_t k = 0; k < m; k++) {
            const Open& o = open[k];
            const GappedSide& g = res[k];
            GappedSide& J = S.side[o.s];
            std::vector<Piece>& ch = S.chain[o.s];
            ch.push_back({o.t.ar, o.t.aq, g.best_i, g.best_j});
            J.best += g.best;
            J.best_i += g.best_i;
            J.best_j += g.best_j;
            J.cells = (uint32_t)std::min<uint64_t>((uint64_t)J.cells + g.cells, 0xffffffffull);
            J.flags = g.flags | SA_GAPPED_CONTINUED;  // the caps of the last piece: a cap that was continued past is no cap
            if (continues(g, ch.size(), J.best)) next.push_back({o.s, next_task(o.t, g)});
        }
        pieces += m;
    }
    if (opt_value("debug"))
        fprintf(stderr, "GappedPieces: %zu sides, %zu continued, %zu further pieces, %zu rounds\n", S.side.size(), continued, pieces, rounds);
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

// Records from the sides: raw (one per HSP, input order) or the selection rules.  Their counts are added to st.
std::vector<sa_gapped_alignment> make_records(const sa_segment_pair* hsps, size_t n, const std::vector<GappedSide>& side, const Params& P,
                                              int raw, sa_gapped_stats& st) {
    std::vector<sa_gapped_alignment> rec(n);
    for (size_t k = 0; k < n; k++) {
        const GappedSide& L = side[2 * k];
        const GappedSide& R = side[2 * k + 1];
        const Point a = anchor(hsps[k]);
        sa_gapped_alignment& o = rec[k];
        o.ref_start = a.t - (uint32_t)L.best_i;
        o.ref_end = a.t + (uint32_t)R.best_i;
        o.query_start = a.q - (uint32_t)L.best_j;
        o.query_end = a.q + (uint32_t)R.best_j;
        o.score = L.best + R.best;
        o.hsp_index = (uint32_t)k;
        o.flags = L.flags | R.flags;
        o.cells = L.cells + R.cells;
        st.cells += o.cells;
        if (o.flags & SA_GAPPED_EXTENT_CAP) st.extent_capped++;
        if (o.flags & SA_GAPPED_BAND_CAP) st.band_capped++;
    }
    st.anchors += n;
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
    st.returned += rec.size();
    return rec;
}

// Traced sides of records: record k's side s (0 left, 1 right) is the n_of[2 k + s] tasks from task_of[2 k + s] on (-1: none), one per
// piece of the side with a best cell beyond its origin, in piece order; task t is owned by record owner[t].  Once walked, task t's
// runs in walk order are res[t].n_runs entries of runs from off[t] on.
struct Traces {
    std::vector<TraceTask> tasks;
    std::vector<int64_t> task_of;
    std::vector<uint32_t> n_of;
    std::vector<uint32_t> owner, runs;
    std::vector<size_t> off;
    std::vector<TraceOut> res;
};

// The sides with a best cell beyond the anchor of the records scoring >= min_score, left before right, a continued side piece by
// piece; h = rec[k].hsp_index indexes record k's HSP and sides.
Traces trace_tasks(const std::vector<sa_gapped_alignment>& rec, const sa_segment_pair* hsps, const Sides& S, int min_score) {
    Traces tt;
    tt.task_of.assign(2 * rec.size(), -1);
    tt.n_of.assign(2 * rec.size(), 0);
    for (size_t k = 0; k < rec.size(); k++) {
        if (rec[k].score < min_score) continue;
        const size_t h = rec[k].hsp_index;
        const Point a = anchor(hsps[h]);
        for (int s = 0; s < 2; s++) {
            const GappedSide& g = S.side[2 * h + s];
            if (g.best_i + g.best_j == 0) continue;
            const size_t first = tt.tasks.size();
            const auto ch = S.chain.find(2 * h + s);
            if (ch == S.chain.end()) {
                tt.tasks.push_back({a.t, a.q, s ? 1 : -1, g.best_i + g.best_j, g.best_i, g.best_j, 0, 0});
            } else {
                for (const Piece& p : ch->second)  // (only a chain's last piece can end at its own origin)
                    if (p.best_i + p.best_j > 0) tt.tasks.push_back({p.ar, p.aq, s ? 1 : -1, p.best_i + p.best_j, p.best_i, p.best_j, 0, 0});
            }
            tt.task_of[2 * k + s] = (int64_t)first;
            tt.n_of[2 * k + s] = (uint32_t)(tt.tasks.size() - first);
            tt.owner.insert(tt.owner.end(), tt.tasks.size() - first, (uint32_t)k);
        }
    }
    return tt;
}

// Called per trace batch, after its walk, while the batch's tasks, walk results and ops are still in the slot's buffer: (device tasks,
// device walk results, device ops, first task, tasks in the batch).  trace_emit emits greedy's cover segments here.
using TraceHook = std::function<void(const TraceTask*, const TraceOut*, const uint32_t*, size_t, size_t)>;

// Pass 2 and the walk of tr's tasks.
void trace_sides(Frame& f, Traces& tr, sa_gapped_align_stats& st, const TraceHook& hook = nullptr) {
    Slot* sl = f.sl;
    const std::vector<TraceTask>& tasks = tr.tasks;
    const size_t nt = tasks.size();
    tr.res.resize(nt);
    tr.off.resize(nt);
    Timer<3> tm(sl->stream, "gapped timing");
    TraceBatch bt;
    std::vector<uint32_t> bops;
    for (size_t b = 0; b < nt;) {
        const size_t e = bt.pack(tasks, b, f.P.max_band), m = e - b;  // the batch: tasks [b, e)
        TraceTask* d_tasks;
        TraceOut* d_out;
        uint32_t* d_ops;
        uint8_t* d_area;
        carve(sl->gapped_trace, "gapped trace", [&](Carve& c) { c.take(d_tasks, m).take(d_out, m).take(d_ops, bt.nops).take(d_area, bt.trace); });
        to_device(d_tasks, bt.tasks.data(), m, sl->stream, "gapped trace tasks");
        tm.mark(0);
        launch(sl, "gapped_trace", [&] { launch_gapped_trace(f.a, d_tasks, (uint32_t)m, d_area, sl->stream); });
        tm.mark(1);
        launch(sl, "gapped_walk", [&] { launch_gapped_walk(f.a, d_tasks, (uint32_t)m, d_area, d_ops, d_out, sl->stream); });
        tm.mark(2);
        bops.resize(bt.nops);
        to_host(tr.res.data() + b, d_out, m, sl->stream, "gapped walk results");
        to_host(bops.data(), d_ops, bt.nops, sl->stream, "gapped ops");
        check_sync(sl->stream, "gapped_align");
        st.trace_ms += tm.ms(0, 1);
        st.walk_ms += tm.ms(1, 2);
        st.trace_bytes += bt.trace;
        st.trace_batches++;
        for (size_t k = 0; k < m; k++)
            if (!take_runs(bt.tasks[k], tr.res[b + k], bops, tr.runs, tr.off[b + k])) {
                fprintf(stderr, "Error: GappedAlign: the path walk left the traced cells (side %zu, code %u)\n", b + k, tr.res[b + k].err);
                exit(1);
            }
        if (hook) hook(d_tasks, d_out, d_ops, b, m);
        b = e;
    }
}

// An entry's records, their paths and the paths' ops.
struct Output {
    std::vector<sa_gapped_alignment> rec;
    std::vector<sa_gapped_path> pa;
    std::vector<uint32_t> ops;
    // the path of record k of tr: genome order, the left side's runs as walked, the right side's reversed; the pieces of a continued
    // side in genome order too (left: the last piece first), their runs not merged where two pieces meet
    void add_path(const Traces& tr, size_t k) {
        sa_gapped_path g;
        memset(&g, 0, sizeof(g));
        g.op_offset = ops.size();
        for (int s = 0; s < 2; s++) {
            const int64_t t0 = tr.task_of[2 * k + s];
            if (t0 < 0) continue;
            const uint32_t np = tr.n_of[2 * k + s];
            for (uint32_t x = 0; x < np; x++) {
                const size_t t = (size_t)t0 + (s == 0 ? np - 1 - x : x);
                const TraceOut& o = tr.res[t];
                const uint32_t* w = tr.runs.data() + tr.off[t];
                if (s == 0) ops.insert(ops.end(), w, w + o.n_runs);
                else for (uint32_t y = o.n_runs; y-- > 0;) ops.push_back(w[y]);
                (s ? g.n_right : g.n_left) += o.n_runs;
                g.matches += o.matches;
                g.mismatches += o.mismatches;
                g.gap_opens += o.gap_opens;
                g.gap_bases += o.gap_bases;
            }
        }
        pa.push_back(g);
    }
    void sort() {  // into output order, the ops repacked in that order
        std::vector<size_t> ord(rec.size());
        for (size_t k = 0; k < ord.size(); k++) ord[k] = k;
        std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return output_order(rec[x], rec[y]); });
        Output o;
        o.rec.reserve(rec.size());
        o.pa.reserve(pa.size());
        o.ops.reserve(ops.size());
        for (size_t k : ord) {
            o.rec.push_back(rec[k]);
            o.pa.push_back(pa[k]);
            o.pa.back().op_offset = o.ops.size();
            o.ops.insert(o.ops.end(), ops.begin() + pa[k].op_offset, ops.begin() + pa[k].op_offset + pa[k].n_left + pa[k].n_right);
        }
        *this = std::move(o);
    }
    // The stats and malloc-ed copies, paths and ops unless paths is nullptr (sa_gapped_extend); returns the number of records.
    template <typename Stats>
    size_t hand_out(const char* who, const Stats& st, Stats* stats, sa_gapped_alignment** out, sa_gapped_path** paths = nullptr,
                    uint32_t** ops_out = nullptr, size_t* n_ops = nullptr) {
        if (stats) *stats = st;
        *out = malloc_copy(rec, who);
        if (paths) {
            *paths = malloc_copy(pa, who);
            *ops_out = malloc_copy(ops, who);
            *n_ops = ops.size();
        }
        return rec.size();
    }
};

// ---- sa_gapped_align_greedy ----

// A priority batch's work area in the slot's cover_work (named as in gapped.h), rocPRIM's temp storage and the segment count.
struct CoverWork {
    uint64_t *akin, *akey, *row, *cursor, *sk, *sdt, *sk2, *sdt2, *mv;
    uint32_t *rin, *rank, *deg, *cnt;
    uint8_t *elig, *state, *qcov;
    void* temp;
    size_t temp_cap, temp_bytes, nseg;
    size_t* tbytes() { return &(temp_bytes = temp_cap); }  // rocPRIM's in-out size, reset for each call
};

// The cover index of one call: R entries, keys and running maxima, in the slot's cover_key[cur] / cover_run[cur].  It also sums the
// device time of the cover launch groups (cover_ms), each waited for, and the resolve passes' in-edges (option debug prints them).
struct CoverIndex {
    Slot* sl;
    Timer<2> tm;
    double ms = 0;
    uint32_t R = 0;
    int cur = 0;
    uint64_t edges = 0, max_edges = 0, passes = 0;
    explicit CoverIndex(Slot* s) : sl(s), tm(s->stream, "gapped timing") {}
    template <typename F>
    void group(const char* name, F&& launches) {
        tm.mark(0);
        launch(sl, name, launches);
        tm.mark(1);
        ms += tm.wait(0, 1);
    }
    // covered[k] = 1 when the point key keys[k] lies on the index (R > 0); d_cov: n bytes on the device
    void query(const uint64_t* keys, size_t n, uint8_t* d_cov, uint8_t* covered) {
        group("cover_query", [&] { launch_cover_query(sl->cover_key[cur].p, sl->cover_run[cur].p, R, keys, (uint32_t)n, d_cov, sl->stream); });
        to_host(covered, d_cov, n, sl->stream, "cover query");
        check_sync(sl->stream, "cover_query");
    }
    // the M selected segments in w.sk / w.sdt merged into the index, written to the other buffer of the pair
    void merge(CoverWork& w, uint32_t M) {
        sl->cover_key[1 - cur].ensure(R + M, "cover index");
        sl->cover_run[1 - cur].ensure(R + M, "cover index");
        group("cover_merge", [&] {
            cover_sort_pairs(w.temp, w.tbytes(), w.sk, w.sk2, w.sdt, w.sdt2, M, sl->stream);
            launch_cover_merge(sl->cover_key[cur].p, sl->cover_run[cur].p, R, w.sk2, w.sdt2, M, sl->cover_key[1 - cur].p, w.mv, sl->stream);
            cover_scan_runmax(w.temp, w.tbytes(), w.mv, sl->cover_run[1 - cur].p, R + M, sl->stream);
        });
        cur = 1 - cur;
        R += M;
    }
};

// The anchors of pi[0, m) that no alignment accepted in an earlier batch covers.
std::vector<uint32_t> survivors(Frame& f, CoverIndex& ix, const sa_segment_pair* hsps, const uint32_t* pi, size_t m) {
    if (ix.R == 0) return std::vector<uint32_t>(pi, pi + m);
    std::vector<uint64_t> qk(m);
    for (size_t k = 0; k < m; k++) qk[k] = point_key(anchor(hsps[pi[k]]), f.a.query_len);
    uint64_t* d_qk;
    uint8_t* d_cov;
    carve(f.sl->cover_work, "cover work", [&](Carve& c) { c.take(d_qk, m).take(d_cov, m); });
    to_device(d_qk, qk.data(), m, f.sl->stream, "cover query keys");
    std::vector<uint8_t> cov(m);
    ix.query(d_qk, m, d_cov, cov.data());
    std::vector<uint32_t> surv;
    surv.reserve(m);
    for (size_t k = 0; k < m; k++)
        if (!cov[k]) surv.push_back(pi[k]);
    return surv;
}

// trace_sides, each trace batch's segments emitted into the slot's cover_segs while its walk is on the device; returns their count.  A
// piece of a continued side is a task of its own, so its runs are placed from the piece's origin and best cell, not the record's.
size_t trace_emit(Frame& f, CoverIndex& ix, Traces& tr, sa_gapped_align_stats& st) {
    Slot* sl = f.sl;
    size_t nseg = 0;
    std::vector<CoverEmit> em;
    trace_sides(f, tr, st, [&](const TraceTask* d_tasks, const TraceOut* d_out, const uint32_t* d_ops, size_t first, size_t cnt) {
        em.resize(cnt);
        size_t add = 0;
        for (size_t k = 0; k < cnt; k++) {
            em[k] = {(uint32_t)(nseg + add), tr.owner[first + k]};
            add += tr.res[first + k].n_runs;
        }
        sl->cover_segs.ensure((nseg + add) * sizeof(CoverSeg), "cover segments", true, sl->stream);
        sl->cover_work.ensure(cnt * sizeof(CoverEmit), "cover work");
        to_device((CoverEmit*)sl->cover_work.p, em.data(), cnt, sl->stream, "cover emit");
        ix.group("cover_emit", [&] {
            launch_cover_emit(d_tasks, d_out, d_ops, (const CoverEmit*)sl->cover_work.p, (uint32_t)cnt, f.a.query_len,
                              (CoverSeg*)sl->cover_segs.p, sl->stream);
        });
        nseg += add;
    });
    return nseg;
}

// rocPRIM temp storage for S survivors, nseg segments and na index entries: the most any of the four steps needs.
size_t cover_temp_bytes(size_t S, size_t nseg, size_t na, hipStream_t s) {
    size_t tb = 0, x = 0;
    cover_sort_anchors(nullptr, &x, nullptr, nullptr, nullptr, nullptr, (uint32_t)S, s), tb = std::max(tb, x);
    cover_scan_offsets(nullptr, &(x = 0), nullptr, nullptr, (uint32_t)S, s), tb = std::max(tb, x);
    cover_sort_pairs(nullptr, &(x = 0), nullptr, nullptr, nullptr, nullptr, (uint32_t)nseg, s), tb = std::max(tb, x);
    cover_scan_runmax(nullptr, &(x = 0), nullptr, nullptr, (uint32_t)na, s), tb = std::max(tb, x);
    return tb;
}

// The work area of the resolve passes: a unit segment per eligible survivor's anchor point after the nseg emitted segments, and the
// survivors' anchor keys sorted with their ranks.
CoverWork cover_work(Frame& f, CoverIndex& ix, const std::vector<sa_segment_pair>& sh, const std::vector<uint8_t>& elig, size_t nseg) {
    Slot* sl = f.sl;
    const hipStream_t s = sl->stream;
    const size_t S = sh.size();
    std::vector<uint64_t> akey(S);
    std::vector<uint32_t> arank(S);
    std::vector<CoverSeg> unit;
    for (size_t r = 0; r < S; r++) {
        const Point a = anchor(sh[r]);
        akey[r] = point_key(a, f.a.query_len);
        arank[r] = (uint32_t)r;
        if (elig[r]) unit.push_back({akey[r], a.t + 1, (uint32_t)r});
    }
    sl->cover_segs.ensure((nseg + unit.size()) * sizeof(CoverSeg), "cover segments", true, s);
    to_device((CoverSeg*)sl->cover_segs.p + nseg, unit.data(), unit.size(), s, "cover anchor segments");
    nseg += unit.size();
    if (nseg > 0xffffffffull) {
        fprintf(stderr, "Error: GappedAlignGreedy: %zu cover segments in one batch\n", nseg);
        exit(1);
    }
    const size_t na = ix.R + nseg;  // entries of the merged index, at most
    CoverWork w;
    carve(sl->cover_work, "cover work", [&](Carve& c) {
        c.take(w.akin, S).take(w.akey, S).take(w.rin, S).take(w.rank, S).take(w.elig, S).take(w.deg, S + 1).take(w.row, S + 1);
        c.take(w.cursor, S + 1).take(w.state, S).take(w.qcov, S).take(w.cnt, 1);
        c.take(w.sk, nseg).take(w.sdt, nseg).take(w.sk2, nseg).take(w.sdt2, nseg).take(w.mv, na);
    });
    sl->cover_temp.ensure(cover_temp_bytes(S, nseg, na, s) + 256, "cover temp");
    w.temp = sl->cover_temp.p;
    w.temp_cap = sl->cover_temp.cap;
    w.nseg = nseg;
    to_device(w.akin, akey.data(), S, s, "cover anchors");
    to_device(w.rin, arank.data(), S, s, "cover anchors");
    hipMemsetAsync(w.state, 0, S, s);
    ix.group("cover_edges", [&] { cover_sort_anchors(w.temp, w.tbytes(), w.akin, w.akey, w.rin, w.rank, (uint32_t)S, s); });
    return w;
}

// Resolve passes over the ranks [lo, hi): the edges of one pass stay within option gapped_greedy_edges (a cluster of anchors that
// cover each other pairwise gives quadratically many), unless one survivor alone has more in-edges.  Survivors below lo are decided;
// the accepted ones among them are in the index, so a query decides their cover of the ranks >= lo and the edges need only owners >= lo.
// One pass is the common case; every split gives the same result.  el: the survivors' eligibility.  Returns their
// states: 1 accepted, 2 covered, 0 below the threshold.
std::vector<uint8_t> resolve_passes(CoverIndex& ix, CoverWork& w, std::vector<uint8_t> el) {
    Slot* sl = ix.sl;
    const hipStream_t s = sl->stream;
    const size_t S = el.size();
    const CoverSeg* d_segs = (const CoverSeg*)sl->cover_segs.p;
    std::vector<uint8_t> state(S, 0), pre(S, 0);
    std::vector<uint64_t> row_h;
    const uint64_t cap = (uint64_t)g_gapped_greedy_edges;
    for (size_t lo = 0; lo < S;) {
        const size_t nr = S - lo;
        if (lo > 0) {
            ix.query(w.akin + lo, nr, w.qcov, pre.data() + lo);
            for (size_t r = lo; r < S; r++)
                if (pre[r]) el[r] = 0;  // covered by an accepted survivor of an earlier pass: final, never accepted, no edges
        }
        to_device(w.elig + lo, el.data() + lo, nr, s, "cover eligible");
        uint64_t total = 0;
        ix.group("cover_edges", [&] {
            hipMemsetAsync(w.deg, 0, (nr + 1) * 4, s);
            launch_cover_edges(d_segs, (uint32_t)w.nseg, w.akey, w.rank, (uint32_t)S, w.elig, (uint32_t)lo, (uint32_t)S, w.deg, nullptr, nullptr, 1, s);
            cover_scan_offsets(w.temp, w.tbytes(), w.deg, w.row, (uint32_t)nr, s);
        });
        to_host(&total, w.row + nr, 1, s, "cover edges");
        check_sync(s, "cover_edges");
        size_t hi = S;
        uint64_t n_edges = total;
        if (total > cap) {  // the longest prefix of ranks whose edges fit, at least one survivor
            row_h.resize(nr + 1);
            to_host(row_h.data(), w.row, nr + 1, s, "cover edges");
            check_sync(s, "cover_edges");
            size_t k = (size_t)(std::upper_bound(row_h.begin(), row_h.end(), cap) - row_h.begin()) - 1;
            if (k < 1) k = 1;
            hi = lo + k;
            n_edges = row_h[k];
        }
        const size_t nh = hi - lo;
        sl->cover_edges.ensure(std::max<size_t>(n_edges, 1), "cover edges");
        ix.group("cover_resolve", [&] {
            check_memcpy(hipMemcpyAsync(w.cursor, w.row, nh * 8, hipMemcpyDeviceToDevice, s), "cover edges");
            launch_cover_edges(d_segs, (uint32_t)w.nseg, w.akey, w.rank, (uint32_t)S, w.elig, (uint32_t)lo, (uint32_t)hi, nullptr, w.cursor,
                               sl->cover_edges.p, 0, s);
            launch_cover_resolve(w.elig + lo, w.row, sl->cover_edges.p, (uint32_t)nh, w.state + lo, s);
            hipMemsetAsync(w.cnt, 0, 4, s);
            launch_cover_select(d_segs, (uint32_t)w.nseg, w.state, (uint32_t)lo, (uint32_t)hi, w.sk, w.sdt, w.cnt, s);
        });
        uint32_t M = 0;
        to_host(state.data() + lo, w.state + lo, nh, s, "cover resolve");
        to_host(&M, w.cnt, 1, s, "cover resolve");
        check_sync(s, "cover_resolve");
        if (M > 0) ix.merge(w, M);
        for (size_t r = lo; r < hi; r++)
            if (pre[r]) state[r] = 2;
        ix.edges += n_edges;
        ix.max_edges = std::max(ix.max_edges, n_edges);
        ix.passes++;
        lo = hi;
    }
    return state;
}

}  // namespace

extern "C" {

size_t sa_gapped_extend(const sa_segment_pair* hsps, size_t n, int rev, uint32_t buffer, const sa_gapped_params* p, int raw,
                        sa_gapped_alignment** out, sa_gapped_stats* stats) {
    Frame f("GappedExtend", n, rev, buffer, p);
    sa_gapped_stats st = {};
    Output o;
    if (n > 0) {
        Sides S = {extend_sides(f, hsps, n, st), {}};
        continue_sides(f, hsps, S, st);
        f.release();
        o.rec = make_records(hsps, n, S.side, f.P, raw, st);
    }
    return o.hand_out(f.who, st, stats, out);
}

void sa_free_gapped(sa_gapped_alignment* p) { free(p); }

size_t sa_gapped_align(const sa_segment_pair* hsps, size_t n, int rev, uint32_t buffer, const sa_gapped_params* p, int raw,
                       sa_gapped_alignment** out, sa_gapped_path** paths, uint32_t** ops, size_t* n_ops, sa_gapped_align_stats* stats) {
    Frame f("GappedAlign", n, rev, buffer, p);
    sa_gapped_align_stats st = {};
    Output o;
    if (n > 0) {
        Sides S = {extend_sides(f, hsps, n, st.extend), {}};
        continue_sides(f, hsps, S, st.extend);
        o.rec = make_records(hsps, n, S.side, f.P, raw, st.extend);
        Traces tr = trace_tasks(o.rec, hsps, S, INT32_MIN);
        trace_sides(f, tr, st);
        f.release();
        o.pa.reserve(o.rec.size());
        o.ops.reserve(tr.runs.size());
        for (size_t k = 0; k < o.rec.size(); k++) o.add_path(tr, k);
    }
    return o.hand_out(f.who, st, stats, out, paths, ops, n_ops);
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
    Frame f("GappedAlignGreedy", n, rev, buffer, p);
    sa_gapped_greedy_stats st = {};
    Output o;  // the accepted records, in acceptance order until sorted
    if (n == 0) return o.hand_out(f.who, st, stats, out, paths, ops, n_ops);
    std::vector<uint32_t> pi(n);  // the priority order
    for (size_t k = 0; k < n; k++) pi[k] = (uint32_t)k;
    std::sort(pi.begin(), pi.end(), [&](uint32_t x, uint32_t y) { return hsps[x].score != hsps[y].score ? hsps[x].score > hsps[y].score : x < y; });

    CoverIndex ix(f.sl);
    const size_t B = (size_t)g_gapped_greedy_batch;
    for (size_t b0 = 0; b0 < n; b0 += B) {
        st.priority_batches++;
        // (1) query: anchors on an alignment accepted in an earlier batch are final and skipped
        const size_t m = std::min(B, n - b0);
        const std::vector<uint32_t> surv = survivors(f, ix, hsps, pi.data() + b0, m);
        const size_t S = surv.size();
        st.skipped += m - S;
        st.covered += m - S;
        if (S == 0) continue;
        if (S > COVER_RESOLVE_MAX) {
            fprintf(stderr, "Error: GappedAlignGreedy: %zu survivors in one batch (at most %u)\n", S, COVER_RESOLVE_MAX);
            exit(1);
        }
        // (2) extend the survivors (rank r = position in pi within the batch), trace the eligible ones' sides and emit their segments
        std::vector<sa_segment_pair> sh(S);
        for (size_t r = 0; r < S; r++) sh[r] = hsps[surv[r]];
        Sides sides = {extend_sides(f, sh.data(), S, st.align.extend), {}};
        continue_sides(f, sh.data(), sides, st.align.extend);
        const std::vector<sa_gapped_alignment> rec = make_records(sh.data(), S, sides.side, f.P, 1, st.align.extend);
        std::vector<uint8_t> elig(S);
        for (size_t r = 0; r < S; r++) elig[r] = rec[r].score >= f.P.gappedthresh;
        Traces tr = trace_tasks(rec, sh.data(), sides, f.P.gappedthresh);
        const size_t nseg = trace_emit(f, ix, tr, st.align);
        // (3) edges between the survivors, (4) resolve, (5) the accepted segments into the index
        CoverWork w = cover_work(f, ix, sh, elig, nseg);
        const std::vector<uint8_t> state = resolve_passes(ix, w, elig);
        for (size_t r = 0; r < S; r++) {
            if (state[r] == 1) {
                o.rec.push_back(rec[r]);
                o.rec.back().hsp_index = surv[r];
                o.add_path(tr, r);
            } else if (state[r] == 2) {
                st.covered++;
            } else {
                st.below_thresh++;
            }
        }
    }
    st.cover_segments = ix.R;
    st.cover_ms = ix.ms;
    f.release();

    if (opt_value("debug"))
        fprintf(stderr, "GappedAlignGreedy: %zu HSPs, %llu priority batches, %llu resolve passes, %llu edges (at most %llu in one pass)\n", n,
                (unsigned long long)st.priority_batches, (unsigned long long)ix.passes, (unsigned long long)ix.edges, (unsigned long long)ix.max_edges);
    st.align.extend.returned = o.rec.size();  // the accepted records, not the sum of the batches' extended ones
    o.sort();
    return o.hand_out(f.who, st, stats, out, paths, ops, n_ops);
}

}  // extern "C"
