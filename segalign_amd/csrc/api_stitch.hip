// api_stitch.hip -- C-ABI sa_stitch_chains: every chain of HSPs as one gapped alignment through all its members (contract:
// include/segalign_amd.h).  The host side as steps: the checked members, the links, the member scores and the link sweeps
// (stitch.hip) in batches by instance under option gapped_trace_mb, each with the walk of its unbroken links (gapped.hip's walk kernel),
// and the records' assembly.
#include <limits.h>

#include "post_host.h"
#include "stitch.h"

using namespace sa;

namespace {

const Fail fail{"StitchChains"};

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

struct Link {
    uint32_t re, qe;  // the rectangle's origin: the end of the member before it
    int32_t score;
    uint32_t n_runs;  // its walk: n_runs entries of runs from run_off on, in walk order
    size_t run_off;
    uint32_t matches, mismatches;
};

// One call's chains as the steps hand them on: the member entries in input order with their scores, the links in input order (lk for
// the caller, li beside it), link_of[k] = the link after member entry k, and the walks' runs.
struct Chains {
    std::vector<StitchMember> mem;
    std::vector<StitchMemberOut> mo;
    std::vector<sa_stitch_link> lk;
    std::vector<Link> li;
    std::vector<size_t> link_of;
    std::vector<uint32_t> runs;
};

// The M member entries, each checked to name an HSP of the input that lies inside the block.
std::vector<StitchMember> checked_members(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, size_t M, const StitchArgs& a) {
    std::vector<StitchMember> mem(M);
    for (size_t k = 0; k < M; k++) {
        const sa_segment_pair& h = checked_member(fail, hsps, n_hsps, members, k, a.ref_len, a.query_len);
        mem[k] = {h.ref_start, h.query_start, h.len, 0};
    }
    return mem;
}

// The links between consecutive members of every chain, in input order; a link longer than max_link is SA_STITCH_LONG from the start.
void make_links(Chains& C, const uint32_t* first, size_t n_chains, const Params& P) {
    C.link_of.assign(C.mem.size(), (size_t)-1);
    for (size_t c = 0; c < n_chains; c++)
        for (size_t k = first[c]; k + 1 < first[c + 1]; k++) {
            const StitchMember &x = C.mem[k], &y = C.mem[k + 1];
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
            C.link_of[k] = C.lk.size();
            C.lk.push_back(l);
            C.li.push_back({(uint32_t)re, (uint32_t)qe, 0, 0, 0, 0, 0});
        }
}

void member_scores(Slot* sl, const StitchArgs& a, Chains& C, sa_stitch_stats& st) {
    const hipStream_t s = sl->stream;
    const size_t M = C.mem.size();
    C.mo.resize(M);
    StitchMember* d_mem;
    StitchMemberOut* d_mo;
    carve(sl->stitch, "stitch", [&](Carve& c) { c.take(d_mem, M).take(d_mo, M); });
    Timer<2> tm(s, "stitch timing");
    to_device(d_mem, C.mem.data(), M, s, "stitch members");
    tm.mark(0);
    launch(sl, "stitch_members", [&] { launch_stitch_members(a, d_mem, (uint32_t)M, d_mo, s); });
    tm.mark(1);
    to_host(C.mo.data(), d_mo, M, s, "stitch member scores");
    check_sync(s, "stitch_members");
    st.member_ms = tm.ms(0, 1);
}

constexpr int KS[5] = {2, 4, 8, 17, 33};  // the sweep's instances

// The links to sweep as trace tasks, binned by instance: the smallest K with 64 K >= dt + 1.  tasks[b][k] is link ids[b][k].
struct Bins {
    std::vector<TraceTask> tasks[5];
    std::vector<size_t> ids[5];
};
Bins bin_links(const Chains& C, sa_stitch_stats& st) {
    Bins B;
    for (size_t k = 0; k < C.lk.size(); k++) {
        const sa_stitch_link& l = C.lk[k];
        if (l.flags) continue;
        st.swept++;
        st.cells += l.cells;
        if (l.dt + l.dq == 0) continue;  // score 0 and no op
        int b = 0;
        while (64 * KS[b] < (int)l.dt + 1) b++;
        B.ids[b].push_back(k);
        B.tasks[b].push_back({C.li[k].re, C.li[k].qe, 1, (int)(l.dt + l.dq), (int32_t)l.dt, (int32_t)l.dq, 0, 0});
    }
    return B;
}

// A batch's areas in the slot's stitch buffer.
struct BatchBufs {
    TraceTask *tasks, *walk;
    TraceOut* out;
    int32_t* score;
    uint32_t* ops;
    uint8_t* area;
};

// The walk of the batch's links that are neither dead nor low: tasks wt of the links widx, their trace areas still in d.area.
void walk_batch(Slot* sl, const GappedArgs& ga, const BatchBufs& d, size_t nops, const std::vector<TraceTask>& wt, const std::vector<size_t>& widx,
                Chains& C, Timer<3>& tm, sa_stitch_stats& st) {
    const hipStream_t s = sl->stream;
    const size_t w = wt.size();
    to_device(d.walk, wt.data(), w, s, "stitch walk tasks");
    tm.mark(1);
    launch(sl, "stitch_walk", [&] { launch_gapped_walk(ga, d.walk, (uint32_t)w, d.area, d.ops, d.out, s); });
    tm.mark(2);
    std::vector<TraceOut> wo(w);
    std::vector<uint32_t> bops(nops);
    to_host(wo.data(), d.out, w, s, "stitch walk results");
    to_host(bops.data(), d.ops, nops, s, "stitch ops");
    check_sync(s, "stitch_walk");
    st.walk_ms += tm.ms(1, 2);
    for (size_t k = 0; k < w; k++) {
        const TraceOut& r = wo[k];
        Link& x = C.li[widx[k]];
        if (!take_runs(wt[k], r, bops, C.runs, x.run_off)) {
            fprintf(stderr, "Error: StitchChains: the path walk left the traced cells (link %zu, code %u)\n", widx[k], r.err);
            exit(1);
        }
        x.n_runs = r.n_runs;
        x.matches = r.matches;
        x.mismatches = r.mismatches;
    }
}

// One batch of one instance: the sweep of the links ids[0, m) as bt's tasks, their scores and flags, then the walk.
void sweep_batch(Slot* sl, const StitchArgs& a, const GappedArgs& ga, const Params& P, const TraceBatch& bt, const size_t* ids, Chains& C,
                 Timer<3>& tm, sa_stitch_stats& st) {
    const hipStream_t s = sl->stream;
    const size_t m = bt.tasks.size();
    BatchBufs d;
    carve(sl->stitch, "stitch", [&](Carve& c) {
        c.take(d.tasks, m).take(d.walk, m).take(d.out, m).take(d.score, m).take(d.ops, bt.nops).take(d.area, bt.trace);
    });
    to_device(d.tasks, bt.tasks.data(), m, s, "stitch tasks");
    tm.mark(0);
    launch(sl, "stitch_sweep", [&] { launch_stitch_sweep(a, ga.max_band, d.tasks, (uint32_t)m, d.area, d.score, s); });
    tm.mark(1);
    std::vector<int32_t> sc(m);
    to_host(sc.data(), d.score, m, s, "stitch scores");
    check_sync(s, "stitch_sweep");
    st.sweep_ms += tm.ms(0, 1);
    st.trace_bytes += bt.trace;
    st.batches++;
    // the links to walk: neither dead nor low
    std::vector<TraceTask> wt;
    std::vector<size_t> widx;
    for (size_t k = 0; k < m; k++) {
        sa_stitch_link& l = C.lk[ids[k]];
        if (sc[k] <= STITCH_NEG / 2) {
            l.flags = SA_STITCH_DEAD;
            l.score = INT_MIN;
            continue;
        }
        l.score = C.li[ids[k]].score = sc[k];
        if (sc[k] < P.min_link_score) {
            l.flags = SA_STITCH_LOW;
            continue;
        }
        wt.push_back(bt.tasks[k]);
        widx.push_back(ids[k]);
    }
    if (!wt.empty()) walk_batch(sl, ga, d, bt.nops, wt, widx, C, tm, st);
}

// Sweep and walk of the links, instance by instance, in batches under option gapped_trace_mb.  ga: the walk's arguments but for max_band.
void sweep_links(Slot* sl, const StitchArgs& a, GappedArgs ga, const Params& P, Chains& C, sa_stitch_stats& st) {
    const Bins B = bin_links(C, st);
    Timer<3> tm(sl->stream, "stitch timing");
    TraceBatch bt;
    for (int b = 0; b < 5; b++) {
        ga.max_band = 64 * KS[b] - 1;
        for (size_t at = 0; at < B.tasks[b].size();) {
            const size_t e = bt.pack(B.tasks[b], at, ga.max_band);  // the batch: links ids[b][at .. e)
            sweep_batch(sl, a, ga, P, bt, B.ids[b].data() + at, C, tm, st);
            at = e;
        }
    }
}

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

// The record that starts at member entry k of chain c (entries [k, end)): its members and unbroken links in genome order up to the first
// broken link or the chain's end, its ops appended to out_ops.  k moves past the record's last member.
sa_stitch_record make_record(const Chains& C, size_t c, size_t begin, size_t end, size_t& k, std::vector<uint32_t>& out_ops) {
    sa_stitch_record r;
    memset(&r, 0, sizeof(r));
    r.chain = (uint32_t)c;
    r.first_member = (uint32_t)(k - begin);
    r.ref_start = C.mem[k].rs;
    r.query_start = C.mem[k].qs;
    r.op_offset = out_ops.size();
    Runs R;
    uint64_t matches = 0, mismatches = 0;
    for (;; k++) {
        R.add((uint64_t)C.mem[k].len + 1, SA_GAPPED_OP_M);
        r.score += C.mo[k].score;
        matches += C.mo[k].matches;
        mismatches += C.mo[k].mismatches;
        r.n_members++;
        r.ref_end = C.mem[k].rs + C.mem[k].len + 1;
        r.query_end = C.mem[k].qs + C.mem[k].len + 1;
        if (k + 1 == end) break;
        const sa_stitch_link& l = C.lk[C.link_of[k]];
        if (l.flags) {
            r.flags = l.flags;
            break;
        }
        const Link& x = C.li[C.link_of[k]];
        r.score += x.score;
        matches += x.matches;
        mismatches += x.mismatches;
        for (uint32_t y = x.n_runs; y-- > 0;) {  // the walk runs from (dt, dq) back: reversed is genome order
            const uint32_t o = C.runs[x.run_off + y];
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
    return r;
}

}  // namespace

extern "C" {

size_t sa_stitch_chains(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, const uint32_t* first, size_t n_chains, int rev,
                        uint32_t buffer, const sa_stitch_params* p, sa_stitch_record** records, uint32_t** ops, size_t* n_ops,
                        sa_stitch_link** links, size_t* n_links, sa_stitch_stats* stats) {
    const char* who = "StitchChains";
    *records = nullptr;
    *ops = nullptr;
    *n_ops = 0;
    if (links) *links = nullptr;
    if (n_links) *n_links = 0;
    sa_stitch_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_proc(who, buffer);
    const Params P = resolve(p);
    const size_t M = checked_first(fail, first, n_chains);
    if (M == 0) return 0;

    Slot* sl = acquire_slot();
    StitchArgs a;
    GappedArgs ga;  // of the walk; max_band is set per instance
    memset(&ga, 0, sizeof(ga));
    resident_block(who, sl, rev, buffer, a);
    resident_block(who, sl, rev, buffer, ga);
    a.gap_open = ga.gap_open = P.gap_open;
    a.gap_extend = ga.gap_extend = P.gap_extend;
    Chains C;
    C.mem = checked_members(hsps, n_hsps, members, M, a);
    make_links(C, first, n_chains, P);
    member_scores(sl, a, C, st);
    sweep_links(sl, a, ga, P, C, st);
    prof_flush(sl);
    release_slot(sl);

    // the records: every chain cut at its broken links
    std::vector<sa_stitch_record> rec;
    std::vector<uint32_t> out_ops;
    for (size_t c = 0; c < n_chains; c++)
        for (size_t k = first[c]; k < first[c + 1];) rec.push_back(make_record(C, c, first[c], first[c + 1], k, out_ops));
    st.links = C.lk.size();
    for (const sa_stitch_link& l : C.lk) {
        if (l.flags & SA_STITCH_LONG) st.long_links++;
        if (l.flags & SA_STITCH_DEAD) st.dead_links++;
        if (l.flags & SA_STITCH_LOW) st.low_links++;
    }
    st.records = rec.size();
    if (stats) *stats = st;
    *records = malloc_copy(rec, who);
    *ops = malloc_copy(out_ops, who);
    *n_ops = out_ops.size();
    if (links) *links = malloc_copy(C.lk, who);
    if (n_links) *n_links = C.lk.size();
    return rec.size();
}

void sa_free_stitch(sa_stitch_record* records, uint32_t* ops, sa_stitch_link* links) {
    free(records);
    free(ops);
    free(links);
}

}  // extern "C"
