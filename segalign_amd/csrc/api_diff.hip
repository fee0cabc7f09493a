// api_diff.hip -- C-ABI sa_diff_alignments: the differences, summaries and pair counts of alignments against the resident sequences
// (contract: include/segalign_amd.h).  The host side as steps: the checked spans; the prepare step (every op entry's span
// and the four prefix sums); the count pass with its two prefix sums and the summaries; the emit pass.
#include "post_host.h"
#include "diff.h"

using namespace sa;

namespace {

const Fail fail{"DiffAlignments"};

constexpr uint64_t MAX_ITEMS = (uint64_t)1 << 30;

// What the prepare step leaves in the slot's diff buffer beside a's arrays.
struct Prepared {
    uint64_t* pairs;  // zeroed
    uint64_t items;
};

// Fills a's spans, ops and prefix sums.
void prepare(Slot* sl, DiffArgs& a, const sa_diff_span* spans, size_t n, const uint32_t* ops, size_t N, Prepared& P, sa_diff_stats& st) {
    const hipStream_t s = sl->stream;
    sa_diff_span* d_spans;
    uint32_t *d_ops, *d_span_of, *d_val;
    uint64_t* sum[4];
    uint8_t* temp;
    carve(sl->diff, "diff", [&](Carve& c) {
        c.take(d_spans, n).take(d_ops, N).take(d_span_of, N).take(d_val, N);
        for (uint64_t*& x : sum) c.take(x, N + 1);
        c.take(temp, std::max<size_t>(scan_temp_bytes(N), 256)).take(P.pairs, 64);
    });
    Timer<2> tm(s, "diff timing");
    to_device(d_spans, spans, n, s, "diff spans");
    to_device(d_ops, ops, N, s, "diff ops");
    check_memcpy(hipMemsetAsync(P.pairs, 0, 64 * sizeof(uint64_t), s), "diff pairs");
    tm.mark(0);
    launch(sl, "diff_prepare", [&] {
        launch_diff_span_of(d_spans, (uint32_t)n, (uint32_t)N, d_span_of, s);
        for (int which = 0; which < 4; which++) {
            launch_diff_values(d_ops, d_span_of, (uint32_t)N, which, a.chunk_shift, d_val, s);
            launch_exclusive_scan_u64(d_val, sum[which], N, temp, s);
        }
    });
    tm.mark(1);
    P.items = read_u64(sum[3] + N, s, "diff items");
    st.prep_ms = (float)tm.ms(0, 1);
    a.spans = d_spans;
    a.n_spans = (uint32_t)n;
    a.ops = d_ops;
    a.n_ops = (uint32_t)N;
    a.tsum = sum[0];
    a.qsum = sum[1];
    a.csum = sum[2];
    a.isum = sum[3];
    a.span_of = d_span_of;
}

}  // namespace

extern "C" {

size_t sa_diff_alignments(const sa_diff_span* spans, size_t n, const uint32_t* ops, size_t n_ops_total, int rev, uint32_t buffer,
                          const sa_diff_params* p, sa_diff_event** events, sa_diff_summary** summaries, sa_diff_stats* stats) {
    const char* who = "DiffAlignments";
    *events = nullptr;
    *summaries = nullptr;
    sa_diff_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_proc(who, buffer);
    const uint32_t flags = p ? p->flags : 0, chunk = p ? p->chunk : 0;

    Slot* sl = acquire_slot();
    const hipStream_t s = sl->stream;
    DiffArgs a;
    memset(&a, 0, sizeof(a));
    resident_block(who, sl, rev, buffer, a);
    const SpanTotals tot = checked_spans(fail, spans, n, ops, n_ops_total, a.ref_len, a.query_len, flags, chunk);
    st.spans = n;
    st.ops = tot.ops;
    st.columns = tot.columns;
    sa_diff_summary* sum = host_alloc<sa_diff_summary>(n, who);
    if (n) memset(sum, 0, n * sizeof(sa_diff_summary));
    sa_diff_event* ev = nullptr;
    size_t n_ev = 0;
    if (tot.ops) {  // otherwise every span is empty
        a.chunk_shift = (uint32_t)__builtin_ctz(chunk ? chunk : DIFF_DEFAULT_CHUNK);
        a.per_base = (flags & SA_DIFF_PER_BASE) != 0;
        Prepared P;
        prepare(sl, a, spans, n, ops, n_ops_total, P, st);
        if (P.items > MAX_ITEMS) fail("%lld work items: at most 1 << 30 (raise chunk)", (long long)P.items);
        const size_t W = (size_t)P.items;
        st.work_items = W;

        uint32_t* d_item;
        uint32_t* cnt[7];
        uint64_t *d_so, *d_eo;
        sa_diff_summary* d_sum;
        uint8_t* temp;
        carve(sl->diff_items, "diff items", [&](Carve& c) {
            c.take(d_item, W);
            for (uint32_t*& x : cnt) c.take(x, W);
            c.take(d_so, W + 1).take(d_eo, W + 1).take(d_sum, n).take(temp, std::max<size_t>(scan_temp_bytes(W), 256));
        });
        const DiffCounts dc = {cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6]};
        Timer<4> tm(s, "diff timing");
        tm.mark(0);
        launch(sl, "diff_count", [&] {
            launch_diff_items(a.isum, a.n_ops, (uint32_t)W, d_item, s);
            launch_diff_count(a, d_item, (uint32_t)W, dc, P.pairs, s);
            launch_exclusive_scan_u64(dc.starts, d_so, W, temp, s);
            launch_exclusive_scan_u64(dc.ends, d_eo, W, temp, s);
            launch_diff_summaries(a, dc, d_so, d_sum, s);
        });
        tm.mark(1);
        uint64_t n_start = 0, n_end = 0;
        to_host(&n_start, d_so + W, 1, s, "diff events");
        to_host(&n_end, d_eo + W, 1, s, "diff event ends");
        to_host(sum, d_sum, n, s, "diff summaries");
        to_host(st.pairs, P.pairs, 64, s, "diff pairs");
        check_sync(s, "diff_count");
        st.count_ms = (float)tm.ms(0, 1);
        if (n_start != n_end) {
            fprintf(stderr, "Error: DiffAlignments: %llu event starts and %llu ends\n", (unsigned long long)n_start, (unsigned long long)n_end);
            exit(1);
        }
        if (n_start >= ((uint64_t)1 << 31)) fail("%lld events: fewer than 2^31 (SA_DIFF_NO_EVENTS leaves the summaries)", (long long)n_start);
        st.events = n_start;
        if (n_start && !(flags & SA_DIFF_NO_EVENTS)) {
            n_ev = (size_t)n_start;
            ev = host_alloc<sa_diff_event>(n_ev, who);
            sa_diff_event* d_ev;
            carve(sl->diff_out, "diff events", [&](Carve& c) { c.take(d_ev, n_ev); });
            tm.mark(2);
            launch(sl, "diff_emit", [&] {
                launch_diff_emit(a, d_item, (uint32_t)W, d_so, d_eo, d_ev, s);
                launch_diff_finish(d_ev, (uint32_t)n_ev, s);
            });
            tm.mark(3);
            to_host(ev, d_ev, n_ev, s, "diff events");
            check_sync(s, "diff_emit");
            st.emit_ms = (float)tm.ms(2, 3);
        }
    }
    prof_flush(sl);
    release_slot(sl);
    if (stats) *stats = st;
    *events = ev;
    *summaries = sum;
    return n_ev;
}

void sa_free_diff(sa_diff_event* events, sa_diff_summary* summaries) {
    free(events);
    free(summaries);
}

}  // extern "C"
