// api_netsubset.hip -- C-ABI sa_net_subset: every fill of a net as sub-chains of its chain, clipped to the fill, rescored and ready to
// stitch (contract: include/segalign_amd.h).  The host side: the validation pass over the CSR and the fills, the slot and
// its one buffer, the kernels of netsubset.hip with the prefix sums of scan.hip between them, one read-back of the two counts that size
// the last launches, and the copy of the results.
#include "post_host.h"
#include "netsubset.h"

using namespace sa;

namespace {

const char* const WHO = "NetSubset";

const Fail fail{"NetSubset"};
static_assert(NETSUBSET_MAX_MEMBERS == POST_MAX_MEMBERS, "checked_first holds the members to the limit netsubset.hip's kernels are written for");

struct Span {  // a member's block on the axis
    uint64_t s, e;
};

Span span_of(const sa_segment_pair& h, int axis) {
    const uint64_t s = axis ? h.query_start : h.ref_start;
    return {s, s + h.len + 1};
}

// The CSR rules of sa_stitch_chains; returns the HSP of every member entry, in member order.
std::vector<sa_segment_pair> checked_members(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, const uint32_t* first,
                                             size_t n_chains, const NetSubsetArgs& a) {
    const size_t M = checked_first(fail, first, n_chains);
    std::vector<sa_segment_pair> mh(M);
    for (size_t k = 0; k < M; k++) mh[k] = checked_member(fail, hsps, n_hsps, members, k, a.ref_len, a.query_len);
    for (size_t c = 0; c < n_chains; c++)
        for (size_t k = first[c]; k + 1 < first[c + 1]; k++) {
            const sa_segment_pair &x = mh[k], &y = mh[k + 1];
            if ((uint64_t)x.ref_start + x.len + 1 > y.ref_start || (uint64_t)x.query_start + x.len + 1 > y.query_start)
                fail("chain %lld: the member at position %lld does not end before the next one starts", (long long)c, (long long)(k - first[c]));
        }
    return mh;
}

struct Counts {
    uint64_t out = 0, cut = 0, bases = 0;
};

// The rules of the fills; counts the output members, the cut ones and their kept columns.
Counts checked_fills(const sa_net_fill* fills, size_t F, const std::vector<sa_segment_pair>& mh, const uint32_t* first, size_t n_chains, int axis) {
    Counts n;
    for (size_t k = 0; k < F; k++) {
        const sa_net_fill& f = fills[k];
        checked_fill_in_chain(fail, f, k, first, n_chains);
        const Span b0 = span_of(mh[f.first_block], axis), b1 = span_of(mh[f.first_block + f.n_blocks - 1], axis);
        if (b0.e <= f.start || b1.s >= f.end) fail("fill %lld: its first block ends before its start or its last block starts after its end", (long long)k);
        n.out += f.n_blocks;
        if (n.out > NETSUBSET_MAX_OUT) fail("more than 1 << 26 output members at fill %lld", (long long)k);
        // the cut members: the first block on the left, the last on the right, one block on both sides
        const bool left = b0.s < f.start, right = b1.e > f.end;
        if (f.n_blocks == 1) {
            if (left || right) {
                n.cut++;
                n.bases += std::min<uint64_t>(b0.e, f.end) - std::max<uint64_t>(b0.s, f.start);
            }
        } else {
            if (left) {
                n.cut++;
                n.bases += b0.e - f.start;
            }
            if (right) {
                n.cut++;
                n.bases += f.end - b1.s;
            }
        }
        if (f.parent == -1) continue;
        if (f.parent < 0 || (size_t)f.parent >= k) fail("fill %lld: parent %lld is neither -1 nor an earlier fill", (long long)k, f.parent);
        // inside a gap of the parent: the last of its blocks 0 .. n_blocks - 2 that ends at or before start, and the block after it
        const sa_net_fill& P = fills[f.parent];
        bool inside = false;
        if (P.n_blocks >= 2 && std::min<uint64_t>(span_of(mh[P.first_block], axis).e, P.end) <= f.start) {
            uint32_t lo = 0, hi = P.n_blocks - 1;
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (std::min<uint64_t>(span_of(mh[P.first_block + mid], axis).e, P.end) <= f.start) lo = mid;
                else hi = mid;
            }
            inside = f.end <= std::max<uint64_t>(span_of(mh[P.first_block + lo + 1], axis).s, P.start);
        }
        if (!inside) fail("fill %lld does not lie in a gap of its parent %lld", (long long)k, f.parent);
    }
    return n;
}

}  // namespace

extern "C" {

size_t sa_net_subset(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, const uint32_t* first, size_t n_chains,
                     const sa_net_fill* fills, size_t n_fills, int axis, int rev, uint32_t buffer, const sa_chain_params* p,
                     const sa_chain_gap_costs* g, uint32_t flags, sa_segment_pair** out_hsps, size_t* n_out, sa_subset_chain** chains,
                     sa_subset_stats* stats) {
    *out_hsps = nullptr;
    *n_out = 0;
    *chains = nullptr;
    sa_subset_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_proc(WHO, buffer);
    if (axis != 0 && axis != 1) fail("axis = %lld: 0 (target) or 1 (query)", axis);
    if (flags > SA_SUBSET_SPLIT) fail("flags = %lld: SA_SUBSET_SPLIT or 0", flags);
    const int32_t diag_pen = p ? p->diag_pen : 0, anti_pen = p ? p->anti_pen : 0;
    if (diag_pen < 0 || diag_pen > (1 << 20)) fail("diag_pen = %lld out of range", diag_pen);
    if (anti_pen < 0 || anti_pen > (1 << 20)) fail("anti_pen = %lld out of range", anti_pen);
    CostImage costs;
    checked_costs(WHO, g, costs);
    if (n_fills > NETSUBSET_MAX_FILLS) fail("%lld fills: at most 2^31 - 1", (long long)n_fills);

    Slot* sl = acquire_slot();
    const hipStream_t s = sl->stream;
    NetSubsetArgs a;
    memset(&a, 0, sizeof(a));
    resident_block(WHO, sl, rev, buffer, a);
    const std::vector<sa_segment_pair> mh = checked_members(hsps, n_hsps, members, first, n_chains, a);
    const Counts n = checked_fills(fills, n_fills, mh, first, n_chains, axis);
    if (n_fills == 0) {
        release_slot(sl);
        return 0;
    }
    const uint32_t F = (uint32_t)n_fills, M = (uint32_t)mh.size(), N = (uint32_t)n.out;
    a.F = F;
    a.M = M;
    a.N = N;
    a.axis = (uint32_t)axis;
    a.diag_pen = diag_pen;
    a.anti_pen = anti_pen;

    // one buffer for the whole call: the run arrays take their upper bound, N runs, so nothing grows between the launches
    sa_net_fill* d_fills;
    sa_segment_pair* d_mh;
    uint32_t* d_image;
    uint8_t* temp;
    const size_t temp_bytes = std::max<size_t>(scan_temp_bytes(std::max(F, N)), 256);
    carve(sl->netsubset, "net subset", [&](Carve& c) {
        c.take(d_fills, F).take(d_mh, M).take(d_image, HSPCOST_WORDS).take(a.cnt, F).take(a.off, (size_t)F + 1);
        c.take(a.mark, N).take(a.fill_of, N).take(a.side, N).take(a.head, N).take(a.run, (size_t)N + 1);
        c.take(a.is_cut, N).take(a.cut_at, (size_t)N + 1).take(a.cut_list, N).take(a.out, N).take(a.score, N);
        c.take(a.lo, N).take(a.hi, N).take(a.sum_lo, (size_t)N + 1).take(a.sum_hi, (size_t)N + 1);
        c.take(a.run_start, (size_t)N + 1).take(a.chains, N).take(temp, temp_bytes);
    });
    a.fills = d_fills;
    a.mh = d_mh;
    a.image = costs.on ? d_image : nullptr;

    Timer<4> ev(s, "net subset timing");  // 0-1 up to the counts, 2-3 the rest
    to_device(d_fills, fills, F, s, "net subset: fills");
    to_device(d_mh, mh.data(), M, s, "net subset: members");
    if (costs.on) check_memcpy(hipMemcpyAsync(d_image, costs.w, sizeof(costs.w), hipMemcpyHostToDevice, s), "net subset: gap costs");
    ev.mark(0);
    launch(sl, "netsubset_offsets", [&] {
        launch_netsubset_counts(a, s);
        launch_exclusive_scan_u64(a.cnt, a.off, F, temp, s);
    });
    check_memcpy(hipMemsetAsync(a.mark, 0, (size_t)N * sizeof(uint32_t), s), "net subset: marks");
    if (flags & SA_SUBSET_SPLIT) launch(sl, "netsubset_mark", [&] { launch_netsubset_mark(a, s); });
    launch(sl, "netsubset_emit", [&] {
        launch_netsubset_emit(a, s);
        launch_exclusive_scan_u64(a.head, a.run, N, temp, s);
        launch_exclusive_scan_u64(a.is_cut, a.cut_at, N, temp, s);
        launch_netsubset_cut_list(a, s);
    });
    ev.mark(1);
    uint64_t runs64 = 0, cut64 = 0;
    to_host(&runs64, a.run + N, 1, s, "net subset: runs");
    to_host(&cut64, a.cut_at + N, 1, s, "net subset: cut members");
    check_sync(s, "netsubset_emit");
    if (runs64 < F || runs64 > N || cut64 != n.cut) {
        fprintf(stderr, "Error: NetSubset: %llu runs and %llu cut members from %u fills, %u members and %llu cut members\n",
                (unsigned long long)runs64, (unsigned long long)cut64, F, N, (unsigned long long)n.cut);
        exit(15);
    }
    const uint32_t R = (uint32_t)runs64;
    ev.mark(2);
    launch(sl, "netsubset_rescore", [&] { launch_netsubset_rescore(a, (uint32_t)cut64, s); });
    launch(sl, "netsubset_chains", [&] {
        launch_netsubset_terms(a, s);
        launch_exclusive_scan_u64(a.lo, a.sum_lo, N, temp, s);
        launch_exclusive_scan_u64(a.hi, a.sum_hi, N, temp, s);
        launch_netsubset_chains(a, R, s);
    });
    ev.mark(3);
    sa_segment_pair* out = host_alloc<sa_segment_pair>(N, WHO);
    sa_subset_chain* rec = host_alloc<sa_subset_chain>(R, WHO);
    to_host(out, a.out, N, s, "net subset: output HSPs");
    to_host(rec, a.chains, R, s, "net subset: sub-chains");
    check_sync(s, "netsubset_chains");
    st.subset_ms = ev.ms(0, 1) + ev.ms(2, 3);
    prof_flush(sl);
    release_slot(sl);

    st.fills = F;
    st.runs = R;
    st.members = N;
    st.cut_members = n.cut;
    st.bases_rescored = n.bases;
    st.splits = R - F;
    if (stats) *stats = st;
    *out_hsps = out;
    *n_out = N;
    *chains = rec;
    return R;
}

void sa_free_net_subset(sa_segment_pair* out_hsps, sa_subset_chain* chains) {
    free(out_hsps);
    free(chains);
}

}  // extern "C"
