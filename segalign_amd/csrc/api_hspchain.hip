// api_hspchain.hip -- C-ABI sa_chain_hsps: the best collinear chain of every group of HSPs (contract: include/segalign_amd.h).
// The host side: checks, the slot, rank (two stable radix sorts), the tile loop (hspchain.hip: cross, resolve), finish (group starts, ends,
// members, nodes) and the counts the kernels' work is reported by.
#include "engine_internal.h"
#include "gapped.h"  // cover.hip's rocPRIM wrappers: cover_sort_anchors, cover_scan_offsets
#include "hspchain.h"

using namespace sa;

namespace {

void bad(const char* what, long long v) {
    fprintf(stderr, "Error: ChainHsps: %s = %lld out of range\n", what, v);
    exit(1);
}

struct Take {  // 256-byte-aligned pieces of one buffer: sized with base == nullptr, then laid out
    uint8_t* base;
    size_t end = 0;
    template <typename T>
    void operator()(T*& p, size_t n) {
        const size_t at = (end + 255) & ~(size_t)255;
        end = at + n * sizeof(T);
        p = base ? (T*)(base + at) : nullptr;
    }
};

struct Events {  // pairs of events on the slot's stream: span k runs from mark(2 k) to mark(2 k + 1)
    static constexpr int N = 8;
    hipStream_t s;
    hipEvent_t e[N];
    explicit Events(hipStream_t st) : s(st) {
        for (hipEvent_t& x : e) ok(hipEventCreate(&x));
    }
    ~Events() {
        for (hipEvent_t x : e) hipEventDestroy(x);
    }
    void mark(int i) { ok(hipEventRecord(e[i], s)); }
    double total() {  // after the stream has been synchronised
        double ms = 0;
        for (int k = 0; k < N; k += 2) {
            float x = 0;
            ok(hipEventElapsedTime(&x, e[k], e[k + 1]));
            ms += x;
        }
        return ms;
    }
    static void ok(hipError_t r) {
        if (r != hipSuccess) die(15, "event", "hsp chain timing", r);
    }
};

}  // namespace

extern "C" {

size_t sa_chain_hsps(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p, sa_chain_member** members,
                     sa_chain_node** nodes, sa_chain_stats* stats) {
    *members = nullptr;
    if (nodes) *nodes = nullptr;
    sa_chain_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_init("ChainHsps");
    sa_chain_params P = {0, 0, 0, 0, 0};
    if (p) P = *p;
    if (P.diag_pen < 0 || P.diag_pen > (1 << 20)) bad("diag_pen", P.diag_pen);
    if (P.anti_pen < 0 || P.anti_pen > (1 << 20)) bad("anti_pen", P.anti_pen);
    if (n > HSPCHAIN_MAX_N) bad("the number of HSPs", (long long)n);
    const int64_t tile_opt = opt_value_now("chain_tile");
    if (tile_opt < 64 || tile_opt > 1024 || (tile_opt & (tile_opt - 1))) bad("option chain_tile", tile_opt);
    if (n == 0) return 0;
    const uint32_t N = (uint32_t)n, T = (uint32_t)tile_opt, tiles = (N + T - 1) / T;

    Slot* sl = acquire_slot_early();
    hipStream_t s = sl->stream;

    sa_segment_pair* d_hsps;
    uint32_t *d_group, *idx_a, *idx_b, *rs, *qs, *ln, *gr, *pred, *head, *first, *gstart, *gend, *glen;
    int32_t* sc;
    uint64_t *key_a, *key_b, *gidx, *goff;
    int64_t* f;
    sa_chain_member* d_members;
    sa_chain_node* d_nodes;
    auto layout = [&](Take& t) {
        t(d_hsps, N); t(d_group, N); t(key_a, N); t(key_b, N); t(idx_a, N); t(idx_b, N);
        t(rs, N); t(qs, N); t(ln, N); t(gr, N); t(sc, N); t(f, N); t(pred, N);
        t(head, (size_t)N + 1); t(gidx, (size_t)N + 1); t(first, tiles);
        t(gstart, N); t(gend, N); t(glen, (size_t)N + 1); t(goff, (size_t)N + 1);
        t(d_members, N); t(d_nodes, N);
    };
    {
        Take size{nullptr};
        layout(size);
        sl->hspchain_work.ensure(size.end, "hsp chain");
        Take t{sl->hspchain_work.p};
        layout(t);
    }
    if (!group) d_group = nullptr;
    sl->hspchain_partial.ensure((size_t)tiles * T * sizeof(HspChainPartial), "hsp chain partials");
    HspChainPartial* partial = (HspChainPartial*)sl->hspchain_partial.p;
    size_t sort_bytes = 0, scan_bytes = 0;
    cover_sort_anchors(nullptr, &sort_bytes, key_a, key_b, idx_a, idx_b, N, s);
    cover_scan_offsets(nullptr, &scan_bytes, head, gidx, N, s);
    size_t temp_bytes = std::max(sort_bytes, scan_bytes);
    sl->hspchain_temp.ensure(std::max<size_t>(temp_bytes, 256), "hsp chain temp");
    void* temp = sl->hspchain_temp.p;

    HspChainArgs a;
    a.rs = rs; a.qs = qs; a.ln = ln; a.gr = gr; a.sc = sc; a.f = f; a.pred = pred;
    a.n = N;
    a.tile = T;
    a.diag_pen = P.diag_pen;
    a.anti_pen = P.anti_pen;
    a.max_gap = P.max_gap;

    check_memcpy(hipMemcpyAsync(d_hsps, hsps, n * sizeof(sa_segment_pair), hipMemcpyHostToDevice, s), "hsp chain: HSPs");
    if (group) check_memcpy(hipMemcpyAsync(d_group, group, n * sizeof(uint32_t), hipMemcpyHostToDevice, s), "hsp chain: groups");
    Events ev(s);

    // rank: stable sort by (query_start, len) with the input index as value, then by (group, ref_start); idx_a ends up as rank -> input index
    std::vector<uint32_t> h_first(tiles);
    ev.mark(0);
    {
        ProfScope ps(sl, "hspchain_rank");
        launch_hspchain_key_minor(d_hsps, N, key_a, idx_a, s);
        cover_sort_anchors(temp, &temp_bytes, key_a, key_b, idx_a, idx_b, N, s);
        launch_hspchain_key_major(d_hsps, d_group, idx_b, N, key_a, s);
        cover_sort_anchors(temp, &temp_bytes, key_a, key_b, idx_b, idx_a, N, s);
        launch_hspchain_gather(d_hsps, d_group, idx_a, N, rs, qs, ln, sc, gr, head, s);
        launch_hspchain_first(gr, N, T, first, s);
        check_launch("hspchain_rank");
    }
    ev.mark(1);
    check_memcpy(hipMemcpyAsync(h_first.data(), first, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, s), "hsp chain: first tiles");
    check_sync(s, "hspchain_rank");
    const uint32_t* order = idx_a;

    // the DP: tile b after every tile before it
    ev.mark(2);
    for (uint32_t b = 0; b < tiles; b++) {
        const uint32_t c0 = h_first[b], nb = std::min(T, N - b * T);
        if (c0 > b) {
            fprintf(stderr, "Error: ChainHsps: tile %u starts at tile %u\n", b, c0);
            exit(15);
        }
        if (b > c0) {
            ProfScope ps(sl, "hspchain_cross");
            launch_hspchain_cross(a, b, c0, partial, s);
        }
        {
            ProfScope ps(sl, "hspchain_resolve");
            launch_hspchain_resolve(a, b, c0, partial, s);
        }
        check_launch("hspchain tile");
        st.pair_evals += (uint64_t)(b - c0) * T * nb + (uint64_t)nb * (nb - 1) / 2;
        st.tile_steps += (uint64_t)(b - c0) + 1;
    }
    cover_scan_offsets(temp, &temp_bytes, head, gidx, N, s);
    ev.mark(3);
    uint64_t groups64 = 0;
    check_memcpy(hipMemcpyAsync(&groups64, gidx + N, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "hsp chain: groups");
    check_sync(s, "hspchain tiles");
    const uint32_t G = (uint32_t)groups64;

    // finish: every group's end and chain length, then the members and the nodes
    ev.mark(4);
    {
        ProfScope ps(sl, "hspchain_finish");
        launch_hspchain_group_starts(head, gidx, N, gstart, s);
        launch_hspchain_ends(a, gstart, G, P.min_score, gend, glen, s);
        cover_scan_offsets(temp, &temp_bytes, glen, goff, G, s);
        check_launch("hspchain_finish");
    }
    ev.mark(5);
    uint64_t total = 0;
    check_memcpy(hipMemcpyAsync(&total, goff + G, sizeof(uint64_t), hipMemcpyDeviceToHost, s), "hsp chain: members");
    check_sync(s, "hspchain_finish");
    ev.mark(6);
    {
        ProfScope ps(sl, "hspchain_finish");
        launch_hspchain_members(a, order, gend, glen, goff, G, d_members, s);
        if (nodes) launch_hspchain_nodes(a, order, d_nodes, s);
        check_launch("hspchain_finish");
    }
    ev.mark(7);
    sa_chain_member* m_out = total ? (sa_chain_member*)malloc(total * sizeof(sa_chain_member)) : nullptr;
    sa_chain_node* n_out = nodes ? (sa_chain_node*)malloc(n * sizeof(sa_chain_node)) : nullptr;
    if ((total && !m_out) || (nodes && !n_out)) {
        fprintf(stderr, "Error: ChainHsps: out of host memory\n");
        exit(12);
    }
    if (total) check_memcpy(hipMemcpyAsync(m_out, d_members, total * sizeof(sa_chain_member), hipMemcpyDeviceToHost, s), "hsp chain: members");
    if (nodes) check_memcpy(hipMemcpyAsync(n_out, d_nodes, n * sizeof(sa_chain_node), hipMemcpyDeviceToHost, s), "hsp chain: nodes");
    check_sync(s, "hspchain_finish");
    st.kernel_ms = ev.total();
    prof_flush(sl);
    release_slot(sl);

    st.hsps = n;
    st.groups = G;
    st.members = total;
    for (uint64_t k = 0; k < total; k++)
        if (k == 0 || m_out[k].group != m_out[k - 1].group) st.chains++;
    if (stats) *stats = st;
    *members = m_out;
    if (nodes) *nodes = n_out;
    return (size_t)total;
}

void sa_free_chain(sa_chain_member* members, sa_chain_node* nodes) {
    free(members);
    free(nodes);
}

}  // extern "C"
