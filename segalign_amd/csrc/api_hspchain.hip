// api_hspchain.hip -- C-ABI sa_chain_hsps: the best collinear chain of every group of HSPs (contract: include/segalign_amd.h),
// and sa_chain_hsps_all: all chains of every group, peeled best first; sa_chain_hsps_costs and sa_chain_hsps_all_costs:
// the two under a piecewise-linear gap-cost table, which only hands the DP's launches the table's device image;
// sa_chain_hsps_ovl and sa_chain_hsps_all_ovl: the two under an overlap allowance, which makes the node weights and picks
// hspovl.hip's launchers for the DP.
// The host side: checks, the slot, rank (two stable radix sorts) and the tile loop (hspchain.hip: cross, resolve), shared by both; then
// sa_chain_hsps's finish (group starts, ends, members, nodes) or the peel (hsppeel.hip: subtree minimum, chain order, members), and the
// counts the kernels' work is reported by.
#include "post_host.h"  // and through it gapped.h: cover.hip's rocPRIM wrappers cover_sort_anchors, cover_scan_offsets
#include "hspchain.h"
#include "hspcost.h"
#include "hsppeel.h"

using namespace sa;

namespace {

void bad(const char* what, long long v) {
    fprintf(stderr, "Error: ChainHsps: %s = %lld out of range\n", what, v);
    exit(1);
}

// The events of one call: marks 0-1 span the rank step and 2-3 the DP (rank_and_dp), 4-7 the finish or the peel.
using ChainTimer = Timer<8>;

// What the rank step and the DP leave on the slot's stream, for the finish of sa_chain_hsps and the peel of sa_chain_hsps_all.
struct ChainDp {
    Slot* sl = nullptr;
    uint32_t N = 0, G = 0;
    sa_chain_params P = {0, 0, 0, 0, 0};
    HspChainArgs a;
    const uint32_t* order = nullptr;  // rank -> input index
    uint32_t *head = nullptr, *gstart = nullptr, *gend = nullptr, *glen = nullptr;  // head[r]: rank r starts a group
    uint64_t *gidx = nullptr, *goff = nullptr, *key_a = nullptr, *key_b = nullptr;
    uint32_t *idx_b = nullptr;  // free after the rank step, like key_a and key_b
    sa_chain_member* d_members = nullptr;
    sa_chain_node* d_nodes = nullptr;
    void* temp = nullptr;
    size_t temp_bytes = 0;
};

// The slot's buffers, the upload, rank and the DP (spans 0 and 1 of ev) for n > 0 HSPs on the slot d.sl.  Returns with the stream
// synchronised, G known and st's pair_evals and tile_steps counted.
// max_overlap != 0: the DP runs under the overlap allowance (hspovl.hip), on node weights made after the rank step.
void rank_and_dp(const sa_segment_pair* hsps, size_t n, const uint32_t* group, uint32_t T, const CostImage& costs, uint32_t max_overlap, ChainDp& d,
                 ChainTimer& ev, sa_chain_stats& st) {
    const uint32_t N = (uint32_t)n, tiles = (N + T - 1) / T;
    d.N = N;
    Slot* sl = d.sl;
    hipStream_t s = sl->stream;

    sa_segment_pair* d_hsps;
    uint32_t *d_group, *idx_a, *rs, *qs, *ln, *gr, *pred, *first, *d_image;
    int32_t* sc;
    int64_t *f, *ovl_w = nullptr;
    uint32_t* ovl_lim = nullptr;
    carve(sl->hspchain_work, "hsp chain", [&](Carve& c) {
        c.take(d_hsps, N).take(d_group, N).take(d.key_a, N).take(d.key_b, N).take(idx_a, N).take(d.idx_b, N);
        c.take(rs, N).take(qs, N).take(ln, N).take(gr, N).take(sc, N).take(f, N).take(pred, N);
        c.take(d.head, (size_t)N + 1).take(d.gidx, (size_t)N + 1).take(first, tiles);
        c.take(d.gstart, N).take(d.gend, N).take(d.glen, (size_t)N + 1).take(d.goff, (size_t)N + 1);
        c.take(d.d_members, N).take(d.d_nodes, N).take(d_image, HSPCOST_WORDS);
        if (max_overlap) c.take(ovl_w, N).take(ovl_lim, N);
    });
    sl->hspchain_partial.ensure((size_t)tiles * T * sizeof(HspChainPartial), "hsp chain partials");
    HspChainPartial* partial = (HspChainPartial*)sl->hspchain_partial.p;
    size_t sort_bytes = 0, scan_bytes = 0;
    cover_sort_anchors(nullptr, &sort_bytes, d.key_a, d.key_b, idx_a, d.idx_b, N, s);
    cover_scan_offsets(nullptr, &scan_bytes, d.head, d.gidx, N, s);
    d.temp_bytes = std::max(sort_bytes, scan_bytes);
    sl->hspchain_temp.ensure(std::max<size_t>(d.temp_bytes, 256), "hsp chain temp");
    void* temp = d.temp = sl->hspchain_temp.p;

    HspChainArgs& a = d.a;
    a.rs = rs; a.qs = qs; a.ln = ln; a.gr = gr; a.sc = sc; a.f = f; a.pred = pred;
    a.n = N;
    a.tile = T;
    a.diag_pen = d.P.diag_pen;
    a.anti_pen = d.P.anti_pen;
    a.max_gap = d.P.max_gap;
    const uint32_t* image = costs.on ? d_image : nullptr;  // picks the DP's instances, and the scope names they are profiled under

    to_device(d_hsps, hsps, n, s, "hsp chain: HSPs");
    d_group = upload(d_group, group, n, s, "hsp chain: groups");
    if (costs.on) check_memcpy(hipMemcpyAsync(d_image, costs.w, sizeof(costs.w), hipMemcpyHostToDevice, s), "hsp chain: gap costs");

    // rank: stable sort by (query_start, len) with the input index as value, then by (group, ref_start); idx_a ends up as rank -> input index
    std::vector<uint32_t> h_first(tiles);
    ev.mark(0);
    launch(sl, "hspchain_rank", [&] {
        launch_hspchain_key_minor(d_hsps, N, d.key_a, idx_a, s);
        cover_sort_anchors(temp, &d.temp_bytes, d.key_a, d.key_b, idx_a, d.idx_b, N, s);
        launch_hspchain_key_major(d_hsps, d_group, d.idx_b, N, d.key_a, s);
        cover_sort_anchors(temp, &d.temp_bytes, d.key_a, d.key_b, d.idx_b, idx_a, N, s);
        launch_hspchain_gather(d_hsps, d_group, idx_a, N, rs, qs, ln, sc, gr, d.head, s);
        launch_hspchain_first(gr, N, T, first, s);
        if (max_overlap) launch_hspovl_weight(a, max_overlap, ovl_w, ovl_lim, s);
    });
    ev.mark(1);
    to_host(h_first.data(), first, tiles, s, "hsp chain: first tiles");
    check_sync(s, "hspchain_rank");
    d.order = idx_a;

    // the DP: tile b after every tile before it
    const HspOvlNodes ovl = {ovl_w, ovl_lim};
    ev.mark(2);
    for (uint32_t b = 0; b < tiles; b++) {
        const uint32_t c0 = h_first[b], nb = std::min(T, N - b * T);
        if (c0 > b) {
            fprintf(stderr, "Error: ChainHsps: tile %u starts at tile %u\n", b, c0);
            exit(15);
        }
        if (b > c0) {
            ProfScope ps(sl, max_overlap ? "hspovl_cross" : image ? "hspcost_cross" : "hspchain_cross");
            if (max_overlap) launch_hspovl_cross(a, ovl, b, c0, partial, image, s);
            else launch_hspchain_cross(a, b, c0, partial, image, s);
        }
        {
            ProfScope ps(sl, max_overlap ? "hspovl_resolve" : image ? "hspcost_resolve" : "hspchain_resolve");
            if (max_overlap) launch_hspovl_resolve(a, ovl, b, c0, partial, image, s);
            else launch_hspchain_resolve(a, b, c0, partial, image, s);
        }
        check_launch("hspchain tile");
        st.pair_evals += (uint64_t)(b - c0) * T * nb + (uint64_t)nb * (nb - 1) / 2;
        st.tile_steps += (uint64_t)(b - c0) + 1;
    }
    cover_scan_offsets(temp, &d.temp_bytes, d.head, d.gidx, N, s);
    ev.mark(3);
    uint64_t groups64 = 0;
    to_host(&groups64, d.gidx + N, 1, s, "hsp chain: groups");
    check_sync(s, "hspchain tiles");
    d.G = (uint32_t)groups64;
}

// The checks both entries make before they touch the device.  Returns the tile.
uint32_t checked(const sa_chain_params* p, size_t n, sa_chain_params& P) {
    if (p) P = *p;
    if (P.diag_pen < 0 || P.diag_pen > (1 << 20)) bad("diag_pen", P.diag_pen);
    if (P.anti_pen < 0 || P.anti_pen > (1 << 20)) bad("anti_pen", P.anti_pen);
    if (n > HSPCHAIN_MAX_N) bad("the number of HSPs", (long long)n);
    const int64_t tile_opt = opt_value_now("chain_tile");
    if (tile_opt < 64 || tile_opt > 1024 || (tile_opt & (tile_opt - 1))) bad("option chain_tile", tile_opt);
    return (uint32_t)tile_opt;
}

// The allowance of a sa_chain_overlap, checked; nullptr is 0, the plain DP.
uint32_t checked_overlap(const sa_chain_overlap* ov) {
    if (!ov) return 0;
    if (ov->max_overlap > SA_CHAIN_MAX_OVERLAP) bad("max_overlap", ov->max_overlap);
    if (ov->reserved != 0) bad("reserved", ov->reserved);
    return ov->max_overlap;
}

size_t chain_hsps(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p, const sa_chain_gap_costs* g,
                  const sa_chain_overlap* ov, sa_chain_member** members, sa_chain_node** nodes, sa_chain_stats* stats) {
    *members = nullptr;
    if (nodes) *nodes = nullptr;
    sa_chain_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_init("ChainHsps");
    ChainDp d;
    const uint32_t T = checked(p, n, d.P);
    CostImage costs;
    checked_costs("ChainHsps", g, costs);
    const uint32_t max_overlap = checked_overlap(ov);
    if (n == 0) return 0;
    Slot* sl = d.sl = acquire_slot_early();
    hipStream_t s = sl->stream;
    ChainTimer ev(s, "hsp chain timing");
    rank_and_dp(hsps, n, group, T, costs, max_overlap, d, ev, st);
    const uint32_t G = d.G;

    // finish: every group's end and chain length, then the members and the nodes
    ev.mark(4);
    launch(sl, "hspchain_finish", [&] {
        launch_hspchain_group_starts(d.head, d.gidx, d.N, d.gstart, s);
        launch_hspchain_ends(d.a, d.gstart, G, d.P.min_score, d.gend, d.glen, s);
        cover_scan_offsets(d.temp, &d.temp_bytes, d.glen, d.goff, G, s);
    });
    ev.mark(5);
    uint64_t total = 0;
    to_host(&total, d.goff + G, 1, s, "hsp chain: members");
    check_sync(s, "hspchain_finish");
    ev.mark(6);
    launch(sl, "hspchain_finish", [&] {
        launch_hspchain_members(d.a, d.order, d.gend, d.glen, d.goff, G, d.d_members, s);
        if (nodes) launch_hspchain_nodes(d.a, d.order, d.d_nodes, s);
    });
    ev.mark(7);
    sa_chain_member* m_out = host_alloc<sa_chain_member>(total, "ChainHsps");
    sa_chain_node* n_out = nodes ? host_alloc<sa_chain_node>(n, "ChainHsps") : nullptr;
    to_host(m_out, d.d_members, total, s, "hsp chain: members");
    if (nodes) to_host(n_out, d.d_nodes, n, s, "hsp chain: nodes");
    check_sync(s, "hspchain_finish");
    st.kernel_ms = ev.ms(0, 1) + ev.ms(2, 3) + ev.ms(4, 5) + ev.ms(6, 7);
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

size_t chain_hsps_all(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p, const sa_chain_gap_costs* g,
                      const sa_chain_overlap* ov, sa_chain_record** chains, size_t* n_chains, sa_chain_all_member** members, sa_chain_node** nodes, uint32_t** chain_of,
                      sa_chain_all_stats* stats) {
    *chains = nullptr;
    *n_chains = 0;
    *members = nullptr;
    if (nodes) *nodes = nullptr;
    if (chain_of) *chain_of = nullptr;
    sa_chain_all_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_init("ChainHsps");
    ChainDp d;
    const uint32_t T = checked(p, n, d.P);
    CostImage costs;
    checked_costs("ChainHsps", g, costs);
    const uint32_t max_overlap = checked_overlap(ov);
    if (n == 0) return 0;
    Slot* sl = d.sl = acquire_slot_early();
    hipStream_t s = sl->stream;
    ChainTimer ev(s, "hsp chain timing");
    rank_and_dp(hsps, n, group, T, costs, max_overlap, d, ev, st.chain);
    const uint32_t N = d.N;

    HspPeelArgs a;
    a.f = d.a.f; a.pred = d.a.pred; a.gr = d.a.gr; a.order = d.order;
    a.n = N;
    a.min_score = d.P.min_score;
    a.key_a = d.key_a; a.key_b = d.key_b;  // free since the rank step
    carve(sl->hsppeel_work, "hsp peel", [&](Carve& c) {
        c.take(a.idx_a, N).take(a.idx_b, N).take(a.byprio, N).take(a.val, N).take(a.ptr_a, N).take(a.ptr_b, N).take(a.head, N);
        c.take(a.cscore, N).take(a.cjoin, N).take(a.corder, N).take(a.cpos, N).take(a.keep, (size_t)N + 1).take(a.kidx, (size_t)N + 1);
        c.take(a.khead, N).take(a.first, (size_t)N + 1).take(a.tot, 3).take(a.chains, N).take(a.members, N).take(a.chain_of, N);
    });
    uint32_t rounds = 1;
    while (rounds < 32 && ((uint64_t)1 << rounds) < N) rounds++;  // max(1, ceil(log2 n)): a pred walk has fewer than n links

    ev.mark(4);
    launch(sl, "hsppeel_subtree", [&] {
        launch_hsppeel_prio_key(a, s);
        cover_sort_anchors(d.temp, &d.temp_bytes, a.key_a, a.key_b, a.idx_a, a.byprio, N, s);  // stable: equal f stay in rank order
        launch_hsppeel_init(a, s);
        const uint32_t* ptr = a.pred;
        for (uint32_t k = 0; k < rounds; k++) {
            uint32_t* next = (k & 1) ? a.ptr_b : a.ptr_a;
            launch_hsppeel_round(a, ptr, next, s);
            ptr = next;
        }
        launch_hsppeel_tails(a, s);
    });
    ev.mark(5);  // ends the subtree span and starts the order span: nothing is enqueued between the two
    launch(sl, "hsppeel_order", [&] {
        // the chains by (group, score descending, head rank): the minor sort starts from rank order, both sorts are stable
        launch_hsppeel_chain_key_minor(a, s);
        cover_sort_anchors(d.temp, &d.temp_bytes, a.key_a, a.key_b, a.idx_a, a.idx_b, N, s);
        launch_hsppeel_chain_key_major(a, a.idx_b, s);
        cover_sort_anchors(d.temp, &d.temp_bytes, a.key_a, a.key_b, a.idx_b, a.corder, N, s);
        launch_hsppeel_keep(a, s);
        cover_scan_offsets(d.temp, &d.temp_bytes, a.keep, a.kidx, N, s);
        launch_hsppeel_assign(a, s);
    });
    ev.mark(6);  // likewise for the order and the members span
    launch(sl, "hsppeel_members", [&] {
        // the nodes by chain: they start in rank order, so the stable sort leaves a chain's members in rank order
        launch_hsppeel_node_key(a, s);
        cover_sort_anchors(d.temp, &d.temp_bytes, a.key_a, a.key_b, a.idx_a, a.idx_b, N, s);
        launch_hsppeel_members(a, a.key_b, a.idx_b, s);
        launch_hsppeel_records(a, s);
        if (nodes) launch_hspchain_nodes(d.a, d.order, d.d_nodes, s);
    });
    ev.mark(7);
    uint64_t tot[3] = {0, 0, 0};
    to_host(tot, a.tot, 3, s, "hsp peel: totals");
    check_sync(s, "hsppeel");
    const size_t K = (size_t)tot[0], M = (size_t)tot[1];
    if (K > n || M > n || K > M || tot[2] < K || tot[2] > n) {
        fprintf(stderr, "Error: ChainHsps: %llu chains of %llu with %llu members from %zu HSPs\n", (unsigned long long)tot[0],
                (unsigned long long)tot[2], (unsigned long long)tot[1], n);
        exit(15);
    }
    sa_chain_record* c_out = host_alloc<sa_chain_record>(K, "ChainHsps");
    sa_chain_all_member* m_out = host_alloc<sa_chain_all_member>(M, "ChainHsps");
    sa_chain_node* n_out = nodes ? host_alloc<sa_chain_node>(n, "ChainHsps") : nullptr;
    uint32_t* o_out = chain_of ? host_alloc<uint32_t>(n, "ChainHsps") : nullptr;
    to_host(c_out, a.chains, K, s, "hsp peel: chains");
    to_host(m_out, a.members, M, s, "hsp peel: members");
    if (nodes) to_host(n_out, d.d_nodes, n, s, "hsp peel: nodes");
    if (chain_of) to_host(o_out, a.chain_of, n, s, "hsp peel: chain_of");
    check_sync(s, "hsppeel");
    st.chain.kernel_ms = ev.ms(0, 1) + ev.ms(2, 3);
    st.peel_ms = ev.ms(4, 5) + ev.ms(5, 6) + ev.ms(6, 7);
    prof_flush(sl);
    release_slot(sl);

    st.chain.hsps = n;
    st.chain.groups = d.G;
    st.chain.chains = K;
    st.chain.members = M;
    st.chains_all = tot[2];
    st.peel_rounds = rounds;
    for (size_t k = 0; k < K; k++)
        if (c_out[k].joined >= 0) st.joined++;
    if (stats) *stats = st;
    *chains = c_out;
    *n_chains = K;
    *members = m_out;
    if (nodes) *nodes = n_out;
    if (chain_of) *chain_of = o_out;
    return M;
}

// The two tables axtChain's usage text prints for -linearGap; q_gap = t_gap in both.
const uint32_t PRESET_POS[11] = {1, 2, 3, 11, 111, 2111, 12111, 32111, 72111, 152111, 252111};
const int64_t PRESET_LOOSE[2][11] = {{325, 360, 400, 450, 600, 1100, 3600, 7600, 15600, 31600, 56600},
                                     {625, 660, 700, 750, 900, 1400, 4000, 8000, 16000, 32000, 57000}};
const int64_t PRESET_MEDIUM[2][11] = {{350, 425, 450, 600, 900, 2900, 22900, 57900, 117900, 217900, 317900},
                                      {750, 825, 850, 1000, 1300, 3300, 23300, 58300, 118300, 218300, 318300}};

}  // namespace

extern "C" {

size_t sa_chain_hsps(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p, sa_chain_member** members,
                     sa_chain_node** nodes, sa_chain_stats* stats) {
    return chain_hsps(hsps, n, group, p, nullptr, nullptr, members, nodes, stats);
}

size_t sa_chain_hsps_costs(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p,
                           const sa_chain_gap_costs* g, sa_chain_member** members, sa_chain_node** nodes, sa_chain_stats* stats) {
    return chain_hsps(hsps, n, group, p, g, nullptr, members, nodes, stats);
}

size_t sa_chain_hsps_ovl(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p, const sa_chain_gap_costs* g,
                         const sa_chain_overlap* ov, sa_chain_member** members, sa_chain_node** nodes, sa_chain_stats* stats) {
    return chain_hsps(hsps, n, group, p, g, ov, members, nodes, stats);
}

void sa_free_chain(sa_chain_member* members, sa_chain_node* nodes) {
    free(members);
    free(nodes);
}

size_t sa_chain_hsps_all(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p, sa_chain_record** chains,
                         size_t* n_chains, sa_chain_all_member** members, sa_chain_node** nodes, uint32_t** chain_of,
                         sa_chain_all_stats* stats) {
    return chain_hsps_all(hsps, n, group, p, nullptr, nullptr, chains, n_chains, members, nodes, chain_of, stats);
}

size_t sa_chain_hsps_all_costs(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p,
                               const sa_chain_gap_costs* g, sa_chain_record** chains, size_t* n_chains, sa_chain_all_member** members,
                               sa_chain_node** nodes, uint32_t** chain_of, sa_chain_all_stats* stats) {
    return chain_hsps_all(hsps, n, group, p, g, nullptr, chains, n_chains, members, nodes, chain_of, stats);
}

size_t sa_chain_hsps_all_ovl(const sa_segment_pair* hsps, size_t n, const uint32_t* group, const sa_chain_params* p,
                             const sa_chain_gap_costs* g, const sa_chain_overlap* ov, sa_chain_record** chains, size_t* n_chains,
                             sa_chain_all_member** members, sa_chain_node** nodes, uint32_t** chain_of, sa_chain_all_stats* stats) {
    return chain_hsps_all(hsps, n, group, p, g, ov, chains, n_chains, members, nodes, chain_of, stats);
}

int sa_chain_gap_preset(const char* name, sa_chain_gap_costs* out) {
    const int64_t (*t)[11] = !name ? nullptr : !strcmp(name, "loose") ? PRESET_LOOSE : !strcmp(name, "medium") ? PRESET_MEDIUM : nullptr;
    if (!t || !out) return -1;
    memset(out, 0, sizeof(*out));
    out->n = 11;
    for (int k = 0; k < 11; k++) {
        out->pos[k] = PRESET_POS[k];
        out->q_gap[k] = out->t_gap[k] = t[0][k];
        out->both_gap[k] = t[1][k];
    }
    return 0;
}

void sa_free_chain_all(sa_chain_record* chains, sa_chain_all_member* members, sa_chain_node* nodes, uint32_t* chain_of) {
    free(chains);
    free(members);
    free(nodes);
    free(chain_of);
}

}  // extern "C"
