// api_net.hip -- C-ABI sa_net_chains: the chains of every group netted into fills and gaps on one axis (contract: include/segalign_amd.h,
// DESIGN.md 19).  The host side: the linear validation pass, the slot, the prepare step (priority order, hulls, group ranges, prefix sums),
// the level-synchronous rounds (net.hip: search, count, one scan, one read-back of two totals, emit) and the final order of the fills.
#include "post_host.h"  // and through it gapped.h: cover.hip's rocPRIM wrapper cover_sort_anchors, cover_scan_offsets
#include "net.h"

using namespace sa;

namespace {

void bad(const char* what, long long v) {
    fprintf(stderr, "Error: NetChains: %s = %lld out of range\n", what, v);
    exit(1);
}

void bad_at(const char* what, size_t chain, size_t block) {
    fprintf(stderr, "Error: NetChains: %s (chain %zu, block %zu)\n", what, chain, block);
    exit(1);
}

// The checks made before the device is touched, in one pass over first[] and the blocks.  Returns the number of blocks.
uint32_t checked(const uint32_t* first, const uint32_t* bs, const uint32_t* be, size_t n, const sa_net_params* p, sa_net_params& P) {
    if (p) P = *p;
    if (P.min_space > NET_TOP) bad("min_space", P.min_space);
    if (P.min_fill > NET_TOP) bad("min_fill", P.min_fill);
    if (!P.min_space) P.min_space = 1;
    if (!P.min_fill) P.min_fill = 1;
    if (n > NET_MAX_CHAINS) bad("the number of chains", (long long)n);
    if (n == 0) return 0;
    if (first[0] != 0) bad("first[0]", first[0]);
    for (size_t c = 0; c < n; c++) {
        if (first[c + 1] < first[c]) bad_at("first[] decreases", c, first[c + 1]);
        if (first[c + 1] > NET_MAX_BLOCKS) bad("the number of blocks", first[c + 1]);
        for (size_t k = first[c]; k < first[c + 1]; k++) {
            if (bs[k] >= be[k]) bad_at("a block with start >= end", c, k);
            if (be[k] >= NET_TOP) bad_at("a block that ends at or past 2^31", c, k);
            if (k > first[c] && be[k - 1] > bs[k]) bad_at("blocks of a chain that overlap or descend", c, k);
        }
    }
    return first[n];
}

}  // namespace

extern "C" {

size_t sa_net_chains(const uint32_t* first, const uint32_t* block_start, const uint32_t* block_end, const int64_t* score,
                     const uint32_t* group, size_t n_chains, const sa_net_params* p, sa_net_fill** fills, sa_net_stats* stats) {
    *fills = nullptr;
    sa_net_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_init("NetChains");
    sa_net_params P = {1, 1};
    const uint32_t B = checked(first, block_start, block_end, n_chains, p, P);
    if (n_chains == 0) return 0;
    const uint32_t N = (uint32_t)n_chains;
    Slot* sl = acquire_slot_early();
    hipStream_t s = sl->stream;
    Timer<4> ev(s, "net timing");  // 0-1 the prepare step, 2-3 the rounds and the final order

    NetArgs a;
    uint32_t *d_first, *d_bs, *d_be, *d_group;
    int64_t* d_score;
    uint8_t* temp;
    size_t sort_bytes = 0, scan_bytes = 0;
    cover_sort_anchors(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, N, s);
    cover_scan_offsets(nullptr, &scan_bytes, nullptr, nullptr, N, s);
    size_t temp_bytes = std::max(std::max(sort_bytes, scan_bytes), std::max<size_t>(scan_temp_bytes(B), 256));
    carve(sl->net_work, "net", [&](Carve& c) {
        c.take(d_first, (size_t)N + 1).take(d_bs, B).take(d_be, B).take(d_score, N).take(d_group, N);
        c.take(a.key_a, N).take(a.key_b, N).take(a.idx_a, N).take(a.idx_b, N).take(a.byprio, N).take(a.hull_s, N).take(a.hull_e, N);
        c.take(a.head, (size_t)N + 1).take(a.gidx, (size_t)N + 1).take(a.gstart, (size_t)N + 1).take(a.len, B).take(a.pre, (size_t)B + 1);
        c.take(temp, temp_bytes);
    });
    a.first = d_first; a.bs = d_bs; a.be = d_be; a.score = d_score;
    a.n = N;
    a.blocks = B;
    a.min_space = P.min_space;
    a.min_fill = P.min_fill;

    to_device(d_first, first, (size_t)N + 1, s, "net: first");
    to_device(d_bs, block_start, B, s, "net: block starts");
    to_device(d_be, block_end, B, s, "net: block ends");
    to_device(d_score, score, N, s, "net: scores");
    a.group = upload(d_group, group, N, s, "net: groups");

    // prepare: stable sort by score descending from input order, then by group; hulls and group ranges; the blocks' prefix sums
    ev.mark(0);
    launch(sl, "net_prepare", [&] {
        launch_net_key_minor(a, s);
        cover_sort_anchors(temp, &temp_bytes, a.key_a, a.key_b, a.idx_a, a.idx_b, N, s);
        launch_net_key_major(a, a.idx_b, s);
        cover_sort_anchors(temp, &temp_bytes, a.key_a, a.key_b, a.idx_b, a.byprio, N, s);
        launch_net_gather(a, s);
        cover_scan_offsets(temp, &temp_bytes, a.head, a.gidx, N, s);
        launch_net_group_starts(a, s);
        launch_net_block_len(a, s);
        launch_exclusive_scan_u64(a.len, a.pre, B, temp, s);
    });
    ev.mark(1);
    uint64_t groups64 = 0;
    to_host(&groups64, a.gidx + N, 1, s, "net: groups");
    check_sync(s, "net_prepare");
    const uint32_t G = (uint32_t)groups64;
    if (G == 0 || G > N) {
        fprintf(stderr, "Error: NetChains: %llu groups of %u chains\n", (unsigned long long)groups64, N);
        exit(15);
    }

    // the rounds: this round's spaces in net_space[cur], the next one's in the other
    int cur = 0;
    uint32_t S = G, F = 0;
    sl->net_space[cur].ensure((size_t)S * sizeof(NetSpace), "net spaces");
    ev.mark(2);
    launch(sl, "net_roots", [&] { launch_net_roots(a, G, (NetSpace*)sl->net_space[cur].p, s); });
    while (S) {
        NetRound r;
        uint8_t* scan_temp;
        carve(sl->net_round, "net round", [&](Carve& c) {
            c.take(r.hit, S).take(r.cnt, 2 * (size_t)S).take(r.off, 2 * (size_t)S + 1).take(scan_temp, std::max<size_t>(scan_temp_bytes(2 * (uint64_t)S), 256));
        });
        r.spaces = (const NetSpace*)sl->net_space[cur].p;
        r.S = S;
        r.next = nullptr;
        r.fills = nullptr;
        r.fill_base = F;
        launch(sl, "net_search", [&] { launch_net_search(a, r, s); });
        launch(sl, "net_count", [&] {
            launch_net_count(a, r, s);
            launch_exclusive_scan_u64(r.cnt, r.off, 2 * (uint64_t)S, scan_temp, s);
        });
        uint64_t children = 0, end = 0;
        to_host(&children, r.off + S, 1, s, "net: children");
        to_host(&end, r.off + 2 * (size_t)S, 1, s, "net: fills");
        check_sync(s, "net round");
        st.rounds++;
        st.spaces += S;
        const uint64_t filled = end - children;
        if (filled > S || (filled == 0 && children != 0)) {
            fprintf(stderr, "Error: NetChains: %llu fills and %llu children from %u spaces\n", (unsigned long long)filled,
                    (unsigned long long)children, S);
            exit(15);
        }
        if (!filled) break;
        if ((uint64_t)F + filled >= NET_TOP || children >= NET_TOP) {
            fprintf(stderr, "Error: NetChains: %llu fills and %llu open spaces: at most 2^31 - 1 of either\n",
                    (unsigned long long)((uint64_t)F + filled), (unsigned long long)children);
            exit(1);
        }
        sl->net_fills.ensure(((size_t)F + filled) * sizeof(sa_net_fill), "net fills", true, s);  // the earlier rounds' fills are kept
        sl->net_space[cur ^ 1].ensure((size_t)children * sizeof(NetSpace), "net spaces");
        r.next = (NetSpace*)sl->net_space[cur ^ 1].p;
        r.fills = (sa_net_fill*)sl->net_fills.p;
        launch(sl, "net_emit", [&] { launch_net_emit(a, r, s); });
        F += (uint32_t)filled;
        S = (uint32_t)children;
        cur ^= 1;
    }

    // the final order: a stable sort of the fills by (group, start), parents through the inverse permutation
    sa_net_fill* out = host_alloc<sa_net_fill>(F, "NetChains");
    if (F) {
        uint64_t *key_a, *key_b;
        uint32_t *idx, *order, *inv;
        sa_net_fill* sorted;
        uint8_t* sort_temp;
        size_t fb = 0;
        cover_sort_anchors(nullptr, &fb, nullptr, nullptr, nullptr, nullptr, F, s);
        fb = std::max<size_t>(fb, 256);
        carve(sl->net_round, "net order", [&](Carve& c) {
            c.take(key_a, F).take(key_b, F).take(idx, F).take(order, F).take(inv, F).take(sorted, F).take(sort_temp, fb);
        });
        const sa_net_fill* d_fills = (const sa_net_fill*)sl->net_fills.p;
        launch(sl, "net_order", [&] {
            launch_net_fill_key(d_fills, F, key_a, idx, s);
            cover_sort_anchors(sort_temp, &fb, key_a, key_b, idx, order, F, s);
            launch_net_inverse(order, F, inv, s);
            launch_net_finish(d_fills, order, inv, F, sorted, s);
        });
        ev.mark(3);
        to_host(out, sorted, F, s, "net: fills");
    } else {
        ev.mark(3);
    }
    check_sync(s, "net_order");
    st.prep_ms = (float)ev.ms(0, 1);
    st.net_ms = (float)ev.ms(2, 3);
    prof_flush(sl);
    release_slot(sl);

    st.chains = N;
    st.blocks = B;
    st.groups = G;
    st.fills = F;
    std::vector<bool> seen(N, false);
    for (uint32_t k = 0; k < F; k++) {
        st.max_depth = std::max<uint64_t>(st.max_depth, out[k].depth);
        if (!seen[out[k].chain]) {
            seen[out[k].chain] = true;
            st.filled++;
        }
    }
    if (stats) *stats = st;
    *fills = out;
    return F;
}

void sa_free_net(sa_net_fill* fills) { free(fills); }

}  // extern "C"
