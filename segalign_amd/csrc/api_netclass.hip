// api_netclass.hip -- C-ABI sa_net_classify: every fill of a net classed against its parent on the other axis, with its duplicated bases
// there and the synteny filter's keep mark (contract: include/segalign_amd.h).  The host side: the linear validation pass
// over the two block sets and the fills, the slot and its one buffer, the kernels of netclass.hip with one sort (cover.hip's wrapper) and
// the prefix sums of scan.hip between them, the copy of the records and the counts taken from them.
#include "post_host.h"  // and through it gapped.h: cover_sort_anchors
#include "netclass.h"

using namespace sa;

namespace {

const char* const WHO = "NetClassify";

const Fail fail{"NetClassify"};
static_assert(NETCLASS_MAX_CHAINS == POST_MAX_CHAINS && NETCLASS_MAX_BLOCKS == POST_MAX_BLOCKS && NETCLASS_TOP == POST_TOP,
              "checked_block_pairs holds the chains to the limits netclass.hip's kernels are written for");

// The rules of the fills; returns the number of clipped blocks.
uint64_t checked_fills(const sa_net_fill* fills, size_t F, const uint32_t* first, const uint32_t* bs, const uint32_t* be, size_t n_chains) {
    uint64_t blocks = 0;
    for (size_t k = 0; k < F; k++) {
        const sa_net_fill& f = fills[k];
        checked_fill_in_chain(fail, f, k, first, n_chains);
        if (be[f.first_block] <= f.start || bs[f.first_block + f.n_blocks - 1] >= f.end)
            fail("fill %lld: its first block ends before its start or its last block starts after its end", (long long)k);
        blocks += f.n_blocks;
        if (blocks > NETCLASS_MAX_BLOCKS) fail("more than 1 << 26 clipped blocks at fill %lld", (long long)k);
        if (f.parent == -1) {
            if (f.depth != 0) fail("fill %lld has no parent and depth %lld", (long long)k, f.depth);
            continue;
        }
        if (f.parent < 0 || (size_t)f.parent >= k) fail("fill %lld: parent %lld is neither -1 nor an earlier fill", (long long)k, f.parent);
        if (f.depth != fills[f.parent].depth + 1) fail("fill %lld: depth %lld is not its parent's and one", (long long)k, f.depth);
    }
    return blocks;
}

}  // namespace

extern "C" {

size_t sa_net_classify(const uint32_t* first, const uint32_t* block_start, const uint32_t* block_end, const uint32_t* oblock_start,
                       const uint32_t* oblock_end, const uint32_t* ogroup, const uint8_t* ostrand, size_t n_chains,
                       const sa_net_fill* fills, size_t n_fills, const sa_net_class_params* p, uint32_t flags, sa_net_class** classes,
                       sa_net_class_stats* stats) {
    *classes = nullptr;
    sa_net_class_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_init(WHO);
    if (flags > SA_NETCLASS_FILTER) fail("flags = %lld: SA_NETCLASS_FILTER or 0", flags);
    sa_net_class_params P;
    memset(&P, 0, sizeof(P));
    if (p) P = *p;
    if (P.min_size > NETCLASS_TOP) fail("min_size = %lld out of range", P.min_size);
    if (P.min_ali > NETCLASS_TOP) fail("min_ali = %lld out of range", P.min_ali);
    if (P.max_far > NETCLASS_TOP) fail("max_far = %lld out of range", P.max_far);
    if (n_fills > NETCLASS_MAX_FILLS) fail("%lld fills: at most 2^31 - 1", (long long)n_fills);
    const uint32_t B = checked_block_pairs(fail, first, block_start, block_end, oblock_start, oblock_end, ostrand, n_chains);
    const uint64_t blocks = checked_fills(fills, n_fills, first, block_start, block_end, n_chains);
    if (n_fills == 0) return 0;
    const uint32_t N = (uint32_t)n_chains, F = (uint32_t)n_fills, M = (uint32_t)blocks, E = 2 * M;

    Slot* sl = acquire_slot_early();
    const hipStream_t s = sl->stream;
    NetClassArgs a;
    memset(&a, 0, sizeof(a));
    a.F = F;
    a.M = M;
    a.E = E;
    a.filter = flags & SA_NETCLASS_FILTER;
    a.p = P;

    // one buffer for the whole call
    sa_net_fill* d_fills;
    uint32_t *d_bs, *d_be, *d_obs, *d_obe, *d_ogroup;
    uint8_t *d_ostrand, *temp;
    size_t sort_bytes = 0;
    cover_sort_anchors(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, E, s);
    size_t temp_bytes = std::max(sort_bytes, std::max<size_t>(scan_temp_bytes(std::max(F, E)), 256));
    carve(sl->netclass, "net class", [&](Carve& c) {
        c.take(d_fills, F).take(d_bs, B).take(d_be, B).take(d_obs, B).take(d_obe, B).take(d_ogroup, N).take(d_ostrand, N);
        c.take(a.cnt, F).take(a.off, (size_t)F + 1).take(a.cs, M).take(a.ce, M);
        c.take(a.key, E).take(a.skey, E).take(a.val, E).take(a.sval, E).take(a.flag, E).take(a.starts, (size_t)E + 1);
        c.take(a.seg, E).take(a.dup, (size_t)E + 1).take(a.pos, E).take(a.bdup, M).take(a.bsum, (size_t)M + 1);
        c.take(a.self, F).take(a.out, F).take(temp, temp_bytes);
    });
    a.fills = d_fills;
    a.bs = d_bs;
    a.be = d_be;
    a.obs = d_obs;
    a.obe = d_obe;

    to_device(d_fills, fills, F, s, "net class: fills");
    to_device(d_bs, block_start, B, s, "net class: block starts");
    to_device(d_be, block_end, B, s, "net class: block ends");
    to_device(d_obs, oblock_start, B, s, "net class: other block starts");
    to_device(d_obe, oblock_end, B, s, "net class: other block ends");
    a.ogroup = upload(d_ogroup, ogroup, N, s, "net class: ogroup");
    a.ostrand = upload(d_ostrand, ostrand, N, s, "net class: ostrand");

    Timer<2> ev(s, "net class timing");
    ev.mark(0);
    launch(sl, "netclass_events", [&] {
        launch_netclass_counts(a, s);
        launch_exclusive_scan_u64(a.cnt, a.off, F, temp, s);
        launch_netclass_emit(a, s);
        cover_sort_anchors(temp, &temp_bytes, a.key, a.skey, a.val, a.sval, E, s);
    });
    launch(sl, "netclass_depth", [&] {
        launch_netclass_flags(a, s);
        launch_exclusive_scan_u32(a.flag, a.starts, E, temp, s);
        launch_netclass_segments(a, s);
        launch_exclusive_scan_u64(a.seg, a.dup, E, temp, s);
        launch_netclass_block_dup(a, s);
        launch_exclusive_scan_u64(a.bdup, a.bsum, M, temp, s);
    });
    launch(sl, "netclass_classes", [&] {
        launch_netclass_classes(a, s);
        if (a.filter) launch_netclass_keep(a, s);
    });
    ev.mark(1);
    sa_net_class* out = host_alloc<sa_net_class>(F, WHO);
    to_host(out, a.out, F, s, "net class: records");
    check_sync(s, "netclass_classes");
    st.class_ms = (float)ev.ms(0, 1);
    prof_flush(sl);
    release_slot(sl);

    st.fills = F;
    st.blocks = M;
    st.events = E;
    std::vector<uint32_t> groups(F);
    for (uint32_t k = 0; k < F; k++) {
        const sa_net_class& c = out[k];
        if (c.type > SA_NETCLASS_NONSYN || c.keep > 1) {
            fprintf(stderr, "Error: NetClassify: fill %u came back with type %u and keep %u\n", k, c.type, c.keep);
            exit(15);
        }
        groups[k] = c.ogroup;
        st.n_type[c.type]++;
        st.kept += c.keep;
        st.dup_bases += c.odup;
    }
    std::sort(groups.begin(), groups.end());
    st.ogroups = std::unique(groups.begin(), groups.end()) - groups.begin();
    if (stats) *stats = st;
    *classes = out;
    return F;
}

void sa_free_net_class(sa_net_class* classes) { free(classes); }

}  // extern "C"
