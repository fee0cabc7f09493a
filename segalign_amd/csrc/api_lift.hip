// api_lift.hip -- C-ABI sa_lift_intervals: intervals of one axis carried through chains to the other axis, every interval with its
// status, its best chain and, under the flags, a hit per qualifying chain and the clipped block pairs of every hit (contract:
// include/segalign_amd.h).  The host side: the linear validation pass over the chains and the intervals, the slot and its
// three buffers, the kernels of lift.hip with one sort and one running maximum (cover.hip's wrappers) and the prefix sums of scan.hip
// between them, the two totals read back to size the hits and the blocks, the copies and the counts taken from the records.
#include "post_host.h"  // and through it gapped.h: cover_sort_anchors, cover_scan_runmax
#include "lift.h"

using namespace sa;

namespace {

const char* const WHO = "LiftIntervals";
const Fail fail{"LiftIntervals"};
static_assert(LIFT_MAX_CHAINS == POST_MAX_CHAINS && LIFT_MAX_BLOCKS == POST_MAX_BLOCKS && LIFT_TOP == POST_TOP,
              "checked_block_pairs holds the chains to the limits lift.hip's kernels are written for");

}  // namespace

extern "C" {

size_t sa_lift_intervals(const uint32_t* first, const uint32_t* block_start, const uint32_t* block_end, const uint32_t* oblock_start,
                         const uint32_t* oblock_end, const uint32_t* group, const uint32_t* ogroup, const uint8_t* ostrand, size_t n_chains,
                         const uint32_t* iv_group, const uint32_t* iv_start, const uint32_t* iv_end, size_t n_intervals,
                         const sa_lift_params* p, uint32_t flags, sa_lift_record** records, sa_lift_hit** hits, size_t* n_hits,
                         sa_lift_block** blocks, size_t* n_blocks, sa_lift_stats* stats) {
    *records = nullptr;
    *hits = nullptr;
    *blocks = nullptr;
    *n_hits = *n_blocks = 0;
    sa_lift_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_init(WHO);
    if (flags > (SA_LIFT_MULTIPLE | SA_LIFT_BLOCKS)) fail("flags = %lld: SA_LIFT_MULTIPLE, SA_LIFT_BLOCKS, both or 0", flags);
    sa_lift_params P = {95, 100};
    if (p) P = *p;
    if (P.den < 1 || P.den > LIFT_MAX_DEN) fail("den = %lld: 1 .. 1 << 20", P.den);
    if (P.num > P.den) fail("num = %lld exceeds den = %lld", P.num, P.den);
    if (n_intervals > LIFT_MAX_INTERVALS) fail("%lld intervals: at most 1 << 26", (long long)n_intervals);
    const uint32_t B = checked_block_pairs(fail, first, block_start, block_end, oblock_start, oblock_end, ostrand, n_chains);
    for (size_t k = 0; k < n_intervals; k++) {
        if (iv_start[k] >= iv_end[k]) fail("interval %lld: start >= end", (long long)k);
        if (iv_end[k] >= LIFT_TOP) fail("interval %lld ends at or past 2^31", (long long)k);
    }
    st.chains = n_chains;
    st.blocks = B;
    if (n_intervals == 0) {
        if (stats) *stats = st;
        return 0;
    }
    const uint32_t N = (uint32_t)n_chains, I = (uint32_t)n_intervals;

    Slot* sl = acquire_slot_early();
    const hipStream_t s = sl->stream;
    LiftArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N;
    a.B = B;
    a.I = I;
    a.num = P.num;
    a.den = P.den;
    a.multiple = flags & SA_LIFT_MULTIPLE;
    a.with_blocks = flags & SA_LIFT_BLOCKS;

    // one buffer for the inputs, what prepare makes of them and what there is per interval
    uint32_t *d_first, *d_bs, *d_be, *d_obs, *d_obe, *d_group, *d_ogroup, *d_ivg, *d_ivs, *d_ive;
    uint8_t *d_ostrand, *temp;
    size_t sort_bytes = 0, max_bytes = 0;
    if (N) {
        cover_sort_anchors(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, N, s);
        cover_scan_runmax(nullptr, &max_bytes, nullptr, nullptr, N, s);
    }
    size_t temp_bytes = std::max(std::max(sort_bytes, max_bytes), std::max<size_t>(scan_temp_bytes(std::max(B, I)), 256));
    carve(sl->lift, "lift", [&](Carve& c) {
        c.take(d_first, (size_t)N + 1).take(d_bs, B).take(d_be, B).take(d_obs, B).take(d_obe, B).take(d_group, N).take(d_ogroup, N);
        c.take(d_ostrand, N).take(d_ivg, I).take(d_ivs, I).take(d_ive, I);
        c.take(a.len, B).take(a.pre, (size_t)B + 1).take(a.key, N).take(a.skey, N).take(a.val, N).take(a.order, N).take(a.hull_e, N);
        c.take(a.hmax, N).take(a.run, N).take(a.range, I).take(a.cnt, I).take(a.off, (size_t)I + 1).take(a.rec, I).take(temp, temp_bytes);
    });
    a.first = d_first;
    a.bs = d_bs;
    a.be = d_be;
    a.obs = d_obs;
    a.obe = d_obe;
    a.iv_s = d_ivs;
    a.iv_e = d_ive;

    if (N) to_device(d_first, first, (size_t)N + 1, s, "lift: first");
    to_device(d_bs, block_start, B, s, "lift: block starts");
    to_device(d_be, block_end, B, s, "lift: block ends");
    to_device(d_obs, oblock_start, B, s, "lift: other block starts");
    to_device(d_obe, oblock_end, B, s, "lift: other block ends");
    a.group = upload(d_group, group, N, s, "lift: group");
    a.ogroup = upload(d_ogroup, ogroup, N, s, "lift: ogroup");
    a.ostrand = upload(d_ostrand, ostrand, N, s, "lift: ostrand");
    a.iv_group = upload(d_ivg, iv_group, I, s, "lift: interval groups");
    to_device(d_ivs, iv_start, I, s, "lift: interval starts");
    to_device(d_ive, iv_end, I, s, "lift: interval ends");

    Timer<3> ev(s, "lift timing");
    ev.mark(0);
    if (N)
        launch(sl, "lift_prepare", [&] {
            launch_lift_block_len(a, s);
            if (B) launch_exclusive_scan_u64(a.len, a.pre, B, temp, s);
            launch_lift_keys(a, s);
            cover_sort_anchors(temp, &temp_bytes, a.key, a.skey, a.val, a.order, N, s);  // stable: equal keys stay in chain order
            launch_lift_gather(a, s);
            cover_scan_runmax(temp, &temp_bytes, a.hmax, a.run, N, s);  // groups ascend, so the segmented maximum is the running one
        });
    ev.mark(1);
    launch(sl, "lift_count", [&] {
        launch_lift_count(a, s);
        launch_exclusive_scan_u64(a.cnt, a.off, I, temp, s);
    });
    const uint64_t H64 = read_u64(a.off + I, s, "lift_count");
    if (H64 > LIFT_MAX_OUT) fail("%lld hits: at most 2^31 - 1", (long long)H64);
    const uint32_t H = (uint32_t)H64;
    a.H = H;
    uint8_t* htemp;
    carve(sl->lift_hits, "lift hits", [&](Carve& c) {
        c.take(a.hits, H).take(a.hn, H).take(a.hoff, (size_t)H + 1).take(htemp, std::max<size_t>(scan_temp_bytes(H), 256));
    });
    launch(sl, "lift_emit", [&] { launch_lift_emit(a, s); });
    uint32_t O = 0;
    if (a.with_blocks && H) {
        launch(sl, "lift_blocks", [&] { launch_exclusive_scan_u64(a.hn, a.hoff, H, htemp, s); });
        const uint64_t O64 = read_u64(a.hoff + H, s, "lift_blocks");
        if (O64 > LIFT_MAX_OUT) fail("%lld output blocks: at most 2^31 - 1", (long long)O64);
        a.O = O = (uint32_t)O64;
        sl->lift_out.ensure((size_t)O * sizeof(sa_lift_block), "lift blocks");
        a.out = (sa_lift_block*)sl->lift_out.p;
        launch(sl, "lift_blocks", [&] { launch_lift_blocks(a, s); });
    }
    ev.mark(2);
    sa_lift_record* rec = host_alloc<sa_lift_record>(I, WHO);
    sa_lift_hit* hit = host_alloc<sa_lift_hit>(H, WHO);
    sa_lift_block* blk = host_alloc<sa_lift_block>(O, WHO);
    std::vector<LiftRange> range(I);
    to_host(rec, a.rec, I, s, "lift: records");
    to_host(range.data(), a.range, I, s, "lift: ranges");
    to_host(hit, a.hits, H, s, "lift: hits");
    to_host(blk, a.out, O, s, "lift: blocks");
    check_sync(s, "lift_emit");
    st.prep_ms = (float)ev.ms(0, 1);
    st.lift_ms = (float)ev.ms(1, 2);
    prof_flush(sl);
    release_slot(sl);

    st.intervals = I;
    st.hits = H;
    st.out_blocks = O;
    for (uint32_t k = 0; k < I; k++) {
        const sa_lift_record& r = rec[k];
        if (r.status > SA_LIFT_DUPLICATED || r.n_qualify > r.n_touch || range[k].hi - range[k].lo < r.n_touch) {
            fprintf(stderr, "Error: LiftIntervals: interval %u came back with status %u, %u touching and %u qualifying chains\n", k, r.status,
                    r.n_touch, r.n_qualify);
            exit(15);
        }
        st.candidates += range[k].hi - range[k].lo;
        st.touches += r.n_touch;
        st.n_status[r.status]++;
    }
    if (stats) *stats = st;
    *records = rec;
    *hits = hit;
    *blocks = blk;
    *n_hits = H;
    *n_blocks = O;
    return I;
}

void sa_free_lift(sa_lift_record* records, sa_lift_hit* hits, sa_lift_block* blocks) {
    free(records);
    free(hits);
    free(blocks);
}

}  // extern "C"
