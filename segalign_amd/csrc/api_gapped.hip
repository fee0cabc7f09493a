// api_gapped.hip -- C-ABI sa_gapped_extend: gapped y-drop extension of HSP anchors (contract: include/segalign_amd.h).
// The host side: parameter defaults and limits, batches of anchors through the slot's stream (gapped.hip), the selection rules.
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
    DevCtx* dc = sl->ctx;
    const SeqBuf& q = rev ? dc->query_rc[buffer] : dc->query[buffer];
    if (!dc->ref.codes || !q.codes) {
        fprintf(stderr, "Error: GappedExtend needs a resident target block and query buffer %u\n", buffer);
        exit(1);
    }
    const size_t batch = std::min(n, GAPPED_BATCH);
    const size_t hsp_bytes = (batch * sizeof(sa_segment_pair) + 255) & ~(size_t)255;
    sl->gapped.ensure(hsp_bytes + 2 * batch * sizeof(GappedSide), "gapped");
    sa_segment_pair* d_hsps = (sa_segment_pair*)sl->gapped.p;
    GappedSide* d_side = (GappedSide*)(sl->gapped.p + hsp_bytes);
    std::vector<GappedSide> side(2 * n);
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
    prof_flush(sl);
    release_slot(sl);

    std::vector<sa_gapped_alignment> rec(n);
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
    if (stats) *stats = st;
    if (rec.empty()) return 0;
    *out = (sa_gapped_alignment*)malloc(rec.size() * sizeof(sa_gapped_alignment));
    memcpy(*out, rec.data(), rec.size() * sizeof(sa_gapped_alignment));
    return rec.size();
}

void sa_free_gapped(sa_gapped_alignment* p) { free(p); }

}  // extern "C"
