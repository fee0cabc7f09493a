// api_introspect.hip -- C-ABI, introspection: call statistics, filter / lookup mode, copies of device state (tests, bench).
#include "engine_internal.h"

#include <vector>

using namespace sa;

// a malloc'ed host copy of n elements of a device array, queued on the stream (sa_probe_call)
template <typename T>
static T* probe_download(const T* src, size_t n, hipStream_t st, const char* what) {
    T* h = (T*)malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (n) check_memcpy(hipMemcpyAsync(h, src, n * sizeof(T), hipMemcpyDeviceToHost, st), what);
    return h;
}

extern "C" {

// ---- introspection --------------------------------------------------------------------------------------------------
void sa_get_last_call_stats(sa_call_stats* o) { *o = t_stats; }
void sa_get_last_call_trace(sa_call_trace* o) { *o = t_trace; }
void sa_set_count_examined(int on) { g_count_examined = on != 0; }
int sa_get_filter_mode(void) {  // which X-drop filter kernel the next plain (non repeat-masker) call uses
    if (g_count_examined) return g_fast_filter ? 1 : 0;
    return g_packed_filter ? 3 : g_fast_filter;
}
int sa_get_lookup_mode(void) {  // how device-seeded calls look seeds up on device 0 right now (builds the table if needed)
    if (g_ndev <= 0 || !g_proc_init) return 0;
    DevCtx* dc = g_dev[0];
    check_set_device(dc->dev, "lookup mode");
    if (!(g_td && g_packed_filter && !g_count_examined && dc->ref2.base && ensure_nbr(dc))) return 0;
    return dc->nbr_ctx ? 2 : 1;
}
uint64_t sa_get_neighbourhood_entries(void) { return (g_ndev > 0 && g_dev[0]->nbr_state == 1) ? g_dev[0]->nbr_total : 0; }

uint32_t sa_get_ref_len(void) { return g_ndev ? g_dev[0]->ref.len : 0; }
uint32_t sa_get_num_index(void) { return g_ndev ? g_dev[0]->num_index : 0; }
uint32_t sa_get_index_table_size(void) { return g_ndev ? g_dev[0]->nkeys : 0; }
uint32_t sa_get_query_len(uint32_t buffer) { return buffer < SA_BUFFER_DEPTH ? g_query_len[buffer] : 0; }

static DevCtx* ctx_of(int dev) {
    if (dev < 0 || dev >= g_ndev) {
        fprintf(stderr, "Error: device %d out of range\n", dev);
        exit(11);
    }
    check_set_device(g_dev[dev]->dev, "copy");
    return g_dev[dev];
}
void sa_copy_ref_codes(int dev, uint8_t* dst) {
    DevCtx* dc = ctx_of(dev);
    check_memcpy(hipMemcpy(dst, dc->ref.codes, dc->ref.len, hipMemcpyDeviceToHost), "ref codes");
}
void sa_copy_index_table(int dev, uint32_t* dst) {
    DevCtx* dc = ctx_of(dev);
    check_memcpy(hipMemcpy(dst, dc->bucket_start + 1, (size_t)dc->nkeys * sizeof(uint32_t), hipMemcpyDeviceToHost), "index table");
}
void sa_copy_pos_table(int dev, uint32_t* dst) {
    DevCtx* dc = ctx_of(dev);
    check_memcpy(hipMemcpy(dst, dc->pos_table, (size_t)dc->num_index * sizeof(uint32_t), hipMemcpyDeviceToHost), "pos table");
}
void sa_copy_query_codes(int dev, uint32_t buffer, int rev, uint8_t* dst) {
    DevCtx* dc = ctx_of(dev);
    SeqBuf& b = rev ? dc->query_rc[buffer] : dc->query[buffer];
    check_memcpy(hipMemcpy(dst, b.codes, b.len, hipMemcpyDeviceToHost), "query codes");
}

// ---- the tables as they were built (tests/test_gpu_table_regimes.py, DESIGN.md 4.2'') ---------------------------------------------------
// What sa_generate_seed_pos_table and ensure_nbr recorded about device 0: which build, how many partitions the finish kernel left to the
// global sort, which neighbourhood fill.  Read-only; builds nothing (sa_get_lookup_mode does).
int sa_get_table_build_info(sa_table_build_info* o) {
    memset(o, 0, sizeof(*o));
    if (g_ndev <= 0) return -1;
    DevCtx* dc = g_dev[0];
    std::lock_guard<std::mutex> lk(dc->nbr_mu);
    o->build = dc->pos_table ? dc->table_build : SA_TABLE_BUILD_NONE;
    o->unsorted_partitions = dc->pos_table ? dc->table_unsorted : 0u;
    o->nbr_fill = dc->nbr_state == 1 ? dc->nbr_fill : SA_NBR_FILL_NONE;
    o->left_skip = (dc->nbr_state == 1 && dc->nbr_ctx) ? dc->nbr_left_skip : 0u;
    return 0;
}
// a range of the neighbourhood table of device `dev`, or nullptr with a message: not built, or the range leaves it
static DevCtx* nbr_range(int dev, uint64_t first, uint64_t count, bool starts, const char* what) {
    if (dev < 0 || dev >= g_ndev) {
        fprintf(stderr, "Error: %s: device %d out of range\n", what, dev);
        return nullptr;
    }
    DevCtx* dc = g_dev[dev];
    const bool have = dc->nbr_state == 1 && dc->nbr_start && (dc->nbr_ctx || dc->nbr_pos || dc->nbr_total == 0);
    if (!have) {
        fprintf(stderr, "Error: %s: the neighbourhood table of device %d is not built\n", what, dev);
        return nullptr;
    }
    const uint64_t limit = starts ? (uint64_t)dc->nkeys + 1 : dc->nbr_total;
    if (first > limit || count > limit - first) {
        fprintf(stderr, "Error: %s: [%llu, +%llu) leaves the table's %llu\n", what, (unsigned long long)first, (unsigned long long)count,
                (unsigned long long)limit);
        return nullptr;
    }
    check_set_device(dc->dev, "copy");
    return dc;
}
int sa_copy_neighbourhood_starts(int dev, uint64_t first_key, uint64_t count, uint64_t* dst) {
    DevCtx* dc = nbr_range(dev, first_key, count, true, "sa_copy_neighbourhood_starts");
    if (!dc) return -1;
    std::lock_guard<std::mutex> lk(dc->nbr_mu);
    if (count) check_memcpy(hipMemcpy(dst, dc->nbr_start + first_key, count * sizeof(uint64_t), hipMemcpyDeviceToHost), "neighbourhood starts");
    return 0;
}
int sa_copy_neighbourhood_records(int dev, uint64_t first_entry, uint64_t count, void* dst) {
    DevCtx* dc = nbr_range(dev, first_entry, count, false, "sa_copy_neighbourhood_records");
    if (!dc) return -1;
    std::lock_guard<std::mutex> lk(dc->nbr_mu);
    if (dc->nbr_ctx) {
        if (count) check_memcpy(hipMemcpy(dst, dc->nbr_ctx + first_entry, count * sizeof(CtxRec), hipMemcpyDeviceToHost), "neighbourhood records");
        return 2;
    }
    if (count) check_memcpy(hipMemcpy(dst, dc->nbr_pos + first_entry, count * sizeof(uint32_t), hipMemcpyDeviceToHost), "neighbourhood positions");
    return 1;
}

// ---- the sequence images as their builders left them (tests/test_gpu_sequence_images.py, DESIGN.md 4.1') ----------------------------------
// Whole spans: a sequence buffer with its guards and over-read room, the 4-bit copies with their pads, the overlapped lines of the
// target's 2-bit copies, the shifted 2-bit copies with their zero tails.  Read-only; the send entries have synchronised their stream.
static_assert(SA_IMAGE_COUNT == 14 && SA_IMAGE_REFQ2_RC == SA_IMAGE_COUNT - 1, "sa_copy_image knows every image");
static_assert(sizeof(sa_image_info) == 32 && offsetof(sa_image_info, len) == 24, "sa_image_info as engine.py restates it");
int sa_copy_image(int dev, int image, uint32_t buffer, uint8_t* dst, uint64_t cap, sa_image_info* o) {
    memset(o, 0, sizeof(*o));
    if (dev < 0 || dev >= g_ndev || image < 0 || image >= SA_IMAGE_COUNT) {
        fprintf(stderr, "Error: sa_copy_image: device %d or image %d out of range\n", dev, image);
        return -1;
    }
    const bool of_query = image == SA_IMAGE_QUERY || image == SA_IMAGE_QUERY_RC || image == SA_IMAGE_QUERY4 || image == SA_IMAGE_QUERY4_RC ||
                          image == SA_IMAGE_QUERY2 || image == SA_IMAGE_QUERY2_RC;
    if (of_query && buffer >= SA_BUFFER_DEPTH) {
        fprintf(stderr, "Error: sa_copy_image: query buffer %u out of range\n", buffer);
        return -1;
    }
    DevCtx* dc = g_dev[dev];
    const uint32_t b = of_query ? buffer : 0;
    const SeqBuf* sb = nullptr;
    const PackedBuf* pb = nullptr;
    switch (image) {
        case SA_IMAGE_REF: sb = &dc->ref; break;
        case SA_IMAGE_REF8: sb = &dc->ref8; break;
        case SA_IMAGE_REF_RC: sb = &dc->ref_rc; break;
        case SA_IMAGE_QUERY: sb = &dc->query[b]; break;
        case SA_IMAGE_QUERY_RC: sb = &dc->query_rc[b]; break;
        case SA_IMAGE_QUERY4: pb = &dc->query4[b]; break;
        case SA_IMAGE_QUERY4_RC: pb = &dc->query4_rc[b]; break;
        case SA_IMAGE_REF4: pb = &dc->ref4; break;
        case SA_IMAGE_REF4_RC: pb = &dc->ref4_rc; break;
        case SA_IMAGE_REF2: pb = &dc->ref2; break;
        case SA_IMAGE_QUERY2: pb = &dc->query2[b]; break;
        case SA_IMAGE_QUERY2_RC: pb = &dc->query2_rc[b]; break;
        case SA_IMAGE_REFQ2: pb = &dc->refq2; break;
        default: pb = &dc->refq2_rc; break;
    }
    const uint8_t* src = nullptr;
    if (sb) {
        if (sb->alloc && sb->codes) {
            src = sb->alloc;
            o->bytes = o->stride = (uint64_t)sb->len + 2 * SEQ_PAD + 64;
            o->origin = SEQ_PAD;
            o->len = sb->len;
            o->copies = 1;
        }
    } else if (pb->alloc && pb->base && pb->stride) {
        const bool four = image == SA_IMAGE_QUERY4 || image == SA_IMAGE_QUERY4_RC || image == SA_IMAGE_REF4 || image == SA_IMAGE_REF4_RC;
        src = pb->alloc;
        o->stride = pb->stride;
        o->copies = four ? (uint32_t)PACK4_COPIES : image == SA_IMAGE_REF2 ? 4u : pb->copies;
        o->origin = (uint64_t)(pb->base - pb->alloc);
        o->bytes = o->stride * o->copies;
        o->len = of_query ? g_query_len[b] : dc->ref.len;
    }
    if (!src || o->bytes > (uint64_t)(sb ? sb->cap : pb->cap)) {
        fprintf(stderr, "Error: sa_copy_image: image %d of device %d is not resident\n", image, dev);
        memset(o, 0, sizeof(*o));
        return -1;
    }
    if (!dst) return 0;
    if (cap < o->bytes) {
        fprintf(stderr, "Error: sa_copy_image: image %d spans %llu bytes, room for %llu\n", image, (unsigned long long)o->bytes, (unsigned long long)cap);
        return -1;
    }
    check_set_device(dc->dev, "copy");
    check_memcpy(hipMemcpy(dst, src, o->bytes, hipMemcpyDeviceToHost), "image");
    return 0;
}
int sa_get_code_presence(int dev, uint32_t* ref_present, uint32_t* query_present) {
    if (dev < 0 || dev >= g_ndev) {
        fprintf(stderr, "Error: sa_get_code_presence: device %d out of range\n", dev);
        return -1;
    }
    *ref_present = g_dev[dev]->ref_present;
    for (int b = 0; b < SA_BUFFER_DEPTH; b++) query_present[b] = g_dev[dev]->query_present[b];
    return 0;
}
int sa_get_class_scores(uint32_t present_t, uint32_t present_q, int32_t* cls4) {
    if (!g_proc_init) {
        fprintf(stderr, "Error: sa_get_class_scores before InitializeProcessor: no matrix is resident\n");
        return -1;
    }
    int cls[4];
    class_scores(present_t, present_q, cls);
    for (int x = 0; x < 4; x++) cls4[x] = cls[x];
    return 0;
}

// ---- the front of a table-direct call alone (tests/test_gpu_probe_regimes.py, DESIGN.md 4.4') -------------------------------------------
// The range is clipped and cut into chunks as chunks_pass (api_calls.hip) does it, a slot is taken as calls take one, the unchanged
// td_front runs, and what it left in the slot is copied out.  Nothing of a call's later stages runs; t_stats is left alone.
static_assert(sizeof(sa_probe_plan) == sizeof(TdPlan) && offsetof(sa_probe_plan, upto) == offsetof(TdPlan, upto) &&
                  offsetof(sa_probe_plan, num_valid) == offsetof(TdPlan, num_valid) && offsetof(sa_probe_plan, n_iter) == offsetof(TdPlan, n_iter) &&
                  SA_PROBE_MAX_ITER == TD_MAX_ITER && SA_PROBE_PLAN_OVERFLOW == TD_PLAN_OVERFLOW,
              "sa_probe_plan is TdPlan");
static_assert(sizeof(sa_probe_record) == sizeof(TdRec) && offsetof(sa_probe_record, off) == offsetof(TdRec, off), "sa_probe_record is TdRec");
static_assert(sizeof(sa_probe_bound) == 16, "sa_probe_bound is the (hits, non-empty, valid) triple of probe.hip");

void sa_free_probe_call(sa_probe_result* r) {
    if (!r) return;
    free(r->plans); free(r->bounds); free(r->records); free(r->head_bits); free(r->td_chunk); free(r->seg_end); free(r->t_off); free(r->t_cnt);
    r->plans = nullptr; r->bounds = nullptr; r->records = nullptr; r->head_bits = nullptr; r->td_chunk = nullptr; r->seg_end = nullptr;
    r->t_off = nullptr; r->t_cnt = nullptr;
}

int sa_probe_call(uint32_t start, uint32_t end, int rev, uint32_t buffer, int rm, sa_probe_result* o) {
    memset(o, 0, sizeof(*o));
    auto leave = [&](int status) { o->status = status; return status; };
    if (g_ndev <= 0 || !g_proc_init || (!rm && buffer >= SA_BUFFER_DEPTH)) return leave(SA_PROBE_NO_TABLE);
    const uint32_t chunk = g_wga_chunk;
    const uint64_t K64 = end > start && chunk ? ((uint64_t)end - start + chunk - 1) / chunk : 0;
    if (K64 > (uint64_t)SA_MAX_CHUNKS) return leave(SA_PROBE_TOO_MANY_CHUNKS);
    const int K = (int)K64;
    Slot* sl = acquire_slot();
    DevCtx* dc = sl->ctx;
    auto give_back = [&](int status) {
        prof_flush(sl);
        t_front_flags = 0;
        release_slot(sl);
        if (status != SA_PROBE_OK) memset(o, 0, sizeof(*o));
        return leave(status);
    };
    for (int d = 0, k = 0; d < g_ndev; d++)
        for (int s = 0; s < SLOTS_PER_DEVICE; s++, k++)
            if (&g_dev[d]->slots[s] == sl) o->slot = k;
    if (!dc->bucket_start || !dc->pos_table) return give_back(SA_PROBE_NO_TABLE);
    const uint8_t* q;
    uint32_t qlen;
    const PackedBuf *q4, *q2_own, *q2_other;
    if (rm) {
        q = rev ? dc->ref_rc.codes : dc->ref.codes;
        qlen = dc->ref.len;
        q4 = rev ? &dc->ref4_rc : &dc->ref4;
        q2_own = rev ? &dc->refq2_rc : &dc->refq2;
        q2_other = rev ? &dc->refq2 : &dc->refq2_rc;
    } else {
        q = rev ? dc->query_rc[buffer].codes : dc->query[buffer].codes;
        qlen = g_query_len[buffer];
        q4 = rev ? &dc->query4_rc[buffer] : &dc->query4[buffer];
        q2_own = rev ? &dc->query2_rc[buffer] : &dc->query2[buffer];
        q2_other = rev ? &dc->query2[buffer] : &dc->query2_rc[buffer];
    }
    if (!q) qlen = 0;
    const uint32_t lim = qlen >= g_seed_size ? qlen - g_seed_size + 1 : 0;
    const uint32_t send = std::min(end, lim);  // a seed window must lie inside the block
    if (K == 0 || send <= start) return give_back(SA_PROBE_EMPTY_RANGE);
    if (!td_eligible(dc, q4, q2_own, q2_other)) return give_back(SA_PROBE_NOT_ELIGIBLE);
    uint32_t bpos[SA_MAX_CHUNKS + 1];
    for (int c = 0; c <= K; c++) bpos[c] = (uint32_t)std::min<uint64_t>((uint64_t)start + (uint64_t)c * chunk, send);
    o->head_words_before = sl->td_bits.cap;
    t_front_flags = 0;
    uint32_t words = 0;
    o->ret = td_front(dc, sl, q, K, bpos, rm ? 1 : 0, &words);  // (synchronises the slot's stream)
    o->regrown = (t_front_flags & SA_PATH_HEAD_BITS_REGROWN) ? 1u : 0u;
    o->words = words;
    o->start = start;
    o->end = send;
    o->chunk = K > 1 ? chunk : send - start;
    o->num_chunks = (uint32_t)K;
    o->lookup_mode = dc->nbr_ctx ? 2u : 1u;
    o->head_words_after = sl->td_bits.cap;
    hipStream_t st = sl->stream;
    const uint32_t n = send - start;
    o->plans = (sa_probe_plan*)malloc((size_t)K * sizeof(sa_probe_plan));
    memcpy(o->plans, sl->h_td_plan, (size_t)K * sizeof(TdPlan));
    o->bounds = probe_download(reinterpret_cast<const sa_probe_bound*>(sl->d_td_bounds), (size_t)K + 1, st, "probe bounds");
    check_sync(st, "probe bounds");
    o->hits = o->bounds[K].hits;
    o->num_records = o->bounds[K].nonempty;
    uint64_t n_iter = 0;
    for (int c = 0; c < K; c++)
        if (o->plans[c].n_iter != TD_PLAN_OVERFLOW) n_iter += o->plans[c].n_iter;
    o->num_seg_end = (uint32_t)n_iter;
    // (what lies beyond these counts was not written by this call; every count is clamped to what the slot owns)
    const uint64_t need_words = ((o->hits + 63) >> 6) * 2 + 16;
    o->num_head_words = dc->nbr_ctx ? std::min<uint64_t>(need_words, sl->td_bits.cap) : 0;
    o->num_td_chunk = std::min<uint64_t>((o->hits + TD_CHUNK_HITS - 1) / TD_CHUNK_HITS, TD_CHUNK_CAP);
    o->records = probe_download(reinterpret_cast<const sa_probe_record*>(sl->td_rec.p), std::min<size_t>((size_t)o->num_records + 1, sl->td_rec.cap), st,
                                "probe records");
    o->head_bits = probe_download(sl->td_bits.p, (size_t)o->num_head_words, st, "probe head bits");
    o->td_chunk = probe_download(sl->td_chunk.p, (size_t)o->num_td_chunk, st, "probe chunk starts");
    o->seg_end = probe_download(sl->d_seg_end, (size_t)std::min<uint64_t>(n_iter, MAX_SEGS), st, "probe segment ends");
    o->t_off = probe_download(sl->td_toff.p, (size_t)n, st, "probe scratch");
    o->t_cnt = probe_download(sl->td_tcnt.p, (size_t)n, st, "probe scratch");
    check_sync(st, "probe copies");
    return give_back(SA_PROBE_OK);
}

// The ordering stage alone (dedup.hip) on records the host hands in, as ONE dedup scope: what the reference does to the anchors of an
// iteration -- stable_sort(hspComp) -> unique_copy(hspEqual) -> stable_sort(hspCompLastz), src/seed_filter.cu:776-782; rm != 0: the
// repeat masker's chain, repeat_masker_src/seed_filter.cu:819-831.  path 0: the per-segment LDS chain (dedup_seg_kernel; plain
// chain only, at most its 2048 records), path 1: rocprim merge sorts + the adjacent-pair unique kernels (what oversized segments
// and the repeat masker take).  Test entry (tests/test_gpu_thrust_order.py holds both paths against rocThrust's stable_sort /
// unique_copy and against the CPU restatement): own buffers, device 0, default stream.  Returns the number of records in *out.
size_t sa_order_hsps(const sa_segment_pair* in, size_t n, int rm, int path, sa_segment_pair** out) {
    *out = nullptr;
    if (g_ndev <= 0) {
        fprintf(stderr, "Error: sa_order_hsps before InitializeInterface\n");
        exit(11);
    }
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFull || (path == 0 && (rm || n > 2048))) {
        fprintf(stderr, "Error: sa_order_hsps: %zu records do not fit path %d\n", n, path);
        exit(1);
    }
    ctx_of(0);
    std::vector<HspRec> h(n);
    for (size_t i = 0; i < n; i++) { h[i].ref_start = in[i].ref_start; h[i].query_start = in[i].query_start; h[i].len = in[i].len; h[i].score = in[i].score; h[i].seg = 0; }
    HspRec *a = nullptr, *b = nullptr;
    uint4* o16 = nullptr;
    uint32_t* misc = nullptr;  // [0]: counter | seg_info
    void *stmp = nullptr, *utmp = nullptr;
    const size_t sbytes = sort_temp_bytes(n), ubytes = unique_temp_bytes((uint32_t)n), iwords = dedup_seg_info_words() + 4;
    check_memcpy(hipMalloc((void**)&a, n * sizeof(HspRec)), "order: records");
    check_memcpy(hipMalloc((void**)&b, n * sizeof(HspRec)), "order: records");
    check_memcpy(hipMalloc((void**)&o16, n * sizeof(uint4)), "order: output");
    check_memcpy(hipMalloc((void**)&misc, iwords * sizeof(uint32_t)), "order: counters");
    check_memcpy(hipMalloc(&stmp, sbytes), "order: sort temp");
    check_memcpy(hipMalloc(&utmp, ubytes), "order: unique temp");
    check_memcpy(hipMemcpy(a, h.data(), n * sizeof(HspRec), hipMemcpyHostToDevice), "order: upload");
    check_memcpy(hipMemset(misc, 0, iwords * sizeof(uint32_t)), "order: counters");
    hipStream_t st = 0;
    size_t m = 0;
    auto count = [&]() { uint32_t c = 0; check_memcpy(hipMemcpy(&c, misc, sizeof(c), hipMemcpyDeviceToHost), "order: count"); return (size_t)c; };
    if (path == 0) {
        uint32_t* info = misc + 4;
        launch_dedup_seg(a, (uint32_t)n, nullptr, 1, o16, info, 0, 0, st);
        check_launch("order: dedup seg");
        std::vector<uint32_t> hi(dedup_seg_info_words());
        check_memcpy(hipMemcpy(hi.data(), info, hi.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), "order: segment info");
        if (hi[hi.size() - 1] != 0) { fprintf(stderr, "Error: sa_order_hsps: the LDS chain refused the segment\n"); exit(15); }
        m = hi[0];
    } else {
        if (!rm) {
            launch_sort(a, b, n, ORDER_DIAG, stmp, sbytes, st);
            launch_unique(b, a, (uint32_t)n, 0, misc, utmp, st);
            m = count();
            launch_sort(a, b, m, ORDER_LASTZ, stmp, sbytes, st);
        } else {
            launch_sort(a, b, n, ORDER_RM_FIRST, stmp, sbytes, st);
            launch_unique(b, a, (uint32_t)n, 1, misc, utmp, st);
            const size_t m1 = count();
            launch_sort(a, b, m1, ORDER_RM_DIAG, stmp, sbytes, st);
            launch_unique(b, a, (uint32_t)m1, 0, misc, utmp, st);
            m = count();
            launch_sort(a, b, m, ORDER_RM_FINAL, stmp, sbytes, st);
        }
        launch_strip(b, (uint32_t)m, o16, nullptr, st);
        check_launch("order: sort chain");
    }
    sa_segment_pair* res = (sa_segment_pair*)malloc(std::max<size_t>(m, 1) * sizeof(sa_segment_pair));
    if (m) check_memcpy(hipMemcpy(res, o16, m * sizeof(sa_segment_pair), hipMemcpyDeviceToHost), "order: download");
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(o16); (void)hipFree(misc); (void)hipFree(stmp); (void)hipFree(utmp);
    *out = res;
    return m;
}

// The ordering stage the way a call runs it: records of SEVERAL dedup scopes (`seg[i]` < nsegs, the reference iteration of record i) in
// one list.  path 0: launch_dedup_seg with one workgroup per segment, `threads` and `seg_max` as the options dedup_threads /
// dedup_seg_max hand them over, the record count as a launch argument or (count_on_device) through a device word as the speculative
// launch of saf_core passes it; the raw slots are downloaded and their gaps closed by saf_core's own close_seg_gaps.  A refusal of the
// kernel (a segment above seg_max, a device-side count above its total) sets *refused and returns nothing: the caller decides what to
// do next, as saf_core does.  path 1: the library chain with the segment as the major key, plain or rm, stripped with out_seg.
// Test entry (tests/test_gpu_order_regimes.py): own buffers, device 0, default stream.  seg_counts: nsegs words.
size_t sa_order_hsps_segs(const sa_segment_pair* in, const uint32_t* seg, size_t n, uint32_t nsegs, int rm, int path, uint32_t threads,
                          uint32_t seg_max, int count_on_device, sa_segment_pair** out, uint32_t** out_seg, uint32_t* seg_counts,
                          int* refused) {
    *out = nullptr;
    *out_seg = nullptr;
    *refused = 0;
    if (g_ndev <= 0) {
        fprintf(stderr, "Error: sa_order_hsps_segs before InitializeInterface\n");
        exit(11);
    }
    for (uint32_t g = 0; g < nsegs; g++) seg_counts[g] = 0;
    if (n > 0x7FFFFFFFull || (path == 0 && (rm || nsegs > dedup_small_max_segs() || (!count_on_device && n > dedup_seg_max_total())))) {
        fprintf(stderr, "Error: sa_order_hsps_segs: %zu records in %u segments (rm %d) do not fit path %d\n", n, nsegs, rm, path);
        exit(1);
    }
    for (size_t i = 0; i < n; i++)
        if (seg[i] >= nsegs) {
            fprintf(stderr, "Error: sa_order_hsps_segs: record %zu has segment %u of %u\n", i, seg[i], nsegs);
            exit(1);
        }
    if (n == 0) return 0;
    ctx_of(0);
    std::vector<HspRec> h(n);
    for (size_t i = 0; i < n; i++) { h[i].ref_start = in[i].ref_start; h[i].query_start = in[i].query_start; h[i].len = in[i].len; h[i].score = in[i].score; h[i].seg = seg[i]; }
    HspRec *a = nullptr, *b = nullptr;
    uint4* o16 = nullptr;
    uint32_t *misc = nullptr, *oseg = nullptr;  // misc: [0] counter, [1] the record count for the kernel | seg_info
    void *stmp = nullptr, *utmp = nullptr;
    const size_t sbytes = sort_temp_bytes(n), ubytes = unique_temp_bytes((uint32_t)n), iwords = dedup_seg_info_words() + 4;
    check_memcpy(hipMalloc((void**)&a, n * sizeof(HspRec)), "order segs: records");
    check_memcpy(hipMalloc((void**)&b, n * sizeof(HspRec)), "order segs: records");
    check_memcpy(hipMalloc((void**)&o16, n * sizeof(uint4)), "order segs: output");
    check_memcpy(hipMalloc((void**)&oseg, n * sizeof(uint32_t)), "order segs: output segments");
    check_memcpy(hipMalloc((void**)&misc, iwords * sizeof(uint32_t)), "order segs: counters");
    check_memcpy(hipMalloc(&stmp, sbytes), "order segs: sort temp");
    check_memcpy(hipMalloc(&utmp, ubytes), "order segs: unique temp");
    check_memcpy(hipMemcpy(a, h.data(), n * sizeof(HspRec), hipMemcpyHostToDevice), "order segs: upload");
    check_memcpy(hipMemset(misc, 0, iwords * sizeof(uint32_t)), "order segs: counters");  // (the segment-info words must be zero on entry)
    hipStream_t st = 0;
    size_t m = 0;
    sa_segment_pair* res = (sa_segment_pair*)malloc(n * sizeof(sa_segment_pair));
    uint32_t* rseg = (uint32_t*)malloc(n * sizeof(uint32_t));
    auto count = [&]() { uint32_t c = 0; check_memcpy(hipMemcpy(&c, misc, sizeof(c), hipMemcpyDeviceToHost), "order segs: count"); return (size_t)c; };
    if (path == 0) {
        uint32_t* info = misc + 4;
        if (count_on_device) {
            const uint32_t n32 = (uint32_t)n;
            check_memcpy(hipMemcpy(misc + 1, &n32, sizeof(n32), hipMemcpyHostToDevice), "order segs: device count");
            launch_dedup_seg(a, 0, misc + 1, nsegs, o16, info, threads, seg_max, st);
        } else {
            launch_dedup_seg(a, (uint32_t)n, nullptr, nsegs, o16, info, threads, seg_max, st);
        }
        check_launch("order segs: dedup seg");
        std::vector<uint32_t> hi(dedup_seg_info_words());
        check_memcpy(hipMemcpy(hi.data(), info, hi.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), "order segs: segment info");
        if (hi[hi.size() - 1] != 0) {
            *refused = 1;
        } else {
            check_memcpy(hipMemcpy(res, o16, n * sizeof(sa_segment_pair), hipMemcpyDeviceToHost), "order segs: download");  // the raw slots
            m = close_seg_gaps(res, rseg, hi.data(), nsegs);
        }
    } else {
        if (!rm) {
            launch_sort(a, b, n, ORDER_DIAG, stmp, sbytes, st);
            launch_unique(b, a, (uint32_t)n, 0, misc, utmp, st);
            m = count();
            launch_sort(a, b, m, ORDER_LASTZ, stmp, sbytes, st);
        } else {
            launch_sort(a, b, n, ORDER_RM_FIRST, stmp, sbytes, st);
            launch_unique(b, a, (uint32_t)n, 1, misc, utmp, st);
            const size_t m1 = count();
            launch_sort(a, b, m1, ORDER_RM_DIAG, stmp, sbytes, st);
            launch_unique(b, a, (uint32_t)m1, 0, misc, utmp, st);
            m = count();
            launch_sort(a, b, m, ORDER_RM_FINAL, stmp, sbytes, st);
        }
        launch_strip(b, (uint32_t)m, o16, oseg, st);
        check_launch("order segs: sort chain");
        if (m) {
            check_memcpy(hipMemcpy(res, o16, m * sizeof(sa_segment_pair), hipMemcpyDeviceToHost), "order segs: download");
            check_memcpy(hipMemcpy(rseg, oseg, m * sizeof(uint32_t), hipMemcpyDeviceToHost), "order segs: segments");
        }
    }
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(o16); (void)hipFree(oseg); (void)hipFree(misc); (void)hipFree(stmp); (void)hipFree(utmp);
    if (*refused) {
        free(res);
        free(rseg);
        return 0;
    }
    for (size_t i = 0; i < m; i++)
        if (rseg[i] < nsegs) seg_counts[rseg[i]]++;
    *out = res;
    *out_seg = rseg;
    return m;
}

// The prefix scan alone (scan.hip: reduce, scan of the tile sums, downsweep) on `n` counts the host hands in.  The scan's `in` is a
// 256-byte-aligned allocation plus `skew` words (0..7: which of load_tile's two loads runs is the caller's pointer's choice), its scratch
// exactly scan_temp_bytes(n) bytes and its output n + 1 values of `width` bits (32: launch_exclusive_scan_u32, 64: _u64), each followed
// directly by SCAN_GUARD bytes of a known pattern; the scratch holds a non-zero pattern on entry, so a partial the kernels do not write
// cannot pass for a zero.  One scan runs, in a slot taken as sa_net_chains takes one (InitializeInterface is enough).  out: the caller's
// n + 1 values of `width` bits; intact[0..2]: the guard behind the scratch, the guard behind the output and the input (with the skew
// words in front of it) came back as they were written, 1 or 0.  Test entry (tests/test_gpu_scan.py holds it to numpy.cumsum): own
// buffers, no kernel of its own, the guards are compared on the host.  A skew above 7, a width other than 32 / 64 or n >= 2^31 ends the
// process with a message and exit code 1.
int sa_scan_counts(const uint32_t* counts, size_t n, uint32_t skew, int width, void* out, uint32_t* intact) {
    require_init("sa_scan_counts");
    if (skew > 7 || (width != 32 && width != 64) || n > 0x7FFFFFFFull) {
        fprintf(stderr, "Error: sa_scan_counts: skew %u (0..7), width %d (32 or 64) or %zu counts (below 2^31) out of range\n", skew, width, n);
        exit(1);
    }
    constexpr size_t SCAN_GUARD = 4096;
    constexpr int PAT_SKEW = 0x3C, PAT_TEMP = 0xA5, PAT_OUT = 0xE7, PAT_GUARD = 0x5C;
    const size_t in_bytes = ((size_t)skew + n) * sizeof(uint32_t), temp_bytes = scan_temp_bytes(n), out_bytes = (n + 1) * (size_t)(width / 8);
    Slot* sl = acquire_slot_early();
    hipStream_t st = sl->stream;
    uint8_t *d_in = nullptr, *d_temp = nullptr, *d_out = nullptr;
    check_memcpy(hipMalloc((void**)&d_in, std::max<size_t>(in_bytes, 256)), "scan counts: input");
    check_memcpy(hipMalloc((void**)&d_temp, temp_bytes + SCAN_GUARD), "scan counts: scratch");
    check_memcpy(hipMalloc((void**)&d_out, out_bytes + SCAN_GUARD), "scan counts: output");
    if ((reinterpret_cast<uintptr_t>(d_in) & 255) != 0) {
        fprintf(stderr, "Error: sa_scan_counts: the input allocation is not 256-byte aligned\n");
        exit(15);
    }
    std::vector<uint32_t> h_in((size_t)skew + n, 0x01010101u * PAT_SKEW), back_in(h_in.size());  // (the skew words keep the pattern)
    if (n) memcpy(h_in.data() + skew, counts, n * sizeof(uint32_t));
    if (in_bytes) check_memcpy(hipMemcpyAsync(d_in, h_in.data(), in_bytes, hipMemcpyHostToDevice, st), "scan counts: upload");
    check_memcpy(hipMemsetAsync(d_temp, PAT_TEMP, temp_bytes, st), "scan counts: scratch pattern");
    check_memcpy(hipMemsetAsync(d_temp + temp_bytes, PAT_GUARD, SCAN_GUARD, st), "scan counts: scratch guard");
    check_memcpy(hipMemsetAsync(d_out, PAT_OUT, out_bytes, st), "scan counts: output pattern");
    check_memcpy(hipMemsetAsync(d_out + out_bytes, PAT_GUARD, SCAN_GUARD, st), "scan counts: output guard");
    const uint32_t* in = reinterpret_cast<const uint32_t*>(d_in) + skew;
    if (width == 32) launch_exclusive_scan_u32(in, reinterpret_cast<uint32_t*>(d_out), n, d_temp, st);
    else launch_exclusive_scan_u64(in, reinterpret_cast<uint64_t*>(d_out), n, d_temp, st);
    check_launch("scan counts");
    std::vector<uint8_t> g_temp(SCAN_GUARD), g_out(SCAN_GUARD);
    check_memcpy(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st), "scan counts: download");
    check_memcpy(hipMemcpyAsync(g_temp.data(), d_temp + temp_bytes, SCAN_GUARD, hipMemcpyDeviceToHost, st), "scan counts: scratch guard");
    check_memcpy(hipMemcpyAsync(g_out.data(), d_out + out_bytes, SCAN_GUARD, hipMemcpyDeviceToHost, st), "scan counts: output guard");
    if (in_bytes) check_memcpy(hipMemcpyAsync(back_in.data(), d_in, in_bytes, hipMemcpyDeviceToHost, st), "scan counts: input back");
    check_sync(st, "scan counts");
    auto all_guard = [&](const std::vector<uint8_t>& g) {
        for (uint8_t b : g)
            if (b != (uint8_t)PAT_GUARD) return 0u;
        return 1u;
    };
    intact[0] = all_guard(g_temp);
    intact[1] = all_guard(g_out);
    intact[2] = back_in == h_in ? 1u : 0u;
    (void)hipFree(d_in); (void)hipFree(d_temp); (void)hipFree(d_out);
    release_slot(sl);
    return 0;
}

}  // extern "C"
