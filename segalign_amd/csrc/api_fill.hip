// api_fill.hip -- C-ABI sa_fill_chains: the links of chains filled with HSPs from an exhaustive diagonal sweep (contract:
// include/segalign_amd.h).  The host side as steps: the checked members and links; the sweep of the links in batches of
// at most FILL_BATCH_LANES diagonals (fill.hip: count, prefix sum, emit in groups of whole links); with the slot given back, the best
// chain of every link's HSPs through sa_chain_hsps_costs; and the assembly of the filled chains.
#include "post_host.h"
#include "fill.h"
#include "hspcost.h"

using namespace sa;

namespace {

const Fail fail{"FillChains"};

struct Params {
    int32_t thresh, xdrop;
    uint32_t max_side, max_link_hsps;
    uint64_t max_cells;
    int64_t min_fill;
};

Params resolve(const sa_fill_params* fp) {
    Params r = {3000, 910, 32768u, 65536u, (uint64_t)1 << 30, 0};
    if (fp) {
        r.thresh = fp->thresh;
        r.xdrop = fp->xdrop;
        if (fp->max_side) r.max_side = fp->max_side;
        if (fp->max_link_hsps) r.max_link_hsps = fp->max_link_hsps;
        if (fp->max_cells) r.max_cells = fp->max_cells;
        r.min_fill = fp->min_fill;
    }
    if (r.thresh < 1) fail("thresh = %lld: at least 1", r.thresh);
    if (r.xdrop < 0) fail("xdrop = %lld: at least 0", r.xdrop);
    if (r.max_side > (1u << 20)) fail("max_side = %lld: at most 1 << 20", r.max_side);
    if (r.max_cells > ((uint64_t)1 << 36)) fail("max_cells = %lld: at most 1 << 36", (long long)r.max_cells);
    if (r.max_link_hsps > (1u << 22)) fail("max_link_hsps = %lld: at most 1 << 22", r.max_link_hsps);
    long long A = 0;
    for (int x = 0; x < 7; x++)
        for (int y = 0; y < 7; y++) A = std::max(A, std::llabs((long long)g_sub_mat[x * 8 + y]));
    // a diagonal has at most max_side cells, so |s| <= max_side A
    if ((long long)r.max_side * A >= (1ll << 31)) fail("max_side = %lld leaves no int32 headroom (max_side * %lld >= 1 << 31)", r.max_side, A);
    return r;
}

struct Origin {  // a link's rectangle
    uint32_t re, qe;
};

// The sweep of the links sw (indices into lk, ascending), all of them to be swept: what they hold, appended to found in the contract's
// order; a crowded link is flagged and adds nothing.
void sweep(Slot* sl, const StitchArgs& a, const Params& P, std::vector<sa_fill_link>& lk, const std::vector<Origin>& org,
           const std::vector<size_t>& sw, std::vector<sa_fill_hsp>& found, sa_fill_stats& st) {
    const hipStream_t s = sl->stream;
    const FillScan f = {P.thresh, P.xdrop};
    const size_t cap = std::max<size_t>((size_t)1 << 20, P.max_link_hsps);  // the HSPs of an emit group; a link that is not crowded fits
    Timer<4> tm(s, "fill timing");
    std::vector<FillTask> tasks;
    std::vector<uint32_t> at;  // a link's first lane; the batch's lanes behind the last
    std::vector<uint64_t> loff;
    std::vector<sa_segment_pair> h_out;
    std::vector<uint32_t> h_link;
    auto waves = [&](size_t l) { return ((uint64_t)lk[l].dt + lk[l].dq - 1 + 63) / 64; };
    for (size_t b = 0; b < sw.size();) {
        size_t e = b;
        uint64_t T = 0;
        while (e < sw.size() && (e == b || (T + waves(sw[e])) * 64 <= FILL_BATCH_LANES)) T += waves(sw[e++]);
        const size_t nl = e - b;
        tasks.clear();
        at.clear();
        for (size_t k = b; k < e; k++) {
            const sa_fill_link& l = lk[sw[k]];
            at.push_back((uint32_t)(tasks.size() * 64));
            const uint64_t w = waves(sw[k]);
            for (uint64_t v = 0; v < w; v++)
                tasks.push_back({org[sw[k]].re, org[sw[k]].qe, l.dt, l.dq, (int32_t)(-(int64_t)(l.dq - 1) + 64 * (int64_t)v), (uint32_t)sw[k]});
        }
        const uint32_t n = (uint32_t)(T * 64);
        at.push_back(n);
        FillTask* d_tasks;
        uint32_t *d_cnt, *d_at, *d_olink;
        uint64_t *d_off, *d_loff;
        sa_segment_pair* d_out;
        uint8_t* temp;
        size_t temp_bytes = 0;
        cover_scan_offsets(nullptr, &temp_bytes, nullptr, nullptr, n, s);
        temp_bytes = std::max<size_t>(temp_bytes, 256);
        carve(sl->fill, "fill", [&](Carve& c) {
            c.take(d_tasks, T).take(d_cnt, (size_t)n + 1).take(d_off, (size_t)n + 1).take(d_at, nl + 1).take(d_loff, nl + 1);
            c.take(temp, temp_bytes).take(d_out, cap).take(d_olink, cap);
        });
        to_device(d_tasks, tasks.data(), T, s, "fill tasks");
        to_device(d_at, at.data(), nl + 1, s, "fill links");
        check_memcpy(hipMemsetAsync(d_cnt + n, 0, sizeof(uint32_t), s), "fill counts");  // the prefix sum reads n + 1 entries
        tm.mark(0);
        launch(sl, "fill_count", [&] {
            launch_fill_count(a, f, d_tasks, (uint32_t)T, d_cnt, s);
            cover_scan_offsets(temp, &temp_bytes, d_cnt, d_off, n, s);
            launch_fill_gather(d_off, d_at, (uint32_t)(nl + 1), d_loff, s);
        });
        tm.mark(1);
        loff.resize(nl + 1);
        to_host(loff.data(), d_loff, nl + 1, s, "fill offsets");
        check_sync(s, "fill_count");
        st.count_ms += tm.ms(0, 1);
        for (size_t k = 0; k < nl; k++) {
            sa_fill_link& l = lk[sw[b + k]];
            const uint64_t c = loff[k + 1] - loff[k];
            l.n_hsps = (uint32_t)std::min<uint64_t>(c, 0xFFFFFFFFu);
            if (c > P.max_link_hsps) l.flags |= SA_FILL_CROWDED;
        }
        // emit in groups of consecutive links that are not crowded and hold at most cap HSPs together
        for (size_t k = 0; k < nl;) {
            if (lk[sw[b + k]].flags & SA_FILL_CROWDED) {
                k++;
                continue;
            }
            size_t k1 = k;
            uint64_t H = 0;
            while (k1 < nl && !(lk[sw[b + k1]].flags & SA_FILL_CROWDED) && H + lk[sw[b + k1]].n_hsps <= cap) H += lk[sw[b + k1++]].n_hsps;
            if (H) {
                tm.mark(2);
                launch(sl, "fill_emit", [&] { launch_fill_emit(a, f, d_tasks, at[k] / 64, at[k1] / 64, d_off, loff[k], d_out, d_olink, s); });
                tm.mark(3);
                h_out.resize(H);
                h_link.resize(H);
                to_host(h_out.data(), d_out, H, s, "fill HSPs");
                to_host(h_link.data(), d_olink, H, s, "fill HSP links");
                check_sync(s, "fill_emit");
                st.emit_ms += tm.ms(2, 3);
                if (found.size() + H >= 0xFFFFFFFFull) fail("more than 2^32 - 1 HSPs found: raise thresh");
                for (size_t i = 0; i < H; i++)
                    found.push_back({h_out[i].ref_start, h_out[i].query_start, h_out[i].len, h_out[i].score, h_link[i], 0u});
            }
            k = k1;
        }
        b = e;
    }
}

}  // namespace

extern "C" {

size_t sa_fill_chains(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, const uint32_t* first, size_t n_chains, int rev,
                      uint32_t buffer, const sa_chain_params* p, const sa_chain_gap_costs* g, const sa_fill_params* fp, uint32_t flags,
                      sa_segment_pair** out_hsps, uint32_t** first_out, uint32_t** origin, sa_fill_chain** chains, sa_fill_link** links,
                      size_t* n_links, sa_fill_hsp** found_out, size_t* n_found, sa_fill_stats* stats) {
    const char* who = "FillChains";
    *out_hsps = nullptr;
    *first_out = nullptr;
    *origin = nullptr;
    *chains = nullptr;
    if (links) *links = nullptr;
    if (n_links) *n_links = 0;
    if (found_out) *found_out = nullptr;
    if (n_found) *n_found = 0;
    sa_fill_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_proc(who, buffer);
    sa_chain_params CP = {0, 0, 0, 0, 0};
    if (p) CP = *p;
    if (CP.diag_pen < 0 || CP.diag_pen > (1 << 20)) fail("diag_pen = %lld out of range", CP.diag_pen);
    if (CP.anti_pen < 0 || CP.anti_pen > (1 << 20)) fail("anti_pen = %lld out of range", CP.anti_pen);
    const Params P = resolve(fp);
    CP.min_score = P.min_fill;
    if (flags & ~(SA_FILL_LINKS | SA_FILL_HSPS)) fail("flags = %lld: unknown bits", flags);
    if ((flags & SA_FILL_LINKS) && (!links || !n_links)) fail("SA_FILL_LINKS needs links and n_links");
    if ((flags & SA_FILL_HSPS) && (!found_out || !n_found)) fail("SA_FILL_HSPS needs found and n_found");
    CostImage costs;
    checked_costs(who, g, costs);
    const size_t M = checked_first(fail, first, n_chains);
    if (n_chains == 0) return 0;

    std::vector<sa_fill_link> lk;
    std::vector<Origin> org;
    std::vector<sa_fill_hsp> found;
    if (M) {
        Slot* sl = acquire_slot();
        StitchArgs a;
        resident_block(who, sl, rev, buffer, a);
        for (size_t k = 0; k < M; k++) checked_member(fail, hsps, n_hsps, members, k, a.ref_len, a.query_len);
        std::vector<size_t> sw;
        for (size_t c = 0; c < n_chains; c++)
            for (size_t k = first[c]; k + 1 < first[c + 1]; k++) {
                const sa_segment_pair &x = hsps[members[k]], &y = hsps[members[k + 1]];
                const uint64_t re = (uint64_t)x.ref_start + x.len + 1, qe = (uint64_t)x.query_start + x.len + 1;
                if (re > y.ref_start || qe > y.query_start)
                    fail("chain %lld: the member at position %lld does not end before the next one starts (trim overlapping chains with "
                         "sa_trim_chains first)", (long long)c, (long long)(k - first[c]));
                sa_fill_link l = {(uint32_t)(y.ref_start - re), (uint32_t)(y.query_start - qe), 0, 0, 0, 0, 0};
                if (l.dt && l.dq) {
                    if (l.dt > P.max_side || l.dq > P.max_side) l.flags = SA_FILL_LONG;
                    else if ((uint64_t)l.dt * l.dq > P.max_cells) l.flags = SA_FILL_LARGE;
                    else {
                        l.cells = (uint64_t)l.dt * l.dq;
                        sw.push_back(lk.size());
                    }
                }
                lk.push_back(l);
                org.push_back({(uint32_t)re, (uint32_t)qe});
            }
        sweep(sl, a, P, lk, org, sw, found, st);
        prof_flush(sl);
        release_slot(sl);  // before the chaining: an entry that holds a slot never calls one that takes a slot
        st.swept = sw.size();
    }

    // the best chain of every link's HSPs: found is in link order, a batch is whole links of at most 1 << 22 HSPs together
    std::vector<uint32_t> fill_at(lk.size() + 1, 0);  // link l's fills are fill_idx[fill_at[l] .. fill_at[l + 1])
    std::vector<uint32_t> fill_idx;
    {
        std::vector<sa_segment_pair> hs;
        std::vector<uint32_t> grp;
        std::vector<uint32_t> n_of(lk.size(), 0);
        for (size_t b = 0; b < found.size();) {
            size_t e = b;
            while (e < found.size()) {
                size_t e1 = e;
                while (e1 < found.size() && found[e1].link == found[e].link) e1++;
                if (e1 - b > ((size_t)1 << 22)) break;  // a link alone fits: max_link_hsps <= 1 << 22
                e = e1;
            }
            hs.resize(e - b);
            grp.resize(e - b);
            for (size_t i = b; i < e; i++) {
                hs[i - b] = {found[i].ref_start, found[i].query_start, found[i].len, found[i].score};
                grp[i - b] = found[i].link;
            }
            sa_chain_member* mem = nullptr;
            sa_chain_stats cs;
            const size_t m = sa_chain_hsps_costs(hs.data(), hs.size(), grp.data(), &CP, g, &mem, nullptr, &cs);
            st.chain_ms += cs.kernel_ms;
            for (size_t i = 0; i < m; i++) {  // groups ascending, members in chain order
                fill_idx.push_back((uint32_t)(b + mem[i].hsp_index));
                n_of[mem[i].group]++;
            }
            sa_free_chain(mem, nullptr);
            b = e;
        }
        for (size_t l = 0; l < lk.size(); l++) {
            fill_at[l + 1] = fill_at[l] + n_of[l];
            lk[l].n_fill = n_of[l];
        }
    }

    // the filled chains
    const uint64_t E64 = (uint64_t)M + fill_idx.size();
    if (E64 >= 0xFFFFFFFFull) fail("the filled chains have more than 2^32 - 1 entries");
    std::vector<sa_segment_pair> out;
    std::vector<uint32_t> org_out, fo(n_chains + 1, 0);
    std::vector<sa_fill_chain> ch(n_chains);
    out.reserve(E64);
    org_out.reserve(E64);
    alignas(16) uint32_t image[HSPCOST_WORDS];  // the lookup reads a row in one 16-byte access
    memcpy(image, costs.w, sizeof(image));
    size_t at = 0;  // the next link
    for (size_t c = 0; c < n_chains; c++) {
        sa_fill_chain r = {0, 0, 0};
        const size_t e0 = out.size();
        for (size_t k = first[c]; k < first[c + 1]; k++) {
            out.push_back(hsps[members[k]]);
            org_out.push_back(members[k]);
            if (k + 1 == first[c + 1]) break;
            const size_t l = at++;
            for (uint32_t i = fill_at[l]; i < fill_at[l + 1]; i++) {
                const sa_fill_hsp& h = found[fill_idx[i]];
                out.push_back({h.ref_start, h.query_start, h.len, h.score});
                org_out.push_back(SA_FILL_NONE);
                r.fills++;
                r.fill_bases += h.len + 1;
            }
            if (lk[l].n_fill) st.filled_links++;
        }
        for (size_t k = e0; k < out.size(); k++) {
            r.score += out[k].score;
            if (k + 1 == out.size()) break;
            const sa_segment_pair &j = out[k], &i = out[k + 1];
            const int64_t dd = ((int64_t)i.ref_start - (int64_t)i.query_start) - ((int64_t)j.ref_start - (int64_t)j.query_start);
            const int64_t gap_r = (int64_t)i.ref_start - ((int64_t)j.ref_start + j.len + 1);
            const int64_t gap_q = (int64_t)i.query_start - ((int64_t)j.query_start + j.len + 1);
            int64_t pen = (int64_t)CP.diag_pen * (dd < 0 ? -dd : dd) + (int64_t)CP.anti_pen * (gap_r + gap_q);
            if (costs.on) pen += hspcost_gapcost(image, gap_r, gap_q);
            r.score -= pen;
        }
        ch[c] = r;
        fo[c + 1] = (uint32_t)out.size();
        st.fills += r.fills;
    }
    st.links = lk.size();
    for (const sa_fill_link& l : lk) {
        st.long_links += (l.flags & SA_FILL_LONG) != 0;
        st.large_links += (l.flags & SA_FILL_LARGE) != 0;
        st.crowded_links += (l.flags & SA_FILL_CROWDED) != 0;
        st.cells += l.cells;
    }
    st.hsps = found.size();
    if (stats) *stats = st;
    *out_hsps = malloc_copy(out, who);
    *origin = malloc_copy(org_out, who);
    *first_out = malloc_copy(fo, who);
    *chains = malloc_copy(ch, who);
    if (flags & SA_FILL_LINKS) {
        *links = malloc_copy(lk, who);
        *n_links = lk.size();
    }
    if (flags & SA_FILL_HSPS) {
        *found_out = malloc_copy(found, who);
        *n_found = found.size();
    }
    return out.size();
}

void sa_free_fill(sa_segment_pair* out_hsps, uint32_t* first_out, uint32_t* origin, sa_fill_chain* chains, sa_fill_link* links,
                  sa_fill_hsp* found) {
    free(out_hsps);
    free(first_out);
    free(origin);
    free(chains);
    free(links);
    free(found);
}

}  // extern "C"
