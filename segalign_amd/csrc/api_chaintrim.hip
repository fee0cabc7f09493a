// api_chaintrim.hip -- C-ABI sa_trim_chains: the overlaps of chains cut at the best crossover (contract: include/segalign_amd.h,
// DESIGN.md 24).  The host side as steps: the checked members and links, the crossover of every overlapping link (chaintrim.hip), the
// exact scores of the cut members (stitch.hip's member kernel, which scores a member's columns), and the chains' exact scores.
#include "post_host.h"
#include "chaintrim.h"
#include "hspcost.h"

using namespace sa;

namespace {

const Fail fail{"TrimChains"};

}  // namespace

extern "C" {

size_t sa_trim_chains(const sa_segment_pair* hsps, size_t n_hsps, const uint32_t* members, const uint32_t* first, size_t n_chains, int rev,
                      uint32_t buffer, const sa_chain_params* p, const sa_chain_gap_costs* g, uint32_t flags, sa_segment_pair** out_hsps,
                      sa_trim_chain** chains, sa_trim_link** links, size_t* n_links, sa_trim_stats* stats) {
    const char* who = "TrimChains";
    *out_hsps = nullptr;
    *chains = nullptr;
    if (links) *links = nullptr;
    if (n_links) *n_links = 0;
    sa_trim_stats st;
    memset(&st, 0, sizeof(st));
    if (stats) *stats = st;
    require_proc(who, buffer);
    sa_chain_params P = {0, 0, 0, 0, 0};
    if (p) P = *p;
    if (P.diag_pen < 0 || P.diag_pen > (1 << 20)) fail("diag_pen = %lld out of range", P.diag_pen);
    if (P.anti_pen < 0 || P.anti_pen > (1 << 20)) fail("anti_pen = %lld out of range", P.anti_pen);
    if (flags & ~SA_TRIM_LINKS) fail("flags = %lld: unknown bits", flags);
    if ((flags & SA_TRIM_LINKS) && (!links || !n_links)) fail("SA_TRIM_LINKS needs links and n_links");
    CostImage costs;
    checked_costs(who, g, costs);
    const size_t M = checked_first(fail, first, n_chains);
    if (M == 0) return 0;

    Slot* sl = acquire_slot();
    const hipStream_t s = sl->stream;
    StitchArgs a;
    resident_block(who, sl, rev, buffer, a);

    // the members, each inside the block; out starts as the input HSPs, so that an untouched member is returned bit for bit
    std::vector<sa_segment_pair> out(M);
    for (size_t k = 0; k < M; k++) out[k] = checked_member(fail, hsps, n_hsps, members, k, a.ref_len, a.query_len);
    // the links in entry order: overlap, gaps between the trimmed members, and a crossover task where o > 0
    std::vector<sa_trim_link> lk;
    std::vector<size_t> lk_entry;  // the entry of the link's first member
    std::vector<TrimLinkTask> tasks;
    std::vector<size_t> task_link;
    for (size_t c = 0; c < n_chains; c++)
        for (size_t k = first[c]; k + 1 < first[c + 1]; k++) {
            const sa_segment_pair &j = out[k], &i = out[k + 1];
            const int64_t bj = (int64_t)j.len + 1, bi = (int64_t)i.len + 1;
            const int64_t re = (int64_t)j.ref_start + bj, qe = (int64_t)j.query_start + bj;
            const int64_t o = std::max<int64_t>(0, std::max(re - (int64_t)i.ref_start, qe - (int64_t)i.query_start));
            if (o > SA_CHAIN_MAX_OVERLAP || 2 * o >= std::min(bj, bi))
                fail("chain %lld: the member at position %lld overlaps the next one by more than 4096 bases or half of the shorter",
                     (long long)c, (long long)(k - first[c]));
            const int64_t gap_r = (int64_t)i.ref_start + o - re, gap_q = (int64_t)i.query_start + o - qe;
            lk.push_back({(uint32_t)o, 0u, (uint32_t)gap_r, (uint32_t)gap_q});
            lk_entry.push_back(k);
            if (o > 0) {
                tasks.push_back({(uint32_t)(re - o), (uint32_t)(qe - o), i.ref_start, i.query_start, (uint32_t)o, 0u});
                task_link.push_back(lk.size() - 1);
            }
        }

    Timer<4> tm(s, "trim timing");
    const size_t T = tasks.size();
    std::vector<StitchMember> cut;
    std::vector<size_t> cut_entry;
    if (T) {
        TrimLinkTask* d_tasks;
        uint32_t* d_x;
        carve(sl->stitch, "trim", [&](Carve& c) { c.take(d_tasks, T).take(d_x, T); });
        to_device(d_tasks, tasks.data(), T, s, "trim tasks");
        tm.mark(0);
        launch(sl, "chaintrim_crossover", [&] { launch_chaintrim_crossover(a, d_tasks, (uint32_t)T, d_x, s); });
        tm.mark(1);
        std::vector<uint32_t> x(T);
        to_host(x.data(), d_x, T, s, "trim crossovers");
        check_sync(s, "chaintrim_crossover");
        st.kernel_ms += tm.ms(0, 1);
        // cut the members: j loses its last o - x columns, i its first x; o1 + o2 < bases leaves every member a base
        std::vector<uint8_t> touched(M, 0);
        for (size_t t = 0; t < T; t++) {
            sa_trim_link& l = lk[task_link[t]];
            if (x[t] > l.o) {
                fprintf(stderr, "Error: TrimChains: crossover %u of an overlap of %u\n", x[t], l.o);
                exit(15);
            }
            l.x = x[t];
            const size_t k = lk_entry[task_link[t]];
            if (l.o - l.x) {
                out[k].len -= l.o - l.x;
                touched[k] = 1;
            }
            if (l.x) {
                out[k + 1].ref_start += l.x;
                out[k + 1].query_start += l.x;
                out[k + 1].len -= l.x;
                touched[k + 1] = 1;
            }
        }
        for (size_t k = 0; k < M; k++)
            if (touched[k]) {
                cut.push_back({out[k].ref_start, out[k].query_start, out[k].len, 0});
                cut_entry.push_back(k);
            }
    }
    if (const size_t K = cut.size()) {  // the cut members' exact scores, one wave each
        StitchMember* d_mem;
        StitchMemberOut* d_mo;
        carve(sl->stitch, "trim", [&](Carve& c) { c.take(d_mem, K).take(d_mo, K); });
        to_device(d_mem, cut.data(), K, s, "trim members");
        tm.mark(2);
        launch(sl, "chaintrim_rescore", [&] { launch_stitch_members(a, d_mem, (uint32_t)K, d_mo, s); });
        tm.mark(3);
        std::vector<StitchMemberOut> mo(K);
        to_host(mo.data(), d_mo, K, s, "trim member scores");
        check_sync(s, "chaintrim_rescore");
        st.kernel_ms += tm.ms(2, 3);
        for (size_t k = 0; k < K; k++) {
            if (mo[k].score > INT32_MAX || mo[k].score < INT32_MIN) fail("the score of member %lld leaves int32", (long long)cut_entry[k]);
            out[cut_entry[k]].score = (int32_t)mo[k].score;
        }
    }
    prof_flush(sl);
    release_slot(sl);

    // the chains: member scores less the links' penalties on the gaps between the trimmed members
    std::vector<sa_trim_chain> ch(n_chains);
    alignas(16) uint32_t image[HSPCOST_WORDS];  // the lookup reads a row in one 16-byte access
    memcpy(image, costs.w, sizeof(image));
    size_t at = 0;  // the next link
    for (size_t c = 0; c < n_chains; c++) {
        sa_trim_chain r = {0, 0, 0};
        for (size_t k = first[c]; k < first[c + 1]; k++) {
            r.score += out[k].score;
            if (k + 1 == first[c + 1]) break;
            const sa_trim_link& l = lk[at++];
            const sa_segment_pair &j = hsps[members[k]], &i = hsps[members[k + 1]];  // the diagonals are the untrimmed ones: a cut moves both axes alike
            const int64_t dd = ((int64_t)i.ref_start - (int64_t)i.query_start) - ((int64_t)j.ref_start - (int64_t)j.query_start);
            int64_t pen = (int64_t)P.diag_pen * (dd < 0 ? -dd : dd) + (int64_t)P.anti_pen * ((int64_t)l.gap_r + (int64_t)l.gap_q);
            if (costs.on) pen += hspcost_gapcost(image, l.gap_r, l.gap_q);
            r.score -= pen;
            if (l.o) {
                r.trimmed_links++;
                r.bases_cut += l.o;
            }
        }
        ch[c] = r;
        st.trimmed_links += r.trimmed_links;
        st.bases_cut += r.bases_cut;
    }
    st.chains = n_chains;
    st.members = M;
    st.links = lk.size();
    st.cut_members = cut.size();
    if (stats) *stats = st;
    *out_hsps = malloc_copy(out, who);
    *chains = malloc_copy(ch, who);
    if (flags & SA_TRIM_LINKS) {
        *links = malloc_copy(lk, who);
        *n_links = lk.size();
    }
    return M;
}

void sa_free_trim(sa_segment_pair* out_hsps, sa_trim_chain* chains, sa_trim_link* links) {
    free(out_hsps);
    free(chains);
    free(links);
}

}  // extern "C"
