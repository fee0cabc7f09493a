// post_checks_main.cpp -- tests/test_post_checks.py's probe of segalign_amd/csrc/post_checks.h: one named case per run, its input built
// here, one shared check called under the entry name "Probe".  Good input prints what the check returned and exits 0; bad input ends in
// the check's own message and exit 1; an unknown case exits 2.
#include <cstring>
#include <string>
#include <vector>

#include "post_checks.h"

using namespace sa;

namespace {

const Fail fail{"Probe"};
const uint32_t OVER_22 = (1u << 22) + 1, OVER_26 = (1u << 26) + 1, TOP = 1u << 31;

// Two chains of two and three blocks; chain 1 runs down the other axis.
struct Pairs {
    std::vector<uint32_t> first = {0, 2, 5};
    std::vector<uint32_t> bs = {10, 30, 5, 50, 70}, be = {20, 40, 15, 60, 80};
    std::vector<uint32_t> obs = {100, 120, 300, 200, 100}, obe = {110, 130, 310, 210, 110};
    std::vector<uint8_t> ostrand = {0, 1};
    int run(size_t n = 2, bool with_strand = true) const {
        printf("%u\n", checked_block_pairs(fail, first.data(), bs.data(), be.data(), obs.data(), obe.data(), with_strand ? ostrand.data() : nullptr, n));
        return 0;
    }
};

int run_first(std::vector<uint32_t> first, size_t n) {
    printf("%zu\n", checked_first(fail, first.empty() ? nullptr : first.data(), n));
    return 0;
}

// Three HSPs in a block of 100 by 80 bases; the last one ends on both of the block's ends.
int run_member(std::vector<sa_segment_pair> hsps, std::vector<uint32_t> members, size_t k) {
    const sa_segment_pair& h = checked_member(fail, hsps.data(), hsps.size(), members.data(), k, 100, 80);
    printf("%u %u %u\n", h.ref_start, h.query_start, h.len);
    return 0;
}
const std::vector<sa_segment_pair> HSPS = {{0, 0, 9, 1}, {10, 10, 19, 2}, {90, 70, 9, 3}};

// Fill 3 of a net over chains of two and three blocks.
int run_fill(uint32_t chain, uint32_t start, uint32_t end, uint32_t first_block, uint32_t n_blocks) {
    const uint32_t first[3] = {0, 2, 5};
    sa_net_fill f;
    memset(&f, 0, sizeof(f));
    f.chain = chain;
    f.start = start;
    f.end = end;
    f.first_block = first_block;
    f.n_blocks = n_blocks;
    checked_fill_in_chain(fail, f, 3, first, 2);
    printf("ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    Pairs p;
    if (c == "first_ok") return run_first({0, 2, 5}, 2);
    if (c == "first_no_chains") return run_first({}, 0);
    if (c == "first_empty_chain") return run_first({0, 0, 3}, 2);
    if (c == "first_too_many_chains") return run_first({}, OVER_22);  // fires before first[] is read
    if (c == "first_not_zero") return run_first({1, 2, 3}, 2);
    if (c == "first_descends") return run_first({0, 2, 1}, 2);
    if (c == "first_too_many_members") return run_first({0, OVER_22}, 1);
    if (c == "first_not_zero_and_descends") return run_first({1, 2, 1}, 2);

    if (c == "member_ok") return run_member(HSPS, {0, 1, 2}, 2);
    if (c == "member_not_in_input") return run_member(HSPS, {0, 3, 1}, 1);
    if (c == "member_past_ref") return run_member({HSPS[0], HSPS[1], {91, 70, 9, 3}}, {0, 1, 2}, 2);
    if (c == "member_past_query") return run_member({HSPS[0], HSPS[1], {90, 71, 9, 3}}, {0, 1, 2}, 2);
    if (c == "member_not_in_input_and_outside") return run_member({HSPS[0], HSPS[1], {91, 70, 9, 3}}, {3, 1, 2}, 0);

    if (c == "pairs_ok") return p.run();
    if (c == "pairs_no_chains") return p.run(0);
    if (c == "pairs_no_ostrand") return p.run(1, false);
    if (c == "pairs_too_many_chains") return p.run(OVER_22);  // fires before any array is read
    if (c == "pairs_first_not_zero") return p.first = {1, 2, 5}, p.run();
    if (c == "pairs_first_descends") return p.first = {0, 2, 1}, p.run();
    if (c == "pairs_too_many_blocks") return p.first = {0, OVER_26}, p.run(1);  // fires before the blocks are read
    if (c == "pairs_ostrand_2") return p.ostrand = {0, 2}, p.run();
    if (c == "pairs_empty_block") return p.bs[1] = p.be[1], p.run();
    if (c == "pairs_ends_at_top") return p.be[4] = TOP, p.run();
    if (c == "pairs_overlap") return p.bs[1] = 19, p.be[1] = 29, p.run();
    if (c == "pairs_other_empty_block") return p.obs[3] = p.obe[3], p.run();
    if (c == "pairs_other_ends_at_top") return p.obe[1] = TOP, p.run();
    if (c == "pairs_lengths_differ") return p.obe[1] = 131, p.run();
    if (c == "pairs_other_descends_on_strand_0") return p.obs[1] = 90, p.obe[1] = 100, p.run();
    if (c == "pairs_other_overlaps_on_strand_0") return p.obs[1] = 109, p.obe[1] = 119, p.run();
    if (c == "pairs_other_ascends_on_strand_1") return p.obs[4] = 400, p.obe[4] = 410, p.run();
    if (c == "pairs_other_overlaps_on_strand_1") return p.obs[4] = 191, p.obe[4] = 201, p.run();
    if (c == "pairs_other_touches_on_strand_1") return p.obs[4] = 190, p.obe[4] = 200, p.run();
    if (c == "pairs_empty_on_both_axes") return p.bs[1] = p.be[1], p.obs[1] = p.obe[1], p.run();
    if (c == "pairs_overlap_and_later_ostrand_2") return p.bs[1] = 19, p.be[1] = 29, p.ostrand = {0, 2}, p.run();

    if (c == "fill_ok") return run_fill(1, 5, 80, 2, 3);
    if (c == "fill_empty") return run_fill(1, 80, 80, 2, 3);
    if (c == "fill_names_chain_n") return run_fill(2, 5, 80, 2, 3);
    if (c == "fill_no_blocks") return run_fill(1, 5, 80, 2, 0);
    if (c == "fill_starts_before_chain") return run_fill(1, 5, 80, 1, 2);
    if (c == "fill_runs_past_chain") return run_fill(0, 10, 40, 1, 2);
    if (c == "fill_empty_and_names_chain_n") return run_fill(2, 80, 80, 2, 3);
    fprintf(stderr, "post_checks_main: no case '%s'\n", c.c_str());
    return 2;
}
